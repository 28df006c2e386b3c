"""The baked hand rendered in another MANO pose (vanerf_amd/csrc/pose_warp.hip).

A BakedVolume (baked.py) is a field in the SOURCE pose's space, and the MANO mesh has the same faces in every pose.  A sample of a ray through
the POSED hand is carried back into source space by the affine map of its closest face (pose_transforms: posed -> source, with the unit face
normal as the third axis, so that skin thickness does not scale with the triangle's area) and looked up in the volume there.  No network runs
per view; the only per-sample geometry work is the mesh query the pass already has, on the posed mesh.  Samples farther than `reach` outside
the posed surface are empty.

This is a PREVIEW, like the baked volume itself: it approximates the field under the usual surface-aligned deformation model (each point
moves with its closest face; nothing is smoothed across face boundaries).  It does not claim what VANeRF would render from a photograph of
the new pose: the networks are conditioned on the source image and the source mesh, and are not evaluated here.  Poses arrive as vertices;
mano_sequence takes MANO pose, shape and translation parameters instead and skins them on the device first (vanerf_amd/mano.py, DESIGN.md
section 0j).

The posed hand also shows its geometry (vanerf_amd/csrc/volume_surface.hip): march_surface_posed / render_posed_surface find,
per ray through the POSED hand, where the warped field first crosses f = iso and return the depth, the posed-space normal and the colour
there; render_posed_surface_views turns them into baked.render_baked_surface_views' depth, normal-map, clay and shaded frames, and
posed_surface_sequence / mano_surface_sequence are the geometry twins of the two sequence drivers.  posed_samples is what colour and geometry
of one pose share -- transforms, rays, sample points and the mesh query, which is nearly all of a posed view's time: both renderers take it
as prepared=.
"""
import dataclasses
from ctypes import c_void_p

import torch

from ._ffi import check, lib
from .baked import (_add_vert_xy, _beta_args, _check_mode, _check_rays, _check_surface, _check_volume, _march_out, _surface_frames, _surface_out,
                    _view_rays)
from .mask_at_box import frame_bounds
from .surface import _dev_ptr, _f3, _stream

REACH = 0.03  # how far outside the posed surface a sample still reads the volume: a documented choice (a few skin thicknesses), not a measurement


def _check_mesh(verts, faces, what):
    if not (torch.is_tensor(verts) and verts.dim() == 2 and verts.shape[1] == 3 and verts.shape[0] >= 1):
        raise ValueError(f"{what}: expected a tensor (nv, 3)")
    if not (torch.is_tensor(faces) and faces.dim() == 2 and faces.shape[1] == 3 and faces.shape[0] >= 1):
        raise ValueError("faces: expected a tensor (nf, 3)")
    vp, fp = _dev_ptr(verts, torch.float32, what), _dev_ptr(faces, torch.int32, "faces")
    if faces.device != verts.device:
        raise ValueError(f"faces: expected a tensor on the device of {what}, {verts.device}")
    return vp, fp


def pose_transforms(verts_src, verts_pose, faces):
    """vanerf_pose_transforms: verts_src, verts_pose (nv, 3) fp32 and faces (nf, 3) int32 on one device -> T (nf, 12) fp32, per face the affine
    map q = A p + t from POSED space to SOURCE space as (A row-major, t).  fp64 inside, rounded once; a face without a frame (zero area in
    either mesh, a non-finite value) gets A = I, t = centroid_src - centroid_pose.  One launch."""
    sp, fp = _check_mesh(verts_src, faces, "verts_src")
    if not (torch.is_tensor(verts_pose) and tuple(verts_pose.shape) == tuple(verts_src.shape)):
        raise ValueError(f"verts_pose: expected a tensor {tuple(verts_src.shape)}, the topology of verts_src")
    if verts_pose.device != verts_src.device:
        raise ValueError(f"verts_pose: expected a tensor on the device of verts_src, {verts_src.device}")
    pp = _dev_ptr(verts_pose, torch.float32, "verts_pose")
    with torch.cuda.device(verts_src.device):
        T = torch.empty(faces.shape[0], 12, dtype=torch.float32, device=verts_src.device)
        check(lib.vanerf_pose_transforms(sp, pp, verts_src.shape[0], fp, faces.shape[0], c_void_p(T.data_ptr()), _stream()))
    return T


def _check_reach(reach):
    reach = float(reach)
    if reach != reach:
        raise ValueError("reach: expected a number (inf disables it), got NaN")
    return reach


def _check_warp(dev, T, face, sdf, shape, reach):
    """What the posed marches take beyond their rays: T (nf, 12) fp32, face int32 and sdf fp32 of z's shape, on dev, and reach -> their pointers
    and reach as a float."""
    if not (torch.is_tensor(T) and T.dim() == 2 and T.shape[1] == 12 and T.shape[0] >= 1):
        raise ValueError("T: expected a tensor (nf, 12) (pose_transforms)")
    for t, what in ((face, "face"), (sdf, "sdf")):
        if not (torch.is_tensor(t) and tuple(t.shape) == shape):
            raise ValueError(f"{what}: expected a tensor {shape}, the shape of z")
    if any(t.device != dev for t in (T, face, sdf)):
        raise ValueError(f"T, face and sdf: expected tensors on the volume's device {dev}")
    return _dev_ptr(T, torch.float32, "T"), _dev_ptr(face, torch.int32, "face"), _dev_ptr(sdf, torch.float32, "sdf"), _check_reach(reach)


def march_volume_posed(volume, T, face, sdf, rays_d, cam_pos, z, hit, reach=REACH, row_rays=None, out=None):
    """vanerf_volume_render_posed: baked.march_volume's rays (rays_d (V, R, 3), cam_pos (V, 4), z (V, R, S) fp32, hit (V, R) uint8) with T
    (nf, 12) fp32 of pose_transforms and, per sample, face (V, R, S) int32 and sdf (V, R, S) fp32: renderer.mesh_query_accel's outputs for the
    POSED mesh at renderer.sample_points of the same rays -> color (V, R, 3), depth (V, R), alpha (V, R).  A sample is empty when face is
    outside [0, nf), sdf is not finite or sdf > reach (reach: any float but NaN; inf disables it); the others read the volume at A p + t.
    row_rays, out: as march_volume takes them; every element of out is written.  One launch."""
    nx, ny, nz = _check_volume(volume)
    V, Rn, S, ptrs = _check_rays(volume, rays_d, cam_pos, z, hit)
    dev = volume.voxels.device
    tp, fp, sp, reach = _check_warp(dev, T, face, sdf, (V, Rn, S), reach)
    row_rays = Rn if row_rays is None else int(row_rays)
    handle, beta = _beta_args(volume)
    with torch.cuda.device(dev):
        color, depth, alpha = _march_out(out, V, Rn, dev)
        check(lib.vanerf_volume_render_posed(c_void_p(volume.voxels.data_ptr()), _f3(volume.origin), _f3(volume.spacing), nx, ny, nz, handle, beta, *ptrs,
                                             V * Rn, Rn, row_rays, S, tp, T.shape[0], fp, sp, reach, c_void_p(color.data_ptr()),
                                             c_void_p(depth.data_ptr()), c_void_p(alpha.data_ptr()), _stream()))
    return color, depth, alpha


def _posed_mesh(volume, faces, verts_pose):
    _check_volume(volume)
    if volume.verts is None:
        raise ValueError("volume.verts: the volume carries no source vertices (bake_volume keeps them)")
    _check_mesh(verts_pose, faces, "verts_pose")
    dev = volume.voxels.device
    if verts_pose.device != dev or volume.verts.device != dev:
        raise ValueError(f"verts_pose, faces and volume.verts: expected tensors on the volume's device {dev}")


@dataclasses.dataclass
class PosedSamples:
    """What every march of one pose and one group of cameras shares (posed_samples): T (nf, 12) of pose_transforms; rays_d (V, R, 3), cam_pos
    (V, 4), hit (V, R) uint8 and index (V, R) int64 of renderer.ray_setup_views on the posed bounds, row_rays the rays of a pixel row;
    z (V, R, S) the depths; face (V, R, S) int32 and sdf (V, R, S) fp32 the mesh query of the POSED mesh at the sample points."""
    T: torch.Tensor
    rays_d: torch.Tensor
    cam_pos: torch.Tensor
    z: torch.Tensor
    hit: torch.Tensor
    index: torch.Tensor
    row_rays: int
    face: torch.Tensor
    sdf: torch.Tensor


def posed_samples(volume, faces, verts_pose, cam_tars, samples=128, bounds=None, accel=None, x0=0, y0=0, step=1, nx=None, ny=None):
    """Steps 1-5 of render_posed_volume, once for every march of the same pose and cameras: pose_transforms, the renderer.MeshAccel of the posed
    mesh (unless accel= hands it in), renderer.ray_setup_views on the posed bounds with `samples` uniform depths, renderer.sample_points and
    renderer.mesh_query_accel(want_face=True, want_knn=False) -> PosedSamples.  Nearly all of a posed view's time is the mesh query: a caller
    who wants colour AND geometry frames of one pose hands the result to render_posed_volume and render_posed_surface as prepared= and pays
    for it once."""
    from . import renderer as R
    _posed_mesh(volume, faces, verts_pose)
    dev = volume.voxels.device
    with torch.cuda.device(dev), torch.no_grad():
        T = pose_transforms(volume.verts, verts_pose, faces)
        if accel is None:
            accel = R.MeshAccel(verts_pose, faces)
        elif not isinstance(accel, R.MeshAccel) or accel.verts3.shape != verts_pose.shape or accel.faces.shape != faces.shape or accel.verts3.device != dev:
            raise ValueError("accel: expected the renderer.MeshAccel of (verts_pose, faces) on the volume's device")
        b = frame_bounds(verts_pose) if bounds is None else torch.as_tensor(bounds)
        rays, z = _view_rays(dataclasses.replace(volume, bounds=b), cam_tars, samples, x0, y0, step, nx, ny)
        V, Rn, S = z.shape
        pts = R.sample_points(rays["rays_d"].view(-1, 3), rays["cam_pos"], z.view(-1, S), rays_per_view=Rn)
        no_vis = torch.zeros(verts_pose.shape[0], dtype=torch.float32, device=dev)  # (the query's visibility output is not used here)
        sdf, _, face = R.mesh_query_accel(accel, verts_pose, faces, no_vis, pts, want_face=True, want_knn=False, grid=(rays["row_rays"], V * (Rn // rays["row_rays"]), S))
    return PosedSamples(T=T, rays_d=rays["rays_d"], cam_pos=rays["cam_pos"], z=z, hit=rays["hit"], index=rays["index"], row_rays=rays["row_rays"],
                        face=face.view(V, Rn, S), sdf=sdf.view(V, Rn, S))


def _prepared(prepared, volume, faces, verts_pose, cam_tars, samples, bounds, accel, grid):
    """prepared= of the two renderers: the caller's PosedSamples, or posed_samples of the other arguments."""
    if prepared is None:
        return posed_samples(volume, faces, verts_pose, cam_tars, samples, bounds, accel, *grid)
    if not isinstance(prepared, PosedSamples):
        raise ValueError("prepared: expected the PosedSamples of posed_samples(volume, faces, verts_pose, cam_tars, ...)")
    _posed_mesh(volume, faces, verts_pose)
    return prepared


def render_posed_volume(volume, faces, verts_pose, cam_tars, samples=128, reach=REACH, bounds=None, accel=None, x0=0, y0=0, step=1, nx=None, ny=None,
                        prepared=None):
    """V target cameras of one size through a BakedVolume whose mesh moved from volume.verts to verts_pose (nv, 3) (faces (nf, 3) int32, the
    same in both).  On the volume's device, with no host read beyond renderer.ray_setup_views' own:
      1. pose_transforms(volume.verts, verts_pose, faces);
      2. a renderer.MeshAccel of the posed mesh (built here unless accel= hands in the one of (verts_pose, faces): once per pose serves every group of cameras);
      3. renderer.ray_setup_views on the POSED bounds (default the dataset's rule, mask_at_box.frame_bounds(verts_pose), computed on the
         device; bounds= overrides it) with `samples` uniform depths, exactly as render_volume sets them up;
      4. renderer.sample_points;  5. renderer.mesh_query_accel(want_face=True, want_knn=False) on the posed mesh;  6. march_volume_posed.
    Steps 1-5 are posed_samples; prepared= hands in its result for the same pose and cameras, and then only step 6 runs.
    -> render_volume's dict {"color" (V, R, 3), "depth", "alpha" (V, R), "hit" (V, R) uint8, "index" (V, R) int64} plus "face" (V, R, S) int32 and
    "sdf" (V, R, S) fp32, the mesh query's outputs."""
    reach = _check_reach(reach)
    p = _prepared(prepared, volume, faces, verts_pose, cam_tars, samples, bounds, accel, (x0, y0, step, nx, ny))
    with torch.cuda.device(volume.voxels.device), torch.no_grad():
        color, depth, alpha = march_volume_posed(volume, p.T, p.face, p.sdf, p.rays_d, p.cam_pos, p.z, p.hit, reach, row_rays=p.row_rays)
    return {"color": color, "depth": depth, "alpha": alpha, "hit": p.hit, "index": p.index, "face": p.face, "sdf": p.sdf}


def render_posed_views(volume, faces, verts_pose, cam_tars, samples=128, reach=REACH, bounds=None, accel=None):
    """Whole frames of the posed hand, one dict per camera laid out as baked.render_baked_views lays them out: tex_fg (3, H, W), depth (1, H, W),
    alpha (1, H, W), tex_fg_fine (the same tensor as tex_fg) and vert_xy (1, nv, 2), the POSED vertices in the target image."""
    cam_tars = list(cam_tars)
    o = render_posed_volume(volume, faces, verts_pose, cam_tars, samples, reach, bounds, accel)
    width, height = int(cam_tars[0]["width"]), int(cam_tars[0]["height"])
    posed = dataclasses.replace(volume, verts=verts_pose)
    outs = []
    for v, cam_tar in enumerate(cam_tars):
        ret = {"tex_fg": o["color"][v].view(height, width, 3).permute(2, 0, 1), "depth": o["depth"][v].view(1, height, width),
               "alpha": o["alpha"][v].view(1, height, width)}
        ret["tex_fg_fine"] = ret["tex_fg"]
        _add_vert_xy(ret, posed, cam_tar)
        outs.append(ret)
    return outs


def _frame_faces(tr_batch, dev):
    """The faces of a tr_batch's mesh as renderer.FrameData keeps them: (nf, 3) int32, contiguous, on dev."""
    faces = tr_batch["targets"]["face_world"]
    return (faces if faces.dim() == 2 else faces[0]).to(device=dev, dtype=torch.int32).contiguous()


def _sequence(net, tr_batch, poses, cam_tars, resolution, volume, render):
    """The animation loop of the sequence drivers: the source frame is baked ONCE (unless volume is given) and render(vol, faces, verts_pose,
    [cam]) called per pose.  The cameras are checked at the call, the bake happens at the first frame."""
    poses = list(poses)
    cams = [cam_tars] * len(poses) if isinstance(cam_tars, dict) else list(cam_tars)
    if len(cams) != len(poses):
        raise ValueError(f"cam_tars: expected one camera, or one per pose ({len(poses)}), got {len(cams)}")

    def frames():
        from . import baked
        vol = baked.bake_volume(net, tr_batch, resolution=resolution) if volume is None else volume  # (looked up at the call: one bake per sequence)
        faces = _frame_faces(tr_batch, vol.voxels.device)
        for verts_pose, cam in zip(poses, cams):
            yield render(vol, faces, verts_pose.to(dtype=torch.float32).contiguous(), [cam])[0]

    return frames()


def posed_sequence(net, tr_batch, poses, cam_tars, resolution=128, samples=128, reach=REACH, volume=None):
    """The animation loop: the source frame is baked ONCE (unless volume= hands one in) and every pose of `poses` ((nv, 3) fp32 device tensors
    of the frame's topology) is rendered from it.  cam_tars: one camera dict for all poses, or a list with one camera per pose.  A generator
    of render_posed_views' dicts, one per pose."""
    return _sequence(net, tr_batch, poses, cam_tars, resolution, volume, lambda vol, faces, verts_pose, cams: render_posed_views(vol, faces, verts_pose, cams, samples, reach))


def mano_sequence(net, tr_batch, right, left, pose, betas, trans, cam_tars, flat_hand_mean=False, seal=True, resolution=128, samples=128, reach=REACH,
                  volume=None):
    """posed_sequence driven by a pose track: right, left are mano.ManoModels and pose (P, 2, nj*3), betas (P, 2, nb), trans (P, 2, 3) the
    parameters of P frames, the right hand at index 0.  All P poses are skinned in ONE mano.skin_two_hands call, on the device, when this is
    called; the result is posed_sequence's generator on those vertices (one bake, at the first frame, unless volume= hands one in): the same
    bits as posed_sequence fed with skin_two_hands' vertices.  The skinned frame must have the topology of tr_batch's mesh."""
    from . import mano
    verts, _ = mano.skin_two_hands(right, left, pose, betas, trans, flat_hand_mean=flat_hand_mean, seal=seal)
    return posed_sequence(net, tr_batch, [verts[p] for p in range(verts.shape[0])], cam_tars, resolution, samples, reach, volume)


# ------------------------------------------------------------------------------------------------
# the surface of the posed hand as a camera sees it (csrc/volume_surface.hip)
# ------------------------------------------------------------------------------------------------
def march_surface_posed(volume, T, face, sdf, rays_d, cam_pos, z, hit, iso=0.0, refine=1, reach=REACH, row_rays=None, out=None):
    """vanerf_volume_surface_posed: march_volume_posed's inputs (T (nf, 12), face and sdf (V, R, S), the rays, reach) searched as
    baked.march_surface searches the source pose -> depth (V, R), normal (V, R, 4) = (nx, ny, nz, n . v) in POSED space, color (V, R, 3) fp32
    and found (V, R) uint8.  A sample is inside when it is not empty (march_volume_posed's rule) and the field at A p + t of its face is
    below iso; per ray the first pair (not inside, inside), and the face F of its INSIDE end carries the whole bracket: both ends are
    evaluated under F, `refine` (0 .. 4) 65-way splits and one linear step follow, and the normal is A_F^T times the volume's gradient.
    found: 1 a crossing, 2 the ray starts inside (depth = its first sample), 3 the near end of the bracket is inside under F as well (depth =
    that sample, nothing refined), 0 nothing (a miss included): every output 0.  out: (depth, normal, color, found) to fill instead of new
    tensors: every element is written, whatever they held.  One launch."""
    iso, refine = _check_surface(iso, refine)
    reach = _check_reach(reach)
    nx, ny, nz = _check_volume(volume)
    V, Rn, S, ptrs = _check_rays(volume, rays_d, cam_pos, z, hit)
    dev = volume.voxels.device
    tp, fp, sp, reach = _check_warp(dev, T, face, sdf, (V, Rn, S), reach)
    row_rays = Rn if row_rays is None else int(row_rays)
    with torch.cuda.device(dev):
        depth, normal, color, found = _surface_out(out, V, Rn, dev)
        check(lib.vanerf_volume_surface_posed(c_void_p(volume.voxels.data_ptr()), _f3(volume.origin), _f3(volume.spacing), nx, ny, nz, iso, refine, *ptrs,
                                              V * Rn, Rn, row_rays, S, tp, T.shape[0], fp, sp, reach, c_void_p(depth.data_ptr()),
                                              c_void_p(normal.data_ptr()), c_void_p(color.data_ptr()), c_void_p(found.data_ptr()), _stream()))
    return depth, normal, color, found


def render_posed_surface(volume, faces, verts_pose, cam_tars, samples=128, iso=0.0, refine=1, reach=REACH, bounds=None, accel=None, prepared=None, x0=0,
                         y0=0, step=1, nx=None, ny=None):
    """render_posed_volume's steps 1-5 (posed_samples, or prepared= for the same pose and cameras) followed by one march_surface_posed.
    -> baked.render_volume_surface's dict {"depth" (V, R), "normal" (V, R, 4), "color" (V, R, 3), "found" (V, R) uint8, "hit" (V, R) uint8,
    "index" (V, R) int64} plus "face" (V, R, S) int32 and "sdf" (V, R, S) fp32, the mesh query's outputs."""
    iso, refine = _check_surface(iso, refine)
    reach = _check_reach(reach)
    p = _prepared(prepared, volume, faces, verts_pose, cam_tars, samples, bounds, accel, (x0, y0, step, nx, ny))
    with torch.cuda.device(volume.voxels.device), torch.no_grad():
        depth, normal, color, found = march_surface_posed(volume, p.T, p.face, p.sdf, p.rays_d, p.cam_pos, p.z, p.hit, iso, refine, reach, row_rays=p.row_rays)
    return {"depth": depth, "normal": normal, "color": color, "found": found, "hit": p.hit, "index": p.index, "face": p.face, "sdf": p.sdf}


def render_posed_surface_views(volume, faces, verts_pose, cam_tars, samples=128, iso=0.0, refine=1, reach=REACH, bounds=None, accel=None, prepared=None,
                               mode="shaded", ambient=0.25, background=0.0):
    """Whole geometry frames of the posed hand, one dict per camera laid out as baked.render_baked_surface_views lays them out (its formulas,
    its modes): depth, found, normal (POSED world space), normal_img, shade, tex_fg, tex_fg_fine (the same tensor as tex_fg) and vert_xy
    (1, nv, 2), the POSED vertices in the target image.  A pixel with found == 3 is seen like any other found pixel."""
    _check_mode(mode)
    cam_tars = list(cam_tars)
    o = render_posed_surface(volume, faces, verts_pose, cam_tars, samples, iso, refine, reach, bounds, accel, prepared)
    return _surface_frames(o, dataclasses.replace(volume, verts=verts_pose), cam_tars, mode, ambient, background)


def posed_surface_sequence(net, tr_batch, poses, cam_tars, resolution=128, samples=128, reach=REACH, volume=None, iso=0.0, refine=1, mode="shaded",
                           ambient=0.25, background=0.0):
    """posed_sequence's geometry twin: one bake (unless volume= hands one in), and per pose render_posed_surface_views' dict.  The arguments are
    checked when this is called, the bake happens at the first frame."""
    _check_mode(mode)
    _check_surface(iso, refine)
    _check_reach(reach)
    return _sequence(net, tr_batch, poses, cam_tars, resolution, volume,
                     lambda vol, faces, verts_pose, cams: render_posed_surface_views(vol, faces, verts_pose, cams, samples, iso, refine, reach, mode=mode,
                                                                                     ambient=ambient, background=background))


def mano_surface_sequence(net, tr_batch, right, left, pose, betas, trans, cam_tars, flat_hand_mean=False, seal=True, resolution=128, samples=128,
                          reach=REACH, volume=None, **kw):
    """mano_sequence's geometry twin: all P poses skinned in ONE mano.skin_two_hands call, then posed_surface_sequence on those vertices (kw: its
    iso, refine, mode, ambient, background): the same bits as posed_surface_sequence fed with skin_two_hands' vertices."""
    from . import mano
    _check_mode(kw.get("mode", "shaded"))
    _check_surface(kw.get("iso", 0.0), kw.get("refine", 1))
    verts, _ = mano.skin_two_hands(right, left, pose, betas, trans, flat_hand_mean=flat_hand_mean, seal=seal)
    return posed_surface_sequence(net, tr_batch, [verts[p] for p in range(verts.shape[0])], cam_tars, resolution, samples, reach, volume, **kw)


__all__ = ["REACH", "PosedSamples", "pose_transforms", "march_volume_posed", "posed_samples", "render_posed_volume", "render_posed_views", "posed_sequence",
           "mano_sequence", "march_surface_posed", "render_posed_surface", "render_posed_surface_views", "posed_surface_sequence", "mano_surface_sequence"]
