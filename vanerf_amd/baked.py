"""The learned field baked into a voxel grid, and orbit views rendered from it (vanerf_amd/csrc/volume_render.hip).

Every camera of an orbit around one source frame asks the same questions of the networks: at one source view the colour of a sample does not
depend on the viewing direction, the density is a function of f = alpha + mesh_sdf alone, and `valid` depends on the source camera only.
bake_volume answers them once, on a regular grid (surface.field_on_grid with colours, packed to (f, r, g, b) per voxel); render_volume then
marches the pass's own rays through the grid: trilinear gathers and the pass's composite, no network and no mesh query per view.

This is an APPROXIMATION of the pass, not a replacement: a grid resolution and uniform samples stand in for the networks evaluated at 64 + 64
importance samples.  It is the preview / interactive path, and a cheap source of depth and alpha maps of the learned hand from any camera.
baked_views_fn plugs it into novel_views.render_novel_views / render_video through their render_views_fn hook.

The same volume also shows its geometry (vanerf_amd/csrc/volume_surface.hip): march_surface / render_volume_surface find,
per ray, where the trilinear field first crosses f = iso and return the depth, the normal and the colour there; render_baked_surface_views
turns them into depth, normal-map, clay and shaded frames, and surface_views_fn is baked_views_fn's twin for geometry orbits.
"""
import dataclasses
from ctypes import c_void_p

import numpy as np
import torch

from ._ffi import check, lib
from .surface import SLAB_POINTS, _default_bounds, _dev_ptr, _f3, _resolve, _stream, field_on_grid, grid_spec

CLIP_PAD = 0.01  # what the ray clip widens the bounds by on every side (ray_bbox_intersection's boffset, src/model.py:1496)


@dataclasses.dataclass
class BakedVolume:
    """voxels (nz, ny, nx, 4) fp32 on the device = (f, r, g, b) at the points of the grid origin + index * spacing (tuples of Python floats that
    are exact fp32 values; dims = (nx, ny, nz)); bounds (2, 3), on the host or on the voxels' device: the FRAME's bounds, what the ray clip gets
    (the grid covers them widened by CLIP_PAD); beta: sigmoid_beta as a float, or the renderer.PackedWeights whose device copy the kernel
    reads; verts (nv, 3): the frame's MANO vertices (for vert_xy) or None; znear, zfar: the source camera's, for target cameras that carry none."""
    voxels: torch.Tensor
    origin: tuple
    spacing: tuple
    dims: tuple
    bounds: torch.Tensor
    beta: object
    verts: object = None
    znear: object = None
    zfar: object = None


def pack_volume(f, rgb):
    """vanerf_volume_pack: f (...,) and rgb (..., 3) fp32 on the device, as field_on_grid returns them -> voxels (..., 4) = (f, r, g, b).
    A non-finite f becomes +1e30 (outside, and finite), a non-finite colour channel 0; everything else is copied bit for bit."""
    if not (torch.is_tensor(f) and torch.is_tensor(rgb) and tuple(rgb.shape) == (*f.shape, 3)):
        raise ValueError("f and rgb: expected tensors (...,) and (..., 3)")
    fp, rp = _dev_ptr(f, torch.float32, "f"), _dev_ptr(rgb, torch.float32, "rgb")
    if rgb.device != f.device:
        raise ValueError("rgb: expected a tensor on the device of f")
    with torch.cuda.device(f.device):
        voxels = torch.empty(*f.shape, 4, dtype=torch.float32, device=f.device)
        check(lib.vanerf_volume_pack(fp, rp, f.numel(), c_void_p(voxels.data_ptr()), _stream()))
    return voxels


def bake_volume(net, frame, resolution=128, voxel_size=None, bounds=None, slab_points=SLAB_POINTS):
    """The learned field of one frame on a regular grid of cubic cells -> BakedVolume.

    net, frame: a VANeRF module and a tr_batch of device tensors, or a renderer.PackedWeights handle and a renderer.FrameData, resolved as
    surface.extract_surface resolves them; bounds: (2, 3)-shaped, default the frame's own.  resolution: grid points along the longest axis
    (unless voxel_size gives the cells' edge).  The grid covers the bounds WIDENED by the ray clip's 0.01 on every side, so that the samples of
    a clipped ray lie inside it (the few a rounding leaves outside read the border voxel); BakedVolume.bounds stays the frame's own, which is
    what the ray clip takes.  surface.field_on_grid(..., want_rgb=True) evaluates (f, rgb) with the pass's own per-sample calls in the
    handle's precision, slab by slab; vanerf_volume_pack interleaves them.  No host read of its own: the one of the bounds, when they are a
    device tensor, is grid_spec's (renderer.host_copy, remembered)."""
    from . import renderer as R
    weights, fd, frame_b = _resolve(net, frame)
    b = _default_bounds(fd, frame_b, bounds)
    bt = torch.as_tensor(b)
    if bt.numel() != 6:
        raise ValueError(f"bounds: expected (2, 3), got {tuple(bt.shape)}")
    bh = np.asarray((R.host_copy(bt) if bt.is_cuda else bt).reshape(2, 3).tolist(), dtype=np.float64)
    wide = bh + np.array([[-CLIP_PAD], [CLIP_PAD]])
    if voxel_size is None:
        resolution = int(resolution)
        if resolution < 2:
            raise ValueError(f"resolution: expected at least 2 points, got {resolution}")
        voxel_size = float((wide[1] - wide[0]).max()) / (resolution - 1)
    wide_t = torch.from_numpy(wide)
    origin, spacing, dims = grid_spec(wide_t, voxel_size=voxel_size)
    f, rgb = field_on_grid(weights, fd, wide_t, voxel_size=voxel_size, want_rgb=True, slab_points=slab_points)
    cam = frame.get("cam") if isinstance(frame, dict) else None
    return BakedVolume(voxels=pack_volume(f, rgb), origin=origin, spacing=spacing, dims=dims, bounds=bt.detach().reshape(2, 3), beta=weights, verts=fd.verts3,
                       znear=None if cam is None else cam.get("znear"), zfar=None if cam is None else cam.get("zfar"))


def _check_volume(volume):
    if not isinstance(volume, BakedVolume):
        raise TypeError("volume: expected a BakedVolume (bake_volume)")
    nx, ny, nz = (int(d) for d in volume.dims)
    v = volume.voxels
    if not (torch.is_tensor(v) and tuple(v.shape) == (nz, ny, nx, 4)):
        raise ValueError(f"volume.voxels: expected a tensor ({nz}, {ny}, {nx}, 4)")
    _dev_ptr(v, torch.float32, "volume.voxels")
    if not (torch.is_tensor(volume.bounds) and volume.bounds.numel() == 6) or (volume.bounds.is_cuda and volume.bounds.device != v.device):
        raise ValueError(f"volume.bounds: expected a (2, 3) tensor on the host or on the voxels' device {v.device}")
    return nx, ny, nz


def _check_rays(volume, rays_d, cam_pos, z, hit):
    """The rays of march_volume / march_surface, as renderer.ray_setup_views lays them out, on the volume's device -> V, R, S and their pointers."""
    if not (torch.is_tensor(z) and z.dim() == 3):
        raise ValueError("z: expected a tensor (V, R, S)")
    V, Rn, S = (int(d) for d in z.shape)
    if S < 1:
        raise ValueError(f"samples: expected at least 1 per ray, got {S}")
    for t, shape, what in ((rays_d, (V, Rn, 3), "rays_d"), (cam_pos, (V, 4), "cam_pos"), (hit, (V, Rn), "hit")):
        if not (torch.is_tensor(t) and tuple(t.shape) == shape):
            raise ValueError(f"{what}: expected a tensor {shape}")
    dev = volume.voxels.device
    if any(t.device != dev for t in (rays_d, cam_pos, z, hit)):
        raise ValueError(f"rays_d, cam_pos, z and hit: expected tensors on the volume's device {dev}")
    ptrs = [_dev_ptr(rays_d, torch.float32, "rays_d"), _dev_ptr(cam_pos, torch.float32, "cam_pos"), _dev_ptr(z, torch.float32, "z"),
            _dev_ptr(hit, torch.uint8, "hit")]
    return V, Rn, S, ptrs


def _check_out(out, shapes, dev):
    """out: the tensors to fill, against (shape, dtype, name) each: contiguous, on dev."""
    if len(out) != len(shapes):
        raise ValueError(f"out: expected {len(shapes)} tensors ({', '.join(what for _, _, what in shapes)})")
    for t, (shape, dtype, what) in zip(out, shapes):
        if not (torch.is_tensor(t) and tuple(t.shape) == shape and t.device == dev):
            raise ValueError(f"out {what}: expected a tensor {shape} on {dev}")
        _dev_ptr(t, dtype, f"out {what}")
    return out


def _beta_args(volume):
    """volume.beta as the marches pass it on: (weight handle or None, the number or 0.0); a handle must live on the voxels' device."""
    from . import renderer as R
    dev = volume.voxels.device
    if not isinstance(volume.beta, R.PackedWeights):
        return None, float(volume.beta)
    if volume.beta.device_index is not None and volume.beta.device_index != dev.index:
        raise ValueError(f"volume.beta: the weight handle lives on device {volume.beta.device_index}, the voxels on {dev}")
    return volume.beta.handle, 0.0


def _march_out(out, V, Rn, dev):
    """(color (V, Rn, 3), depth (V, Rn), alpha (V, Rn)) of a march on dev: the caller's `out`, checked, or new tensors."""
    if out is None:
        out = (torch.empty(V, Rn, 3, dtype=torch.float32, device=dev), *(torch.empty(V, Rn, dtype=torch.float32, device=dev) for _ in range(2)))
    return _check_out(out, (((V, Rn, 3), torch.float32, "color"), ((V, Rn), torch.float32, "depth"), ((V, Rn), torch.float32, "alpha")), dev)


def march_volume(volume, rays_d, cam_pos, z, hit, row_rays=None, out=None):
    """vanerf_volume_render on rays laid out as renderer.ray_setup_views lays them out: rays_d (V, R, 3), cam_pos (V, 4), z (V, R, S) fp32 and
    hit (V, R) uint8 on the volume's device -> color (V, R, 3), depth (V, R), alpha (V, R).  row_rays: the rays of one pixel row (default R:
    it only decides which rays share a block).  out: (color, depth, alpha), contiguous fp32 device tensors to fill instead of new ones: every
    element is written, whatever they held.  One launch."""
    nx, ny, nz = _check_volume(volume)
    V, Rn, S, ptrs = _check_rays(volume, rays_d, cam_pos, z, hit)
    dev = volume.voxels.device
    row_rays = Rn if row_rays is None else int(row_rays)
    handle, beta = _beta_args(volume)
    with torch.cuda.device(dev):
        color, depth, alpha = _march_out(out, V, Rn, dev)
        check(lib.vanerf_volume_render(c_void_p(volume.voxels.data_ptr()), _f3(volume.origin), _f3(volume.spacing), nx, ny, nz, handle, beta, *ptrs,
                                       V * Rn, Rn, row_rays, S, c_void_p(color.data_ptr()), c_void_p(depth.data_ptr()), c_void_p(alpha.data_ptr()), _stream()))
    return color, depth, alpha


def _cameras(volume, cam_tars):
    cam_tars = list(cam_tars)
    if not cam_tars:
        raise ValueError("at least one target camera")
    sizes = {(int(c["width"]), int(c["height"])) for c in cam_tars}
    if len(sizes) != 1:
        raise ValueError(f"the views of one group share one width / height, got {sorted(sizes)}")
    dev = volume.voxels.device
    for c in cam_tars:
        for k in ("K", "RT"):
            if torch.is_tensor(c[k]) and c[k].is_cuda and c[k].device != dev:
                raise ValueError(f"cam_tar['{k}']: on {c[k].device}, the volume on {dev}")
    missing = [k for k in ("znear", "zfar") if any(k not in c for c in cam_tars) and getattr(volume, k) is None]
    if missing:
        raise ValueError(f"cam_tar: no {' / '.join(missing)}, and the volume carries none")
    return [dict(c, znear=c.get("znear", volume.znear), zfar=c.get("zfar", volume.zfar)) for c in cam_tars], sizes.pop()


def _view_rays(volume, cam_tars, samples, x0, y0, step, nx, ny):
    """renderer.ray_setup_views for render_volume / render_volume_surface: the rays of V cameras of one size on the pixel grid (x0, y0, step,
    nx, ny; default the whole frame) with `samples` uniform depths each -> (its outputs, with "row_rays" = nx added, and z (V, R, samples))."""
    from . import renderer as R
    samples = int(samples)
    if samples < 1:
        raise ValueError(f"samples: expected at least 1 per ray, got {samples}")
    _check_volume(volume)
    cams, (width, height) = _cameras(volume, cam_tars)
    step = int(step)
    if step < 1:
        raise ValueError(f"step: expected at least 1, got {step}")
    nx = (width - int(x0) + step - 1) // step if nx is None else int(nx)
    ny = (height - int(y0) + step - 1) // step if ny is None else int(ny)
    if nx < 1 or ny < 1:
        raise ValueError(f"an empty pixel grid ({nx} x {ny})")
    dev = volume.voxels.device
    with torch.cuda.device(dev), torch.no_grad():
        rays = dict(R.ray_setup_views(cams, volume.bounds, x0, y0, step, nx, ny, max(samples, 2), device=dev), row_rays=nx)  # (the ray setup takes S >= 2)
        z = rays["z"] if samples >= 2 else rays["z"][..., :1].contiguous()  # linspace(0, 1, 1) is [0]: the near end, the first of any S
    return rays, z


def render_volume(volume, cam_tars, samples=128, x0=0, y0=0, step=1, nx=None, ny=None):
    """V target cameras of one size through a BakedVolume: renderer.ray_setup_views(cam_tars, volume.bounds, ..., S=samples) -- so rays, clip,
    hit and the uniform depths are the pass's own bits -- followed by one vanerf_volume_render.  Two launches per group of views.
    x0, y0, step, nx, ny: the pixel grid (default the whole frame).  samples = 1 puts the one sample at the near end of the clipped ray.
    -> {"color" (V, R, 3), "depth" (V, R), "alpha" (V, R), "hit" (V, R) uint8, "index" (V, R) int64}, R = nx ny."""
    rays, z = _view_rays(volume, cam_tars, samples, x0, y0, step, nx, ny)
    with torch.cuda.device(volume.voxels.device), torch.no_grad():
        color, depth, alpha = march_volume(volume, rays["rays_d"], rays["cam_pos"], z, rays["hit"], row_rays=rays["row_rays"])
    return {"color": color, "depth": depth, "alpha": alpha, "hit": rays["hit"], "index": rays["index"]}


def _add_vert_xy(ret, volume, cam_tar):
    """ret["vert_xy"] (1, nv, 2): the frame's vertices in the target image, when the volume carries them."""
    if volume.verts is not None and "KRT" in cam_tar:
        vimg = volume.verts[None] @ cam_tar["KRT"][:, :3, :3].transpose(1, 2) + cam_tar["KRT"][:, :3, 3][:, None]
        ret["vert_xy"] = vimg[..., :2] / (vimg[..., 2:3] + 1e-8)
        if "transf" in cam_tar:  # src/model.py:1093-1095
            ret["vert_xy"] = ret["vert_xy"] @ cam_tar["transf"][:, :2, :2].transpose(1, 2) + cam_tar["transf"][:, :, 2][:, None]


def render_baked_views(volume, cam_tars, samples=128):
    """Whole frames from a BakedVolume, one dict per camera laid out as VANeRF.render_pifu_nerf_views lays its views out: tex_fg (3, H, W),
    depth (1, H, W), alpha (1, H, W), tex_fg_fine (the same tensor as tex_fg: what novel_views.arrange_nerf_images reads; there is no second
    march here) and, when the volume carries the frame's vertices, vert_xy (1, nv, 2)."""
    cam_tars = list(cam_tars)
    o = render_volume(volume, cam_tars, samples)
    width, height = int(cam_tars[0]["width"]), int(cam_tars[0]["height"])
    outs = []
    for v, cam_tar in enumerate(cam_tars):
        ret = {"tex_fg": o["color"][v].view(height, width, 3).permute(2, 0, 1), "depth": o["depth"][v].view(1, height, width),
               "alpha": o["alpha"][v].view(1, height, width)}
        ret["tex_fg_fine"] = ret["tex_fg"]
        _add_vert_xy(ret, volume, cam_tar)
        outs.append(ret)
    return outs


def baked_views_fn(resolution=128, samples=128):
    """A render_views_fn(net, tr_batch, cam_tars, level) for novel_views.render_novel_views / render_video: the orbit's source frame is baked
    once (the same tr_batch OBJECT on every call of an orbit; a different one is baked anew) and every group of cameras is rendered from the
    volume.  The volume is not rebuilt when the weights change under the same batch object: take a new function (or batch) after an update.
    The frames are the approximation this module describes, not the pass's."""
    state = {"batch": None, "volume": None}

    def render_views(net, tr_batch, cam_tars, level):
        if state["batch"] is not tr_batch:
            state["volume"] = bake_volume(net, tr_batch, resolution=resolution)
            state["batch"] = tr_batch
        return render_baked_views(state["volume"], cam_tars, samples)

    return render_views


# ------------------------------------------------------------------------------------------------
# the surface of the volume as a camera sees it (csrc/volume_surface.hip)
# ------------------------------------------------------------------------------------------------
SURFACE_MODES = ("shaded", "clay", "normal", "depth")
MAX_REFINE = 4


def _check_surface(iso, refine):
    iso, refine = float(iso), int(refine)
    if not np.isfinite(iso):
        raise ValueError(f"iso: expected a finite level, got {iso}")
    if not 0 <= refine <= MAX_REFINE:
        raise ValueError(f"refine: expected 0 .. {MAX_REFINE} rounds, got {refine}")
    return iso, refine


def _surface_out(out, V, Rn, dev):
    """(depth (V, Rn), normal (V, Rn, 4), color (V, Rn, 3), found (V, Rn) uint8) of a surface march on dev: the caller's `out`, checked, or new tensors."""
    if out is None:
        out = (torch.empty(V, Rn, dtype=torch.float32, device=dev), torch.empty(V, Rn, 4, dtype=torch.float32, device=dev),
               torch.empty(V, Rn, 3, dtype=torch.float32, device=dev), torch.empty(V, Rn, dtype=torch.uint8, device=dev))
    return _check_out(out, (((V, Rn), torch.float32, "depth"), ((V, Rn, 4), torch.float32, "normal"), ((V, Rn, 3), torch.float32, "color"),
                            ((V, Rn), torch.uint8, "found")), dev)


def march_surface(volume, rays_d, cam_pos, z, hit, iso=0.0, refine=1, row_rays=None, out=None):
    """vanerf_volume_surface on the rays march_volume takes (rays_d (V, R, 3), cam_pos (V, 4), z (V, R, S), hit (V, R) uint8, on the volume's
    device) -> depth (V, R), normal (V, R, 4) = (nx, ny, nz, n . v), color (V, R, 3) fp32 and found (V, R) uint8.  Per ray the first sample
    pair (outside, inside) of f < iso, refined by `refine` (0 .. 4) 65-way splits and one linear step; depth in the units of z, the normal
    the normalised gradient of the trilinear field (outward), the colour interpolated there.  found: 1 a crossing, 2 the ray starts inside
    (depth = its first sample), 0 nothing (a miss included): every output 0.  out: (depth, normal, color, found) to fill instead of new
    tensors: every element is written, whatever they held.  One launch."""
    iso, refine = _check_surface(iso, refine)
    nx, ny, nz = _check_volume(volume)
    V, Rn, S, ptrs = _check_rays(volume, rays_d, cam_pos, z, hit)
    dev = volume.voxels.device
    row_rays = Rn if row_rays is None else int(row_rays)
    with torch.cuda.device(dev):
        depth, normal, color, found = _surface_out(out, V, Rn, dev)
        check(lib.vanerf_volume_surface(c_void_p(volume.voxels.data_ptr()), _f3(volume.origin), _f3(volume.spacing), nx, ny, nz, iso, refine, *ptrs,
                                        V * Rn, Rn, row_rays, S, c_void_p(depth.data_ptr()), c_void_p(normal.data_ptr()), c_void_p(color.data_ptr()),
                                        c_void_p(found.data_ptr()), _stream()))
    return depth, normal, color, found


def render_volume_surface(volume, cam_tars, samples=128, iso=0.0, refine=1, x0=0, y0=0, step=1, nx=None, ny=None):
    """render_volume's rays (renderer.ray_setup_views on volume.bounds, `samples` uniform depths; samples = 1: the near end of the clipped ray)
    followed by one vanerf_volume_surface.  Two launches per group of views.
    -> {"depth" (V, R), "normal" (V, R, 4), "color" (V, R, 3), "found" (V, R) uint8, "hit" (V, R) uint8, "index" (V, R) int64}, R = nx ny."""
    iso, refine = _check_surface(iso, refine)
    rays, z = _view_rays(volume, cam_tars, samples, x0, y0, step, nx, ny)
    with torch.cuda.device(volume.voxels.device), torch.no_grad():
        depth, normal, color, found = march_surface(volume, rays["rays_d"], rays["cam_pos"], z, rays["hit"], iso, refine, row_rays=rays["row_rays"])
    return {"depth": depth, "normal": normal, "color": color, "found": found, "hit": rays["hit"], "index": rays["index"]}


def _rotation(rt, dev):
    """RT[:3, :3] of a camera's (1, 4, 4) / (4, 4) / (3, 4) world-to-camera matrix, on dev."""
    rt = torch.as_tensor(rt).to(device=dev, dtype=torch.float32)
    return rt.reshape(-1, *rt.shape[-2:])[0, :3, :3]


def _per_view(values, dev):
    """znear / zfar of the cameras of a group, numbers or one-element tensors -> (V, 1, 1, 1) on dev; no host read."""
    if any(torch.is_tensor(x) for x in values):
        return torch.stack([torch.as_tensor(x).to(device=dev, dtype=torch.float32).reshape(()) for x in values]).view(-1, 1, 1, 1)
    return torch.tensor([float(x) for x in values], dtype=torch.float32, device=dev).view(-1, 1, 1, 1)


def render_baked_surface_views(volume, cam_tars, samples=128, iso=0.0, refine=1, mode="shaded", ambient=0.25, background=0.0):
    """Whole geometry frames from a BakedVolume, one dict per camera: depth (1, H, W), found (1, H, W) uint8 and normal (3, H, W) in world
    space are the kernel's outputs (0 where nothing is found);
        normal_img (3, H, W) = 0.5 + 0.5 (n_cam.x, -n_cam.y, -n_cam.z), n_cam = RT[:3, :3] n (the usual normal-map colours: towards the camera is blue),
        shade (1, H, W) = ambient + (1 - ambient) n . v (a headlight),
        tex_fg (3, H, W) by `mode`: "shaded" colour x shade, "clay" 0.8 shade, "normal" normal_img, "depth" (zfar - depth) / (zfar - znear);
    these three hold `background` where found == 0.  tex_fg_fine is the same tensor as tex_fg (what novel_views.arrange_nerf_images reads),
    vert_xy as in render_baked_views.  The images are elementwise torch ops on H x W; no host read."""
    _check_mode(mode)
    cam_tars = list(cam_tars)
    return _surface_frames(render_volume_surface(volume, cam_tars, samples, iso, refine), volume, cam_tars, mode, ambient, background)


def _check_mode(mode):
    if mode not in SURFACE_MODES:
        raise ValueError(f"mode: expected one of {SURFACE_MODES}, got {mode!r}")


def _surface_frames(o, volume, cam_tars, mode, ambient, background):
    """The image half of render_baked_surface_views, which documents the formulas: o, the maps of a surface march over whole frames of the
    cameras cam_tars (render_volume_surface's dict, or posed.render_posed_surface's) -> one dict per camera.  A pixel is seen iff
    found != 0; vert_xy comes from volume.verts."""
    cams, (width, height) = _cameras(volume, cam_tars)
    dev = volume.voxels.device
    ambient, background = float(ambient), float(background)
    V = len(cams)
    with torch.cuda.device(dev), torch.no_grad():  # (the whole group at once: a dozen launches per group, not per view)
        seen = (o["found"] != 0).view(V, 1, height, width)
        depth = o["depth"].view(V, 1, height, width)
        n4 = o["normal"].view(V, height, width, 4).permute(0, 3, 1, 2)
        rot = torch.stack([_rotation(cam["RT"], dev) for cam in cams])
        n_cam = (rot[:, :, :, None, None] * n4[:, None, :3]).sum(2)
        normal_img = torch.where(seen, 0.5 + torch.tensor([0.5, -0.5, -0.5], device=dev).view(1, 3, 1, 1) * n_cam, background)
        lit = ambient + (1.0 - ambient) * n4[:, 3:]
        if mode == "shaded":
            tex = o["color"].view(V, height, width, 3).permute(0, 3, 1, 2) * lit
        elif mode == "clay":
            tex = (0.8 * lit).expand(V, 3, height, width)
        elif mode == "normal":
            tex = normal_img
        else:
            znear, zfar = (_per_view([cam[k] for cam in cams], dev) for k in ("znear", "zfar"))
            tex = ((zfar - depth) / (zfar - znear)).expand(V, 3, height, width)
        shade, tex = torch.where(seen, lit, background), torch.where(seen, tex, background)
    outs = []
    for v, cam_tar in enumerate(cam_tars):
        ret = {"depth": depth[v], "found": o["found"][v].view(1, height, width), "normal": n4[v, :3], "normal_img": normal_img[v], "shade": shade[v],
               "tex_fg": tex[v]}
        ret["tex_fg_fine"] = ret["tex_fg"]
        _add_vert_xy(ret, volume, cam_tar)
        outs.append(ret)
    return outs


def surface_views_fn(resolution=128, samples=128, mode="shaded", **kw):
    """baked_views_fn's twin for geometry orbits: a render_views_fn(net, tr_batch, cam_tars, level) for novel_views.render_novel_views /
    render_video that bakes the source frame once per tr_batch OBJECT and renders every group of cameras with render_baked_surface_views
    (kw: its iso, refine, ambient, background)."""
    if mode not in SURFACE_MODES:
        raise ValueError(f"mode: expected one of {SURFACE_MODES}, got {mode!r}")
    _check_surface(kw.get("iso", 0.0), kw.get("refine", 1))
    state = {"batch": None, "volume": None}

    def render_views(net, tr_batch, cam_tars, level):
        if state["batch"] is not tr_batch:
            state["volume"] = bake_volume(net, tr_batch, resolution=resolution)
            state["batch"] = tr_batch
        return render_baked_surface_views(state["volume"], cam_tars, samples, mode=mode, **kw)

    return render_views


__all__ = ["CLIP_PAD", "BakedVolume", "pack_volume", "bake_volume", "march_volume", "render_volume", "render_baked_views", "baked_views_fn",
           "SURFACE_MODES", "march_surface", "render_volume_surface", "render_baked_surface_views", "surface_views_fn"]
