"""The learned hand surface as a triangle mesh, on the GPU (vanerf_amd/csrc/surface.hip).

The network predicts a residual on the MANO signed distance: eval_func returns alpha = valid relu(rad) and the composite turns
f = alpha + mesh_sdf into a density (src/model.py:1158, 1480-1481), so the hand is the zero level set of f.  field_on_grid evaluates f on a
regular grid with the calls the render pass makes per sample (mesh query, validity partition, per-sample networks); extract_surface runs
marching tetrahedra over it (vanerf_surface_count / vanerf_surface_emit) and returns an indexed, welded mesh on the device.  The only wait
for the GPU is the read of the two counts between those calls (and of `bounds` when it is a device tensor: it goes to the kernels by value).

register_surface (vanerf_amd/csrc/surface_lines.hip) answers "where did each MANO vertex move to": it samples f on the
line through every vertex along its normal (field_at_points), brackets the crossing of f = iso nearest to the vertex (line_bracket), refines
it (line_refine) and returns the input mesh with its vertices moved there: the same faces for every frame, no host read of its own.
"""
import math
from ctypes import c_float, c_void_p

import numpy as np
import torch

from ._ffi import check, lib

# Points per slab of field_on_grid.  A slab holds its points, the mesh query's three outputs, the partition with its scratch and the
# per-sample output: about 50 bytes per point, 100 MiB at this size -- a 256^3 grid with colours (64 + 192 MiB) stays well under 1 GiB.
SLAB_POINTS = 1 << 21


def _f3(values):
    return (c_float * 3)(*[float(v) for v in values])


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_ptr(t, dtype, what):
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"{what}: expected a contiguous {dtype} device tensor (no CPU fallback)")
    return c_void_p(t.data_ptr())


def grid_spec(bounds, dims=None, voxel_size=None):
    """The regular grid over `bounds` ((2, 3)-shaped: min xyz, max xyz) as (origin, spacing, (nx, ny, nz)), origin and spacing tuples of
    Python floats that are exact fp32 values.  dims = (nx, ny, nz): the grid spans the bounds, spacing = extent / (n - 1) per axis.
    voxel_size: cubic cells of that edge from the lower corner, as many as it takes to cover the bounds.  Exactly one of the two."""
    if (dims is None) == (voxel_size is None):
        raise ValueError("give exactly one of dims and voxel_size")
    b = torch.as_tensor(bounds)
    if b.numel() != 6:
        raise ValueError(f"bounds: expected (2, 3), got {tuple(b.shape)}")
    if b.is_cuda:
        from . import renderer as R
        b = R.host_copy(b)
    b = np.asarray(b.reshape(2, 3).tolist(), dtype=np.float64)
    lo, hi = b[0], b[1]
    if not (np.isfinite(b).all() and (hi > lo).all()):
        raise ValueError(f"bounds: need finite min < max on every axis, got {b.tolist()}")
    if dims is not None:
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 2:
            raise ValueError(f"dims: expected (nx, ny, nz) with at least 2 points per axis, got {dims}")
        spacing = (hi - lo) / (np.asarray(dims, dtype=np.float64) - 1.0)
    else:
        voxel_size = float(voxel_size)
        if not (math.isfinite(voxel_size) and voxel_size > 0.0):
            raise ValueError(f"voxel_size: expected a positive number, got {voxel_size}")
        dims = tuple(max(2, int(math.ceil(e / voxel_size - 1e-9)) + 1) for e in (hi - lo))
        spacing = np.full(3, voxel_size)
    if 7 * dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"a grid of {dims} points is too large: 7 nx ny nz must stay below 2^31")
    origin = tuple(float(v) for v in lo.astype(np.float32))
    spacing = tuple(float(v) for v in spacing.astype(np.float32))
    if min(spacing) <= 0.0:
        raise ValueError(f"the grid spacing {spacing} underflows fp32")
    return origin, spacing, dims


def grid_points(origin, spacing, dims, z0=0, nz_out=None, device=None):
    """vanerf_grid_points: the points of layers z0 ... z0 + nz_out - 1 of the grid as (nz_out ny nx, 3), x fastest."""
    nx, ny, nz = (int(d) for d in dims)
    nz_out = nz - z0 if nz_out is None else int(nz_out)
    if not 0 <= z0 <= z0 + nz_out <= nz:
        raise ValueError(f"layers [{z0}, {z0 + nz_out}) are outside the grid's [0, {nz})")
    pts = torch.empty(max(nz_out, 0) * ny * nx, 3, dtype=torch.float32, device=device or torch.device("cuda", torch.cuda.current_device()))
    if not pts.is_cuda:
        raise ValueError("grid_points runs on the GPU (no CPU fallback)")
    with torch.cuda.device(pts.device):
        check(lib.vanerf_grid_points(_f3(origin), _f3(spacing), nx, ny, nz, int(z0), nz_out, c_void_p(pts.data_ptr()), _stream()))
    return pts


def _resolve(net, frame):
    """(weights, FrameData, the frame's bounds or None) from (VANeRF module, tr_batch) or (PackedWeights, FrameData)."""
    from . import renderer as R
    if isinstance(net, R.PackedWeights):
        if not isinstance(frame, R.FrameData):
            raise TypeError("with a PackedWeights handle the frame is a renderer.FrameData")
        return net, frame, None
    if not (hasattr(net, "packed_weights") and hasattr(net, "frame_data")):
        raise TypeError("net: expected a VANeRF module or a renderer.PackedWeights handle")
    if not isinstance(frame, dict) or "im" not in frame or "targets" not in frame:
        raise TypeError("with a VANeRF module the frame is a tr_batch dict (im, cam, targets, sp_data, src_foreground_mask, dr_data)")
    if not frame["im"].is_cuda:
        raise ValueError("the surface is extracted on the GPU and takes a batch of device tensors (no CPU fallback)")
    with torch.no_grad():
        cam_in = net.fold_transf(frame["cam"])
        feat_geo, feat_tex = net.encoded(frame["im"])
        fd = net.frame_data(frame["im"], cam_in, frame["targets"], feat_geo, feat_tex, frame["sp_data"], frame["src_foreground_mask"])
        weights = net.packed_weights()
    return weights, fd, (frame.get("dr_data") or {}).get("bounds")


def _default_bounds(fd, bounds, given):
    if given is not None:
        return given
    if bounds is not None:
        return bounds
    from .mask_at_box import frame_bounds
    return frame_bounds(fd.verts3)  # what the dataset hands the ray clip and mask_at_box: the vertices' box, z widened by 0.05


def field_at_points(net, frame, pts, want_rgb=False, slab_points=SLAB_POINTS, out=None):
    """f = alpha + mesh_sdf at arbitrary points: pts (n, 3) fp32 on the device -> f (n,) fp32[, rgb (n, 3)].  net, frame: as field_on_grid takes
    them.  Per chunk of at most slab_points points: vanerf_mesh_query_accel with the 1-NN vertex -> vanerf_query_order -> vanerf_query_samples
    (raw = 0, no noise) -> vanerf_field_values.  Every step is a per-point function, so neither the chunk size nor a point's neighbours change
    a bit.  out: (f, rgb or None), contiguous device tensors to fill instead of new ones."""
    from . import renderer as R
    slab_points = int(slab_points)
    if slab_points < 1:
        raise ValueError(f"slab_points: expected a positive number of points, got {slab_points}")
    weights, fd, _ = _resolve(net, frame)
    if not (torch.is_tensor(pts) and pts.dim() == 2 and pts.shape[1] == 3):
        raise ValueError("pts: expected a tensor (n, 3)")
    _dev_ptr(pts, torch.float32, "pts")
    dev, n = fd.verts3.device, pts.shape[0]
    if pts.device != dev:
        raise ValueError(f"pts: expected a tensor on the frame's device {dev}")
    with torch.cuda.device(dev), torch.no_grad():
        f, rgb = out if out is not None else (torch.empty(n, dtype=torch.float32, device=dev),
                                              torch.empty(n, 3, dtype=torch.float32, device=dev) if want_rgb else None)
        if tuple(f.shape) != (n,) or (rgb is not None and tuple(rgb.shape) != (n, 3)):
            raise ValueError(f"out: expected f ({n},) and rgb ({n}, 3) or None")
        fp, rp = _dev_ptr(f, torch.float32, "out f"), _dev_ptr(rgb, torch.float32, "out rgb")
        for a in range(0, n, slab_points):
            p = pts[a:a + slab_points]
            sdf, vis, knn = R.mesh_query_accel(fd.accel, fd.verts3, fd.faces, fd.vert_vis, p)
            o = R.query_samples(weights, fd, p, sdf, vis, knn, order=R.query_order(fd, p))
            check(lib.vanerf_field_values(c_void_p(o.data_ptr()), c_void_p(sdf.data_ptr()), p.shape[0], c_void_p(fp.value + 4 * a),
                                          None if rp is None else c_void_p(rp.value + 12 * a), _stream()))
    return (f, rgb) if want_rgb else f


def field_on_grid(net, frame, bounds=None, dims=None, voxel_size=None, want_rgb=False, slab_points=SLAB_POINTS):
    """f = alpha + mesh_sdf on a regular grid -> (nz, ny, nx) fp32 on the device[, rgb (nz, ny, nx, 3)].

    net, frame: a VANeRF module and a tr_batch of device tensors, or a renderer.PackedWeights handle and a renderer.FrameData: the handle and
    frame data of the render pass, in the handle's precision.  bounds: (2, 3)-shaped, default the frame's own (dr_data['bounds'], or the
    vertices' box as mask_at_box.frame_bounds gives it); dims / voxel_size: grid_spec.  Per slab of whole z-layers with at most slab_points
    points (at least one layer): vanerf_grid_points -> field_at_points.  Every step is a per-point function, so the slab size changes no bit."""
    if (dims is None) == (voxel_size is None):
        raise ValueError("give exactly one of dims and voxel_size")
    slab_points = int(slab_points)
    if slab_points < 1:
        raise ValueError(f"slab_points: expected a positive number of points, got {slab_points}")
    weights, fd, frame_b = _resolve(net, frame)
    origin, spacing, (nx, ny, nz) = grid_spec(_default_bounds(fd, frame_b, bounds), dims, voxel_size)
    dev = fd.verts3.device
    layers = max(1, slab_points // (nx * ny))
    with torch.cuda.device(dev), torch.no_grad():
        f = torch.empty(nz, ny, nx, dtype=torch.float32, device=dev)
        rgb = torch.empty(nz, ny, nx, 3, dtype=torch.float32, device=dev) if want_rgb else None
        for z0 in range(0, nz, layers):
            k = min(layers, nz - z0)
            pts = grid_points(origin, spacing, (nx, ny, nz), z0, k, dev)
            field_at_points(weights, fd, pts, want_rgb, pts.shape[0], out=(f[z0:z0 + k].view(-1), None if rgb is None else rgb[z0:z0 + k].view(-1, 3)))
    return (f, rgb) if want_rgb else f


def march(f, origin, spacing, iso=0.0, rgb=None):
    """Marching tetrahedra over f (nz, ny, nx) fp32 on the device (vanerf_surface_count, the read of the two counts, vanerf_surface_emit) ->
    verts (nv, 3) fp32, faces (nt, 3) int32, colors (nv, 3) fp32 or None.  rgb: (nz, ny, nx, 3) fp32 on the same device.  Inside is f < iso;
    triangles are wound with their normals towards growing f; the mesh is indexed, one vertex per crossed grid edge."""
    if not (torch.is_tensor(f) and f.dim() == 3):
        raise ValueError("f: expected a tensor (nz, ny, nx)")
    nz, ny, nx = (int(d) for d in f.shape)
    if min(nx, ny, nz) < 2 or 7 * nx * ny * nz >= 2 ** 31:
        raise ValueError(f"a grid of ({nx}, {ny}, {nz}) points: every dimension must be at least 2 and 7 nx ny nz below 2^31")
    if not math.isfinite(float(iso)):
        raise ValueError("iso must be finite")
    fp = _dev_ptr(f, torch.float32, "f")
    if rgb is not None and (tuple(rgb.shape) != (nz, ny, nx, 3) or rgb.device != f.device):
        raise ValueError(f"rgb: expected ({nz}, {ny}, {nx}, 3) on {f.device}")
    rp = _dev_ptr(rgb, torch.float32, "rgb")
    dev = f.device
    with torch.cuda.device(dev):
        nbytes = int(lib.vanerf_surface_scratch(nx, ny, nz))
        scratch = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        sp = c_void_p(scratch.data_ptr())
        check(lib.vanerf_surface_count(fp, nx, ny, nz, float(iso), sp, scratch.numel() * 8, c_void_p(counts.data_ptr()), _stream()))
        nv, nt = counts.tolist()  # the one host read
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(nt, 3, dtype=torch.int32, device=dev)
        colors = torch.empty(nv, 3, dtype=torch.float32, device=dev) if rgb is not None else None
        check(lib.vanerf_surface_emit(fp, rp, _f3(origin), _f3(spacing), nx, ny, nz, float(iso), sp, scratch.numel() * 8, nv, nt,
                                      c_void_p(verts.data_ptr()), None if colors is None else c_void_p(colors.data_ptr()),
                                      c_void_p(faces.data_ptr()), nv, nt, _stream()))
    return verts, faces, colors


def extract_surface(net, tr_batch, resolution=128, voxel_size=None, iso=0.0, colors=True, bounds=None, slab_points=SLAB_POINTS):
    """The level set f = iso of the learned field as a mesh: {"verts" (nv, 3) fp32, "faces" (nt, 3) int32, "colors" (nv, 3) fp32 or None,
    "mano_verts", "mano_faces"} on the device, the last two being the frame's input mesh, unchanged, for comparison.
    resolution: grid points along the longest axis of the bounds, cubic cells (unless voxel_size gives their edge).  net, tr_batch, bounds:
    as field_on_grid takes them.  At one source view the colour does not depend on the viewing direction."""
    weights, fd, frame_b = _resolve(net, tr_batch)
    b = _default_bounds(fd, frame_b, bounds)
    if voxel_size is None:
        resolution = int(resolution)
        if resolution < 2:
            raise ValueError(f"resolution: expected at least 2 points, got {resolution}")
        from . import renderer as R
        bt = torch.as_tensor(b)
        bh = np.asarray((R.host_copy(bt) if bt.is_cuda else bt).reshape(2, 3).tolist(), dtype=np.float64)
        voxel_size = float((bh[1] - bh[0]).max()) / (resolution - 1)
    origin, spacing, dims = grid_spec(b, voxel_size=voxel_size)
    res = field_on_grid(weights, fd, b, voxel_size=voxel_size, want_rgb=bool(colors), slab_points=slab_points)
    f, rgb = res if colors else (res, None)
    verts, faces, cols = march(f, origin, spacing, iso, rgb)
    return {"verts": verts, "faces": faces, "colors": cols, "mano_verts": fd.verts3, "mano_faces": fd.faces}


LINE_STATE_FLOATS = 16  # VANERF_LINE_STATE_FLOATS
_LINE_FIELDS = {"ta": 0, "tb": 1, "ga": 2, "gb": 3, "rgb_a": slice(4, 7), "found": 7, "rgb_b": slice(8, 11), "t_est": 11, "rgb_est": slice(12, 15),
                "t_next": 15}  # the VANERF_LS_* offsets of include/vanerf_hip.h
MAX_LINE_SAMPLES = 256  # VANERF_LINE_MAX_SAMPLES


def _lines(t, what, n=None):
    if not (torch.is_tensor(t) and t.dim() == 2 and t.shape[1] == 3 and (n is None or t.shape[0] == n)):
        raise ValueError(f"{what}: expected a tensor ({'n' if n is None else n}, 3)")
    return _dev_ptr(t, torch.float32, what)


def vertex_normals(verts, faces):
    """vanerf_vertex_normals: the unit vertex normals (nv, 3) of a mesh, verts (nv, 3) fp32 and faces (nf, 3) int32 on the device, with the
    bits render_vis's vertex pass computes."""
    vp = _lines(verts, "verts")
    if not (torch.is_tensor(faces) and faces.dim() == 2 and faces.shape[1] == 3):
        raise ValueError("faces: expected a tensor (nf, 3)")
    fp = _dev_ptr(faces, torch.int32, "faces")
    if faces.device != verts.device:
        raise ValueError("faces: expected a tensor on the vertices' device")
    with torch.cuda.device(verts.device):
        normals = torch.empty_like(verts)
        check(lib.vanerf_vertex_normals(vp, verts.shape[0], fp, faces.shape[0], c_void_p(normals.data_ptr()), _stream()))
    return normals


def line_points(base, direction, samples=1, t0=0.0, dt=1.0, t=None):
    """vanerf_line_points: the points base + t direction of n lines (base, direction: (n, 3) fp32 on the device) as (n samples, 3), line-major.
    t = None: t_k = fmaf(k, dt, t0), k < samples.  t: (n,) fp32 on the device, one parameter per line (samples must be 1); a non-finite
    entry gives the base itself."""
    samples = int(samples)
    bp = _lines(base, "base")
    n = base.shape[0]
    dp = _lines(direction, "direction", n)
    if t is not None and not (torch.is_tensor(t) and tuple(t.shape) == (n,)):
        raise ValueError(f"t: expected a tensor ({n},)")
    tp = _dev_ptr(t, torch.float32, "t")
    if any(x is not None and x.device != base.device for x in (direction, t)):
        raise ValueError("direction and t: expected tensors on the device of base")
    with torch.cuda.device(base.device):
        pts = torch.empty(n * max(samples, 0), 3, dtype=torch.float32, device=base.device)
        check(lib.vanerf_line_points(bp, dp, n, samples, float(t0), float(dt), tp, c_void_p(pts.data_ptr()), _stream()))
    return pts


def line_bracket(f, t0, dt, iso=0.0, rgb=None):
    """vanerf_line_bracket: f (n, K) fp32 on the device, the field at line_points(..., K, t0, dt)[, rgb (n, K, 3)] -> the state tensor
    (n, LINE_STATE_FLOATS) with the bracket of the crossing of f = iso nearest to t = 0 on every line (line_state names its columns)."""
    if not (torch.is_tensor(f) and f.dim() == 2):
        raise ValueError("f: expected a tensor (n, K)")
    n, K = (int(d) for d in f.shape)
    fp = _dev_ptr(f, torch.float32, "f")
    if rgb is not None and (tuple(rgb.shape) != (n, K, 3) or rgb.device != f.device):
        raise ValueError(f"rgb: expected ({n}, {K}, 3) on {f.device}")
    rp = _dev_ptr(rgb, torch.float32, "rgb")
    with torch.cuda.device(f.device):
        state = torch.empty(n, LINE_STATE_FLOATS, dtype=torch.float32, device=f.device)
        check(lib.vanerf_line_bracket(fp, rp, n, K, float(t0), float(dt), float(iso), c_void_p(state.data_ptr()), _stream()))
    return state


def line_refine(state, f_new, iso=0.0, rgb_new=None):
    """vanerf_line_refine: one round in place on `state` (returned) with f_new (n,) fp32[, rgb_new (n, 3)], the field at state's t_next."""
    if not (torch.is_tensor(state) and state.dim() == 2 and state.shape[1] == LINE_STATE_FLOATS):
        raise ValueError(f"state: expected a tensor (n, {LINE_STATE_FLOATS})")
    sp = _dev_ptr(state, torch.float32, "state")
    n = state.shape[0]
    if not (torch.is_tensor(f_new) and tuple(f_new.shape) == (n,)):
        raise ValueError(f"f_new: expected a tensor ({n},)")
    fp = _dev_ptr(f_new, torch.float32, "f_new")
    if rgb_new is not None and tuple(rgb_new.shape) != (n, 3):
        raise ValueError(f"rgb_new: expected ({n}, 3)")
    rp = _dev_ptr(rgb_new, torch.float32, "rgb_new")
    if any(x is not None and x.device != state.device for x in (f_new, rgb_new)):
        raise ValueError("f_new and rgb_new: expected tensors on the device of state")
    with torch.cuda.device(state.device):
        check(lib.vanerf_line_refine(fp, rp, n, float(iso), sp, _stream()))
    return state


def line_state(state):
    """Named views of a state tensor (n, LINE_STATE_FLOATS): ta, tb, ga, gb, found, t_est, t_next (n,) and rgb_a, rgb_b, rgb_est (n, 3)."""
    if not (torch.is_tensor(state) and state.dim() == 2 and state.shape[1] == LINE_STATE_FLOATS):
        raise ValueError(f"state: expected a tensor (n, {LINE_STATE_FLOATS})")
    return {k: state[:, at] for k, at in _LINE_FIELDS.items()}


def register_surface(net, tr_batch, band=0.004, samples=9, refine=4, iso=0.0, colors=True):
    """The MANO mesh registered onto the learned surface: every vertex v moves along its vertex normal n to the crossing of f = iso nearest to
    it on the line v + t n, |t| <= band.  Steps: vertex_normals -> line_points (t0 = -band, dt = 2 band / (samples - 1)) -> field_at_points ->
    line_bracket -> `refine` rounds of (line_points at t_next -> field_at_points -> line_refine) -> line_points at t_est.

    -> {"verts" (nv, 3): a vertex without a crossing keeps its MANO position bit for bit; "faces": the frame's own (nf, 3) int32;
    "colors" (nv, 3) or None: the learned colour at the crossing, zeros without one; "displacement" (nv,): t_est, NaN without a crossing;
    "found" (nv,) bool; "normals" (nv, 3); "mano_verts" (nv, 3); "state" (nv, LINE_STATE_FLOATS): the final brackets (line_state names its
    columns)}, all on the device.  net, tr_batch: as field_on_grid takes them, in the
    handle's precision.  samples is odd, so t = 0 is a sample.  Beyond what resolving the frame does, nothing is read back to the host."""
    band, iso, samples, refine = float(band), float(iso), int(samples), int(refine)
    if not (math.isfinite(band) and band > 0.0):
        raise ValueError(f"band: expected a positive number, got {band}")
    if samples < 3 or samples % 2 == 0 or samples > MAX_LINE_SAMPLES:
        raise ValueError(f"samples: expected an odd number from 3 to {MAX_LINE_SAMPLES - 1}, got {samples}")
    if refine < 0:
        raise ValueError(f"refine: expected a number of rounds >= 0, got {refine}")
    if not math.isfinite(iso):
        raise ValueError("iso must be finite")
    t0, dt = float(np.float32(-band)), float(np.float32(2.0 * band / (samples - 1)))
    if not dt > 0.0:
        raise ValueError(f"the step {dt} underflows fp32")
    weights, fd, _ = _resolve(net, tr_batch)
    want = bool(colors)
    with torch.cuda.device(fd.verts3.device), torch.no_grad():
        verts, nv = fd.verts3, fd.verts3.shape[0]
        normals = vertex_normals(verts, fd.faces)
        res = field_at_points(weights, fd, line_points(verts, normals, samples, t0, dt), want_rgb=want)
        f, rgb = res if want else (res, None)
        state = line_bracket(f.view(nv, samples), t0, dt, iso, None if rgb is None else rgb.view(nv, samples, 3))
        S = line_state(state)
        for _ in range(refine):
            res = field_at_points(weights, fd, line_points(verts, normals, t=S["t_next"].contiguous()), want_rgb=want)
            f, rgb = res if want else (res, None)
            line_refine(state, f, iso, rgb)
        t_est = S["t_est"].contiguous()
        out = line_points(verts, normals, t=t_est)
    return {"verts": out, "faces": fd.faces, "colors": S["rgb_est"].contiguous() if want else None, "displacement": t_est,
            "found": S["found"] != 0, "normals": normals, "mano_verts": verts, "state": state}


def save_ply(path, verts, faces, colors=None):
    """Binary little-endian PLY: float x y z[, uchar red green blue] per vertex, `list uchar int vertex_indices` per face.  colors in
    [0, 1] (clamped, rounded to 8 bits).  Tensors (any device) or arrays."""
    def host(a):
        return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    v = np.ascontiguousarray(host(verts), dtype="<f4")
    t = np.ascontiguousarray(host(faces)).astype("<i4")
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"verts: expected (nv, 3), got {v.shape}")
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"faces: expected (nt, 3), got {t.shape}")
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("faces index outside the vertices")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if colors is not None:
        c = host(colors)
        if c.shape != v.shape:
            raise ValueError(f"colors: expected {v.shape}, got {c.shape}")
        c8 = np.rint(np.clip(np.nan_to_num(c.astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(len(v), dtype=fields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        vrec["red"], vrec["green"], vrec["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.empty(len(t), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = t
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())
    return path


__all__ = ["SLAB_POINTS", "LINE_STATE_FLOATS", "grid_spec", "grid_points", "field_at_points", "field_on_grid", "march", "extract_surface", "vertex_normals",
           "line_points", "line_bracket", "line_refine", "line_state", "register_surface", "save_ply"]
