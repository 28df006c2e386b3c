"""The learned hand surface as a triangle mesh, on the GPU (vanerf_amd/csrc/surface.hip).

The network predicts a residual on the MANO signed distance: eval_func returns alpha = valid relu(rad) and the composite turns
f = alpha + mesh_sdf into a density (src/model.py:1158, 1480-1481), so the hand is the zero level set of f.  field_on_grid evaluates f on a
regular grid with the calls the render pass makes per sample (mesh query, validity partition, per-sample networks); extract_surface runs
marching tetrahedra over it (vanerf_surface_count / vanerf_surface_emit) and returns an indexed, welded mesh on the device.  The only wait
for the GPU is the read of the two counts between those calls (and of `bounds` when it is a device tensor: it goes to the kernels by value).
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


def field_on_grid(net, frame, bounds=None, dims=None, voxel_size=None, want_rgb=False, slab_points=SLAB_POINTS):
    """f = alpha + mesh_sdf on a regular grid -> (nz, ny, nx) fp32 on the device[, rgb (nz, ny, nx, 3)].

    net, frame: a VANeRF module and a tr_batch of device tensors, or a renderer.PackedWeights handle and a renderer.FrameData: the handle and
    frame data of the render pass, in the handle's precision.  bounds: (2, 3)-shaped, default the frame's own (dr_data['bounds'], or the
    vertices' box as mask_at_box.frame_bounds gives it); dims / voxel_size: grid_spec.  Per slab of whole z-layers with at most slab_points
    points (at least one layer): vanerf_grid_points -> vanerf_mesh_query_accel with the 1-NN vertex -> vanerf_query_order ->
    vanerf_query_samples (raw = 0, no noise) -> vanerf_field_values.  Every step is a per-point function, so the slab size changes no bit."""
    from . import renderer as R
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
            sdf, vis, knn = R.mesh_query_accel(fd.accel, fd.verts3, fd.faces, fd.vert_vis, pts)
            out = R.query_samples(weights, fd, pts, sdf, vis, knn, order=R.query_order(fd, pts))
            check(lib.vanerf_field_values(c_void_p(out.data_ptr()), c_void_p(sdf.data_ptr()), pts.shape[0], c_void_p(f[z0:z0 + k].data_ptr()),
                                          None if rgb is None else c_void_p(rgb[z0:z0 + k].data_ptr()), _stream()))
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


__all__ = ["SLAB_POINTS", "grid_spec", "grid_points", "field_on_grid", "march", "extract_surface", "save_ply"]
