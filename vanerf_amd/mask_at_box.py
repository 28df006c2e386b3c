"""The dataset's mask_at_box and near / far range of target views on the GPU (vanerf_amd/csrc/mask_at_box.hip): Dataset.get_mask_at_box ->
get_rays / get_near_far (src/dataset.py:122-129, 609-658) and the bounds of load_human_bounds* (src/dataset.py:131-138, 191-196), restated
(DESIGN.md section 0d).  With these, metrics.evaluate_views needs cameras and ground-truth images only.  Nothing here waits for the GPU
except the read-back of `bounds` when it is a device tensor (it is passed to the kernel by value, as everywhere in this package).
"""
from ctypes import c_void_p

import torch

from ._ffi import check, lib

SLOTS = ("near_min", "far_max", "n_mask", "box_x", "box_y", "box_w", "box_h", "pad")


def frame_bounds(verts, pad_z=0.05):
    """load_human_bounds_pred and the tail of load_human_bounds: verts (..., 3) -> (2, 3) per-axis min / max over all vertices, z widened by
    pad_z on both sides.  A reduction on the device of `verts`; nothing is read back."""
    if not torch.is_tensor(verts) or verts.shape[-1] != 3 or verts.numel() == 0:
        raise ValueError("verts: expected a tensor (..., 3) with at least one vertex")
    xyz = verts.reshape(-1, 3)
    lo, hi = xyz.min(dim=0).values, xyz.max(dim=0).values
    pad = torch.tensor([0.0, 0.0, float(pad_z)], dtype=xyz.dtype, device=xyz.device)
    return torch.stack([lo - pad, hi + pad])


def mask_at_box(cam_tars, bounds, per_ray=False, out=None):
    """cam_tars: the V target cameras of one frame (dicts with K, RT, width, height, as render_pifu_nerf_views takes them; device tensors);
    bounds: (2, 3)-shaped, min xyz then max xyz.  Returns (mask (V, H, W) uint8 0 / 1, table (V, 8) fp32 of `SLOTS`) on the device, and with
    per_ray also near, far (V, H, W) fp32: the ray's range on mask pixels, NaN elsewhere.  near_min / far_max are NaN and the rectangle is
    0, 0, 0, 0 for a view that misses the box.  The camera table is renderer.camera_table's, the one the render pass marches.
    out: a contiguous fp32 device tensor (V, 8) to write the table into."""
    from . import renderer as R
    cam_tars = list(cam_tars)
    if not cam_tars:
        raise ValueError("mask_at_box needs at least one target camera")
    K = cam_tars[0]["K"]
    if not torch.is_tensor(K) or not K.is_cuda:
        raise ValueError("mask_at_box runs on the GPU and takes cameras with device tensors (no CPU fallback)")
    dev = K.device
    if torch.is_tensor(bounds) and bounds.is_cuda and bounds.device != dev:
        raise ValueError(f"bounds is on {bounds.device}, the cameras on {dev}")
    bounds = torch.as_tensor(bounds)
    if bounds.numel() != 6:
        raise ValueError(f"bounds: expected (2, 3), got {tuple(bounds.shape)}")
    V, H, W = len(cam_tars), int(cam_tars[0].get("height", 0)), int(cam_tars[0]["width"])
    if H < 1 or W < 1:
        raise ValueError(f"the cameras carry height={H} width={W}")
    b6 = R._farr(R.host_copy(bounds).reshape(-1).tolist(), 6)
    with torch.cuda.device(dev):
        # (znear / zfar are columns of the table that this kernel does not read: a camera that has none yet -- near_far is how it gets them -- gets 0)
        cams = R.camera_table([c if "znear" in c and "zfar" in c else dict(c, znear=c.get("znear", 0.0), zfar=c.get("zfar", 0.0)) for c in cam_tars], dev)
        mask = torch.empty(V, H, W, dtype=torch.uint8, device=dev)
        near = torch.empty(V, H, W, dtype=torch.float32, device=dev) if per_ray else None
        far = torch.empty(V, H, W, dtype=torch.float32, device=dev) if per_ray else None
        if out is None:
            out = torch.empty(V, 8, dtype=torch.float32, device=dev)
        elif not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()
                  and tuple(out.shape) == (V, 8)):
            raise ValueError(f"out: expected a contiguous fp32 device tensor of shape ({V}, 8)")
        nbytes = lib.vanerf_mask_at_box_scratch(V, H, W)
        scratch = torch.empty(max(nbytes, 16) // 8 + 1, dtype=torch.float64, device=dev)  # an invalid shape (0 bytes) is refused by the call below
        ptr = lambda t: None if t is None else c_void_p(t.data_ptr())  # noqa: E731
        check(lib.vanerf_mask_at_box(ptr(cams), V, H, W, b6, ptr(mask), ptr(near), ptr(far), ptr(scratch), scratch.numel() * 8, ptr(out),
                                     c_void_p(torch.cuda.current_stream().cuda_stream)))
    return (mask, out, near, far) if per_ray else (mask, out)


def near_far(table, view=0):
    """(znear, zfar) of a view as 0-d device tensors, for callers that set provide_znear_zfar (the dataset's near.min(), far.max())."""
    if table.dim() == 1:
        table = table[None]
    return table[view, 0], table[view, 1]
