"""render_vis with the reference's signature (src/render_vis.py:181-226), on the HIP rasteriser of vanerf_amd/csrc/vis_render.hip.

A user of the reference rebinds `src.model.render_vis` to this function; VANeRF.batch_render_pifu_nerf of this package
calls the same kernel when its `render_vis` switch is on.  The semantics are pytorch3d 0.7.5's, restated.
"""
import torch

from . import renderer


def _pair(a, b, dev):
    """(a, b) as a (2,) fp32 device tensor: floats, or tensors of shape (1,) / () that stay on the device (no .item())."""
    return torch.cat([torch.as_tensor(x, dtype=torch.float32, device=dev).reshape(1) for x in (a, b)])


def render_vis(verts, faces, vert_vis, R, T, fx, fy, px, py, mask_path=None, image_size=(256, 256), device=None):
    """verts (1,NV,3) world coordinates, faces (1,NF,3) or (NF,3), vert_vis NV values in {0, 1} (any shape, e.g. (1,NV,1)), R (1,3,3) and
    T (1,3) in pytorch3d's convention (Xv = X R + T), fx fy px py screen-space values (floats or tensors of shape (1,)), image_size (H, W).
    Returns (vis_img_rbg (1,3,H,W), vis_img (1,1,H,W)) as the reference does.  `mask_path` is accepted and unused, as there.
    Face indices outside [0, NV) draw nothing (they are not checked on the host: that would wait for the GPU)."""
    dev = torch.device(device) if device is not None else verts.device
    if dev.type != "cuda":
        raise ValueError("render_vis runs on the GPU (no CPU fallback)")
    H, W = (int(s) for s in image_size)
    f32 = torch.float32
    v = verts.to(dev, f32).reshape(-1, 3).contiguous()
    f = faces.to(dev).reshape(-1, 3).to(torch.int32).contiguous()
    vis = vert_vis.to(dev, f32).reshape(-1).contiguous()
    if vis.numel() != v.shape[0]:
        raise ValueError(f"vert_vis has {vis.numel()} values for {v.shape[0]} vertices")
    if v.shape[0] == 0 or f.shape[0] == 0:
        raise ValueError("render_vis needs at least one vertex and one face")
    rot = R.to(dev, f32).reshape(3, 3).contiguous()
    tr = T.to(dev, f32).reshape(3).contiguous()
    rgb, img = renderer.render_vis(v, f, vis, rot, tr, _pair(fx, fy, dev), _pair(px, py, dev), H, W)
    return rgb[None], img[None, None]
