"""Image scores of the reference's validation and test steps on the GPU (vanerf_amd/csrc/image_metrics.hip): MSE, PSNR, scikit-image's SSIM on
the crop to the bounding rectangle of mask_at_box (Evaluator.compute_score, src/evaluator.py:84-114) and kornia's masked PSNR / Gaussian SSIM
(compute_test_metric, src/model.py:210-235).  Neither library is a dependency; the arithmetic is restated and parity
against kornia 0.7.1 / scikit-image 0.16.2 is unpinned.  Nothing here waits for the GPU except compute_score, which returns Python floats.
"""
from ctypes import c_void_p

import torch

from ._ffi import check, lib

SLOTS = ("mse", "psnr", "ssim_box", "psnr_masked", "ssim_masked", "n_mask", "box_w", "box_h")


def _images(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{name}: image_metrics runs on the GPU and takes device tensors (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected torch.float32, got {t.dtype}")
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError(f"{name}: expected (3, H, W) or (V, 3, H, W), got {tuple(t.shape)}")
    return t.contiguous()


def _mask(m, name, V, H, W, dev):
    if m is None:
        return None
    if not torch.is_tensor(m) or not m.is_cuda:
        raise ValueError(f"{name}: image_metrics takes device tensors (no CPU fallback)")
    if m.device != dev:
        raise ValueError(f"{name} is on {m.device}, the images on {dev}")
    if m.numel() != V * H * W or tuple(m.shape[-2:]) != (H, W):
        raise ValueError(f"{name}: expected {V} mask(s) of {H} x {W}, got {tuple(m.shape)}")
    if m.dtype != torch.uint8:
        m = (m != 0).to(torch.uint8)  # bool and number masks alike, on the device
    return m.reshape(V, H, W).contiguous()


def image_metrics(pred, gt, mask=None, mask_at_box=None, max_val=1.0, clamp_pred=False, out=None):
    """pred, gt: (3, H, W) or (V, 3, H, W) fp32 device tensors; mask, mask_at_box: (H, W), (V, H, W) or (V, 1, H, W), bool / uint8 / numbers
    (nonzero = set).  Returns the device tensor (V, 8) of `SLOTS`: mse, psnr, ssim_box (evaluator flavour, on the crop to the bounding rectangle
    of mask_at_box), psnr_masked, ssim_masked (compute_test_metric flavour, over the pixels of mask), n_mask, box_w, box_h.  NaN where the
    reference raises or divides by zero: ssim_box for an empty mask_at_box or a crop below 7 x 7, the masked pair for an empty mask.
    clamp_pred: pred is clamped to [0, 1] as it is read.  out: a contiguous fp32 device tensor (V, 8) to write into."""
    pred, gt = _images(pred, "pred"), _images(gt, "gt")
    if pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError(f"pred {tuple(pred.shape)} on {pred.device} and gt {tuple(gt.shape)} on {gt.device} differ")
    V, _, H, W = pred.shape
    dev = pred.device
    mask, mask_at_box = _mask(mask, "mask", V, H, W, dev), _mask(mask_at_box, "mask_at_box", V, H, W, dev)
    nbytes = lib.vanerf_image_metrics_scratch(V, H, W)
    if out is None:
        out = torch.empty(V, 8, dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.dtype == torch.float32 and out.is_contiguous()
              and tuple(out.shape) == (V, 8)):
        raise ValueError(f"out: expected a contiguous fp32 device tensor of shape ({V}, 8)")
    scratch = torch.empty(max(nbytes, 16) // 8 + 1, dtype=torch.float64, device=dev)  # an invalid shape (0 bytes) is refused by the call below
    ptr = lambda t: None if t is None else c_void_p(t.data_ptr())  # noqa: E731
    with torch.cuda.device(dev):
        check(lib.vanerf_image_metrics(ptr(pred), ptr(gt), ptr(mask), ptr(mask_at_box), V, H, W, float(max_val), int(bool(clamp_pred)),
                                       ptr(scratch), scratch.numel() * 8, ptr(out), c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def compute_test_metric(rendered_img, gt_img, mask=None, max_val=1.0):
    """VANeRFLightningModule.compute_test_metric (src/model.py:210-235) without kornia: rendered_img, gt_img (3, H, W) or (B, 3, H, W) in
    [0, max_val], mask (H, W)-shaped bool (one image, as in the reference).  Returns {'psnr', 'ssim'} as 0-d device tensors; nothing is read back."""
    if rendered_img.shape != gt_img.shape:
        raise ValueError(f"rendered_img {tuple(rendered_img.shape)} and gt_img {tuple(gt_img.shape)} differ")
    B = 1 if rendered_img.dim() == 3 else rendered_img.shape[0]
    if mask is not None:
        if B != 1:
            raise ValueError("a mask goes with one image (the reference views it as (1, H, W))")
        mask = mask.reshape(1, *mask.shape[-2:])
    s = image_metrics(rendered_img, gt_img, mask=mask, max_val=max_val)
    if B == 1:
        return {"psnr": s[0, 3], "ssim": s[0, 4]}
    # a batch is pooled: the mean of S over all images, the PSNR of the mean squared error of all of them
    return {"psnr": -10.0 * torch.log10(torch.pow(10.0, -0.1 * s[:, 3]).mean()), "ssim": s[:, 4].mean()}


def compute_score(rgb_pred, rgb_gt, mask_at_box):
    """Evaluator.compute_score (src/evaluator.py:84-114) without scikit-image and OpenCV: rgb_pred, rgb_gt (3, H, W) or (1, 3, H, W),
    mask_at_box (H, W)-shaped.  Returns {'mse', 'psnr', 'ssim'} as Python floats with ONE read-back.  Unlike the reference it writes no image
    files, and it has no 'lpips' key: LPIPS needs the AlexNet weights, which are not shipped.  'ssim' is NaN where the reference raises (an
    empty mask, a bounding rectangle below 7 x 7)."""
    if (rgb_pred.dim() == 4 and rgb_pred.shape[0] != 1) or rgb_pred.dim() not in (3, 4):
        raise ValueError(f"compute_score scores one image, got {tuple(rgb_pred.shape)}")
    if mask_at_box is not None:
        mask_at_box = mask_at_box.reshape(1, *mask_at_box.shape[-2:])
    mse, psnr, ssim = image_metrics(rgb_pred, rgb_gt, mask_at_box=mask_at_box)[0, :3].tolist()
    return {"mse": mse, "psnr": psnr, "ssim": ssim}


def evaluate_views(net, tr_batch, cam_tars, tar_imgs, masks_at_box, masks=None, views_per_pass=None, mask_from_bounds=False):
    """The test loop of one source frame: renders the target views `cam_tars` through VANeRF.render_pifu_nerf_views, `views_per_pass` at a time
    (default: all in one pass), and scores each view's tex_fg_fine, clamped to [0, 1] as the reference clamps before it scores, against
    tar_imgs (V, 3, H, W) with masks_at_box (V, H, W) [and masks (V, H, W) for the masked pair; None: every pixel].  Returns (scores (V, 8) on
    the device -- `SLOTS` --, list of the V rendered images (3, H, W)).  Never waits for the GPU: the caller reads the scores back when it
    wants them, once for the whole frame.
    mask_from_bounds: masks_at_box must be None; the masks are made on the device from tr_batch["dr_data"]["bounds"] and the same cameras
    (mask_at_box.mask_at_box, the dataset's get_mask_at_box) on the stream of the pass, before the first render."""
    from .novel_views import _default_render_views
    if mask_from_bounds and masks_at_box is not None:
        raise ValueError("evaluate_views: masks_at_box and mask_from_bounds are two sources of one mask, give one of them")
    cam_tars = list(cam_tars)
    V = len(cam_tars)
    if V == 0:
        raise ValueError("evaluate_views needs at least one target camera")
    group = V if views_per_pass is None else int(views_per_pass)
    if group < 1:
        raise ValueError("views_per_pass must be at least 1")
    if not net.kwargs["dr_kwargs"]["fine"]:
        raise ValueError("evaluate_views scores tex_fg_fine: the model's dr_kwargs must have fine=True")
    if torch.is_tensor(tar_imgs):
        tar_imgs = tar_imgs[None] if tar_imgs.dim() == 3 else tar_imgs
    else:
        tar_imgs = torch.stack([t.reshape(3, *t.shape[-2:]) for t in tar_imgs])
    if tar_imgs.shape[0] != V:
        raise ValueError(f"{tar_imgs.shape[0]} target images for {V} cameras")
    H, W = tar_imgs.shape[-2:]

    def per_view(m, name):
        if m is None:
            return None
        m = m if torch.is_tensor(m) else torch.stack([x.reshape(H, W) for x in m])
        if m.numel() != V * H * W:
            raise ValueError(f"{name}: expected {V} mask(s) of {H} x {W}, got {tuple(m.shape)}")
        return m.reshape(V, H, W)

    if mask_from_bounds:
        from .mask_at_box import mask_at_box
        masks_at_box = mask_at_box(cam_tars, tr_batch["dr_data"]["bounds"])[0]
    masks_at_box, masks = per_view(masks_at_box, "masks_at_box"), per_view(masks, "masks")
    scores = torch.empty(V, 8, dtype=torch.float32, device=tar_imgs.device)
    images = []
    for v0 in range(0, V, group):
        v1 = min(v0 + group, V)
        outs = _default_render_views(net, tr_batch, cam_tars[v0:v1], 1)
        pred = torch.stack([o["tex_fg_fine"] for o in outs])
        image_metrics(pred, tar_imgs[v0:v1], mask=None if masks is None else masks[v0:v1],
                      mask_at_box=None if masks_at_box is None else masks_at_box[v0:v1], clamp_pred=True, out=scores[v0:v1])
        images.extend(pred[i] for i in range(v1 - v0))
    return scores, images
