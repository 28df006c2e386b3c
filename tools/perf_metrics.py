"""Image scores (vanerf_image_metrics, vanerf_amd/metrics.py) at the two shapes of the reference's loops: the 5 target views of a test frame
at 512x334 and one 256x256 validation view.  Per shape, in one process: the time of one image_metrics call from device events (the
scores stay on the device), the same call followed by the one read-back of the table, and a plain PyTorch-ROCm restatement of the same
eight quantities (conv2d with the two windows, boolean indexing) followed by .cpu() -- what a caller without the kernels would write.
The two paths alternate; each figure is the median of `--reps` windows of `--calls` calls.  The restatement's values are compared with the
kernels' before anything is timed.  Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf_metrics.py
(im_box_kernel, im_tile_kernel, im_finish_kernel)."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vanerf_amd import metrics  # noqa: E402


def torch_scores(pred, gt, mask, box, max_val=1.0):
    """The eight slots per view with torch ops, one view at a time as the reference's loops go; returns a host tensor (V, 8).  The bounding
    rectangle is read back to crop (cv2.boundingRect needs the mask on the host in the reference as well)."""
    V, _, H, W = pred.shape
    k = torch.arange(7, dtype=torch.float32, device=pred.device) - 3.0
    g = torch.exp(-(k * k) / (2.0 * 1.5 * 1.5))
    g = g / g.sum()
    wg = torch.outer(g, g)[None, None].expand(3, 1, 7, 7).contiguous()
    wu = torch.full((3, 1, 7, 7), 1.0 / 49.0, device=pred.device)
    rows = []
    for v in range(V):
        x, y = pred[v:v + 1].clamp(0.0, 1.0), gt[v:v + 1]
        d2 = (x - y) ** 2
        mse = d2.mean()
        cols_any, rows_any = box[v].any(0).nonzero(), box[v].any(1).nonzero()
        bx, by = int(cols_any[0]), int(rows_any[0])
        bw, bh = int(cols_any[-1]) - bx + 1, int(rows_any[-1]) - by + 1
        xc, yc = x[..., by:by + bh, bx:bx + bw], y[..., by:by + bh, bx:bx + bw]
        ux, uy = F.conv2d(xc, wu, groups=3), F.conv2d(yc, wu, groups=3)
        vx = 49.0 / 48.0 * (F.conv2d(xc * xc, wu, groups=3) - ux * ux)
        vy = 49.0 / 48.0 * (F.conv2d(yc * yc, wu, groups=3) - uy * uy)
        vxy = 49.0 / 48.0 * (F.conv2d(xc * yc, wu, groups=3) - ux * uy)
        su = ((2 * ux * uy + 0.02 ** 2) * (2 * vxy + 0.06 ** 2)) / ((ux * ux + uy * uy + 0.02 ** 2) * (vx + vy + 0.06 ** 2))
        xp, yp = F.pad(x, (3, 3, 3, 3), mode="reflect"), F.pad(y, (3, 3, 3, 3), mode="reflect")
        m1, m2 = F.conv2d(xp, wg, groups=3), F.conv2d(yp, wg, groups=3)
        s1, s2, s12 = F.conv2d(xp * xp, wg, groups=3) - m1 * m1, F.conv2d(yp * yp, wg, groups=3) - m2 * m2, F.conv2d(xp * yp, wg, groups=3) - m1 * m2
        C1, C2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
        sg = ((2 * m1 * m2 + C1) * (2 * s12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2) + 1e-12)
        m = mask[v].bool()
        sel = d2[0].permute(1, 2, 0)[m]
        rows.append(torch.stack([mse, -10.0 * torch.log10(mse), su.mean(), 10.0 * torch.log10(max_val ** 2 / sel.mean()),
                                 sg[0].permute(1, 2, 0)[m].mean(), m.sum().float(), torch.tensor(float(bw), device=pred.device),
                                 torch.tensor(float(bh), device=pred.device)]))
    return torch.stack(rows).cpu()


def inputs(V, H, W, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    low = torch.rand(V, 3, H // 16 + 2, W // 16 + 2, device="cuda", generator=gen)
    gt = F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False).clamp(0.0, 1.0).contiguous()
    pred = gt + 0.05 * torch.randn(V, 3, H, W, device="cuda", generator=gen)  # leaves [0, 1] in places: the clamp has work to do
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    ell = (((yy - H / 2) / (0.4 * H)) ** 2 + ((xx - W / 2) / (0.36 * W)) ** 2 <= 1.0).to(torch.uint8)
    mask = ell[None].expand(V, H, W).contiguous()
    return pred, gt, mask, mask.clone()


def window(fn, calls):
    """ms per call over `calls` calls: device events around the window, and the host clock around window + synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls, 1e3 * (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_metrics.py measures on the GPU: no device found")
    for V, H, W in ((5, 512, 334), (1, 256, 256)):
        pred, gt, mask, box = inputs(V, H, W)
        out = torch.empty(V, 8, device="cuda")
        paths = {
            "kernels, scores left on the device": lambda: metrics.image_metrics(pred, gt, mask=mask, mask_at_box=box, clamp_pred=True, out=out),
            "kernels + one read-back": lambda: metrics.image_metrics(pred, gt, mask=mask, mask_at_box=box, clamp_pred=True, out=out).cpu(),
            "torch restatement + .cpu()": lambda: torch_scores(pred, gt, mask, box),
        }
        got, want = paths["kernels + one read-back"](), paths["torch restatement + .cpu()"]()
        print(f"V={V} {H}x{W}: largest |kernels - torch restatement| per slot " + " ".join(f"{e:.1e}" for e in (got - want).abs().amax(0).tolist()))
        for fn in paths.values():  # warm-up of every shape the windows use
            for _ in range(5):
                fn()
        times = {k: [] for k in paths}
        for _ in range(a.reps):  # the paths alternate
            for k, fn in paths.items():
                times[k].append(window(fn, a.calls))
        for k, t in times.items():
            dev, host = statistics.median(x[0] for x in t), statistics.median(x[1] for x in t)
            print(f"V={V} {H}x{W}  {k:36s} {1e3 * dev:9.1f} us per call by device events (min {1e3 * min(x[0] for x in t):.1f}, max {1e3 * max(x[0] for x in t):.1f}), "
                  f"{1e3 * host:9.1f} us by the host clock; {a.reps} windows of {a.calls} calls")


if __name__ == "__main__":
    main()
