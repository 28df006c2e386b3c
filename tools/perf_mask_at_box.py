"""mask_at_box and the near / far range (vanerf_mask_at_box, vanerf_amd/mask_at_box.py) at the two shapes of the reference's loops: the 5 target
views of a test frame at 512x334 and one 256x256 validation view.  Per shape, in one process: the time of one mask_at_box call from device
events (camera table upload and the two launches; everything stays on the device), the two launches alone on a table that is already there,
the call followed by the read-back of the table, and a plain PyTorch-ROCm restatement of the same quantities in fp64 (one view at a time, as
the dataset goes) followed by .cpu() -- what a caller without the kernels would write.  The paths alternate; each figure is the median of
`--reps` windows of `--calls` calls.  The restatement's values are compared with the kernels' before anything is timed.  Kernel times:
rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf_mask_at_box.py (mb_tile_kernel, mb_finish_kernel)."""
import argparse
import math
import os
import statistics
import sys
import time
from ctypes import c_float, c_void_p

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vanerf_amd import _ffi, mask_at_box as mab, renderer  # noqa: E402


def cameras(V, H, W, centre, dist=0.8):
    """V cameras on a circle around `centre` that look at it; the focal length puts the box on roughly half of the image."""
    cams = []
    for v in range(V):
        a = 2.0 * math.pi * v / max(V, 1) + 0.3
        eye = centre + torch.tensor([dist * math.cos(a), 0.15, dist * math.sin(a)])
        z = (centre - eye) / (centre - eye).norm()
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), z)
        x = x / x.norm()
        R = torch.stack([x, torch.linalg.cross(z, x), z])
        K, RT = torch.eye(4), torch.eye(4)
        K[0, 0] = K[1, 1] = 1.6 * min(H, W)
        K[0, 2], K[1, 2] = W / 2.0 - 0.3, H / 2.0 + 0.2
        RT[:3, :3], RT[:3, 3] = R, -R @ eye
        cams.append({"K": K[None].cuda(), "RT": RT[None].cuda(), "width": W, "height": H, "znear": 0.1, "zfar": 2.0})
    return cams


def torch_mask_at_box(table, bounds, H, W):
    """The mask and the table per view with torch ops in fp64 on the device; returns host tensors (mask (V, H, W) uint8, table (V, 8))."""
    dev = table.device
    masks, rows = [], []
    b = bounds.double().reshape(2, 3) + torch.tensor([[-0.01], [0.01]], dtype=torch.float64, device=dev)
    lo, hi = b[0] - 1e-6, b[1] + 1e-6
    r, c = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    xy1 = torch.stack([c, r, torch.ones_like(c)], dim=-1)
    for row in table.double():
        Kt, M = row[:9].reshape(3, 3), row[9:21].reshape(3, 4)
        R, T = M[:, :3], M[:, 3]
        o64 = -(R.t() @ T)
        d = (((xy1 @ Kt) - T) @ R - o64).float()
        d = torch.where(d.abs() < 1e-5, torch.full_like(d, 1e-5), d).double()
        o = o64.float().double()
        t = (b.reshape(1, 1, 2, 3) - o) / d[..., None, :]                      # (H, W, 2, 3)
        p = t.reshape(H, W, 6, 1) * d[..., None, :] + o                        # (H, W, 6, 3)
        inside = ((p >= lo) & (p <= hi)).all(-1)
        mask = inside.sum(-1) == 2
        dist = (p - o).norm(dim=-1) / d.norm(dim=-1, keepdim=True)
        near = torch.where(inside, dist, torch.full_like(dist, float("inf"))).amin(-1)[mask]
        far = torch.where(inside, dist, torch.full_like(dist, float("-inf"))).amax(-1)[mask]
        cols, rws = mask.any(0).nonzero(), mask.any(1).nonzero()
        rect = [float(cols[0]), float(rws[0]), float(cols[-1] - cols[0] + 1), float(rws[-1] - rws[0] + 1)] if cols.numel() else [0.0] * 4
        rows.append(torch.stack([near.min(), far.max(), mask.sum().double()] + [torch.tensor(x, dtype=torch.float64, device=dev) for x in rect + [0.0]]))
        masks.append(mask.to(torch.uint8))
    return torch.stack(masks).cpu(), torch.stack(rows).float().cpu()


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
        raise SystemExit("perf_mask_at_box.py measures on the GPU: no device found")
    bounds = torch.tensor([[-0.07, -0.10, 0.75], [0.15, 0.06, 0.95]])
    b6 = (c_float * 6)(*bounds.reshape(-1).tolist())
    bounds_dev = bounds.cuda()
    for V, H, W in ((5, 512, 334), (1, 256, 256)):
        cams = cameras(V, H, W, bounds.mean(0))
        table = renderer.camera_table(cams, torch.device("cuda"))
        mask, out = torch.empty(V, H, W, dtype=torch.uint8, device="cuda"), torch.empty(V, 8, device="cuda")
        scratch = torch.empty(_ffi.lib.vanerf_mask_at_box_scratch(V, H, W) // 8 + 1, dtype=torch.float64, device="cuda")
        ptr = lambda t: c_void_p(t.data_ptr())  # noqa: E731

        def launches():
            _ffi.check(_ffi.lib.vanerf_mask_at_box(ptr(table), V, H, W, b6, ptr(mask), None, None, ptr(scratch), scratch.numel() * 8, ptr(out),
                                                   c_void_p(torch.cuda.current_stream().cuda_stream)))

        paths = {
            "the two launches, table on the device": launches,
            "mask_at_box(), results left on the device": lambda: mab.mask_at_box(cams, bounds, out=out),
            "mask_at_box() + read-back of the table": lambda: mab.mask_at_box(cams, bounds, out=out)[1].cpu(),
            "torch restatement + .cpu()": lambda: torch_mask_at_box(table, bounds_dev, H, W),
        }
        got_mask, got = mab.mask_at_box(cams, bounds)
        want_mask, want = paths["torch restatement + .cpu()"]()
        cover = got_mask.float().mean(dim=(1, 2)).tolist()
        print(f"V={V} {H}x{W}: box on {min(cover):.2f}-{max(cover):.2f} of the image; masks differ on {int((got_mask.cpu() != want_mask).sum())} pixels; "
              "largest |kernels - torch restatement| per slot " + " ".join(f"{e:.1e}" for e in (got.cpu() - want).abs().amax(0).tolist()))
        for fn in paths.values():  # warm-up of every shape the windows use
            for _ in range(5):
                fn()
        times = {k: [] for k in paths}
        for _ in range(a.reps):  # the paths alternate
            for k, fn in paths.items():
                times[k].append(window(fn, a.calls))
        for k, t in times.items():
            dev, host = statistics.median(x[0] for x in t), statistics.median(x[1] for x in t)
            print(f"V={V} {H}x{W}  {k:44s} {1e3 * dev:9.1f} us per call by device events (min {1e3 * min(x[0] for x in t):.1f}, max {1e3 * max(x[0] for x in t):.1f}), "
                  f"{1e3 * host:9.1f} us by the host clock; {a.reps} windows of {a.calls} calls")


if __name__ == "__main__":
    main()
