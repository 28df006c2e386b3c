"""The baked volume (vanerf_amd/baked.py, csrc/volume_render.hip) on the synthetic two-hand frame, from device events, each
figure the median of `--reps` windows after a warm-up of every shape:
  * bake_volume at 64, 128 and 256 grid points along the longest axis (field_on_grid with colours in slabs, then vanerf_volume_pack);
  * render_baked_views per view at 256 x 256 for 64, 128 and 256 samples per ray and groups of 1, 8 and 20 views of a get_360cameras orbit
    (one ray setup and one march per group);
  * the same cameras through VANeRF.render_pifu_nerf_views, the exact pass (64 + 64 samples);
  * per resolution, the PSNR of the baked colour against the exact pass's fine colour over the mask_at_box pixels of the 20 views.
Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf_baked.py (volume_render_kernel, volume_pack_kernel)."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vanerf_amd import baked, synth  # noqa: E402
from vanerf_amd.config import default_config  # noqa: E402
from vanerf_amd.mask_at_box import mask_at_box  # noqa: E402
from vanerf_amd.model import VANeRF, get_360cameras  # noqa: E402
from vanerf_amd.novel_views import camera_to_cam_tar  # noqa: E402


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def median_ms(fn, calls, reps):
    fn()  # warm-up of this shape
    t = [window(fn, calls) for _ in range(reps)]
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 8, 20])
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_baked.py measures on the GPU: no device found")
    torch.manual_seed(0)
    cfg = default_config()
    cfg["models"]["VANeRF"]["mfma_precision"] = a.precision
    net = VANeRF(cfg).cuda().eval()
    net.load_state_dict(synth.make_full_weights(0), strict=False)
    frame_cpu = synth.make_frame(seed=3, tar_h=a.image, tar_w=a.image)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    headpose = torch.eye(4)
    headpose[:3, 3] = frame_cpu["targets"]["vert_world"][0].mean(0)
    n_views = max(a.groups)
    cams = [camera_to_cam_tar(c) for c in get_360cameras(headpose[:3, :4].cuda(), 4.0 * a.image, 1.0, 1.0, a.image, a.image, 0.71, 1.42, n_frames=n_views)]
    kw = cfg["models"]["VANeRF"]["dr_kwargs"]
    fmt = lambda t: f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"  # noqa: E731

    def exact(group):
        return net.render_pifu_nerf_views(trb["im"], trb["cam"], trb["hand_type"], trb["targets"], group, sp_data=dict(trb["sp_data"]), fine=True, uniform=True,
                                          sample_per_ray_c=kw["sample_per_ray_c"], sample_per_ray_f=kw["sample_per_ray_f"],
                                          src_foreground_mask=trb["src_foreground_mask"], bounds=trb["dr_data"]["bounds"])

    with torch.no_grad():
        mask, _ = mask_at_box(cams, trb["dr_data"]["bounds"])
        want = torch.stack([o["tex_fg_fine"].clamp(0.0, 1.0) for g0 in range(0, n_views, 8) for o in exact(cams[g0:g0 + 8])])  # (V, 3, H, W)
        m = mask.bool()[:, None].expand_as(want)
        print(f"{a.image} x {a.image}, {n_views} orbit views [{a.precision}]; mask_at_box covers {100.0 * float(mask.float().mean()):.1f} % of the pixels")
        for g in a.groups:
            t = median_ms(lambda: exact(cams[:g]), max(1, 8 // g), a.reps)
            print(f"exact pass ({kw['sample_per_ray_c']} + {kw['sample_per_ray_f']} samples), group of {g:2d}: {fmt(t)} per group, {t[0] / g:8.3f} ms per view", flush=True)
        for n in a.sizes:
            vol = baked.bake_volume(net, trb, resolution=n)
            t = median_ms(lambda: baked.bake_volume(net, trb, resolution=n), 3 if n >= 256 else 10, a.reps)
            nx, ny, nz = vol.dims
            print(f"bake_volume, resolution {n}: grid {nx} x {ny} x {nz}, {16 * nx * ny * nz / 2 ** 20:7.1f} MiB: {fmt(t)}   {nx * ny * nz / t[0] / 1e3:8.1f} M points/s", flush=True)
            for S in a.samples:
                got = torch.stack([o["tex_fg"].clamp(0.0, 1.0) for g0 in range(0, n_views, 8) for o in baked.render_baked_views(vol, cams[g0:g0 + 8], S)])
                mse = float(((got - want) ** 2)[m].mean())
                print(f"  resolution {n}, {S:3d} samples: PSNR against the exact pass over the mask_at_box pixels {-10.0 * math.log10(max(mse, 1e-30)):6.2f} dB")
                for g in a.groups:
                    t = median_ms(lambda: baked.render_baked_views(vol, cams[:g], S), max(2, 40 // g), a.reps)
                    print(f"  resolution {n}, {S:3d} samples, group of {g:2d}: {fmt(t)} per group, {t[0] / g:8.3f} ms per view", flush=True)
            del vol


if __name__ == "__main__":
    main()
