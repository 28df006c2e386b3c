"""The surface maps of the baked volume (vanerf_amd/baked.py, csrc/volume_surface.hip) on the synthetic two-hand frame, from
device events, each figure the median of `--reps` windows after a warm-up of every shape: section 0g's orbit (20 views of 256 x 256, one
group) at 64, 128 and 256 grid points along the longest axis and 64, 128 and 256 samples per ray.  One row per shape:
  * render_volume_surface (the ray setup and vanerf_volume_surface) per `refine`, beside render_volume (the ray setup and the composite
    march) on the same volume and cameras;
  * the two marches alone on rays set up once (march_surface, march_volume), which is the kernels' own time plus a launch;
  * render_baked_surface_views (the maps turned into frames by elementwise torch ops), per view.
Also the share of the pixels that find a surface.
Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf_baked_surface.py (volume_surface_kernel, volume_render_kernel)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vanerf_amd import baked, synth  # noqa: E402
from vanerf_amd import renderer as R  # noqa: E402
from vanerf_amd.config import default_config  # noqa: E402
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
    return statistics.median(window(fn, calls) for _ in range(reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--refine", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_baked_surface.py measures on the GPU: no device found")
    torch.manual_seed(0)
    cfg = default_config()
    cfg["models"]["VANeRF"]["mfma_precision"] = a.precision
    net = VANeRF(cfg).cuda().eval()
    net.load_state_dict(synth.make_full_weights(0), strict=False)
    frame_cpu = synth.make_frame(seed=3, tar_h=a.image, tar_w=a.image)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    headpose = torch.eye(4)
    headpose[:3, 3] = frame_cpu["targets"]["vert_world"][0].mean(0)
    cams = [camera_to_cam_tar(c) for c in get_360cameras(headpose[:3, :4].cuda(), 4.0 * a.image, 1.0, 1.0, a.image, a.image, 0.71, 1.42, n_frames=a.views)]
    V = a.views
    print(f"{a.image} x {a.image}, one group of {V} orbit views [{a.precision}]; ms per VIEW, median of {a.reps} windows of {a.calls} calls", flush=True)
    with torch.no_grad():
        for n in a.sizes:
            vol = baked.bake_volume(net, trb, resolution=n)
            nx, ny, nz = vol.dims
            print(f"resolution {n}: grid {nx} x {ny} x {nz}, {16 * nx * ny * nz / 2 ** 20:.1f} MiB", flush=True)
            for S in a.samples:
                rays = R.ray_setup_views(cams, vol.bounds, 0, 0, 1, a.image, a.image, S)
                args = (vol, rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
                t_colour = median_ms(lambda: baked.render_volume(vol, cams, S), a.calls, a.reps) / V
                k_colour = median_ms(lambda: baked.march_volume(*args, row_rays=a.image), a.calls, a.reps) / V
                found = baked.march_surface(*args, row_rays=a.image)[3]
                row = f"  resolution {n:3d}, {S:3d} samples: render_volume {t_colour:7.4f} (march alone {k_colour:7.4f});"
                for refine in a.refine:
                    t = median_ms(lambda: baked.render_volume_surface(vol, cams, S, refine=refine), a.calls, a.reps) / V
                    k = median_ms(lambda: baked.march_surface(*args, refine=refine, row_rays=a.image), a.calls, a.reps) / V
                    row += f" surface refine={refine} {t:7.4f} (march alone {k:7.4f});"
                t_img = median_ms(lambda: baked.render_baked_surface_views(vol, cams, S), max(2, a.calls // 4), a.reps) / V
                print(row + f" shaded frames (refine=1) {t_img:7.4f}; found on {100.0 * float((found != 0).float().mean()):.1f} % of the pixels", flush=True)
            del vol


if __name__ == "__main__":
    main()
