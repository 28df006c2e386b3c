"""The learned surface (vanerf_amd/surface.py, csrc/surface.hip) on the synthetic two-hand frame at 64^3, 128^3 and 256^3 grid points over the
frame's bounds: the time of field_on_grid (grid points, mesh query, validity partition, per-sample networks, field values, in slabs) and of
the extraction (vanerf_surface_count, the read of the two counts, vanerf_surface_emit) from device events, each the median of `--reps`
windows; the two launches of the count and the launch of the emit also alone, on buffers that are already there.  Printed beside them: the
mesh's size and the bytes each march kernel has to move at least (computed from the shapes: f once, a word per point written by the count
and read by the emit, 12 bytes of rgb per end of a crossed edge, the mesh itself), over its time, as a share of the HBM rate in `--hbm-gbs`.
Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf_surface.py (sf_count_kernel, sf_scan_kernel, sf_emit_kernel,
grid_points_kernel, field_values_kernel beside the mesh query's and the per-sample kernels).
--register times the registration of the MANO mesh instead (surface.register_surface, csrc/surface_lines.hip): the whole
call at 9 samples and 4 refinements, and vanerf_line_bracket alone on `--lines` random lines of 128 samples with rgb (the size it is written
for), over the bytes it has to move: f and the 64-byte record per line (the rgb of one pair per line is read beside them)."""
import argparse
import os
import statistics
import sys
from ctypes import c_void_p

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vanerf_amd import _ffi, renderer, surface, synth  # noqa: E402


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
    t = [window(fn, calls) for _ in range(reps)]
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM rate the shares are taken of, GB/s")
    ap.add_argument("--register", action="store_true", help="time register_surface and vanerf_line_bracket instead of the grid sizes")
    ap.add_argument("--lines", type=int, default=200000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_surface.py measures on the GPU: no device found")
    sd = synth.make_full_weights(0)
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    fd = synth.to_device(frame, "cuda")
    sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
    fdat = renderer.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
    w = renderer.PackedWeights(sd, mode=a.precision)
    lib, ptr = _ffi.lib, (lambda t: None if t is None else c_void_p(t.data_ptr()))
    fmt = lambda t: f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"  # noqa: E731
    if a.register:
        register = lambda: surface.register_surface(w, fdat, band=0.004, samples=9, refine=4)  # noqa: E731
        reg = register()
        t_reg = median_ms(register, 10, a.reps)
        print(f"register_surface [{a.precision}], 9 samples, 4 refinements: {fmt(t_reg)}   {int(reg['found'].sum())} of {len(reg['found'])} vertices found")
        K, n = 128, a.lines
        g = torch.Generator(device="cuda").manual_seed(0)
        f = torch.randn(n, K, device="cuda", generator=g)
        rgb = torch.rand(n, K, 3, device="cuda", generator=g)
        bracket = lambda: surface.line_bracket(f, -0.5, 1.0 / (K - 1), 0.0, rgb)  # noqa: E731
        bracket()
        t_br = median_ms(bracket, 50, a.reps)
        b_br = 4 * n * K + 64 * n
        print(f"vanerf_line_bracket, {n} lines x {K} samples: {fmt(t_br)}   {b_br / 1e6:9.1f} MB -> {b_br / t_br[0] / 1e6:8.1f} GB/s, "
              f"{100.0 * b_br / t_br[0] / 1e6 / a.hbm_gbs:5.1f} % of {a.hbm_gbs:.0f} GB/s", flush=True)
        return
    for n in a.sizes:
        dims = (n, n, n)
        origin, spacing, _ = surface.grid_spec(frame["bounds"], dims=dims)
        field = lambda: surface.field_on_grid(w, fdat, frame["bounds"], dims=dims, want_rgb=True)  # noqa: E731
        f, rgb = field()
        extract = lambda: surface.march(f, origin, spacing, 0.0, rgb)  # noqa: E731
        verts, faces, cols = extract()
        nv, nt = len(verts), len(faces)
        scratch = torch.empty(lib.vanerf_surface_scratch(n, n, n) // 8 + 2, dtype=torch.float64, device="cuda")
        counts = torch.empty(2, dtype=torch.int64, device="cuda")
        st = lambda: c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

        def count():
            _ffi.check(lib.vanerf_surface_count(ptr(f), n, n, n, 0.0, ptr(scratch), scratch.numel() * 8, ptr(counts), st()))

        def emit():
            _ffi.check(lib.vanerf_surface_emit(ptr(f), ptr(rgb), surface._f3(origin), surface._f3(spacing), n, n, n, 0.0, ptr(scratch), scratch.numel() * 8,
                                               nv, nt, ptr(verts), ptr(cols), ptr(faces), nv, nt, st()))

        count()
        assert counts.tolist() == [nv, nt]
        for fn in (field, extract, count, emit):  # warm-up of every shape the windows use
            fn()
        calls = 3 if n >= 256 else 10
        t_field = median_ms(field, calls, a.reps)
        t_extract = median_ms(extract, calls, a.reps)
        t_count = median_ms(count, 10 * calls, a.reps)
        t_emit = median_ms(emit, 10 * calls, a.reps)
        N = n ** 3
        b_count = 4 * N + 4 * N                                        # f read, the word per point written (block totals: negligible)
        b_emit = 4 * N + 4 * N + 24 * nv + 24 * nv + 12 * nt           # f, the words, rgb at both ends, verts + colors, tris
        print(f"{n}^3 [{a.precision}]: {nv} vertices, {nt} triangles")
        print(f"{n}^3  field_on_grid with rgb            {fmt(t_field)}   {N / t_field[0] / 1e3:8.1f} M points/s")
        print(f"{n}^3  extraction (count, read, emit)    {fmt(t_extract)}   {100.0 * t_extract[0] / t_field[0]:6.2f} % of field_on_grid")
        print(f"{n}^3  vanerf_surface_count (2 launches) {fmt(t_count)}   {b_count / 1e6:9.1f} MB -> {b_count / t_count[0] / 1e6:8.1f} GB/s, "
              f"{100.0 * b_count / t_count[0] / 1e6 / a.hbm_gbs:5.1f} % of {a.hbm_gbs:.0f} GB/s")
        print(f"{n}^3  vanerf_surface_emit  (1 launch)   {fmt(t_emit)}   {b_emit / 1e6:9.1f} MB -> {b_emit / t_emit[0] / 1e6:8.1f} GB/s, "
              f"{100.0 * b_emit / t_emit[0] / 1e6 / a.hbm_gbs:5.1f} % of {a.hbm_gbs:.0f} GB/s", flush=True)


if __name__ == "__main__":
    main()
