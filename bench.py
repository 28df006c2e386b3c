"""bench.py -- rendered rays/s of the VANeRF volume-rendering hot path on MI355X.

One step = one pass of the hot path over one 512x334 target view (171 008 rays, 64 coarse + 64 importance
samples per ray: the networks are evaluated on 192 points per ray, reference src/model.py:1289, 1345), with all
frame inputs already resident in HBM.  With --gpus N the rays of the view are sharded across N ranks (interleaved
rows, one process per GPU) and the fine RGB tiles are gathered with one RCCL all_gather (strong scaling: the view
is the unit of work).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times --steps steps and prints the headline (rays/s, ms_per_step).  --full adds what takes work of its own:
the per-source-frame setup time, the roofline of the dominant kernel (HIP events around it in the timed steps), the CPU baseline, the parity
leg against the oracle with its outlier check, and (--gpus N > 1) the check of the gathered image.  --dump-outputs DIR writes what the last
timed step computed as DIR/<name>.npy (float32 / float64; the inputs are seeded, so two builds can be compared output for output).

  python bench.py --gpus 1 --steps 5 --warmup 2 [--full] [--dump-outputs DIR]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FLOP_PER_SAMPLE = 2 * 143772          # 143 772 MAC per sample evaluation (V = 1)
FLOP_PER_INVALID_SAMPLE = 2 * (3072 + 22848)  # ibr_compress + TexVisFusion only: all that an invalid sample needs
# bf16x3 kernel: a block of all-invalid groups reads ibr_compress's (constant) output from LDS instead of running the layer, so those samples are
# priced WITHOUT it (the groups that sit in a block with valid samples still run it: priced low, never high)
FLOP_PER_INVALID_SAMPLE_BF16X3 = 2 * 22848
PEAK_F32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2516.8        # MI355X_MICROARCH.md: ~2.5 PF dense bf16 (16 x the fp32 matrix rate)
DEFAULT_PRECISION = "bf16x3"    # the north star asks for bf16 MFMA tiles at 1e-4 of the fp32 reference: met by the split-bf16 mode


def usable_cores():
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota (a GPU box hands each
    job a share of the host, typically 16 cores per GPU, while os.cpu_count() still reports the whole machine)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except (OSError, ValueError):
            pass
    return min(n, int(os.environ.get("VANERF_CPU_THREADS", "16")))


def cpu_baseline(sd, frame, S, rays_side):
    """The oracle (a PyTorch-CPU port of the reference renderer, same unfused op sequence) on a bounded sample of the
    same workload: a strided rays_side x rays_side grid of the 512x334 view at 64+64 samples."""
    from oracle import vanerf_oracle as orc
    W, H = frame["cam_tar"]["width"], frame["cam_tar"]["height"]
    sx, sy = W // rays_side, H // rays_side
    gy, gx = torch.meshgrid(torch.arange(rays_side) * sy + sy // 2, torch.arange(rays_side) * sx + sx // 2, indexing="ij")
    grids = torch.stack([gx, gy], -1).view(1, -1, 2)
    fr = dict(frame)
    fr["out_hw"] = (rays_side, rays_side)
    cores = usable_cores()
    os.environ["OMP_NUM_THREADS"] = str(cores)  # read by the oracle's C library (OpenMP) when it is first loaded
    torch.set_num_threads(cores)
    t0 = time.perf_counter()
    with torch.no_grad():
        out = orc.batch_render(sd, fr, 1, None, S, S, grids=grids)
    dt = time.perf_counter() - t0
    n = rays_side * rays_side
    return {"value": n / dt, "unit": "rays/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{rays_side}x{rays_side} strided rays of the 512x334 view, {S}+{S} samples/ray, {dt:.1f} s"}, out, grids


def explain_outliers(renderer, weights, fdat, frame, px, S, ref, err):
    """Every sampled pixel of the timed image that differs from the oracle by more than 1e-4 must show a FLIPPED DISCRETE DECISION at one of its
    samples (DESIGN.md section 5 ii): the HIP ray generator and torch-CPU differ in the last bit of a sample position, and the renderer's
    thresholds / arg-mins turn that into an O(0.1) change of that sample.  The same pixels are marched again with the intermediates kept and
    compared, sample by sample, with the oracle's: visibility flag (interpolated visibility >= 0.1), inside flag (sign of the mesh distance),
    validity mask, a per-sample network output that jumps by more than 1e-3 (nearest vertex / closest face / mask-tap decisions), a fine sample
    that sits elsewhere (importance sampling's cdf bin, src/model.py:1460).  Checked on every --full run, not just explained."""
    o = renderer.render_pass(weights, fdat, frame["cam_tar"], frame["bounds"], 0, 0, 1, px.shape[0], 1, S, S, pixels=px, debug=True, reuse_coarse=False)
    R = px.shape[0]
    bad = (err.max(1)[0] > 1e-4).nonzero().view(-1)
    flips = {}
    for name, part, refp, zs, zr in (("coarse", o["coarse"], ref["coarse"], o["z"].cpu(), ref["z"][0]), ("fine", o["fine"], ref["fine"], o["z_fine"].cpu(), ref["z_fine"][0])):
        Sx = zs.shape[1]
        vis = part["q_vis"].cpu().view(R, Sx).bool() != refp["q_vis"].view(R, Sx).bool()
        sdf_h, sdf_r = part["q_sdf"].cpu().view(R, Sx), refp["q_sdf"].view(R, Sx)
        inside = (sdf_h < 0) != (sdf_r < 0)
        rg_h, rg_r = part["rgba"].cpu().view(R, Sx, 5), refp["rgba"].view(R, Sx, 5)
        valid = (rg_h[..., 0] == 0) != (rg_r[..., 0] == 0)
        jump = (rg_h - rg_r).abs().max(-1)[0] > 1e-3
        moved = (zs - zr).abs() > 1e-5
        for k, m in (("visibility", vis), ("inside", inside), ("valid", valid), ("output_jump", jump), ("sample_moved", moved)):
            flips[name + "_" + k] = m.any(1)
    any_flip = torch.stack(list(flips.values())).any(0)
    unexplained = [int(i) for i in bad.tolist() if not bool(any_flip[i])]
    kinds = {k: int(v[bad].sum()) for k, v in flips.items() if int(v[bad].sum())}
    if unexplained:
        print(f"bench.py: {len(unexplained)} pixels above 1e-4 WITHOUT a flipped discrete decision: {unexplained[:10]}", file=sys.stderr, flush=True)
    return {"pixels_above_1e-4": int(bad.numel()), "pixels_above_1e-4_with_a_flipped_decision": int(bad.numel()) - len(unexplained),
            "flipped_decisions_by_kind": kinds, "pixels_with_a_flip_among_all": int(any_flip.sum())}


DUMP_MAX_BYTES = 64 << 20
DUMP_SAMPLE_RAYS = 4096  # rays whose per-sample depths are written (fixed seed)


def dump_outputs(path, image, out):
    """What the last timed step computed: `image` (the step's result, the fine RGB view (H, W, 3)) and the flat per-ray tensors render_pass
    returned.  The per-sample depths (z, z_new, z_fine: tens of MB) are written for a fixed, seeded sample of the rays (sample_rays.npy); a
    per-ray array goes at the same sample only if writing it whole would pass DUMP_MAX_BYTES.  Integer / byte outputs as float64 / float32."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    R = out["color_fine"].shape[0]
    g = torch.Generator().manual_seed(0)
    rays = torch.randperm(R, generator=g)[:min(R, DUMP_SAMPLE_RAYS)].sort()[0]
    arrays = {"image": image, "sample_rays": rays}
    for k in ("color", "depth", "alpha", "color_fine", "depth_fine", "alpha_fine", "sdf", "index", "hit", "rays_d", "cam_pos"):
        arrays[k] = out[k]
    for k in ("z", "z_new", "z_fine"):
        if out.get(k) is not None:
            arrays[k] = out[k][rays.to(out[k].device)]
    for k, v in arrays.items():
        v = v.detach().cpu()
        arrays[k] = v.double() if v.dtype in (torch.int64, torch.int32, torch.float64) else v.float()
    total = sum(v.numel() * v.element_size() for v in arrays.values())
    for k, v in arrays.items():  # too large to write whole: per-ray arrays at the sampled rays
        if total > DUMP_MAX_BYTES and k not in ("image", "sample_rays", "cam_pos") and v.shape[0] == R:
            total -= v.numel() * v.element_size()
            arrays[k] = v[rays]
            total += arrays[k].numel() * arrays[k].element_size()
    if total > DUMP_MAX_BYTES:  # (only at very large views) the image at a seeded sample of its pixels as well
        pix = arrays["image"].reshape(-1, arrays["image"].shape[-1])
        arrays["image_pixels"] = torch.randperm(pix.shape[0], generator=g)[:DUMP_SAMPLE_RAYS].sort()[0]
        arrays["image"] = pix[arrays["image_pixels"]]
        arrays["image_pixels"] = arrays["image_pixels"].double()
    for k, v in arrays.items():
        np.save(os.path.join(path, k + ".npy"), v.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=334)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for --gpus > 1 (nccl = RCCL; gloo only for single-GPU rehearsals)")
    ap.add_argument("--precision", choices=["fp32", "bf16x3"], default=DEFAULT_PRECISION,
                    help="arithmetic of the per-sample dense layers: fp32 MFMA, or bf16 MFMA on split (hi + lo) operands with fp32 accumulate")
    ap.add_argument("--cpu-rays-side", type=int, default=64, help="--full: cpu_baseline sample: side of the strided ray grid (0 = skip)")
    ap.add_argument("--full", action="store_true",
                    help="also the per-source-frame setup time, roofline, CPU baseline, parity vs the oracle and (--gpus N > 1) the gathered-image check")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if os.environ.get("VANERF_SHARE_GPU0"):  # rehearsal of the N-rank flow on a one-GPU box (with --backend gloo)
        local = 0
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(args.backend)

    from vanerf_amd import renderer, synth
    from vanerf_amd.parallel import shard_rows

    S, H, W = args.samples, args.height, args.width
    sd = synth.make_full_weights(0)
    frame = synth.make_frame(seed=11, tar_h=H, tar_w=W, orbit_deg=15.0)
    fd = synth.to_device(frame, "cuda")
    sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
    def frame_setup():
        return renderer.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])

    fdat = frame_setup()  # (the first construction of a process also pays the library's one-time solver selection)
    # Per-source-frame setup (vertex tables, TexVisFusion's global vertex feature, visibility raster, mesh clusters): reported beside the step,
    # outside `value` -- in a data set where every target view has its own source frame (BASELINE config 2) a view costs step + this.
    torch.cuda.synchronize()
    if args.full:
        fs = []
        for _ in range(3):
            t0 = time.perf_counter()
            frame_setup()
            torch.cuda.synchronize()
            fs.append((time.perf_counter() - t0) * 1e3)  # wall: includes the host-side table building between the launches
        frame_setup_ms = min(fs)
    weights = renderer.PackedWeights(sd, mode=args.precision)
    bf = args.precision == "bf16x3"
    peak = PEAK_BF16_MFMA_TFLOPS if bf else PEAK_F32_MFMA_TFLOPS
    rows = shard_rows(H, world, rank)  # (y0, step, ny): interleaved rows -> even load
    events = []

    def step(record=None):
        out = renderer.render_pass(weights, fdat, frame["cam_tar"], frame["bounds"], 0, rows[0], 1, W, rows[2], S, S,
                                   kernel_events=record, y_step=rows[1], y_block=rows[3])
        tile = out["color_fine"]
        if world > 1:
            if args.backend == "nccl":
                full = torch.empty(world * tile.shape[0], 3, device=tile.device)
                dist.all_gather_into_tensor(full, tile)
            else:  # gloo rehearsal: host-staged gather
                parts = [torch.empty_like(tile, device="cpu") for _ in range(world)]
                dist.all_gather(parts, tile.cpu())
                full = torch.cat(parts, 0).to(tile.device)
            return full, out
        return tile, out

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    short0 = weights.short_groups() if args.full else None
    record = events if args.full else None  # HIP events around the dominant kernel: the roofline's figures
    t0 = time.perf_counter()
    for i in range(args.steps):
        img, out = step(record)
        if i < args.steps - 1:
            out = None  # only the last step's outputs are held (--dump-outputs): a step allocates beside the same live tensors as before
    barrier()
    dt = time.perf_counter() - t0
    t = torch.tensor([dt], device="cuda" if args.backend == "nccl" else "cpu", dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    if args.dump_outputs and rank == 0:
        from vanerf_amd.parallel import deinterleave
        dump_outputs(args.dump_outputs, deinterleave(img, H, W, world), out)
    del out

    rays_total = H * W
    result = {
        "metric": "rendered rays/sec (64 samples/ray) + PSNR vs ref, 512x334 view", "value": rays_total * args.steps / dt, "unit": "rays/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "bf16x3 (bf16 MFMA on hi+lo split operands, f32 accumulate; per-sample outputs within 3.3e-5 of the f32 kernel)" if bf else "f32", "data": "synthetic",
    }
    if args.full:
        result.update({"frame_setup_ms": frame_setup_ms, "ms_per_view_incl_frame": 1e3 * dt / args.steps + frame_setup_ms})
    result["config"] = {"workload": f"configs/vanerf.json eval view {H}x{W}, {S} coarse + {S} importance samples/ray, "
                                    "two-hand mesh 1558 verts / 3108 faces, 1 source view 256x256, random trained-like weights",
                        "network_evaluations_per_ray": {"reference": 3 * S, "executed": 2 * S,
                                                        "note": "fine composite re-uses the coarse evaluations (bit-identical, tests/test_hip_parity.py)"},
                        "rays": rays_total, "parallelism": f"rays{world}" if world > 1 else "single"}

    if args.full:
        # dominant kernel: query_kernel, two launches per step (R*S coarse samples, R*S new importance samples).
        # Algorithmic FLOPs of a launch = 287 544 per sample, except that a 32-sample group whose samples ALL miss the source view
        # needs only the colour branch (51 840 FLOP per sample): the kernel counts those groups and they are priced at that figure,
        # so skipped work never inflates `achieved`.
        k_ms = [e0.elapsed_time(e1) for e0, e1, _ in events]
        k_samples = [n for _, _, n in events]
        kern_s = sum(k_ms) / 1e3
        short_samples = 32 * (weights.short_groups() - short0)
        flops = (sum(k_samples) - short_samples) * FLOP_PER_SAMPLE + short_samples * (FLOP_PER_INVALID_SAMPLE_BF16X3 if bf else FLOP_PER_INVALID_SAMPLE)
        achieved = flops / kern_s / 1e12
        # HBM bytes per launch.  NOT measured in this run (counters need a rocprofv3 --pmc pass of their own): a static figure from the committed
        # PMC passes of this kernel, scaled by samples per launch; FETCH_SIZE doubled per MI355X_MICROARCH.md (gfx950 tallies 128-B requests at 64 B).
        traffic, traffic_src = None, None
        try:
            pm = json.load(open(os.path.join(REPO, "profiles", "r03_query_kernel_traffic.json")))
            per = pm["per_kernel"]["query_kernel<1>" if bf else "query_kernel<0>"]
            traffic = (2.0 * per["fetch_kb"] + per["write_kb"]) * 1024.0 / pm["samples"] * (sum(k_samples) / len(events))
            traffic_src = "static: 2 x FETCH_SIZE + WRITE_SIZE of profiles/r03_query_kernel_traffic.json (rocprofv3 --pmc, one counter per pass), not measured in this run"
        except (OSError, KeyError, ValueError):
            pass
        result["roofline"] = {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                              "traffic": traffic, "traffic_unit": "HBM bytes per launch", "traffic_source": traffic_src, "kernel": "query_kernel<1> (v_mfma_f32_32x32x16_bf16, 3 MFMA FLOPs executed per algorithmic FLOP)" if bf else "query_kernel<0> (v_mfma_f32_32x32x2_f32)", "launches": len(events),
                              "avg_launch_ms": statistics.mean(k_ms), "kernel_ms_per_step": sum(k_ms) / args.steps,
                              "flop_per_launch_avg": flops / len(events), "samples_per_launch_avg": sum(k_samples) / len(events),
                              "all_invalid_group_fraction": short_samples / max(1, sum(k_samples))}
    if args.full and rank == 0 and world == 1 and args.cpu_rays_side > 0:
        base, ref, grids = cpu_baseline(sd, frame, S, args.cpu_rays_side)
        result["cpu_baseline"] = base
        # PSNR of the rendered view against the CPU oracle on the sampled pixels (src/evaluator.py:16-19)
        from oracle import vanerf_oracle as orc
        idx = (grids[0, :, 0] + grids[0, :, 1] * W).long()
        got = img.view(H * W, 3)[idx.cuda()].cpu()
        want = ref["tex_fg_fine"][0].reshape(3, -1).t()
        err = (got - want).abs()
        result["parity"] = {"psnr_db": orc.psnr(got, want), "max_abs_err": err.max().item(),
                            "frac_pixels_above_1e-4": (err.max(1)[0] > 1e-4).float().mean().item(), "pixels": int(idx.numel())}
        # the same pixels once more with the oracle's own rays and depths injected (identical sample positions on both sides): what is left of
        # the difference when the ray generator's last bit is taken out (tests/test_hip_injected.py holds this to 1e-4 with no allowance)
        px = grids[0].to(torch.int32).cuda().contiguous()
        inj = {"rays_d": ref["cam_rays"][0].contiguous().cuda(), "cam_pos": ref["cam_pos"].reshape(3).contiguous().cuda(),
               "z": ref["z"][0].contiguous().cuda(), "z_fine": ref["z_fine"][0].contiguous().cuda()}
        oi = renderer.render_pass(weights, fdat, frame["cam_tar"], frame["bounds"], 0, 0, 1, px.shape[0], 1, S, S, pixels=px, inject=inj)
        erri = (oi["color_fine"].cpu() - want).abs()
        result["parity"].update({"max_abs_err_same_rays": erri.max().item(), "frac_pixels_above_1e-4_same_rays": (erri.max(1)[0] > 1e-4).float().mean().item(),
                                 "note": "first three figures: the timed image (HIP ray generator) vs the oracle; *_same_rays: the oracle's rays and depths injected"})
        result["parity"].update(explain_outliers(renderer, weights, fdat, frame, px, S, ref, err))
        result["speedup_vs_cpu"] = result["value"] / base["value"]
    if args.full and world > 1:  # the gathered, de-interleaved image must contain this rank's own rows at their place
        from vanerf_amd.parallel import deinterleave, rank_rows
        full_img = deinterleave(img, H, W, world)
        own = step()[0]
        own = own.view(world, rows[2], W, 3)[rank]
        rr = rank_rows(H, world, rank)
        keep = rr < H  # (a height that is not a multiple of 8 * world is padded below the image)
        assert torch.equal(full_img[rr[keep].to(full_img.device)], own[keep.to(own.device)]), "gathered image does not contain this rank's rows"
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
