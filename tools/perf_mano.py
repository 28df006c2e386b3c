"""MANO skinning (vanerf_amd/mano.py, csrc/mano_skin.hip) for two hands, from device events, each figure the median of
`--reps` windows of `--calls` calls after a warm-up of every shape.  Per batch size P (`--poses`, default 1 64 1024):
  * mano.skin_two_hands into preallocated outputs: milliseconds per call and microseconds per pose;
  * a straight PyTorch restatement of the definition on the same device in fp32 (batched matmuls, the chain joint by joint, the seal and the
    concatenation of the hands): what a caller with smplx would run on the GPU -- nothing in this project precedes the HIP path;
  * the bytes the kernels must move -- the packed fp32 tables once per hand, parameters in, workspace out and in, vertices and joints out --
    the rate that implies, and its share of the HBM bandwidth a copy reaches (6.3 TB/s) and of the L2's (34.5 TB/s); and what the vertex
    kernel actually asks of the L2: the tables once per group of vanerf_mano_poses_per_lane poses.
The count of poses a lane carries is a build constant: time a library built with VANERF_HIPCC_FLAGS=-DMANO_POSES_PER_LANE=n (vanerf_amd.build,
out=) by naming it in VANERF_HIP_LIB.  Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf_mano.py."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vanerf_amd import mano, synth  # noqa: E402
from vanerf_amd._ffi import LIB_PATH, lib  # noqa: E402

HBM_COPY, L2_RATE = 6.3e12, 34.5e12  # bytes per second: a float4 copy through HBM, and the aggregate L2


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


def rodrigues(r):
    angle = (r + 1e-8).norm(dim=-1, keepdim=True)
    d = r / angle
    z = torch.zeros_like(d[..., 0])
    K = torch.stack([z, -d[..., 2], d[..., 1], d[..., 2], z, -d[..., 0], -d[..., 1], d[..., 0], z], -1).view(*r.shape[:-1], 3, 3)
    return torch.eye(3, device=r.device) + torch.sin(angle)[..., None] * K + (1 - torch.cos(angle))[..., None] * (K @ K)


def torch_hand(m, pose, betas, trans, ring):
    """The definition in PyTorch, fp32: m a dict of device tensors under smplx's names, parents a list."""
    P, nj, nv = pose.shape[0], m["J_regressor"].shape[0], m["v_template"].shape[0]
    full = torch.cat([pose[:, :3], pose[:, 3:] + m["hands_mean"]], 1)
    v_shaped = m["v_template"] + torch.einsum("vkb,pb->pvk", m["shapedirs"], betas)
    J = torch.einsum("jv,pvk->pjk", m["J_regressor"], v_shaped)
    R = rodrigues(full.view(P, nj, 3))
    feat = (R[:, 1:] - torch.eye(3, device=pose.device)).reshape(P, -1)
    v_posed = v_shaped + (feat @ m["posedirs"]).view(P, nv, 3)
    rel = J.clone()
    rel[:, 1:] = J[:, 1:] - J[:, m["parents"][1:]]
    L = torch.cat([torch.cat([R, rel[..., None]], -1), torch.tensor([0.0, 0, 0, 1], device=pose.device).expand(P, nj, 1, 4)], 2)
    G = [L[:, 0]]
    for j in range(1, nj):
        G.append(G[m["parents"][j]] @ L[:, j])
    G = torch.stack(G, 1)
    A = G[:, :, :3, :].clone()
    A[..., 3] = A[..., 3] - (G[:, :, :3, :3] @ J[..., None])[..., 0]
    T = torch.einsum("vj,pjrc->pvrc", m["weights"], A)
    verts = (T[..., :3] @ v_posed[..., None])[..., 0] + T[..., 3] + trans[:, None]
    return torch.cat([verts, verts[:, ring].mean(1, keepdim=True)], 1), G[:, :, :3, 3] + trans[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true", help="time the HIP path only (for comparing builds)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_mano.py measures on the GPU: no device found")
    rings = (mano.MANO_SEAL_RING, mano.MANO_SEAL_RING[::-1])
    arrays = [synth.mano_like_model(1 + h) for h in range(2)]
    hands = [mano.ManoModel.from_arrays(**arrays[h], seal_ring=rings[h]) for h in range(2)]
    tens = [dict({k: torch.from_numpy(v).cuda() for k, v in arrays[h].items() if k != "parents"}, parents=[int(p) for p in arrays[h]["parents"]]) for h in range(2)]
    ring_t = [torch.tensor(r, device="cuda") for r in rings]
    L = int(lib.vanerf_mano_poses_per_lane())
    nv, nj, nb = hands[0].nv, hands[0].nj, hands[0].nb
    table_bytes = 4 * nv * (3 + 3 * nb + 27 * (nj - 1) + nj)  # the fp32 tables of one hand
    print(f"library {LIB_PATH}: {L} poses per lane; two hands of nv={nv} nj={nj} nb={nb}; fp32 tables {table_bytes / 1e6:.2f} MB per hand; "
          f"{a.reps} windows of {a.calls} calls", flush=True)
    fmt = lambda t: f"{t[0]:8.4f} ms (min {t[1]:.4f}, max {t[2]:.4f})"  # noqa: E731
    rng = np.random.default_rng(0)
    for P in a.poses:
        pose = torch.from_numpy((rng.standard_normal((P, 2, nj * 3)) * 0.5).astype(np.float32)).cuda()
        betas = torch.from_numpy(rng.standard_normal((P, 2, nb)).astype(np.float32)).cuda()
        trans = torch.from_numpy(rng.uniform(-1, 1, (P, 2, 3)).astype(np.float32)).cuda()
        out = torch.empty(P, 2 * (nv + 1), 3, device="cuda"), torch.empty(P, 2 * nj, 3, device="cuda")
        t = median_ms(lambda: mano.skin_two_hands(*hands, pose, betas, trans, out=out), a.calls, a.reps)
        ws = 4 * (nj * 12 + (nj - 1) * 9)
        must = 2 * table_bytes + P * 2 * (4 * (nj * 3 + nb + 3) + 2 * ws + 4 * 3 * (nv + 1) + 4 * 3 * nj)
        asked = 2 * table_bytes * ((P + L - 1) // L) + must - 2 * table_bytes
        rate = must / (t[0] * 1e-3)
        print(f"P={P:5d}: skin_two_hands {fmt(t)} per call, {1e3 * t[0] / P:9.3f} us per pose; must move {must / 1e6:8.2f} MB = {rate / 1e9:7.1f} GB/s, "
              f"{100 * rate / HBM_COPY:5.2f} % of HBM copy rate, {100 * rate / L2_RATE:5.2f} % of L2; the vertex kernel asks the L2 for {asked / 1e6:8.1f} MB "
              f"= {asked / (t[0] * 1e-3) / 1e12:5.2f} TB/s", flush=True)
        if a.no_torch:
            continue

        def by_torch():
            vj = [torch_hand(tens[h], pose[:, h], betas[:, h], trans[:, h], ring_t[h]) for h in range(2)]
            return torch.cat([vj[0][0], vj[1][0]], 1), torch.cat([vj[0][1], vj[1][1]], 1)

        with torch.no_grad():
            tt = median_ms(by_torch, max(1, a.calls // 4), a.reps)
            ref = by_torch()
        worst = max(float((ref[0] - out[0]).abs().max()), float((ref[1] - out[1]).abs().max()))
        print(f"P={P:5d}: PyTorch fp32 restatement {fmt(tt)} per call, {1e3 * tt[0] / P:9.3f} us per pose: {tt[0] / t[0]:6.1f} x the HIP path; "
              f"largest difference between the two {worst:.2e}", flush=True)


if __name__ == "__main__":
    main()
