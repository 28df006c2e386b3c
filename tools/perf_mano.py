"""MANO skinning (vanerf_amd/mano.py, csrc/mano_skin.hip) for two hands, from device events, each figure the median of
`--reps` windows of `--calls` calls after a warm-up of every shape.  Per batch size P (`--poses`, default 1 64 1024):
  * mano.skin_two_hands into preallocated outputs: milliseconds per call and microseconds per pose;
  * a straight PyTorch restatement of the definition on the same device in fp32 (batched matmuls, the chain joint by joint, the seal and the
    concatenation of the hands): what a caller with smplx would run on the GPU -- nothing in this project precedes the HIP path;
  * the bytes the kernels must move -- the packed fp32 tables once per hand, parameters in, workspace out and in, vertices and joints out --
    the rate that implies, and its share of the HBM bandwidth a copy reaches (6.3 TB/s) and of the L2's (34.5 TB/s); and what the vertex
    kernel actually asks of the L2: the tables once per group of vanerf_mano_poses_per_lane poses.
The count of poses a lane carries is a build constant: time a library built with VANERF_HIPCC_FLAGS=-DMANO_POSES_PER_LANE=n (vanerf_amd.build,
out=) by naming it in VANERF_HIP_LIB.  Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf_mano.py.
`--backward` adds, per P: the backward alone (two vanerf_mano_skin_backward calls into preallocated gradients), and
skin_two_hands under autograd with torch.autograd.grad for given upstream gradients of the vertices and joints -- forward + backward -- against
the same of the PyTorch fp32 restatement, with the largest difference between the two sets of gradients relative to each gradient's largest
value.  `--fit` adds mano.fit_two_hands at `--fit-steps` steps from a tracking start against the same count of steps of torch.optim.Adam on
the restatement (one loss for both hands), per call and per step.  `--lm` adds, per P: one vanerf_mano_skin_normal call
per hand (two calls) and one vanerf_mano_lm_solve call per hand, and mano.fit_two_hands_lm at its default iterations next to mano.fit_two_hands at
300 steps from the same tracking start, each with the worst rms over poses and hands."""
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


def torch_two_hands(tens, ring_t, pose, betas, trans):
    vj = [torch_hand(tens[h], pose[:, h], betas[:, h], trans[:, h], ring_t[h]) for h in range(2)]
    return torch.cat([vj[0][0], vj[1][0]], 1), torch.cat([vj[0][1], vj[1][1]], 1)


def backward_rows(a, P, hands, tens, ring_t, pose, betas, trans, fmt):
    nv, nj = hands[0].nv, hands[0].nj
    gen = torch.Generator(device="cuda").manual_seed(1)
    gv, gj = torch.randn(P, 2 * (nv + 1), 3, device="cuda", generator=gen), torch.randn(P, 2 * nj, 3, device="cuda", generator=gen)
    grads = [torch.empty_like(t) for t in (pose, betas, trans)]

    def backward_alone():
        for h in range(2):
            mano._skin_backward(hands[h], pose[:, h], betas[:, h], False, True, gv[:, (nv + 1) * h:(nv + 1) * (h + 1)], gj[:, nj * h:nj * (h + 1)],
                                out=[g[:, h] for g in grads])

    leaves = [t.clone().requires_grad_() for t in (pose, betas, trans)]
    by_hip = lambda: torch.autograd.grad(mano.skin_two_hands(*hands, *leaves), leaves, (gv, gj))  # noqa: E731
    by_torch = lambda: torch.autograd.grad(torch_two_hands(tens, ring_t, *leaves), leaves, (gv, gj))  # noqa: E731
    tb, th = median_ms(backward_alone, a.calls, a.reps), median_ms(by_hip, a.calls, a.reps)
    print(f"P={P:5d}: backward alone {fmt(tb)} per call, {1e3 * tb[0] / P:9.3f} us per pose; skin_two_hands forward + backward through autograd {fmt(th)}, "
          f"{1e3 * th[0] / P:9.3f} us per pose", flush=True)
    if a.no_torch:
        return
    tt = median_ms(by_torch, max(1, a.calls // 4), a.reps)
    worst = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(by_hip(), by_torch()))
    print(f"P={P:5d}: PyTorch fp32 forward + backward {fmt(tt)} per call, {1e3 * tt[0] / P:9.3f} us per pose: {tt[0] / th[0]:6.1f} x the HIP path; "
          f"largest difference between the gradients, relative to the largest of each, {worst:.2e}", flush=True)


def fit_rows(a, P, hands, tens, ring_t, pose, betas, trans, fmt):
    steps, n = a.fit_steps, hands[0].nv + 1
    with torch.no_grad():
        target = mano.skin_two_hands(*hands, pose, betas, trans)[0]
    gen = torch.Generator(device="cuda").manual_seed(9)
    init = (pose + 0.2 * torch.randn(pose.shape, device="cuda", generator=gen), torch.zeros_like(betas),
            trans + 0.02 * torch.randn(trans.shape, device="cuda", generator=gen))
    tf = median_ms(lambda: mano.fit_two_hands(*hands, target, init=init, steps=steps), max(1, a.calls // 10), a.reps)
    rms = mano.fit_two_hands(*hands, target, init=init, steps=300)["rms"]
    print(f"P={P:5d}: fit_two_hands, {steps} steps {fmt(tf)} per call, {1e3 * tf[0] / steps:8.2f} us per step; 300 steps from 0.2 rad / 2 cm off end at "
          f"{1e3 * float(rms.max()):.4f} mm rms (worst pose and hand)", flush=True)
    if a.no_torch:
        return

    def by_torch():
        leaves = [t.clone().requires_grad_() for t in init]
        opt = torch.optim.Adam([{"params": [leaves[0]], "lr": 0.03}, {"params": [leaves[1]], "lr": 0.06}, {"params": [leaves[2]], "lr": 0.006}])
        for _ in range(steps):
            opt.zero_grad()
            v = torch_two_hands(tens, ring_t, *leaves)[0]
            ((v[:, :n] - target[:, :n]) ** 2).sum(-1).mean(1).sum().add(((v[:, n:] - target[:, n:]) ** 2).sum(-1).mean(1).sum()).backward()
            opt.step()

    tt = median_ms(by_torch, 1, a.reps)
    print(f"P={P:5d}: torch.optim.Adam on the PyTorch fp32 restatement, {steps} steps {fmt(tt)} per call, {1e3 * tt[0] / steps:8.2f} us per step: "
          f"{tt[0] / tf[0]:6.1f} x the HIP path", flush=True)


def lm_rows(a, P, hands, pose, betas, trans, fmt):
    with torch.no_grad():
        target = mano.skin_two_hands(*hands, pose, betas, trans)[0]
    nvo, n = hands[0].nv + 1, hands[0].nj * 3 + hands[0].nb + 3
    gen = torch.Generator(device="cuda").manual_seed(9)
    init = (pose + 0.2 * torch.randn(pose.shape, device="cuda", generator=gen), torch.zeros_like(betas),
            trans + 0.02 * torch.randn(trans.shape, device="cuda", generator=gen))
    tv = [target[:, nvo * h:nvo * (h + 1)].contiguous() for h in range(2)]
    outs = [(torch.empty(P, n, n, device="cuda"), torch.empty(P, n, device="cuda"), torch.empty(P, device="cuda")) for _ in range(2)]

    def normal():
        for h in range(2):
            mano._skin_normal(hands[h], init[0][:, h], init[1][:, h], init[2][:, h], tv[h], None, None, False, True, out=outs[h])

    tn = median_ms(normal, a.calls, a.reps)
    M = [o[0] + 1e-3 * torch.diag_embed(torch.diagonal(o[0], dim1=1, dim2=2) + 1e-9) for o in outs]
    ts = median_ms(lambda: [mano.lm_solve(M[h], outs[h][1]) for h in range(2)], a.calls, a.reps)
    print(f"P={P:5d}: skin_normal, two hands {fmt(tn)} per call pair, {1e3 * tn[0] / P:9.3f} us per pose; lm_solve (n = {n}), two hands {fmt(ts)}, "
          f"{1e3 * ts[0] / P:9.3f} us per pose", flush=True)
    tl = median_ms(lambda: mano.fit_two_hands_lm(*hands, target, init=init), max(1, a.calls // 10), a.reps)
    ta = median_ms(lambda: mano.fit_two_hands(*hands, target, init=init, steps=300), 1, max(1, a.reps // 2))
    lm, adam = mano.fit_two_hands_lm(*hands, target, init=init), mano.fit_two_hands(*hands, target, init=init, steps=300)
    print(f"P={P:5d}: fit_two_hands_lm, default iterations {fmt(tl)} per call, worst rms {1e3 * float(lm['rms'].max()):.5f} mm, fewest accepted steps "
          f"{int(lm['accepted'].min())}; fit_two_hands, 300 steps {fmt(ta)} per call, worst rms {1e3 * float(adam['rms'].max()):.5f} mm: {ta[0] / tl[0]:6.1f} x the time",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true", help="time the HIP path only (for comparing builds)")
    ap.add_argument("--backward", action="store_true", help="also time the backward and forward + backward against PyTorch autograd")
    ap.add_argument("--fit", action="store_true", help="also time mano.fit_two_hands against torch.optim.Adam on the restatement")
    ap.add_argument("--fit-steps", type=int, default=50)
    ap.add_argument("--lm", action="store_true", help="also time skin_normal, lm_solve and mano.fit_two_hands_lm against mano.fit_two_hands at 300 steps")
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
        if not a.no_torch:
            with torch.no_grad():
                tt = median_ms(lambda: torch_two_hands(tens, ring_t, pose, betas, trans), max(1, a.calls // 4), a.reps)
                ref = torch_two_hands(tens, ring_t, pose, betas, trans)
            worst = max(float((ref[0] - out[0]).abs().max()), float((ref[1] - out[1]).abs().max()))
            print(f"P={P:5d}: PyTorch fp32 restatement {fmt(tt)} per call, {1e3 * tt[0] / P:9.3f} us per pose: {tt[0] / t[0]:6.1f} x the HIP path; "
                  f"largest difference between the two {worst:.2e}", flush=True)
        if a.backward:
            backward_rows(a, P, hands, tens, ring_t, pose, betas, trans, fmt)
        if a.fit:
            fit_rows(a, P, hands, tens, ring_t, pose, betas, trans, fmt)
        if a.lm:
            lm_rows(a, P, hands, pose, betas, trans, fmt)

if __name__ == "__main__":
    main()
