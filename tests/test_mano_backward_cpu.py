"""What tests/test_mano_backward.py rests on, checked without a GPU: the torch restatement of MANO skinning that fp64
autograd differentiates, held to the numpy restatement of tests/test_mano_skin_cpu.py and to central finite differences; what the bar of the
GPU tests can tell apart; the argument checks of the new C entries before any device call; the rigid start and the optimiser of mano.fit_hand
on the restatement; and the Python layer's refusals.

`skin(model, pose, betas, trans, flat, ring)` is the yardstick: the definition in the comment of vanerf_mano_skin (include/vanerf_hip.h), steps
1-7, in the dtype of `pose`.  `gradients(case)` gives, per case of test_mano_skin_cpu.cases(), the fp64 gradients for seeded N(0, 1) upstream
gradients, and the bar of the GPU tests: E_o = max |fp32 autograd - fp64 autograd| and S_o = max |g64_o| per output o (pose, betas, trans),
Erel = max_o E_o / S_o, bar_o = 4 Erel S_o (the factor 4 is section 0j's margin; `zero_gradient_bar` where S_o = 0)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import test_mano_skin_cpu as C
from vanerf_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("grad_pose", "grad_betas", "grad_trans")


# ------------------------------------------------------------------------------------------------
# the yardstick
# ------------------------------------------------------------------------------------------------
def rodrigues(r):
    e = r + 1e-8
    angle = (e * e).sum(-1, keepdim=True).sqrt()
    d = r / angle
    z = torch.zeros_like(d[..., 0])
    K = torch.stack([z, -d[..., 2], d[..., 1], d[..., 2], z, -d[..., 0], -d[..., 1], d[..., 0], z], -1).reshape(*r.shape[:-1], 3, 3)
    return torch.eye(3, dtype=r.dtype) + torch.sin(angle)[..., None] * K + (1 - torch.cos(angle))[..., None] * (K @ K)


def skin(model, pose, betas, trans, flat=False, ring=None, drop=None):
    """model: a dict of arrays under smplx's names; pose (P, nj*3), betas (P, nb), trans (P, 3) torch tensors of one dtype -> verts (P, nv, 3)
    (the sealed vertex appended when a ring is given; its ids may repeat) and joints (P, nj, 3).  drop: a structural mistake of a backward, made
    by detaching one path -- "posedirs" (the pose feature's way into the vertices), "J" (the joints' dependence on betas), "seal" (the
    appended vertex)."""
    dt = pose.dtype
    c = lambda k: torch.as_tensor(np.asarray(model[k]), dtype=dt)  # noqa: E731
    vt, sd, pd, Jr, W, hm = (c(k) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "hands_mean"))
    parents = [int(p) for p in model["parents"]]
    P, nj, nv = pose.shape[0], Jr.shape[0], vt.shape[0]
    full = pose if flat else torch.cat([pose[:, :3], pose[:, 3:] + hm], 1)
    v_shaped = vt[None] + torch.einsum("vkb,pb->pvk", sd, betas)
    J = torch.einsum("jv,pvk->pjk", Jr, v_shaped)
    if drop == "J":
        J = J.detach()
    R = rodrigues(full.reshape(P, nj, 3))
    feat = (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(P, (nj - 1) * 9)
    if drop == "posedirs":
        feat = feat.detach()
    v_posed = v_shaped + (feat @ pd).reshape(P, nv, 3)
    Gs = []
    last = torch.tensor([0, 0, 0, 1], dtype=dt).expand(P, 1, 4)
    for j in range(nj):
        t = J[:, j] if j == 0 else J[:, j] - J[:, parents[j]]
        L = torch.cat([torch.cat([R[:, j], t[:, :, None]], 2), last], 1)
        Gs.append(L if j == 0 else Gs[parents[j]] @ L)
    G = torch.stack(Gs, 1)
    joints = G[:, :, :3, 3] + trans[:, None]
    At = G[:, :, :3, 3] - torch.einsum("pjrc,pjc->pjr", G[:, :, :3, :3], J)
    A = torch.cat([G[:, :, :3, :3], At[..., None]], -1)
    T = torch.einsum("vj,pjrc->pvrc", W, A)
    verts = torch.einsum("pvrc,pvc->pvr", T[..., :3], v_posed) + T[..., 3] + trans[:, None]
    if ring is not None:
        s = verts[:, ring[0]]
        for u in ring[1:]:
            s = s + verts[:, u]
        s = s * (1.0 / len(ring))
        verts = torch.cat([verts, (s.detach() if drop == "seal" else s)[:, None]], 1)
    return verts, joints


def autograd(model, pose, betas, trans, flat, ring, gv, gj, dtype=torch.float64, drop=None):
    """-> (grad_pose, grad_betas, grad_trans) as fp64 numpy arrays: autograd of the yardstick in dtype, for upstream gradients gv and gj
    (None: that output does not enter)."""
    leaves = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in (pose, betas, trans)]
    verts, joints = skin(model, *leaves, flat, ring, drop)
    total = 0
    if gv is not None:
        total = total + (verts * torch.tensor(gv, dtype=dtype)).sum()
    if gj is not None:
        total = total + (joints * torch.tensor(gj, dtype=dtype)).sum()
    return tuple(g.numpy().astype(np.float64) for g in torch.autograd.grad(total, leaves, allow_unused=True))


def upstream(nv_out, nj, P, seed):
    """Upstream gradients of the vertices (P, nv_out, 3) and the joints (P, nj, 3): N(0, 1), fp32, seeded."""
    rng = np.random.default_rng([77, seed, nv_out, nj, P])
    return rng.standard_normal((P, nv_out, 3)).astype(np.float32), rng.standard_normal((P, nj, 3)).astype(np.float32)


def bar_of(model, pose, betas, trans, flat, ring, gv, gj):
    """-> (g64: three arrays, S: three floats, Erel, bars: three floats) for one set of inputs."""
    g64 = autograd(model, pose, betas, trans, flat, ring, gv, gj, torch.float64)
    g32 = autograd(model, pose, betas, trans, flat, ring, gv, gj, torch.float32)
    S = [float(np.abs(a).max()) for a in g64]
    E = [float(np.abs(a - b).max()) for a, b in zip(g32, g64)]
    erel = max(e / s for e, s in zip(E, S) if s > 0)
    return g64, S, erel, [4 * erel * s if s > 0 else zero_gradient_bar(model, pose, betas, flat, gv, gj) for s in S]


def zero_gradient_bar(model, pose, betas, flat, gv, gj):
    """An output whose fp64 gradient is identically zero has no relative bar (S_o = 0): a model of one vertex and one joint whose joint IS the
    vertex has no lever arm, so grad_pose = 0.  The kernels take the vertex in fp32 and the joint in fp64, each within 2^-24 of the hand's
    extent L (the largest coordinate before the translation), so the lever arm they see is up to 2 * 2^-24 L and the gradient up to that times
    the sum of a pose's upstream gradients; the bar is 4 times it (section 0j's margin)."""
    verts, joints = C.restate(model, pose, betas, np.zeros((pose.shape[0], 3)), np.float64, flat)
    L = max(float(np.abs(verts).max()), float(np.abs(joints).max()))
    total = max(float((0 if gv is None else np.abs(gv[p]).sum()) + (0 if gj is None else np.abs(gj[p]).sum())) for p in range(pose.shape[0]))
    return 4 * 2 * 2.0 ** -24 * L * total


@functools.lru_cache(maxsize=None)
def gradients(nv, nj, nb, P, tree_name, flat, seed=0):
    """A case of C.cases(), sealed with its drawn ring -> (gv, gj, g64, S, Erel, bars): computed once per case and shared."""
    model, ring, pose, betas, trans = C.draw(nv, nj, nb, P, tree_name, seed)
    gv, gj = upstream(nv + 1, nj, P, seed)
    return (gv, gj) + bar_of(model, pose, betas, trans, flat, ring, gv, gj)


# ------------------------------------------------------------------------------------------------
# the yardstick on its own
# ------------------------------------------------------------------------------------------------
def test_the_yardstick_is_the_restatement():
    for case, flat in (((257, 16, 10, 4, "mano"), False), ((65, 16, 10, 3, "chain"), True), ((20, 2, 1, 2, "star"), False)):
        model, ring, pose, betas, trans = C.draw(*case)
        for rg in (ring, None, ring[:3] + ring[:2]):
            want = C.restate(model, pose, betas, trans, np.float64, flat, rg)
            got = skin(model, *(torch.tensor(a, dtype=torch.float64) for a in (pose, betas, trans)), flat, rg)
            err = max(float(np.abs(g.numpy() - w).max()) for g, w in zip(got, want))
            print(f"{case} flat={flat} ring of {None if rg is None else len(rg)}: yardstick against restate {err:.1e}")
            assert err <= 1e-12


def tiny(seed):
    """The tiny two-joint model with seeded shape and pose directions, so that every gradient has every path."""
    m = C.tiny_model(2)
    rng = np.random.default_rng(seed)
    m["shapedirs"] = 0.1 * rng.standard_normal((3, 3, 1))
    m["posedirs"] = 0.1 * rng.standard_normal((9, 9))
    m["hands_mean"] = 0.2 * rng.standard_normal(3)
    m["J_regressor"] = np.array([[0.75, 0.25, 0.0], [0.0, 0.5, 0.5]])
    m["weights"] = np.array([[1.0, 0.0], [0.5, 0.5], [0.25, 0.75]])
    return m


def test_the_gradient_against_central_differences():
    """Central differences of the NUMPY restatement in fp64, step h = 1e-6: truncation h^2 f''' / 6 ~ 1e-12 and rounding 1e-16 / h ~ 1e-10 of
    values of order 1, against gradients of order 1 to 10: the bar is 1e-8 of the largest gradient."""
    rng = np.random.default_rng(5)
    h = 1e-6
    for m, ring in ((tiny(0), (2, 0, 2)), (C.tiny_model(2), None)):
        P = 2
        pose, betas, trans = rng.standard_normal((P, 6)) * 0.7, rng.standard_normal((P, 1)), rng.standard_normal((P, 3))
        gv, gj = rng.standard_normal((P, 3 + (ring is not None), 3)), rng.standard_normal((P, 2, 3))
        got = autograd(m, pose, betas, trans, False, ring, gv, gj)

        def value(args):
            v, j = C.restate(m, *args, np.float64, False, ring)
            return float((v * gv).sum() + (j * gj).sum())

        for which, g in enumerate(got):
            fd = np.zeros_like(g)
            for idx in np.ndindex(*g.shape):
                hi, lo = [a.copy() for a in (pose, betas, trans)], [a.copy() for a in (pose, betas, trans)]
                hi[which][idx] += h
                lo[which][idx] -= h
                fd[idx] = (value(hi) - value(lo)) / (2 * h)
            err, scale = float(np.abs(fd - g).max()), float(np.abs(fd).max())
            print(f"{OUTPUTS[which]} (ring {ring}): autograd against central differences {err:.2e}, largest {scale:.2e}")
            assert err <= 1e-8 * max(scale, 1.0)


def test_the_gradient_at_zero_pose_is_finite():
    case = (65, 16, 10, 3, "mano")
    model, ring, pose, betas, trans = C.draw(*case)
    gv, gj = upstream(66, 16, 3, 0)
    for flat in (True, False):
        zero = np.zeros_like(pose)
        if not flat:
            zero[:, 3:] = -model["hands_mean"]  # full = 0 for the fingers as well, to fp32's rounding of the mean
        for dtype in (torch.float64, torch.float32):
            g = autograd(model, zero, betas, trans, flat, ring, gv, gj, dtype)
            assert all(np.isfinite(a).all() for a in g) and np.abs(g[0]).max() > 1e-3


def test_structural_mistakes_show_up_far_above_the_bar():
    """With the posedirs path of grad_pose dropped, with the J path of grad_betas dropped and with the seal's share dropped, some gradient
    moves by a large multiple of its bar on the (257, 16, 10, 4) case."""
    case = (257, 16, 10, 4, "mano", False)
    model, ring, pose, betas, trans = C.draw(*case[:5])
    gv, gj, g64, S, erel, bars = gradients(*case)
    print(f"{case}: E/S pooled {erel:.2e}; S {[f'{s:.2e}' for s in S]}; bars {[f'{b:.2e}' for b in bars]}")
    for drop, moved in (("posedirs", 0), ("J", 1), ("seal", 0)):
        wrong = autograd(model, pose, betas, trans, False, ring, gv, gj, torch.float64, drop)
        multiples = [float(np.abs(w - g).max()) / b for w, g, b in zip(wrong, g64, bars)]
        print(f"{drop} dropped: {', '.join(f'{o} moves by {m:.0f} bars' for o, m in zip(OUTPUTS, multiples))}")
        assert multiples[moved] >= 100, (drop, multiples)


def test_the_gpu_cases_have_a_bar():
    for case in C.cases():
        gv, gj, g64, S, erel, bars = gradients(*case)
        print(f"{case}: Erel {erel:.2e}, S {[f'{s:.2e}' for s in S]}")
        assert gv.shape == (case[3], case[0] + 1, 3) and sum(a.size for a in g64) >= 61
        assert all(np.isfinite(a).all() for a in g64) and 0 < erel <= 1e-5 and min(bars) > 0, case
        assert min(S) > 0 or case[:3] == (1, 1, 1)  # (one vertex that is its own joint: no lever arm, grad_pose = 0)


# ------------------------------------------------------------------------------------------------
# the fit's parts, on the restatement
# ------------------------------------------------------------------------------------------------
def test_the_rigid_start_recovers_a_rigid_motion():
    from vanerf_amd import mano
    model = synth.mano_like_model(3, nv=120)
    rest = torch.tensor(model["v_template"], dtype=torch.float64)
    root = torch.tensor([0.01, -0.02, 0.03], dtype=torch.float64)
    r = torch.tensor([[0.3, -1.2, 0.5], [0.0, 0.0, 0.0], [2.0, 1.0, -1.5]], dtype=torch.float64)
    t = torch.tensor([[0.5, 0.1, -0.3], [0.0, 0.2, 0.0], [-1.0, 1.0, 1.0]], dtype=torch.float64)
    R = rodrigues(r)
    target = torch.einsum("pij,nj->pni", R, rest - root) + root + t[:, None]
    for use_svd in (True, False):
        got_r, got_t = mano._rigid_start(rest, root, target, use_svd)
        err_R, err_t = float((rodrigues(got_r) - R).abs().max()), float((got_t - t).abs().max())
        print(f"rigid start ({'svd' if use_svd else 'polar iteration'}): rotation {err_R:.1e}, translation {err_t:.1e}")
        assert err_R <= 1e-7 and err_t <= 1e-7  # (the 1e-8 of the definition's angle is in `rodrigues`)
    noisy = target + 1e-3 * torch.randn(target.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    a, b = mano._kabsch(rest, noisy, True), mano._kabsch(rest, noisy, False)
    assert float((a - b).abs().max()) <= 1e-9 and float((a @ a.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-12


def test_the_optimiser_is_adam_and_fits_the_restatement():
    """mano._fit on the fp64 yardstick, tracking from 0.2 rad and 2 cm off on a small model: the loss's gradients through the same code the GPU
    path runs, against torch.optim.Adam on the written-out loss for five steps; and 300 steps end below 0.1 mm."""
    from vanerf_amd import mano
    case = (65, 16, 10, 2, "mano")
    model, ring, pose, betas, trans = C.draw(*case)
    f64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    with torch.no_grad():
        tv, tj = skin(model, f64(pose), f64(betas), f64(trans), False, ring)
    gen = torch.Generator().manual_seed(9)
    start = [f64(pose) + 0.2 * torch.randn(pose.shape, dtype=torch.float64, generator=gen), torch.zeros(betas.shape, dtype=torch.float64),
             f64(trans) + 0.02 * torch.randn(trans.shape, dtype=torch.float64, generator=gen)]
    hm = f64(model["hands_mean"])
    w = torch.linspace(0.5, 1.5, 66, dtype=torch.float64)[:, None]
    prior = (1e-3, 1e-4)

    def forward(p, b, t):
        with torch.no_grad():
            return skin(model, p, b, t, False, ring)

    def backward(p, b, gv, gj):
        leaves = [x.detach().clone().requires_grad_() for x in (p, b, torch.zeros(p.shape[0], 3, dtype=p.dtype))]
        v, j = skin(model, *leaves, False, ring)
        return [g.clone() for g in torch.autograd.grad((v * gv).sum() + (j * gj).sum(), leaves)]

    mine = [x.clone() for x in start]
    mano._fit(forward, backward, mine, tv, tj, w, hm, 5, 0.03, prior)
    theirs = [x.clone().requires_grad_() for x in start]
    opt = torch.optim.Adam([{"params": [theirs[0]], "lr": 0.03}, {"params": [theirs[1]], "lr": 0.06}, {"params": [theirs[2]], "lr": 0.006}])
    for _ in range(5):
        opt.zero_grad()
        v, j = skin(model, *theirs, False, ring)
        loss = ((w[None, :, 0] * ((v - tv) ** 2).sum(-1)).mean(1) + ((j - tj) ** 2).sum(-1).mean(1)
                + prior[0] * ((theirs[0][:, 3:] + hm) ** 2).sum(1) + prior[1] * (theirs[1] ** 2).sum(1)).sum()
        loss.backward()
        opt.step()
    err = max(float((a - b.detach()).abs().max()) for a, b in zip(mine, theirs))
    print(f"five steps of mano._fit against torch.optim.Adam on the written-out loss: {err:.1e}")
    assert err <= 1e-12
    mine = [x.clone() for x in start]
    before = float(((forward(*mine)[0] - tv) ** 2).sum(-1).mean(-1).sqrt().max())
    mano._fit(forward, backward, mine, tv, tj, None, hm, 300, 0.03, (0.0, 0.0))
    after = float(((forward(*mine)[0] - tv) ** 2).sum(-1).mean(-1).sqrt().max())
    print(f"tracking fit of the fp64 restatement, {case}: rms {1e3 * before:.1f} mm -> {1e3 * after:.4f} mm")
    assert before > 5e-3 and after < 1e-4


# ------------------------------------------------------------------------------------------------
# the C entries and the Python layer, without a device
# ------------------------------------------------------------------------------------------------
def backward_args(**change):
    p = ctypes.c_void_p(64)
    ring = (ctypes.c_int * 64)(*range(64))
    good = dict(packed=p, nv=778, nj=16, nb=10, pose=p, pose_stride=48, betas=p, betas_stride=10, P=4, flat=0, ring=ring, n_ring=16, grad_verts=p,
                grad_verts_stride=779 * 3, grad_joints=p, grad_joints_stride=48, workspace=p, workspace_bytes=1 << 40, grad_pose=p, grad_pose_stride=48,
                grad_betas=p, grad_betas_stride=10, grad_trans=p, grad_trans_stride=3, stream=None)
    return dict(good, **change)


def entry_refusals(lib):
    tried = []

    def refused(args, msg):
        rc = lib.vanerf_mano_skin_backward(*args.values())
        assert rc == -22 and msg in lib.vanerf_last_error().decode(), (msg, rc, lib.vanerf_last_error())
        tried.append(msg)

    for change, msg in ((dict(nv=0), "nv=0"), (dict(nv=-5), "nv=-5"), (dict(nj=0), "nj=0"), (dict(nj=33), "nj=33"), (dict(nb=0), "nb=0"), (dict(nb=17), "nb=17"),
                        (dict(P=-1), "P=-1"), (dict(n_ring=65), "n_ring=65"), (dict(n_ring=-1), "n_ring=-1"), (dict(ring=None), "null argument"),
                        (dict(pose_stride=47), "pose_stride=47"), (dict(betas_stride=9), "betas_stride=9"),
                        (dict(grad_verts_stride=779 * 3 - 1), "grad_verts_stride"), (dict(n_ring=0, grad_verts_stride=778 * 3 - 1), "grad_verts_stride"),
                        (dict(grad_joints_stride=47), "grad_joints_stride=47"), (dict(grad_pose_stride=47), "grad_pose_stride=47"),
                        (dict(grad_betas_stride=9), "grad_betas_stride=9"), (dict(grad_trans_stride=2), "grad_trans_stride=2"),
                        (dict(packed=None), "null argument"), (dict(pose=None), "null argument"), (dict(betas=None), "null argument"),
                        (dict(workspace=None), "null argument"), (dict(grad_verts=None, grad_joints=None), "both null"),
                        (dict(packed=ctypes.c_void_p(72)), "16-byte aligned"), (dict(workspace=ctypes.c_void_p(68)), "8-byte aligned"),
                        (dict(workspace_bytes=lib.vanerf_mano_skin_backward_workspace_bytes(778, 16, 10, 4) - 1), "workspace_bytes")):
        refused(backward_args(**change), msg)
    ring = (ctypes.c_int * 64)(*range(64))
    ring[3] = 778
    refused(backward_args(ring=ring), "ring[3]=778")
    ring[3] = -1
    refused(backward_args(ring=ring), "ring[3]=-1")
    ring[3], ring[40] = 2, -1  # a repeated id is fine, and ids past n_ring are not read: what refuses this call is the stride alone
    refused(backward_args(ring=ring, pose_stride=1), "pose_stride=1")
    return len(tried)


def test_the_entries_check_their_arguments_before_any_device_call():
    from vanerf_amd import _ffi
    lib = _ffi.lib
    assert _ffi.ABI_VERSION == 12 and lib.vanerf_abi_version() == 12
    assert entry_refusals(lib) >= 29
    # P = 0 is valid and a no-op, whatever the pointers
    assert lib.vanerf_mano_skin_backward(*backward_args(P=0).values()) == 0
    nothing = dict(packed=None, pose=None, betas=None, ring=None, n_ring=0, grad_verts=None, grad_joints=None, workspace=None, workspace_bytes=0,
                   grad_pose=None, grad_betas=None, grad_trans=None)
    assert lib.vanerf_mano_skin_backward(*backward_args(P=0, **nothing).values()) == 0
    # nothing wanted: checked, then nothing launched
    assert lib.vanerf_mano_skin_backward(*backward_args(grad_pose=None, grad_betas=None, grad_trans=None).values()) == 0
    # the workspace: per pose and chunk of 256 vertices one fp64 value per reduced sum (12 nj + 9 (nj-1) + nb + 3), then A and the pose feature
    size = lib.vanerf_mano_skin_backward_workspace_bytes
    assert size(778, 16, 10, 0) == 0 and size(778, 16, 10, 3) == 3 * (4 * 340 * 8 + 4 * (16 * 12 + 15 * 9))
    assert size(256, 16, 10, 1) == 340 * 8 + 4 * 327 and size(257, 16, 10, 1) == 2 * 340 * 8 + 4 * 327 and size(1, 1, 1, 2) == 2 * (16 * 8 + 4 * 12)
    assert size(0, 16, 10, 1) == -22 and b"nv=0" in lib.vanerf_last_error()
    assert size(778, 33, 10, 1) == -22 and size(778, 16, 17, 1) == -22 and size(778, 16, 10, -1) == -22


def test_the_exports_match_the_header():
    from vanerf_amd import _ffi
    header = open(os.path.join(REPO, "include", "vanerf_hip.h")).read()
    assert set(re.findall(r"\b(vanerf_[a-z0-9_]+)\s*\(", header)) == set(_ffi.EXPORTS)
    for name in ("vanerf_mano_skin_backward", "vanerf_mano_skin_backward_workspace_bytes"):
        assert name in _ffi.EXPORTS and hasattr(_ffi.lib, name) and f"{name}(" in header
    assert "#define VANERF_ABI_VERSION 12" in header
    assert len(_ffi._SIGS["vanerf_mano_skin_backward"][1]) == 25  # the header's argument list, one for one
    declared = header[header.index("int vanerf_mano_skin_backward("):]
    assert declared[:declared.index(";")].count(",") == 24


def test_the_python_layer_refuses_out_with_grad_and_cpu_tensors():
    from vanerf_amd import mano
    pose, betas, trans = torch.zeros(2, 48, requires_grad=True), torch.zeros(2, 10), torch.zeros(2, 3)
    with pytest.raises(ValueError, match="requires grad"):
        mano.skin_hand(None, pose, betas, trans, out=(torch.zeros(2, 779, 3), torch.zeros(2, 16, 3)))
    with pytest.raises(ValueError, match="requires grad"):
        mano.skin_two_hands(None, None, torch.zeros(2, 2, 48), torch.zeros(2, 2, 10, requires_grad=True), torch.zeros(2, 2, 3), out=(None, None))
    with torch.no_grad(), pytest.raises(ValueError, match="no CPU fallback"):  # without grad mode the out= is today's, and so is the refusal
        mano.skin_hand(None, pose, betas, trans, out=(torch.zeros(2, 779, 3), torch.zeros(2, 16, 3)))
    with pytest.raises(ValueError, match="no CPU fallback"):
        mano.skin_hand(None, pose, betas, trans)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mano.skin_two_hands(None, None, torch.zeros(2, 2, 48, requires_grad=True), torch.zeros(2, 2, 10), torch.zeros(2, 2, 3))
    with pytest.raises(ValueError, match="ManoModel"):
        mano.fit_hand(None, torch.zeros(2, 779, 3))
    with pytest.raises(ValueError, match="two ManoModels"):
        mano.fit_two_hands(None, None, torch.zeros(2, 1558, 3))
    assert {"fit_hand", "fit_two_hands", "skin_hand", "skin_two_hands"} <= set(mano.__all__)
