"""The backward of MANO skinning and the fit on top of it (vanerf_amd/mano.py, vanerf_amd/csrc/mano_skin_backward.hip) on
a real MI355X: grad_pose, grad_betas and grad_trans against fp64 autograd of the torch restatement on every case of
tests/test_mano_skin_cpu.py, the variants of the calling rules, the rules that hold bit for bit, and mano.fit_hand / fit_two_hands.

The restatement, the upstream gradients and the bars are those of tests/test_mano_backward_cpu.py (`gradients`, `bar_of`): output o within
4 Erel S_o of the fp64 gradient, Erel = max_o E_o / S_o with E_o = max |fp32 autograd - fp64 autograd| of the restatement and S_o = max |g64_o|;
every figure is printed, as a multiple of Erel S_o, before it is asserted.  The fit's bar, 1e-4 m rms per pose, is 10 x what the fp64 restatement
reaches under the same optimiser (section 0l)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_baked_volume as B
from tests import test_mano_backward_cpu as Y
from tests import test_mano_skin_cpu as C
from tests.test_mano_skin import dev, device_case
from vanerf_amd import synth

pytestmark = pytest.mark.gpu

R = B.R  # the module fixture: the renderer, or a failure without a GPU
bits = B.bits
MAIN = (778, 16, 10, 130, "mano", False)
SMALL = (65, 16, 10, 3, "mano")


def leaves(*tensors):
    return [t.detach().clone().requires_grad_() for t in tensors]


def check(got, g64, S, erel, bars, what):
    for name, g, want, s, bar in zip(Y.OUTPUTS, got, g64, S, bars):
        err = float(np.abs(g.detach().cpu().numpy().astype(np.float64) - want).max())
        print(f"{what} {name}: err {err:.3e} = {err / (erel * s) if s > 0 else float('nan'):.2f} Erel S (Erel {erel:.2e}, S {s:.2e}, bar {bar:.2e})")
        assert np.isfinite(err) and err <= bar, (what, name, err, bar)


# ------------------------------------------------------------------------------------------------
# 1. values
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: "nv{}-nj{}-nb{}-P{}-{}-{}".format(*c[:5], "flat" if c[5] else "mean"))
def test_gradients_against_fp64(R, case):
    from vanerf_amd import mano
    mm, pose, betas, trans = device_case(case)
    gv, gj, g64, S, erel, bars = Y.gradients(*case)
    p, b, t = leaves(pose, betas, trans)
    verts, joints = mano.skin_hand(mm, p, b, t, flat_hand_mean=case[5])
    assert verts.requires_grad and joints.requires_grad
    got = torch.autograd.grad((verts, joints), (p, b, t), (dev(gv), dev(gj)))
    assert [tuple(g.shape) for g in got] == [tuple(pose.shape), tuple(betas.shape), tuple(trans.shape)] and all(g.dtype == torch.float32 and g.is_cuda for g in got)
    check(got, g64, S, erel, bars, str(case))


_VARIANTS = {}


def variant(name):
    """One small case under the calling rules' variants -> (ManoModel, seal, inputs on the device, gv, gj, reference)."""
    from vanerf_amd import mano
    if name not in _VARIANTS:
        model, ring, pose, betas, trans = C.draw(*SMALL)
        gv, gj = Y.upstream(66, 16, 3, 1)
        seal = name != "open"
        if name == "verts only":
            gj = None
        if name == "joints only":
            gv = None
        if name == "open":
            gv = gv[:, :65]
        if name == "repeated ring":
            ring = ring[:5] + ring[1:3]
            assert len(set(ring)) == 5 and len(ring) == 7
        mm = mano.ManoModel.from_arrays(**model, seal_ring=ring)
        _VARIANTS[name] = (mm, seal, dev(pose), dev(betas), dev(trans), gv, gj, Y.bar_of(model, pose, betas, trans, False, ring if seal else None, gv, gj))
    return _VARIANTS[name]


@pytest.mark.parametrize("name", ["both", "verts only", "joints only", "open", "repeated ring"])
def test_variants_of_the_calling_rules(R, name):
    from vanerf_amd import mano
    mm, seal, pose, betas, trans, gv, gj, ref = variant(name)
    p, b, t = leaves(pose, betas, trans)
    verts, joints = mano.skin_hand(mm, p, b, t, seal=seal)
    outs, ups = [], []
    for o, g in ((verts, gv), (joints, gj)):
        if g is not None:  # an output that does not enter: autograd hands the backward None, which becomes a null pointer
            outs.append(o)
            ups.append(dev(g))
    got = torch.autograd.grad(outs, (p, b, t), ups)
    check(got, *ref, name)
    if name == "joints only":  # the joints do not see the vertices' tables: one launch, and grad_trans is the sum of the joints' gradients
        want = gj.astype(np.float64).sum(1)
        assert float(np.abs(got[2].cpu().numpy() - want).max()) <= 4 * 2.0 ** -24 * float(np.abs(want).max())


def test_an_input_without_grad_is_not_written(R):
    from vanerf_amd import mano
    from vanerf_amd._ffi import lib
    mm, seal, pose, betas, trans, gv, gj, ref = variant("both")
    p, t = leaves(pose, trans)
    verts, joints = mano.skin_hand(mm, p, betas, t)
    full = mano._skin_backward(mm, pose, betas, False, True, dev(gv), dev(gj))
    got = torch.autograd.grad((verts, joints), (p, t), (dev(gv), dev(gj)))
    assert torch.equal(bits(got[0]), bits(full[0])) and torch.equal(bits(got[1]), bits(full[2]))
    with pytest.raises(RuntimeError):
        torch.autograd.grad(mano.skin_hand(mm, p, betas, t)[0].sum(), betas)  # betas is no part of the graph
    # the raw entry: a null output is not wanted; the NaN-filled tensor that would have been it stays as it is, the others have their bits
    for skip in range(3):
        outs = [torch.full_like(g, float("nan")) for g in full]
        ptrs = []
        for i, o in enumerate(outs):
            ptrs += [None if i == skip else ctypes.c_void_p(o.data_ptr()), o.shape[1]]
        nbytes = lib.vanerf_mano_skin_backward_workspace_bytes(mm.nv, mm.nj, mm.nb, 3)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ring = (ctypes.c_int * len(mm.seal_ring))(*mm.seal_ring)
        g_v, g_j = dev(gv), dev(gj)
        rc = lib.vanerf_mano_skin_backward(ctypes.c_void_p(mm.packed.data_ptr()), mm.nv, mm.nj, mm.nb, ctypes.c_void_p(pose.data_ptr()), 48,
                                           ctypes.c_void_p(betas.data_ptr()), 10, 3, 0, ring, len(mm.seal_ring), ctypes.c_void_p(g_v.data_ptr()), 66 * 3,
                                           ctypes.c_void_p(g_j.data_ptr()), 48, ctypes.c_void_p(ws.data_ptr()), nbytes, *ptrs,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        for i, (o, g) in enumerate(zip(outs, full)):
            assert torch.isnan(o).all() if i == skip else torch.equal(bits(o), bits(g)), (skip, i)
    # and through the Python layer: an `out` entry that is not wanted is ignored
    keep = torch.full_like(full[1], float("nan"))
    some = mano._skin_backward(mm, pose, betas, False, True, dev(gv), dev(gj), want=(True, False, True), out=(None, keep, None))
    assert some[1] is None and torch.isnan(keep).all() and torch.equal(bits(some[0]), bits(full[0])) and torch.equal(bits(some[2]), bits(full[2]))


# ------------------------------------------------------------------------------------------------
# 2. rules that hold bit for bit
# ------------------------------------------------------------------------------------------------
def test_two_hands_are_two_calls_on_the_halves(R):
    from vanerf_amd import mano
    right = mano.ManoModel.from_arrays(**synth.mano_like_model(1), seal_ring=mano.MANO_SEAL_RING)
    left = mano.ManoModel.from_arrays(**synth.mano_like_model(2), seal_ring=mano.MANO_SEAL_RING[::-1])
    rng = np.random.default_rng(9)
    P = 5
    pose, betas, trans = dev((rng.standard_normal((P, 2, 48)) * 0.5).astype(np.float32)), dev(rng.standard_normal((P, 2, 10)).astype(np.float32)), \
        dev(rng.uniform(-1, 1, (P, 2, 3)).astype(np.float32))
    gv, gj = dev(rng.standard_normal((P, 1558, 3)).astype(np.float32)), dev(rng.standard_normal((P, 32, 3)).astype(np.float32))
    plain = mano.skin_two_hands(right, left, pose, betas, trans)
    p, b, t = leaves(pose, betas, trans)
    verts, joints = mano.skin_two_hands(right, left, p, b, t)
    assert torch.equal(bits(verts), bits(plain[0])) and torch.equal(bits(joints), bits(plain[1]))
    got = torch.autograd.grad((verts, joints), (p, b, t), (gv, gj))
    assert [tuple(g.shape) for g in got] == [(P, 2, 48), (P, 2, 10), (P, 2, 3)]
    for h, mm in enumerate((right, left)):
        ph, bh, th = leaves(pose[:, h].contiguous(), betas[:, h].contiguous(), trans[:, h].contiguous())
        v, j = mano.skin_hand(mm, ph, bh, th)
        one = torch.autograd.grad((v, j), (ph, bh, th), (gv[:, 779 * h:779 * (h + 1)].contiguous(), gj[:, 16 * h:16 * (h + 1)].contiguous()))
        assert all(torch.equal(bits(a[:, h]), bits(o)) and torch.isfinite(o).all() for a, o in zip(got, one)), h
    assert not torch.equal(got[0][:, 0], got[0][:, 1])
    # a scalar loss: autograd's expanded gradient is made contiguous, and only the vertices enter
    p, b, t = leaves(pose, betas, trans)
    mano.skin_two_hands(right, left, p, b, t)[0].sum().backward()
    want = torch.autograd.grad(mano.skin_two_hands(right, left, *leaves(pose, betas, trans)[:2], t)[0], t, torch.ones(P, 1558, 3, device="cuda"))[0]
    assert torch.equal(bits(t.grad), bits(want)) and float((t.grad - 779.0).abs().max()) <= 1e-3
    with pytest.raises(ValueError, match="requires grad"):
        mano.skin_two_hands(right, left, p, b, t, out=plain)
    p0, b0, t0 = leaves(pose[:0], betas[:0], trans[:0])  # P = 0 is valid, forward and backward
    empty = mano.skin_two_hands(right, left, p0, b0, t0)
    assert empty[0].shape == (0, 1558, 3) and [tuple(g.shape) for g in torch.autograd.grad(empty[0].sum(), (p0, b0, t0))] == [(0, 2, 48), (0, 2, 10), (0, 2, 3)]


def main_gradients():
    from vanerf_amd import mano
    mm, pose, betas, trans = device_case(MAIN)
    gv, gj = Y.gradients(*MAIN)[:2]
    return mm, pose, betas, dev(gv), dev(gj), mano._skin_backward(mm, pose, betas, False, True, dev(gv), dev(gj))


def test_the_same_bits_every_call(R):
    from vanerf_amd import mano
    mm, pose, betas, gv, gj, first = main_gradients()
    again = mano._skin_backward(mm, pose, betas, False, True, gv, gj)
    filled = tuple(torch.full_like(g, float("nan")) for g in first)
    into = mano._skin_backward(mm, pose, betas, False, True, gv, gj, out=filled)
    assert all(a is b for a, b in zip(into, filled))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = mano._skin_backward(mm, pose, betas, False, True, gv, gj, out=tuple(torch.full_like(g, float("nan")) for g in first))
    side.synchronize()
    for a, b, c, d in zip(first, again, into, on_side):
        assert torch.isfinite(a).all() and torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c)) and torch.equal(bits(a), bits(d))


def test_a_pose_has_the_gradient_bits_it_has_alone(R):
    from vanerf_amd import mano
    mm, pose, betas, gv, gj, full = main_gradients()
    for p in (0, 1, 2, 3, 64, 127, 129):
        one = mano._skin_backward(mm, pose[p:p + 1], betas[p:p + 1], False, True, gv[p:p + 1], gj[p:p + 1])
        assert all(torch.equal(bits(o[0]), bits(f[p])) for o, f in zip(one, full)), p
    part = mano._skin_backward(mm, pose[3:10], betas[3:10], False, True, gv[3:10], gj[3:10])  # another row in the batch
    assert all(torch.equal(bits(o), bits(f[3:10])) for o, f in zip(part, full))


@pytest.mark.parametrize("where", ["verts", "sealed vertex", "joints"])
def test_a_nan_stays_in_its_pose(R, where):
    from vanerf_amd import mano
    mm, pose, betas, gv, gj, full = main_gradients()
    pose, betas, gv, gj = pose[:9], betas[:9], gv[:9].clone(), gj[:9].clone()
    if where == "joints":
        gj[5, 7, 1] = float("nan")
    else:
        gv[5, 778 if where == "sealed vertex" else 300, 1] = float("nan")
    got = mano._skin_backward(mm, pose, betas, False, True, gv, gj)
    others = [p for p in range(9) if p != 5]
    assert all(torch.equal(bits(g[others]), bits(f[:9][others])) for g, f in zip(got, full))
    assert all(not torch.isfinite(g[5]).all() for g in got)  # every one of the pose's three gradients
    if where != "joints":  # a vertex's gradient reaches every joint's rotation (no weight is skipped) and every shape coefficient
        assert not torch.isfinite(got[0][5]).any() and not torch.isfinite(got[1][5]).any()


def test_the_forward_is_untouched_under_grad(R):
    from vanerf_amd import mano
    mm, pose, betas, trans = device_case(MAIN)
    plain = mano.skin_hand(mm, pose, betas, trans)
    with torch.no_grad():
        off = mano.skin_hand(mm, *leaves(pose, betas, trans))
    assert not off[0].requires_grad
    for which in range(3):
        args = [pose, betas, trans]
        args[which] = args[which].detach().clone().requires_grad_()
        under = mano.skin_hand(mm, *args)
        assert under[0].requires_grad and under[1].requires_grad
        for a, b, c in zip(plain, under, off):
            assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c))
    with pytest.raises(ValueError, match="requires grad"):
        mano.skin_hand(mm, *args, out=plain)
    with pytest.raises(RuntimeError):  # first order only
        p = pose.detach().clone().requires_grad_()
        g, = torch.autograd.grad(mano.skin_hand(mm, p, betas, trans)[0].sum(), p, create_graph=True)
        g.sum().backward()


# ------------------------------------------------------------------------------------------------
# 3. the fit
# ------------------------------------------------------------------------------------------------
def fit_case(P, sealed):
    from vanerf_amd import mano
    case = (257, 16, 10, P, "mano")
    model, ring, pose, betas, trans = C.draw(*case)
    f64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    with torch.no_grad():
        tv, tj = Y.skin(model, f64(pose), f64(betas), f64(trans), False, ring if sealed else None)
    mm = mano.ManoModel.from_arrays(**model, seal_ring=ring)
    return mm, pose, betas, trans, tv.float().cuda(), tj.float().cuda()


def test_fit_tracking(R):
    """Bar: every pose below 1e-4 m rms; the fp64 restatement under the same optimiser ends at 0.004 mm (section 0l)."""
    from vanerf_amd import mano
    mm, pose, betas, trans, tv, tj = fit_case(4, True)
    gen = torch.Generator().manual_seed(9)
    init = (torch.from_numpy(pose) + 0.2 * torch.randn(pose.shape, generator=gen), torch.zeros(betas.shape),
            torch.from_numpy(trans) + 0.02 * torch.randn(trans.shape, generator=gen))
    init = tuple(t.float().cuda() for t in init)
    given = tuple(t.clone() for t in init)
    start = ((mano.skin_hand(mm, *init)[0] - tv) ** 2).sum(-1).mean(-1).sqrt()
    fit = mano.fit_hand(mm, tv, tj, init=init, steps=300, lr=0.03)
    print("tracking fit: rms", [f"{1e3 * float(s):.1f}" for s in start], "mm ->", [f"{1e3 * float(r):.4f}" for r in fit["rms"]], "mm")
    assert float(start.min()) > 0.01 and fit["rms"].is_cuda and fit["rms"].shape == (4,)
    assert set(fit) == {"pose", "betas", "trans", "verts", "joints", "rms"} and fit["verts"].shape == (4, 258, 3) and fit["joints"].shape == (4, 16, 3)
    assert float(fit["rms"].max()) < 1e-4
    v, j = mano.skin_hand(mm, fit["pose"], fit["betas"], fit["trans"])
    assert torch.equal(bits(v), bits(fit["verts"])) and torch.equal(bits(j), bits(fit["joints"]))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(init, given))  # (init is left as it was given)
    again = mano.fit_hand(mm, tv, tj, init=init, steps=300, lr=0.03)
    assert all(torch.equal(bits(fit[k]), bits(again[k])) for k in fit)  # no atomics anywhere in the loop: the same bits


def test_fit_cold(R):
    """Bar: every pose below 1e-4 m rms from the rigid start alone; the fp64 restatement ends at 0.011 mm (section 0l)."""
    from vanerf_amd import mano
    mm, pose, betas, trans, tv, tj = fit_case(8, False)
    rigid = mano.fit_hand(mm, tv, tj, steps=0, seal=False)
    fit = mano.fit_hand(mm, tv, tj, init=None, steps=300, lr=0.03, seal=False)
    print("cold fit: rigid start rms", [f"{1e3 * float(s):.1f}" for s in rigid["rms"]], "mm ->", [f"{1e3 * float(r):.4f}" for r in fit["rms"]], "mm")
    assert float(rigid["rms"].max()) < 0.05 and float(rigid["pose"][:, 3:].abs().max()) == 0 and float(rigid["betas"].abs().max()) == 0
    assert fit["verts"].shape == (8, 257, 3) and float(fit["rms"].max()) < 1e-4


def test_fit_refusals(R):
    from vanerf_amd import mano
    mm, pose, betas, trans, tv, tj = fit_case(4, True)
    with pytest.raises(ValueError, match="at least one target"):
        mano.fit_hand(mm)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mano.fit_hand(mm, tv.cpu())
    with pytest.raises(ValueError, match="target_verts: expected"):
        mano.fit_hand(mm, tv[:, :-1])
    with pytest.raises(ValueError, match="target_joints: expected"):
        mano.fit_hand(mm, tv, tj[:-1])
    with pytest.raises(ValueError, match=r"init\[1\]"):
        mano.fit_hand(mm, tv, init=(dev(pose), dev(betas)[:, :-1], dev(trans)))
    with pytest.raises(ValueError, match="vert_weight"):
        mano.fit_hand(mm, tv, vert_weight=torch.ones(257, device="cuda"))
    weighted = mano.fit_hand(mm, tv, None, init=(dev(pose), dev(betas), dev(trans)), steps=2, vert_weight=torch.ones(258, device="cuda"), prior=(1e-3, 1e-3))
    # from the truth two steps do not go far: a step of Adam moves a parameter by at most (1 - b1) / sqrt(1 - b2) = 3.17 times its rate
    assert torch.isfinite(weighted["rms"]).all() and float((weighted["pose"] - dev(pose)).abs().max()) <= 2 * 3.17 * 0.03
    assert float((weighted["betas"] - dev(betas)).abs().max()) <= 2 * 3.17 * 0.06 and float((weighted["trans"] - dev(trans)).abs().max()) <= 2 * 3.17 * 0.006
    joints_only = mano.fit_hand(mm, None, tj, init=(dev(pose), dev(betas), dev(trans)), steps=2)
    assert joints_only["rms"].shape == (4,) and torch.isfinite(joints_only["rms"]).all()


def test_end_to_end_on_the_synthetic_frame(R):
    from vanerf_amd import mano, posed
    from vanerf_amd.novel_views import camera_to_cam_tar
    net = B._net("fp32")
    frame_cpu = synth.make_frame(seed=3, tar_h=16, tar_w=16)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    cams = [camera_to_cam_tar(c) for c in B._orbit(frame_cpu, 8)[:3]]
    frame_verts = frame_cpu["targets"]["vert_world"][0].numpy()
    hands = [mano.ManoModel.from_arrays(**dict(synth.mano_like_model(20 + h, nv=779), v_template=frame_verts[779 * h:779 * (h + 1)])) for h in range(2)]
    rng = np.random.default_rng(11)
    P = 3
    pose, betas, trans = dev((rng.standard_normal((P, 2, 48)) * 0.03).astype(np.float32)), dev((rng.standard_normal((P, 2, 10)) * 0.3).astype(np.float32)), \
        dev(rng.uniform(-0.005, 0.005, (P, 2, 3)).astype(np.float32))
    kw = dict(flat_hand_mean=True, seal=False)
    target, _ = mano.skin_two_hands(*hands, pose, betas, trans, **kw)
    assert target.shape == (P, 1558, 3)
    gen = torch.Generator().manual_seed(9)
    init = (pose + 0.2 * torch.randn(pose.shape, generator=gen).cuda(), torch.zeros_like(betas), trans + 0.02 * torch.randn(trans.shape, generator=gen).cuda())
    fit = mano.fit_two_hands(*hands, target, init=init, steps=300, lr=0.03, **kw)
    print("fit_two_hands on the synthetic frame: rms", [[f"{1e3 * float(r):.4f}" for r in row] for row in fit["rms"]], "mm")
    assert fit["pose"].shape == (P, 2, 48) and fit["betas"].shape == (P, 2, 10) and fit["trans"].shape == (P, 2, 3) and fit["rms"].shape == (P, 2)
    assert fit["verts"].shape == (P, 1558, 3) and fit["joints"].shape == (P, 32, 3)
    assert float(fit["rms"].max()) < 1e-4 and float(((fit["verts"] - target) ** 2).sum(-1).mean(-1).sqrt().max()) < 1e-4
    again, _ = mano.skin_two_hands(*hands, fit["pose"], fit["betas"], fit["trans"], **kw)
    assert torch.equal(bits(again), bits(fit["verts"]))
    frames = list(posed.mano_sequence(net, trb, *hands, fit["pose"], fit["betas"], fit["trans"], cams[0], resolution=32, samples=32, **kw))
    assert len(frames) == P and all(torch.isfinite(f["alpha"]).all() for f in frames) and float(frames[0]["alpha"].max()) > 0.5
