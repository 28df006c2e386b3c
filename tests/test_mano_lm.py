"""The normal equations of MANO skinning, the SPD solve and the Levenberg-Marquardt fit on top of them (vanerf_amd/mano.py,
vanerf_amd/csrc/mano_skin_normal.hip) on a real MI355X: H, g and loss against the fp64 yardstick on every case of
tests/test_mano_skin_cpu.py (P capped at 9), the variants of the calling rules, the cross-check against vanerf_mano_skin_backward, the rules that
hold bit for bit, vanerf_mano_lm_solve against numpy in fp64, and mano.fit_hand_lm / fit_two_hands_lm.

The yardstick, the targets and the bars are those of tests/test_mano_lm_cpu.py (`reference`, `bars_of`, `held`): scale-aware, with
s_c = sqrt(H64[c, c]): |H - H64|[c, c'] <= 4 Erel_H s_c s_c', |g - g64|[c] <= 4 Erel_g s_c sqrt(loss64), |loss - loss64| <= 4 E32, the Erel and
E32 being the errors of the yardstick run in fp32; every figure is printed as a multiple of its Erel scale before it is asserted.  The fit's
bar, 1e-4 m rms per pose, is the project's; its second bar is 4 x the final rms of the yardstick's loop run in fp32 (1e-6 m where that is smaller)."""
import numpy as np
import pytest
import torch

from tests import test_baked_volume as B
from tests import test_mano_backward_cpu as Y
from tests import test_mano_lm_cpu as N
from tests import test_mano_skin_cpu as C
from tests.test_mano_skin import dev, device_case
from vanerf_amd import synth

pytestmark = pytest.mark.gpu

R = B.R  # the module fixture: the renderer, or a failure without a GPU
bits = B.bits
SMALL = (65, 16, 10, 3, "mano")
MAIN = (778, 16, 10, 130, "mano", False)


def host(*tensors):
    return tuple(t.detach().cpu().numpy().astype(np.float64) for t in tensors)


# ------------------------------------------------------------------------------------------------
# 1. values
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: "nv{}-nj{}-nb{}-P{}-{}-{}".format(*c[:5], "flat" if c[5] else "mean"))
def test_normal_equations_against_fp64(R, case):
    from vanerf_amd import mano
    mm = device_case(case)[0]
    pose, betas, trans, tv, tj, w, ref = N.reference(*case)
    P, n = pose.shape[0], 3 * case[1] + case[2] + 3
    H, g, loss = mano.skin_normal_equations(mm, dev(pose), dev(betas), dev(trans), dev(tv), dev(tj), dev(w), flat_hand_mean=case[5])
    assert H.shape == (P, n, n) and g.shape == (P, n) and loss.shape == (P,) and H.dtype == g.dtype == loss.dtype == torch.float32 and H.is_cuda
    assert torch.equal(bits(H), bits(H.transpose(1, 2).contiguous()))
    N.held(*host(H, g, loss), ref, str(case))


_VARIANTS = {}


def variant(name):
    """The small case under the calling rules' variants -> (ManoModel, seal, device inputs, keyword arguments, reference)."""
    from vanerf_amd import mano
    if name not in _VARIANTS:
        model, ring, pose, betas, trans = C.draw(*SMALL)
        if name == "repeated ring":
            ring = ring[:5] + ring[1:3]
            assert len(set(ring)) == 5 and len(ring) == 7
        seal = name != "open"
        tv, tj, w = N.targets(model, ring if seal else None, pose, betas, trans, False, 1)
        if name == "verts only":
            tj = None
        if name == "joints only":
            tv = w = None
        if name == "shared weights":
            w = w[0]
        if name == "no weights":
            w = None
        mm = mano.ManoModel.from_arrays(**model, seal_ring=ring)
        ref = N.bars_of(model, pose, betas, trans, tv, tj, w, False, ring if seal else None)
        opt = lambda a: None if a is None else dev(a)  # noqa: E731
        _VARIANTS[name] = (mm, seal, (dev(pose), dev(betas), dev(trans)), dict(target_verts=opt(tv), target_joints=opt(tj), vert_weight=opt(w)), ref)
    return _VARIANTS[name]


@pytest.mark.parametrize("name", ["both", "verts only", "joints only", "open", "repeated ring", "shared weights", "no weights"])
def test_variants_of_the_calling_rules(R, name):
    from vanerf_amd import mano
    mm, seal, params, kw, ref = variant(name)
    out = mano.skin_normal_equations(mm, *params, seal=seal, **kw)
    N.held(*host(*out), ref, name)
    if name == "shared weights":  # one row shared by all poses (stride 0) against the same row per pose
        per_pose = mano.skin_normal_equations(mm, *params, seal=seal, **dict(kw, vert_weight=kw["vert_weight"].expand(3, 66).contiguous()))
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(out, per_pose))


def test_g_is_half_the_backward_of_twice_the_weighted_residual(R):
    """g = J^T W r against vanerf_mano_skin_backward fed 2 W r, halved: two kernels, two orders of summation; within the sum of both bars."""
    from vanerf_amd import mano
    mm, seal, (pose, betas, trans), kw, ref = variant("both")
    g = mano.skin_normal_equations(mm, pose, betas, trans, **kw)[1]
    verts, joints = mano.skin_hand(mm, pose, betas, trans)
    gv = (verts - kw["target_verts"]) * (2.0 / 66) * kw["vert_weight"][..., None]
    gj = (joints - kw["target_joints"]) * (2.0 / 16)
    back = torch.cat(mano._skin_backward(mm, pose, betas, False, True, gv, gj), 1)
    model, ring = C.draw(*SMALL)[:2]
    bar_back = Y.bar_of(model, *host(pose, betas, trans), False, ring, gv.cpu().numpy(), gj.cpu().numpy())[3]
    bar_back = np.concatenate([np.full(48, bar_back[0]), np.full(10, bar_back[1]), np.full(3, bar_back[2])])
    s = np.sqrt(np.einsum("pcc->pc", ref["H64"]))
    bar = 4 * ref["Erel_g"] * s * np.sqrt(ref["loss64"])[:, None] + bar_back[None] / 2
    err = np.abs(host(g)[0] - host(back)[0] / 2)
    print(f"g against half the backward of 2 W r: worst {float((err / bar).max()):.3f} of the summed bars, largest g {float(g.abs().max()):.2e}")
    assert (err <= bar).all()


# ------------------------------------------------------------------------------------------------
# 2. rules that hold bit for bit
# ------------------------------------------------------------------------------------------------
def main_inputs():
    mm = device_case(MAIN)[0]
    pose, betas, trans, tv, tj, w, ref = N.reference(*MAIN)
    return mm, tuple(dev(a) for a in (pose, betas, trans)), dict(target_verts=dev(tv), target_joints=dev(tj), vert_weight=dev(w))


def test_a_null_output_is_not_written(R):
    from vanerf_amd import mano
    mm, params, kw = main_inputs()
    full = mano.skin_normal_equations(mm, *params, **kw)
    for skip in range(3):
        outs = [torch.full_like(t, float("nan")) for t in full]
        mano._skin_normal(mm, *params, kw["target_verts"], kw["target_joints"], kw["vert_weight"], False, True,
                          out=tuple(None if i == skip else o for i, o in enumerate(outs)))
        torch.cuda.synchronize()
        for i, (o, f) in enumerate(zip(outs, full)):
            assert torch.isnan(o).all() if i == skip else torch.equal(bits(o), bits(f)), (skip, i)


def test_a_pose_has_the_bits_it_has_alone_and_every_call_the_same(R):
    from vanerf_amd import mano
    mm, params, kw = main_inputs()
    full = mano.skin_normal_equations(mm, *params, **kw)
    assert all(torch.isfinite(t).all() for t in full) and torch.equal(bits(full[0]), bits(full[0].transpose(1, 2).contiguous()))
    for p in range(7):
        one = mano.skin_normal_equations(mm, *(t[p:p + 1] for t in params), **{k: v[p:p + 1] for k, v in kw.items()})
        assert all(torch.equal(bits(o[0]), bits(f[p])) for o, f in zip(one, full)), p
    part = mano.skin_normal_equations(mm, *(t[2:9] for t in params), **{k: v[2:9] for k, v in kw.items()})  # another row in the batch
    assert all(torch.equal(bits(o), bits(f[2:9])) for o, f in zip(part, full))
    again = mano.skin_normal_equations(mm, *params, **kw)
    filled = tuple(torch.full_like(t, float("nan")) for t in full)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mano._skin_normal(mm, *params, kw["target_verts"], kw["target_joints"], kw["vert_weight"], False, True, out=filled)
    side.synchronize()
    assert all(torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c)) for a, b, c in zip(full, again, filled))


@pytest.mark.parametrize("where", ["verts", "sealed vertex", "joints"])
def test_a_nan_target_stays_in_its_pose(R, where):
    from vanerf_amd import mano
    mm, params, kw = main_inputs()
    full = mano.skin_normal_equations(mm, *params, **kw)
    kw = {k: v.clone() for k, v in kw.items()}
    if where == "joints":
        kw["target_joints"][5, 7, 1] = float("nan")
    else:
        kw["target_verts"][5, 778 if where == "sealed vertex" else 300, 1] = float("nan")
    got = mano.skin_normal_equations(mm, *params, **kw)
    others = [p for p in range(9) if p != 5]
    assert all(torch.equal(bits(a[others]), bits(f[others])) for a, f in zip(got, full))
    assert not torch.isfinite(got[1][5]).all() and not torch.isfinite(got[2][5]).all()  # (H does not see the targets)


@pytest.mark.parametrize("case, seal", [((257, 16, 10, 5, "mano"), True), ((65, 32, 16, 2, "chain"), False)], ids=["sealed", "open"])
def test_the_forward_is_its_own_exact_target(R, case, seal):
    """What the shared forward of csrc/mano_forward.h is for: skin_hand's vertices and joints, passed as the targets, leave no residual at all --
    loss is exactly 0.0 and g is zero in every element (the sign of a zero is not pinned) -- because the normal equations' vertex, joint and
    sealed vertex are the forward's, operation for operation, and a chain fmaf(a, w * 0, acc) from +0 stays +0.  nv = 257 crosses a border of
    64-vertex and of 256-vertex chunks, P = 5 is no multiple of the poses a lane carries.
    Mutant: two addends of one ((a + b) + c) swapped.  With one vertex_forward() for all three files no single consumer can be edited so;
    swapped inside the shared function all consumers move together and this test still holds, as it should."""
    from vanerf_amd import mano
    mm, pose, betas, trans = device_case(case)
    verts, joints = mano.skin_hand(mm, pose, betas, trans, flat_hand_mean=False, seal=seal)
    gen = torch.Generator(device="cuda").manual_seed(5)
    w = torch.rand(verts.shape[:2], device="cuda", generator=gen) + 0.5
    H, g, loss = mano.skin_normal_equations(mm, pose, betas, trans, verts, joints, w, flat_hand_mean=False, seal=seal)
    print(f"{case}: largest |g| {float(g.abs().max()):.3e}, largest loss {float(loss.abs().max()):.3e}, largest |H| {float(H.abs().max()):.3e}")
    assert float(H.abs().max()) > 0 and torch.isfinite(H).all()
    assert g.abs().max() == 0
    assert (loss == 0.0).all()


# ------------------------------------------------------------------------------------------------
# 3. the solve
# ------------------------------------------------------------------------------------------------
def spd(n, P, seed):
    """M = B^T B + 1e-3 I drawn in fp64 and rounded to fp32, g N(0, 1) -> fp32 arrays."""
    rng = np.random.default_rng([3, n, P, seed])
    Bm = rng.standard_normal((P, n + 3, n)) / np.sqrt(n + 3)
    M = (Bm.transpose(0, 2, 1) @ Bm + 1e-3 * np.eye(n)).astype(np.float32)
    return np.maximum(M, M.transpose(0, 2, 1)), rng.standard_normal((P, n)).astype(np.float32)  # (symmetric in fp32 as well)


@pytest.mark.parametrize("n", [1, 7, 61, 64, 65, 115, 128])
def test_the_solve_against_fp64(R, n):
    """delta against numpy.linalg.solve in fp64 of the rounded inputs; E32 = the error of an fp32 Cholesky solve of the same systems, margin 4."""
    from vanerf_amd import mano
    M, g = spd(n, 3, 0)
    want = -np.linalg.solve(M.astype(np.float64), g.astype(np.float64)[:, :, None])[:, :, 0]
    chol = torch.linalg.cholesky(torch.from_numpy(M))
    d32 = -torch.cholesky_solve(torch.from_numpy(g)[:, :, None], chol)[:, :, 0].numpy().astype(np.float64)
    e32 = float(np.abs(d32 - want).max())
    delta, ok = mano.lm_solve(dev(M), dev(g))
    err = float(np.abs(host(delta)[0] - want).max())
    print(f"n = {n}: err {err:.3e} (E32 {e32:.3e}, bar {4 * e32:.3e}), largest delta {np.abs(want).max():.2e}")
    assert delta.shape == (3, n) and ok.dtype == torch.int32 and ok.tolist() == [1, 1, 1] and err <= 4 * e32


def test_a_failed_system_stays_in_its_row(R):
    from vanerf_amd import mano
    M, g = spd(61, 5, 1)
    good, _ = mano.lm_solve(dev(M), dev(g))
    M[1, 30, 30] = -1.0       # indefinite
    M[3, 40, 12] = np.nan     # (in the lower triangle, which is what is read)
    delta, ok = mano.lm_solve(dev(M), dev(g))
    assert ok.tolist() == [1, 0, 1, 0, 1] and float(delta[1].abs().max()) == 0 and float(delta[3].abs().max()) == 0
    assert torch.equal(bits(delta[[0, 2, 4]]), bits(good[[0, 2, 4]])) and torch.isfinite(delta).all()
    again, _ = mano.lm_solve(dev(M), dev(g))
    assert torch.equal(bits(again), bits(delta))


# ------------------------------------------------------------------------------------------------
# 4. the fit
# ------------------------------------------------------------------------------------------------
_FITS = {}


def fit_case(name):
    """-> (ManoModel, seal, tv, tj on the device, init on the device or None, the final rms per pose of the yardstick's loop in fp32)."""
    from vanerf_amd import mano
    if name not in _FITS:
        case, sealed = {"tracking": (N.TRACKING, True), "cold": (N.COLD, False), "mano": ((778, 16, 10, 2, "mano"), True)}[name]
        model, ring, pose, betas, trans, tv, tj = N.fit_targets(case, sealed)
        tv32, tj32 = tv.astype(np.float32), tj.astype(np.float32)
        start = N.rigid_start(model, tv) if name == "cold" else N.tracking_start(pose, betas, trans)
        rms32 = N.lm(model, tv32, tj32, [s.float() for s in start], ring=ring, dtype=torch.float32)[1][-1]
        mm = mano.ManoModel.from_arrays(**model, seal_ring=C.draw(*case)[1])
        _FITS[name] = (mm, sealed, dev(tv32), dev(tj32), None if name == "cold" else tuple(s.float().cuda() for s in start), rms32)
    return _FITS[name]


@pytest.mark.parametrize("name", ["tracking", "cold", "mano"])
def test_fit_lm(R, name):
    from vanerf_amd import mano
    mm, seal, tv, tj, init, rms32 = fit_case(name)
    given = None if init is None else tuple(t.clone() for t in init)
    fit = mano.fit_hand_lm(mm, tv, tj, init=init, seal=seal)
    rms = host(fit["rms"])[0]
    bar = np.maximum(4 * rms32, 1e-6)
    print(f"{name}: rms in mm", " ".join(f"{1e3 * r:.5f}" for r in rms), "| the yardstick's loop in fp32:", " ".join(f"{1e3 * r:.5f}" for r in rms32),
          "| accepted", fit["accepted"].tolist(), "| damping", [f"{float(d):.0e}" for d in fit["damping"]])
    P = tv.shape[0]
    assert set(fit) == {"pose", "betas", "trans", "verts", "joints", "rms", "damping", "accepted"}
    assert fit["rms"].shape == fit["damping"].shape == fit["accepted"].shape == (P,) and fit["rms"].is_cuda and fit["verts"].shape == tv.shape
    assert (rms < 1e-4).all() and (rms <= bar).all() and int(fit["accepted"].min()) >= 1
    v, j = mano.skin_hand(mm, fit["pose"], fit["betas"], fit["trans"], seal=seal)
    assert torch.equal(bits(v), bits(fit["verts"])) and torch.equal(bits(j), bits(fit["joints"]))
    assert init is None or all(torch.equal(bits(a), bits(b)) for a, b in zip(init, given))  # (init is left as it was given)
    again = mano.fit_hand_lm(mm, tv, tj, init=init, seal=seal)
    assert all(torch.equal(bits(fit[k]), bits(again[k])) for k in fit)
    if name == "tracking":
        with pytest.raises(ValueError, match="iterations: at least 0"):  # (the shared check names this function's own argument)
            mano.fit_hand_lm(mm, tv, tj, init=init, iterations=-1, seal=seal)
        with pytest.raises(ValueError, match="steps: at least 0"):
            mano.fit_hand(mm, tv, tj, init=init, steps=-1, seal=seal)
        # a NaN target in one pose leaves the others' results as they are
        bad = tv.clone()
        bad[3, 100, 2] = float("nan")
        other = mano.fit_hand_lm(mm, bad, tj, init=init, seal=seal)
        keep = [p for p in range(P) if p != 3]
        assert all(torch.equal(bits(fit[k][keep]), bits(other[k][keep])) for k in fit if k not in ("verts", "rms")) and int(other["accepted"][3]) == 0
        assert torch.equal(bits(fit["verts"][keep]), bits(other["verts"][keep])) and not torch.isfinite(other["rms"][3])


def test_the_trace_floor_holds_a_direction_the_data_does_not_see(R):
    """The one-vertex model whose joint is the vertex: the pose turns nothing, its columns of J vanish (to the kernels' 2 * 2^-24 L lever arm,
    tests/test_mano_lm_cpu.zero_column_bar) and only lambda 1e-9 trace(H) / n keeps M positive definite there: the fit must return finite
    parameters below 1e-4 m with steps accepted, and leave the pose where it was.
    Bar on the pose's movement, after one iteration and after the default iterations alike: 4 x the movement of the yardstick's loop run in fp32
    on the same model, or the floor below where that is smaller.  The yardstick moves the pose by exactly 0 -- in torch's fp32 the vertex and
    the joint of this model are one number bit for bit, so its columns are exact zeros, which a kernel that takes the vertex in fp32 and the
    joint in fp64, as section 0j defines them, cannot have -- so the floor is the bar.  The floor is the zero column's scale carried through
    the damped step: with C_c a pose column (|C_c| <= eps = sqrt(3) 2 2^-24 L), Wt = sum W and phi = 1e-9 trace(H) / n the step is
    delta_c = -C_c^T W (S + I)^-1 rho / (lambda (|C_c|^2 Wt + phi)), S the other columns' share.  The part of rho in which vertex, sealed vertex
    and joint move as one point is spanned by the trans columns, S >= I / lambda there, and it moves the pose by eps |rho| Wt / phi
    <= eps |rho| n / 3e-9 at most (trace(H) >= 3 Wt); the residual shrinks by lambda or better per accepted step, so all steps together give 1.01
    times that.  The rest of rho is the forward's own rounding between the fp32 vertex and the fp64 joint, |rho'| <= 2 2^-24 L' with L' the
    largest coordinate WITH the translation; no column reaches it, and at lambda = 1e-3 it moves the pose by eps |rho'| n / (3e-9 lambda).  The
    floor is 4 times their sum (the margin).  Without the trace term the same algebra gives |rho| / eps (printed, not measured).
    What the floor does not cover: past the first step lambda falls towards 1e-12 and the second term grows as 1 / lambda; if the movement at the
    default iterations ever exceeds the floor, that is the damping rule spending a nearly-zero column on rounding noise, and a question for the
    rule, not for this bar.  Measured: 1.1e-2 rad after one iteration, 1.5e-2 rad after ten, floor 7.2e-1 rad."""
    from vanerf_amd import mano
    case = (1, 1, 1, 5, "chain")
    model, ring, pose, betas, trans = C.draw(*case)
    tv, tj, w = N.targets(model, ring, pose, betas, trans, False, 2)
    mm = mano.ManoModel.from_arrays(**model, seal_ring=ring)
    init = (dev(pose), dev(betas), dev(trans))
    v0, j0 = C.restate(model, pose, betas, np.zeros_like(trans), np.float64, False, ring)
    L = max(float(np.abs(v0).max()), float(np.abs(j0).max()))
    Lt = max(float(np.abs(v0 + trans[:, None]).max()), float(np.abs(tv).max()))
    rho = float(np.abs(np.concatenate([(v0 + trans[:, None]) - tv, (j0 + trans[:, None]) - tj], 1)).max()) * np.sqrt(3)
    eps = np.sqrt(3) * 2 * 2.0 ** -24 * L
    floor = 4 * (1.01 * eps * rho * 7 / 3e-9 + eps * (2 * 2.0 ** -24 * Lt) * 7 / (3e-9 * 1e-3))
    start = [torch.tensor(a) for a in (pose, betas, trans)]
    for iterations in (1, N.DEFAULT_ITERATIONS):
        x32 = N.lm(model, tv, tj, start, iterations=iterations, ring=ring, dtype=torch.float32)[0]
        yard = float((x32[:, :3] - start[0]).abs().max())
        bar = max(4 * yard, floor)
        fit = mano.fit_hand_lm(mm, dev(tv), dev(tj), init=init, iterations=iterations)
        moved = float((fit["pose"] - init[0]).abs().max())
        print(f"one vertex on its joint, {iterations} iterations: the pose moves by {moved:.2e} rad (the yardstick in fp32 by {yard:.2e}, floor {floor:.2e}, "
              f"bar {bar:.2e}; without the trace term, by the algebra, {rho / eps:.1e}), rms {[f'{float(r):.1e}' for r in fit['rms']]}, accepted {fit['accepted'].tolist()}")
        assert all(torch.isfinite(fit[k]).all() for k in ("pose", "betas", "trans", "verts", "rms")) and int(fit["accepted"].min()) >= 1
        assert moved <= bar
    assert float(fit["rms"].max()) < 1e-4


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
    gen = torch.Generator().manual_seed(9)
    init = (pose + 0.2 * torch.randn(pose.shape, generator=gen).cuda(), torch.zeros_like(betas), trans + 0.02 * torch.randn(trans.shape, generator=gen).cuda())
    fit = mano.fit_two_hands_lm(*hands, target, init=init, **kw)
    print("fit_two_hands_lm on the synthetic frame: rms", [[f"{1e3 * float(r):.5f}" for r in row] for row in fit["rms"]], "mm, accepted", fit["accepted"].tolist())
    assert fit["pose"].shape == (P, 2, 48) and fit["betas"].shape == (P, 2, 10) and fit["trans"].shape == (P, 2, 3)
    assert fit["rms"].shape == fit["damping"].shape == fit["accepted"].shape == (P, 2) and fit["verts"].shape == (P, 1558, 3) and fit["joints"].shape == (P, 32, 3)
    assert float(fit["rms"].max()) < 1e-4 and float(((fit["verts"] - target) ** 2).sum(-1).mean(-1).sqrt().max()) < 1e-4
    again, _ = mano.skin_two_hands(*hands, fit["pose"], fit["betas"], fit["trans"], **kw)
    assert torch.equal(bits(again), bits(fit["verts"]))
    frames = list(posed.mano_sequence(net, trb, *hands, fit["pose"], fit["betas"], fit["trans"], cams[0], resolution=32, samples=32, **kw))
    assert len(frames) == P and all(torch.isfinite(f["alpha"]).all() for f in frames) and float(frames[0]["alpha"].max()) > 0.5
