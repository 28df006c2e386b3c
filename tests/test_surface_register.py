"""The learned surface along lines (vanerf_amd/csrc/surface_lines.hip, surface.register_surface): the four kernels on
synthetic data against the fp64 restatement below, and register_surface end to end on the synthetic two-hand frame.  Needs a real MI355X.

The restatement (ref_bracket, ref_refine) needs no device; tests/test_surface_register_cpu.py checks it on hand-made rows.

Tolerances.  eps32 = 2^-23.  line_points: t_k and the point are one fused multiply-add each, so a coordinate is within one fp32 ulp of the fp64
value wherever an ulp of t is no larger than an ulp of the coordinate: half an ulp of its own rounding plus what the half ulp of t_k moves it
(|dir| <= 1).  The test's lines have |t| < 0.5 and coordinates of 1.5 to 4.5, as register_surface's have |t| of millimetres on a hand in
metres (measured: 0.60 ulp).  t_est / t_next: 4 eps32 max(|t0|, |t0 + (K - 1) dt|) (measured: 1.3e-9 against 7.1e-8 at K = 65).  The chosen pair
is compared exactly: rows are drawn so that the restatement's best and second-best |tc| differ by more than 1e-5 dt, far above the kernel's
rounding of a |tc| near the minimum (a few eps32 dt); 18 of the 3150 random rows had to be drawn again.  rgb_est: colours in [0, 1] and a weight
with three roundings, then a product and a sum: 8 eps32."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
FLT_MAX = float(np.finfo(np.float32).max)
STATE_FLOATS = 16
COLS = {"ta": 0, "tb": 1, "ga": 2, "gb": 3, "rgb_a": slice(4, 7), "found": 7, "rgb_b": slice(8, 11), "t_est": 11, "rgb_est": slice(12, 15), "t_next": 15}
GAP = 1e-5  # in units of dt


# ------------------------------------------------------------------------------------------------------------------------------------
# the fp64 restatement
# ------------------------------------------------------------------------------------------------------------------------------------
def clean(f):
    """A field value as the kernels read it: non-finite -> FLT_MAX (outside).  fp32 in, fp64 out."""
    f = np.asarray(f, dtype=np.float32)
    return np.where(np.isfinite(f), f, np.float32(FLT_MAX)).astype(np.float64)


def _weight(ga, gb, iso):
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (iso - ga) / (gb - ga)
    return np.clip(np.where(np.isnan(w), 0.0, w), 0.0, 1.0)


def _estimates(ta, tb, ga, gb, iso):
    w = _weight(ga, gb, iso)
    return w, ta + w * (tb - ta), ta + np.clip(w, 0.125, 0.875) * (tb - ta)


def ref_bracket(f, t0, dt, iso, rgb=None):
    """vanerf_line_bracket in fp64: f (n, K) fp32 -> dict of per-line arrays: found (bool), k (the lower sample of the chosen pair, -1 without
    one), ta, tb, ga, gb, t_est, t_next (NaN / 0 as the kernel leaves them), rgb_a, rgb_b, rgb_est, and gap = second-best |tc| - best |tc| (inf
    with fewer than two crossings)."""
    g = clean(f)
    n, K = g.shape
    t0, dt, iso = float(t0), float(dt), float(iso)
    inside = g < iso
    cross = inside[:, :-1] != inside[:, 1:]
    tk = t0 + np.arange(K, dtype=np.float64) * dt
    w = _weight(g[:, :-1], g[:, 1:], iso)
    atc = np.where(cross, np.abs(tk[None, :-1] + w * dt), np.inf)
    k = np.argmin(atc, 1)  # the first minimum: a tie goes to the smaller k
    found = cross.any(1)
    two = np.sort(atc, 1)[:, :2] if K > 2 else np.concatenate([atc, np.full((n, 1), np.inf)], 1)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(two[:, 1]), two[:, 1] - two[:, 0], np.inf)
    rows = np.arange(n)
    z = np.zeros(n)
    ta, tb = np.where(found, tk[k], z), np.where(found, tk[np.minimum(k + 1, K - 1)], z)
    ga, gb = np.where(found, g[rows, k], z), np.where(found, g[rows, np.minimum(k + 1, K - 1)], z)
    _, t_est, t_next = _estimates(ta, tb, np.where(found, ga, -1.0), np.where(found, gb, 1.0), iso)
    out = dict(found=found, k=np.where(found, k, -1), ta=ta, tb=tb, ga=ga, gb=gb, t_est=np.where(found, t_est, np.nan),
               t_next=np.where(found, t_next, np.nan), gap=gap)
    c = np.zeros((n, K, 3)) if rgb is None else np.asarray(rgb, dtype=np.float64)
    out["rgb_a"] = np.where(found[:, None], c[rows, k], 0.0)
    out["rgb_b"] = np.where(found[:, None], c[rows, np.minimum(k + 1, K - 1)], 0.0)
    wk = _weight(np.where(found, ga, -1.0), np.where(found, gb, 1.0), iso)
    out["rgb_est"] = np.where(found[:, None], out["rgb_a"] + wk[:, None] * (out["rgb_b"] - out["rgb_a"]), 0.0)
    return out


def ref_refine(state, f_new, iso, rgb_new=None):
    """vanerf_line_refine in fp64 on a state array (n, 16) (any float dtype) -> the new state as fp64."""
    s = np.array(state, dtype=np.float64)
    g = clean(f_new)
    iso = float(iso)
    found = s[:, COLS["found"]] == 1.0
    to_a = found & ((g < iso) == (s[:, COLS["ga"]] < iso))
    to_b = found & ~to_a
    t = s[:, COLS["t_next"]].copy()
    s[to_a, COLS["ta"]], s[to_a, COLS["ga"]] = t[to_a], g[to_a]
    s[to_b, COLS["tb"]], s[to_b, COLS["gb"]] = t[to_b], g[to_b]
    if rgb_new is not None:
        c = np.asarray(rgb_new, dtype=np.float64)
        s[to_a, COLS["rgb_a"]] = c[to_a]
        s[to_b, COLS["rgb_b"]] = c[to_b]
    w, t_est, t_next = _estimates(s[found, 0], s[found, 1], s[found, 2], s[found, 3], iso)
    s[found, COLS["t_est"]], s[found, COLS["t_next"]] = t_est, t_next
    s[found, COLS["rgb_est"]] = s[found, COLS["rgb_a"]] + w[:, None] * (s[found, COLS["rgb_b"]] - s[found, COLS["rgb_a"]])
    return s


# ------------------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import surface
    return surface


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _ulp(want):
    return np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


def _fma32(a, b, c):
    """fmaf of fp32 values, one rounding: the product and the sum are exact in the 64-bit significand of the x87 long double for the magnitudes
    used here (24 + 24 bits, terms within 2^15 of each other)."""
    assert np.finfo(np.longdouble).nmant >= 63
    return (np.asarray(a, np.float32).astype(np.longdouble) * np.asarray(b, np.float32).astype(np.longdouble)
            + np.asarray(c, np.float32).astype(np.longdouble)).astype(np.float32)


def draw_rows(rng, n, K, t0, dt, iso, patterns=None):
    """Rows (n, K) fp32 whose restated best and second-best |tc| differ by more than GAP dt; the lines that had to be drawn again are counted.
    patterns: (n, K) bool, the inside flags to realise with random magnitudes; None: random signs, about 5 % non-finite entries and some
    entries equal to iso."""
    def rows(m, pat):
        mag = rng.uniform(0.05, 1.0, (m, K)).astype(np.float32)
        if pat is not None:
            return (np.float32(iso) + np.where(pat, -mag, mag)).astype(np.float32)
        f = (np.float32(iso) + mag * rng.choice(np.float32([-1.0, 1.0]), (m, K))).astype(np.float32)
        u = rng.random((m, K))
        f[u < 0.05] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), int((u < 0.05).sum()))
        f[(u >= 0.05) & (u < 0.055)] = np.float32(iso)  # few: one between two inside samples makes two pairs with the same tc
        return f
    f = rows(n, patterns)
    redrawn = np.zeros(n, bool)
    for _ in range(8):
        bad = ref_bracket(f, t0, dt, iso)["gap"] <= GAP * dt
        if not bad.any():
            break
        redrawn |= bad
        f[bad] = rows(int(bad.sum()), None if patterns is None else patterns[bad])
    assert not (ref_bracket(f, t0, dt, iso)["gap"] <= GAP * dt).any()
    return f, int(redrawn.sum())


def check_bracket(S, f, rgb, t0, dt, iso):
    """Runs line_bracket and holds the state to the restatement; returns the state (host)."""
    n, K = f.shape
    ref = ref_bracket(f, t0, dt, iso, rgb)
    state = S.line_bracket(torch.from_numpy(f).cuda(), t0, dt, iso, None if rgb is None else torch.from_numpy(rgb).cuda()).cpu().numpy()
    assert state.shape == (n, STATE_FLOATS)
    found = state[:, COLS["found"]]
    assert np.isin(found, (0.0, 1.0)).all() and np.array_equal(found == 1.0, ref["found"])
    fd, k = ref["found"], np.maximum(ref["k"], 0)
    rows = np.arange(n)
    # the chosen pair and the ends of the bracket: the input's bits (a non-finite sample as the clean value)
    ta, tb = _fma32(k.astype(np.float32), np.float32(dt), np.float32(t0)), _fma32((k + 1).astype(np.float32), np.float32(dt), np.float32(t0))
    g32 = clean(f).astype(np.float32)
    want = {"ta": ta, "tb": tb, "ga": g32[rows, k], "gb": g32[rows, np.minimum(k + 1, K - 1)]}
    for name, w in want.items():
        assert np.array_equal(_bits(state[fd, COLS[name]]), _bits(w[fd])), name
    c = np.zeros((n, K, 3), np.float32) if rgb is None else rgb
    assert np.array_equal(_bits(state[fd, COLS["rgb_a"]]), _bits(c[rows, k][fd]))
    assert np.array_equal(_bits(state[fd, COLS["rgb_b"]]), _bits(c[rows, np.minimum(k + 1, K - 1)][fd]))
    tol = 4.0 * EPS32 * max(abs(t0), abs(t0 + (K - 1) * dt))
    for name in ("t_est", "t_next"):
        err = np.abs(state[fd, COLS[name]].astype(np.float64) - ref[name][fd]).max() if fd.any() else 0.0
        print(f"n={n} K={K}: max |{name} - fp64| = {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, name
    if rgb is not None and fd.any():
        assert np.abs(state[fd, COLS["rgb_est"]] - ref["rgb_est"][fd]).max() <= 8.0 * EPS32  # colours in [0, 1], w to 3 roundings
    # a line without a crossing: found = 0, t_est = t_next = NaN, zeros elsewhere
    miss = state[~fd]
    assert np.isnan(miss[:, [COLS["t_est"], COLS["t_next"]]]).all()
    assert (np.delete(miss, [COLS["t_est"], COLS["t_next"]], 1).view(np.int32) == 0).all()
    return state


# ------------------------------------------------------------------------------------------------------------------------------------
# normals
# ------------------------------------------------------------------------------------------------------------------------------------
def _render_vis_normals(verts, faces, vert_vis):
    """Floats 12..14 of vanerf_render_vis's per-vertex scratch record, through the C ABI, for a camera that looks down +z from 5 units away."""
    from vanerf_amd import _ffi
    nv, nf, H, W = verts.shape[0], faces.shape[0], 32, 32
    dev = dict(device="cuda")
    Rm, T = torch.eye(3, **dev), torch.tensor([0.0, 0.0, 5.0], **dev)
    focal, pp = torch.tensor([50.0, 50.0], **dev), torch.tensor([16.0, 16.0], **dev)
    scratch = torch.full((nv, 16), float("nan"), **dev)
    rgb, vis = torch.empty(3, H, W, **dev), torch.empty(H, W, **dev)
    _ffi.check(_ffi.lib.vanerf_render_vis(_ptr(verts), nv, _ptr(faces), nf, _ptr(vert_vis), _ptr(Rm), _ptr(T), _ptr(focal), _ptr(pp), H, W, _ptr(scratch),
                                          scratch.numel() * 4, _ptr(rgb), _ptr(vis), None, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return scratch[:, 12:15].contiguous()


def test_normals_equal_render_vis_on_the_synthetic_frame(S):
    from tests.test_vis_render import _scene
    _, fdat, _ = _scene(3, 15.0, 64, 64)
    assert fdat.verts3.shape == (1558, 3) and fdat.faces.shape == (3108, 3)
    got = S.vertex_normals(fdat.verts3, fdat.faces)
    want = _render_vis_normals(fdat.verts3, fdat.faces, fdat.vert_vis)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert (got.norm(dim=1) - 1).abs().max() < 1e-5
    assert torch.equal(S.vertex_normals(fdat.verts3, fdat.faces).view(torch.int32), got.view(torch.int32))


def test_normals_equal_render_vis_on_an_icosahedron_with_a_bad_face(S):
    p = (1 + 5 ** 0.5) / 2
    v = np.float32([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]])
    f = np.int32([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    f[13, 1] = 12  # outside [0, 12): the face is left out
    verts, faces = torch.from_numpy(v * 0.3).cuda(), torch.from_numpy(f).cuda()
    got = S.vertex_normals(verts, faces)
    want = _render_vis_normals(verts, faces, torch.ones(12, device="cuda"))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # the vertices of the dropped face lost a term: their normals are no longer radial, the others' are (by symmetry, to rounding)
    radial = torch.nn.functional.normalize(verts, dim=1)
    off = torch.minimum((got - radial).abs().max(1).values, (got + radial).abs().max(1).values).cpu().numpy()
    assert (off[[3, 6, 8]] > 1e-2).all() and (np.delete(off, [3, 6, 8]) < 1e-5).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# line_points
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_line_points_within_one_ulp(S, n):
    rng = np.random.default_rng(100 + n)
    base = (rng.uniform(2, 4, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    t0, dt = float(np.float32(-0.37)), float(np.float32(0.8 / 255))  # t in [-0.37, 0.43] at every K
    bt, dtn = torch.from_numpy(base).cuda(), torch.from_numpy(d).cuda()
    for K in (1, 2, 9, 65, 256):
        got = S.line_points(bt, dtn, K, t0, dt).cpu().numpy()
        assert got.shape == (n * K, 3)
        t = t0 + np.arange(K, dtype=np.float64) * dt
        want = base.astype(np.float64)[:, None, :] + t[None, :, None] * d.astype(np.float64)[:, None, :]
        err = np.abs(got.reshape(n, K, 3).astype(np.float64) - want) / _ulp(want)
        print(f"n={n} K={K}: max error {err.max():.3f} ulp")
        assert err.max() <= 1.0
    # one parameter per line; a non-finite one gives the base bit for bit
    t = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    bad = np.arange(n) % 3 == 0
    t[bad] = np.float32([np.nan, np.inf, -np.inf])[np.arange(int(bad.sum())) % 3]
    base[0, 0] = np.float32(-0.0)
    bt = torch.from_numpy(base).cuda()
    got = S.line_points(bt, dtn, t=torch.from_numpy(t).cuda()).cpu().numpy()
    assert got.shape == (n, 3) and np.array_equal(_bits(got[bad]), _bits(base[bad]))
    want = base.astype(np.float64) + t.astype(np.float64)[:, None] * d.astype(np.float64)
    assert (np.abs(got.astype(np.float64) - want)[~bad] <= 0.5 * (1 + 1e-6) * _ulp(want)[~bad]).all()  # one rounding


# ------------------------------------------------------------------------------------------------------------------------------------
# bracket
# ------------------------------------------------------------------------------------------------------------------------------------
def test_bracket_all_patterns_of_five_samples(S):
    rng = np.random.default_rng(5)
    K, rep = 5, 8
    pat = np.repeat((np.arange(32)[:, None] >> np.arange(K)[None, :] & 1).astype(bool), rep, 0)  # (256, 5), every pattern eight times
    dt, iso = float(np.float32(0.01)), 0.25
    t0 = float(np.float32(-1.7 * dt))
    f, redrawn = draw_rows(rng, len(pat), K, t0, dt, iso, pat)
    assert np.array_equal(clean(f) < iso, pat)
    print(f"patterns: {redrawn} of {len(pat)} lines drawn again")
    assert redrawn <= 0.01 * len(pat)
    rgb = rng.random((len(pat), K, 3)).astype(np.float32)
    state = check_bracket(S, f, rgb, t0, dt, iso)
    assert (state[:, COLS["found"]] == 0).sum() == 2 * rep  # all inside, all outside
    check_bracket(S, f, None, t0, dt, iso)


def test_bracket_random_rows(S):
    """K in {2, 3, 9, 64, 65, 130, 256} x n in {1, 63, 64, 65, 257}.  A row has to be drawn again when its two best |tc| tie in the restatement,
    which two patterns do exactly -- an inside sample between two non-finite ones, and a sample equal to iso between two inside ones: both
    pairs then cut at the middle sample -- so the share of such rows is counted over all 3150 lines of the test."""
    sizes, Ks, total = (1, 63, 64, 65, 257), (2, 3, 9, 64, 65, 130, 256), 0
    dt, iso = float(np.float32(0.0037)), -0.5
    for K in Ks:
        rng = np.random.default_rng(1000 + K)
        t0 = float(np.float32(-0.37 * (K - 1) * dt))
        for n in sizes:
            f, redrawn = draw_rows(rng, n, K, t0, dt, iso)
            total += redrawn
            print(f"K={K} n={n}: {redrawn} lines drawn again, {np.isfinite(f).mean():.3f} finite, {(f == np.float32(iso)).mean():.3f} equal to iso")
            check_bracket(S, f, rng.random((n, K, 3)).astype(np.float32) if n != 64 else None, t0, dt, iso)
    print(f"{total} of {len(Ks) * sum(sizes)} lines drawn again")
    assert total <= 0.01 * len(Ks) * sum(sizes)


def test_bracket_is_deterministic(S):
    from vanerf_amd import _ffi
    rng = np.random.default_rng(9)
    n, K, dt, iso = 257, 130, float(np.float32(0.0037)), 0.0
    t0 = float(np.float32(-0.37 * (K - 1) * dt))
    f, _ = draw_rows(rng, n, K, t0, dt, iso)
    ft, ct = torch.from_numpy(f).cuda(), torch.from_numpy(rng.random((n, K, 3)).astype(np.float32)).cuda()
    first = S.line_bracket(ft, t0, dt, iso, ct)
    filled = torch.full((n, STATE_FLOATS), float("nan"), device="cuda")
    _ffi.check(_ffi.lib.vanerf_line_bracket(_ptr(ft), _ptr(ct), n, K, t0, dt, iso, _ptr(filled), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = S.line_bracket(ft, t0, dt, iso, ct)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), filled.view(torch.int32)) and torch.equal(first.view(torch.int32), third.view(torch.int32))
    assert int(_ffi.lib.vanerf_line_state_floats()) == STATE_FLOATS == S.LINE_STATE_FLOATS
    assert set(S.line_state(first)) == set(COLS) and all(torch.equal(v, first[:, COLS[k]]) for k, v in S.line_state(first).items())


# ------------------------------------------------------------------------------------------------------------------------------------
# refine
# ------------------------------------------------------------------------------------------------------------------------------------
def test_refine_on_a_quadratic_field(S):
    """Lines run radially through points on the sphere of radius 0.9 about o; the field |p - c|^2 - 1 (c = 0) is quadratic in t.  The last 16
    lines have a zero direction: they stay inside, have no crossing and must be left alone."""
    rng = np.random.default_rng(21)
    n, dead, K, iso, rounds = 321, 16, 9, 0.0, 6
    o = np.float32([0.05, -0.03, 0.02])
    u = rng.standard_normal((n, 3))
    u = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    base = (o + np.float32(0.9) * u).astype(np.float32)
    u[n - dead:] = 0.0
    t0, dt = float(np.float32(-0.3)), float(np.float32(0.075))
    bt, ut = torch.from_numpy(base).cuda(), torch.from_numpy(u).cuda()

    def field(pts):  # fp64 from the kernel's own points, rounded to fp32
        p = pts.cpu().numpy().astype(np.float64)
        return torch.from_numpy(((p * p).sum(-1) - 1.0).astype(np.float32)).cuda()

    state = S.line_bracket(field(S.line_points(bt, ut, K, t0, dt)).view(n, K), t0, dt, iso)
    start = state.clone()
    st = state.cpu().numpy().astype(np.float64)
    live = st[:, COLS["found"]] == 1.0
    assert live[:n - dead].all() and not live[n - dead:].any()
    width = st[live, 1] - st[live, 0]
    assert (np.abs(width - dt) <= 2 * EPS32 * 0.3).all()  # a coarse pair
    for r in range(rounds):
        f_new = field(S.line_points(bt, ut, t=S.line_state(state)["t_next"].contiguous()))
        want = ref_refine(state.cpu().numpy(), f_new.cpu().numpy(), iso)
        assert S.line_refine(state, f_new, iso) is state
        st = state.cpu().numpy().astype(np.float64)
        ta, tb, ga, gb, t_est = (st[live, COLS[k]] for k in ("ta", "tb", "ga", "gb", "t_est"))
        assert ((ga < iso) != (gb < iso)).all(), r                       # the ends still straddle iso
        assert (ta <= t_est).all() and (t_est <= tb).all(), r
        ratio = (tb - ta) / width
        print(f"round {r}: width ratio max {ratio.max():.9f} (bound {0.875 * (1 + 4 * EPS32):.9f}), widest {(tb - ta).max():.3e}")
        assert (tb - ta <= 0.875 * width * (1.0 + 4.0 * EPS32)).all(), r
        width = tb - ta
        # the new ends are the restatement's, bit for bit; the estimates to the bracket tolerance
        for k in ("ta", "tb", "ga", "gb"):
            assert np.array_equal(st[:, COLS[k]], want[:, COLS[k]]), (r, k)
        assert np.abs(st[live][:, [11, 15]] - want[live][:, [11, 15]]).max() <= 4.0 * EPS32 * 0.3, r
    # the exact crossing of |b + t u - c|^2 = 1 on each line (fp64, from the fp32 base and direction): t = -b.u + sqrt((b.u)^2 - |b|^2 + 1)
    b64, u64 = base.astype(np.float64)[live], u.astype(np.float64)[live]
    uu, bu = (u64 * u64).sum(-1), (b64 * u64).sum(-1)
    t_star = (-bu + np.sqrt(bu * bu - uu * ((b64 * b64).sum(-1) - 1.0))) / uu
    err = np.abs(st[live, COLS["t_est"]] - t_star)
    print(f"after {rounds} rounds: max |t_est - t*| = {err.max():.3e}, widths {width.min():.3e} .. {width.max():.3e}")
    assert (err <= width).all()
    assert torch.equal(state[n - dead:].view(torch.int32), start[n - dead:].view(torch.int32))  # not found: untouched, bit for bit


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end on the synthetic two-hand frame (frame seed 3, the recipe of tests/test_surface_field.py)
# ------------------------------------------------------------------------------------------------------------------------------------
BAND, SAMPLES, REFINE = 0.004, 9, 4


@pytest.fixture(scope="module")
def batch(S):
    from vanerf_amd import synth
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    return frame, synth.to_tr_batch(synth.to_device(frame, "cuda"))


def _steps():
    return float(np.float32(-BAND)), float(np.float32(2.0 * BAND / (SAMPLES - 1)))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_register_surface_random_weights(S, batch, precision):
    """On the MI355X, both precisions: 1301 of the 1558 vertices have a crossing within the band; the widest final bracket is 5.862e-4, the bound
    dt (7/8)^4 itself (where f jumps across the surface the secant step is held at 1/8 of the bracket in every round)."""
    from tests.test_surface_field import _net
    net = _net(precision)
    _, trb = batch
    reg = S.register_surface(net, trb, samples=SAMPLES, band=BAND, refine=REFINE)
    mano, faces = trb["targets"]["vert_world"][0], trb["targets"]["face_world"][0]
    nv = mano.shape[0]
    assert nv == 1558 and torch.equal(reg["mano_verts"], mano) and torch.equal(reg["faces"].long(), faces.long()) and reg["faces"].shape == (3108, 3)
    assert all(reg[k].is_cuda for k in ("verts", "faces", "colors", "displacement", "found", "normals", "mano_verts"))
    assert reg["found"].dtype == torch.bool and reg["verts"].shape == (nv, 3) and reg["colors"].shape == (nv, 3) and reg["displacement"].shape == (nv,)
    assert torch.equal(reg["normals"].view(torch.int32), S.vertex_normals(reg["mano_verts"], reg["faces"]).view(torch.int32))

    # the found set, from the coarse field recomputed on the same points (a per-point function: the same bits)
    t0, dt = _steps()
    iso = 0.0
    coarse = S.field_at_points(net, trb, S.line_points(mano, reg["normals"], SAMPLES, t0, dt)).view(nv, SAMPLES).cpu().numpy()
    inside = clean(coarse) < iso
    want_found = (inside[:, :-1] != inside[:, 1:]).any(1)
    found = reg["found"].cpu().numpy()
    print(f"{precision}: {found.sum()} of {nv} vertices have a crossing within {BAND} m")
    assert np.array_equal(found, want_found)  # (so no consecutive coarse pair of a vertex that was not found straddles iso)
    assert not (inside[~found, :-1] != inside[~found, 1:]).any()
    assert 0 < found.sum()

    # the final bracket: one end inside, one outside, when the field is evaluated there again; and its width
    st = S.line_state(reg["state"])
    fa = S.field_at_points(net, trb, S.line_points(mano, reg["normals"], t=st["ta"].contiguous())).cpu().numpy()
    fb = S.field_at_points(net, trb, S.line_points(mano, reg["normals"], t=st["tb"].contiguous())).cpu().numpy()
    assert ((clean(fa) < iso) != (clean(fb) < iso))[found].all()
    ta, tb = st["ta"].cpu().numpy().astype(np.float64), st["tb"].cpu().numpy().astype(np.float64)
    print(f"{precision}: final widths up to {(tb - ta)[found].max():.3e} (bound {dt * 0.875 ** REFINE:.3e})")
    assert ((tb - ta)[found] <= dt * 0.875 ** REFINE * (1 + 1e-6)).all()

    # the vertices: fmaf(t_est, n, v) within one ulp where found, the MANO bits and a NaN displacement elsewhere
    disp = reg["displacement"].cpu().numpy()
    assert np.isfinite(disp[found]).all() and np.isnan(disp[~found]).all() and np.array_equal(_bits(disp), _bits(st["t_est"].cpu().numpy()))
    assert (ta[found] <= disp[found]).all() and (disp[found] <= tb[found]).all() and (np.abs(disp[found]) <= BAND * (1 + 1e-6)).all()
    v64, n64 = mano.cpu().numpy().astype(np.float64), reg["normals"].cpu().numpy().astype(np.float64)
    want = v64 + np.where(found, disp, 0.0).astype(np.float64)[:, None] * n64
    got = reg["verts"].cpu().numpy()
    assert (np.abs(got.astype(np.float64) - want) <= _ulp(want))[found].all()
    assert np.array_equal(_bits(got[~found]), _bits(mano.cpu().numpy()[~found]))
    assert torch.isfinite(reg["colors"][reg["found"]]).all()

    # the module's method, no colours, and a second call
    again = net.register_surface(trb, samples=SAMPLES, band=BAND, refine=REFINE)
    for k in ("verts", "faces", "colors", "displacement", "found", "normals", "mano_verts", "state"):
        assert torch.equal(again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k],
                           reg[k].view(torch.int32) if reg[k].dtype == torch.float32 else reg[k]), k
    bare = S.register_surface(net, trb, samples=SAMPLES, band=BAND, refine=REFINE, colors=False)
    assert bare["colors"] is None and torch.equal(bare["verts"].view(torch.int32), reg["verts"].view(torch.int32))
    assert torch.equal(bare["found"], reg["found"])


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_register_surface_zero_weights_stays_on_mano(S, batch, precision):
    """f = mesh_sdf: the surface is the MANO mesh itself.  Checked on the CPU with the oracle's mesh query when this test was written: 1556 of
    the 1558 vertices have a crossing and the largest |t| is 4.99e-4; the two misses have a negative mesh distance along the whole line.  The
    oracle's distance has a floor (it reads +-1.000e-3 at a vertex) and jumps through zero at the surface, so refinement bisects towards the jump.
    On the MI355X, both precisions: 1556 found, largest |displacement| 3.018e-5."""
    from tests.test_surface_field import _net
    net = _net(precision, zero=True)
    _, trb = batch
    reg = S.register_surface(net, trb, samples=SAMPLES, band=BAND, refine=REFINE, colors=False)
    _, dt = _steps()
    found = reg["found"].cpu().numpy()
    disp = reg["displacement"].cpu().numpy()
    print(f"{precision}: {found.sum()} of {len(found)} found, max |displacement| = {np.abs(disp[found]).max():.3e} (dt {dt:.3e})")
    assert found.sum() >= 1550
    assert (np.abs(disp[found]) <= dt).all()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_field_at_points_equals_field_on_grid(S, batch, precision):
    from tests.test_surface_field import DIMS, _net
    net = _net(precision)
    frame, trb = batch
    f, rgb = S.field_on_grid(net, trb, dims=DIMS, want_rgb=True)
    pts = S.grid_points(*S.grid_spec(trb["dr_data"]["bounds"], dims=DIMS))
    for slab in (1000, pts.shape[0]):
        g, c = S.field_at_points(net, trb, pts, want_rgb=True, slab_points=slab)
        assert torch.equal(g.view(torch.int32), f.reshape(-1).view(torch.int32)) and torch.equal(c.view(torch.int32), rgb.reshape(-1, 3).view(torch.int32)), slab
    alone = S.field_at_points(net, trb, pts, slab_points=1000)
    assert torch.equal(alone.view(torch.int32), f.reshape(-1).view(torch.int32))
