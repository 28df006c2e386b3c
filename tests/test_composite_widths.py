"""The forward and backward composite and the importance kernels at every width their launchers dispatch on (vanerf_amd/csrc/render_kernels.hip; the composite's scan, sums, gather and width dispatch are csrc/wave_ray.h's).

`launch_composite` picks composite_wave_kernel<1|2|3|4> for S <= 64 / 128 / 192 / 256 samples per ray and the one-thread-per-ray
composite_kernel above; `vanerf_importance_merge` picks importance_merge_wave_kernel<1|2|4> for max(Sc, Sf) <= 64 / 128 / 256 and the serial
importance_merge_kernel<false> above; `vanerf_importance_sample` always runs the serial <true> (mid-point) form.  Each instantiation is run
here against the fp64 oracle on ray counts that are no multiple of the 4 rays of a block (nor of the 64 of the serial kernels), on both
sides of every threshold, with lanes past the end of a ray, through the two-table gather, without the contribution output and with
sigmoid_beta read from the device.  All inputs are drawn on the CPU from seeded generators, so the same numbers exist on every machine.

Bars.  Composite: per output and per case max(2e-5, 4 E32), E32 = max |fp32 oracle - fp64 oracle| of that output on the same rays (the
2e-5 floor is what test_hip_parity.py::test_composite holds the kernel to).  depth and sdf are sums divided by acc + 1e-8: on a nearly
empty ray the fp32 oracle itself is O(1e-3 .. 1e-1) off fp64, so they are held on CLEAN rays only (fp64 acc > 0.05 or acc < 1e-13: the
criterion of test_weight_families.py::test_composite_with_the_familys_sigmoid_beta), with E32 taken over those rays; at least 80 % of the
rays of every case must be clean.  Importance: z_new within 1e-6 of the oracle; the searchsorted index is equal to the oracle's at every
DECIDED draw (further than 2^-20 from every interior entry of the fp32 oracle's cdf: where the inner contributions vanish the cdf is k / nb
and a uniform draw j / (Sf - 1) can hit it exactly) and within one elsewhere; at least 98 % of the draws of every case must be decided.  One refinement, which only asks more of the kernel:
a draw of exactly 0 (the first uniform draw) is decided whatever the cdf, because cdf[0] is 0 exactly and cdf[1] = (c + 1e-5) / sum is
positive on every side, so its index is 1 everywhere.  With 255 bins the first bin of a ray is often narrower than 2^-20 (1e-5 / sum =
3e-7), and without this (257, 8) would have 22 of its 560 uniform draws undecided: the 11 at u = 0 and 11 at u = 1 next to such a bin.
The 11 at u = 1 stay undecided (98.04 % decided).  Both conditions are re-derived from the oracle alone by the first test here that needs no GPU.

The backward composite (`vanerf_composite_backward`, composite_backward_kernel<1|2|3|4> for S <= 64 / 128 / 192 / 256, refused above) is held in
sections 4 and 5 against torch.autograd through the same oracle in fp64 on the CPU, with the clamped sigmoid_beta as a per-ray leaf, so that one
backward call yields every ray's share of d_beta.  Bars per RAY: |HIP - fp64|_max <= max(2e-4, 4 E32) x (largest |fp64 gradient| of that ray)
+ 1e-6, and per ray's d_beta the same with the largest |fp64 d_beta| of the case as the scale; E32 is what the fp32 oracle's own autograd is off
by in the same units (at most 2.1e-5 / 3.9e-6, so the 2e-4 floor of test_autograd.py::test_composite_backward_against_autograd governs).  With
gradients on depth and sdf the gradients contain 1 / (acc + 1e-8) and the clean rays are held (the same >= 80 % condition); with gradients on
colour and alpha only, every ray is.  The second test that needs no GPU re-derives these conditions."""
import ctypes
import functools

import pytest
import torch

from oracle import vanerf_oracle as orc

gpu = pytest.mark.gpu

RAYS = 37  # no multiple of the 4 rays of a wave-kernel block, nor of the 64 threads of a serial-kernel block
COMPOSITE_S = [1, 2, 3, 63, 64, 65, 128, 129, 192, 193, 255, 256, 257, 300]
BETAS = [0.1, 0.01, 1e-3]  # the last one is clamped to 2e-3 by both sides
FLOOR = 2e-5
MIN_CLEAN = 0.8
IMPORTANCE_SHAPES = [(3, 1), (3, 64), (16, 64), (64, 64), (65, 17), (128, 128), (129, 40), (40, 200), (256, 256), (257, 8), (8, 257)]
Z_NEW_BAR = 1e-6
DECIDED_MARGIN = 2.0 ** -20
MIN_DECIDED = 0.98
OUTPUTS = ("color", "depth", "alpha", "contrib", "sdf")  # the order rgba2out and renderer.composite return them in
BACKWARD_S = [1, 2, 3, 63, 64, 65, 128, 129, 192, 193, 255, 256]  # composite_backward_kernel<1|2|3|4> on both sides of 64 / 128 / 192
BACKWARD_TABLES = [(1, 1), (40, 24), (33, 32), (64, 64), (100, 29), (100, 92), (100, 93), (128, 128), (255, 1), (1, 255)]  # 2 .. 256 merged samples
BACKWARD_TABLE_BETAS = [0.05, 1e-3]
GRAD_FLOOR = 2e-4  # relative, and
GRAD_ABS = 1e-6    # absolute: test_autograd.py::test_composite_backward_against_autograd's own, here per ray
UPSTREAM = ("full", "part")  # gradients on all four outputs / on colour and alpha only


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


def dev(t):
    return t.cuda()


def bits(t):
    """The bit patterns of an fp32 tensor on the host (equal NaNs compare equal)."""
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------
# inputs and references (computed once per case, never modified)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def composite_inputs(S, rays=RAYS):
    """test_composite's distribution plus three degenerate rays (near == far), three empty ones and, for S > 1, three with one opaque sample."""
    g = torch.Generator().manual_seed(100 * S)
    rgba = torch.rand(rays, S, 5, generator=g)
    rgba[..., 0] = torch.relu(torch.randn(rays, S, generator=g)) * 0.05
    z = torch.sort(torch.rand(rays, S, generator=g) * 0.3 + 0.8, -1)[0]
    msdf = torch.randn(rays, S, generator=g) * 0.02
    z[:3] = z[:3, :1]
    rgba[3:6, :, 0] = 5.0
    if S > 1:
        rgba[6:9, S // 2, 0] = -5.0
    return rgba.contiguous(), z.contiguous(), msdf.contiguous()


@functools.lru_cache(maxsize=None)
def composite_reference(S, beta):
    """fp64 oracle, clean rays and E32 per output (depth and sdf: over the clean rays) of one case."""
    rgba, z, msdf = composite_inputs(S)
    sd = {"sigmoid_beta": torch.tensor([beta])}
    want32 = orc.rgba2out(sd, rgba[None], z[None], msdf[None, ..., None])
    sd64 = {"sigmoid_beta": sd["sigmoid_beta"].double()}
    want64 = orc.rgba2out(sd64, rgba[None].double(), z[None].double(), msdf[None, ..., None].double())
    want32 = dict(zip(OUTPUTS, (t[0] for t in want32)))
    want64 = dict(zip(OUTPUTS, (t[0] for t in want64)))
    acc = want64["alpha"]
    clean = (acc > 0.05) | (acc < 1e-13)
    held = {k: clean if k in ("depth", "sdf") else torch.ones_like(clean) for k in OUTPUTS}
    e32 = {k: (want32[k].double() - want64[k])[held[k]].abs().max().item() for k in OUTPUTS}
    return want64, held, e32, clean.float().mean().item()


@functools.lru_cache(maxsize=None)
def importance_inputs(Sc, Sf):
    rays = 70 if max(Sc, Sf) > 256 else 9  # the serial kernel runs 64 rays a block
    g = torch.Generator().manual_seed(1000 * Sc + Sf)
    contrib = torch.rand(rays, Sc, generator=g) ** 6
    contrib[0] = 0.0
    z = torch.sort(torch.rand(rays, Sc, generator=g) * 0.3 + 0.8, -1)[0]
    z[1] = z[1, :1]
    u = torch.rand(rays, Sf, generator=g)
    return contrib.contiguous(), z.contiguous(), u.contiguous()


def oracle_cdf(contrib_inner):
    """The cdf of orc.importance_sample, by its own operations (fp64 total, fp32 pdf, torch's CPU cumsum)."""
    c = contrib_inner + 1e-5
    pdf = c / c.double().sum(-1, keepdim=True).float()
    return torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)


@functools.lru_cache(maxsize=None)
def importance_reference(Sc, Sf, uniform):
    """Oracle z_new and searchsorted index, and which draws are decided (further than 2^-20 from every interior cdf entry)."""
    contrib, z, u = importance_inputs(Sc, Sf)
    inner = contrib[:, 1:-1].contiguous()
    z_mid = 0.5 * (z[:, 1:] + z[:, :-1])
    want, _, idx = orc.importance_sample(inner[None], z_mid[None], Sf, uniform=uniform, u=None if uniform else u[None], return_idx=True)
    draws = torch.linspace(0.0, 1.0, steps=Sf).expand(z.shape[0], -1) if uniform else u
    interior = oracle_cdf(inner)[:, 1:-1]  # cdf[0] = 0 exactly and the index is clamped at the last entry on every side
    decided = draws == 0.0  # index 1 on every side, however small the first bin is (module docstring)
    if interior.shape[1]:
        decided = decided | ((draws[:, :, None].double() - interior[:, None, :].double()).abs().min(-1)[0] > DECIDED_MARGIN)
    else:
        decided = torch.ones_like(draws, dtype=torch.bool)
    return want[0], idx[0], decided, inner, z_mid.contiguous()


@functools.lru_cache(maxsize=None)
def backward_inputs(Sa, Sn=0):
    """The tables, depths and origin map of one backward case -- composite_inputs(Sa), or for Sn > 0 the two tables and the random origin map of
    test_two_tables_give_the_bits_of_one_table -- and its upstream gradients, from a generator of their own."""
    if Sn == 0:
        ra, z, ma = composite_inputs(Sa)
        rn = mn = src = None
    else:
        ra, ma, rn, mn, g = _two_tables(Sa, Sn, 100 * Sa + Sn)
        z = torch.sort(torch.rand(RAYS, Sa + Sn, generator=g) * 0.3 + 0.8, -1)[0].contiguous()
        perm = torch.argsort(torch.rand(RAYS, Sa + Sn, generator=g), dim=1)  # merged position -> table entry
        src = torch.where(perm < Sa, perm, -(perm - Sa) - 1).to(torch.int32).contiguous()
        assert (src >= 0).any() and (src < 0).any() and torch.equal(torch.sort(perm, -1)[0], torch.arange(Sa + Sn).expand(RAYS, -1))
    gu = torch.Generator().manual_seed(500000 + 1000 * Sa + Sn)
    g_color, g_depth, g_alpha, g_sdf = torch.randn(RAYS, 3, generator=gu), *(torch.randn(RAYS, generator=gu) for _ in range(3))
    ups = {"full": (g_color, g_depth, g_alpha, g_sdf), "part": (g_color, None, g_alpha, None)}
    return ra, z, ma, rn, mn, src, ups


def _oracle_gradients(Sa, Sn, beta, dtype):
    """torch.autograd through orc.rgba2out on the CPU in `dtype`: per upstream set (d_rgba, d_rgba_n or None, d_beta per ray), and acc.  The leaf
    is the CLAMPED sigmoid_beta, one per ray (the header defines d_beta against it; below 2e-3 the oracle's own clamp would give 0 everywhere)."""
    ra, z, ma, rn, mn, src, ups = backward_inputs(Sa, Sn)
    clamped = max(torch.tensor(beta, dtype=torch.float32).item(), 2e-3)
    b = torch.full((RAYS, 1), clamped, dtype=dtype, requires_grad=True)
    xa = ra.to(dtype).requires_grad_(True)
    xn = None
    if Sn:
        xn = rn.to(dtype).requires_grad_(True)
        rgba, msdf = _gathered(xa, ma.to(dtype), xn, mn.to(dtype), src)
    else:
        rgba, msdf = xa, ma.to(dtype)
    color, depth, acc, _, sdf = (t[0] for t in orc.rgba2out({"sigmoid_beta": b}, rgba[None], z.to(dtype)[None], msdf[None, ..., None]))
    leaves = [xa, b] + ([xn] if Sn else [])
    grads = {}
    for name, (gc, gd, ga, gs) in ups.items():
        loss = (color * gc.to(dtype)).sum() + (acc * ga.to(dtype)).sum()
        if gd is not None:
            loss = loss + (depth * gd.to(dtype)).sum() + (sdf * gs.to(dtype)).sum()
        d = torch.autograd.grad(loss, leaves, retain_graph=True)
        grads[name] = (d[0], d[2] if Sn else None, d[1][:, 0])
    return grads, acc.detach()


def _per_ray_max(tables):
    """max |.| per ray over the tables of one ray-major gradient (d_rgba and, when there is one, d_rgba_n: together the ray's gradient)."""
    return torch.stack([t.double().abs().flatten(1).amax(1) for t in tables if t is not None]).amax(0)


def _ray_errors(have, want):
    return _per_ray_max([None if w is None else h.detach().cpu().double() - w for h, w in zip(have, want)])


@functools.lru_cache(maxsize=None)
def backward_reference(Sa, Sn, beta):
    """Per upstream set of one case: the fp64 gradients, the held rays (full: the clean ones, gradients there divide by acc + 1e-8; part: all),
    each ray's scale, the case's d_beta scale, and E32 / E32_beta: what the fp32 oracle's own autograd is off by, in the units of the bars."""
    want64, acc = _oracle_gradients(Sa, Sn, beta, torch.float64)
    want32, _ = _oracle_gradients(Sa, Sn, beta, torch.float32)
    clean = (acc > 0.05) | (acc < 1e-13)
    ref = {}
    for name in UPSTREAM:
        d_a, d_n, d_b = want64[name]
        held = clean if name == "full" else torch.ones_like(clean)
        scale_ray = _per_ray_max([d_a, d_n])
        excess = (_ray_errors(want32[name][:2], (d_a, d_n)) - GRAD_ABS).clamp_min(0.0)
        e32 = (excess / scale_ray.clamp_min(1e-300))[held].max().item()  # (a ray whose fp64 gradient is exactly 0: no excess, 0)
        scale_case = d_b[held].abs().max().item()
        e32_b = ((want32[name][2].double() - d_b).abs() - GRAD_ABS).clamp_min(0.0)[held].max().item() / max(scale_case, 1e-300)
        ref[name] = {"want": (d_a, d_n, d_b), "held": held, "scale_ray": scale_ray, "scale_case": scale_case, "e32": e32, "e32_beta": e32_b}
    return ref, clean.float().mean().item()


def backward_cases():
    return [(S, 0, beta) for S in BACKWARD_S for beta in BETAS] + [(Sa, Sn, beta) for Sa, Sn in BACKWARD_TABLES for beta in BACKWARD_TABLE_BETAS]


def test_the_recipes_keep_their_conditions():
    """From the oracle alone (no GPU): at least 80 % of the rays of every composite case are clean and at least 98 % of the draws of every
    importance case are decided, so the recipes cannot drift under what the GPU tests hold without this failing."""
    for S in COMPOSITE_S:
        for beta in BETAS:
            want64, held, e32, clean = composite_reference(S, beta)
            print(f"composite S={S} beta={beta}: clean {clean:.3f}, E32 " + " ".join(f"{k} {e32[k]:.2e}" for k in OUTPUTS))
            assert all(torch.isfinite(v).all() for v in want64.values())
            assert clean >= MIN_CLEAN, (S, beta, clean)
    for Sc, Sf in IMPORTANCE_SHAPES:
        for uniform in (True, False):
            want, idx, decided, _, _ = importance_reference(Sc, Sf, uniform)
            frac = decided.float().mean().item()
            print(f"importance Sc={Sc} Sf={Sf} {'uniform' if uniform else 'random'}: {int((~decided).sum())} of {decided.numel()} draws undecided")
            assert torch.isfinite(want).all()
            assert frac >= MIN_DECIDED, (Sc, Sf, uniform, frac)


def test_the_backward_recipes_keep_their_conditions():
    """From the oracle alone (no GPU), for every backward case: the fp64 gradients are finite, at least 80 % of the rays are clean, and four times
    the fp32 oracle's own error stays below the 2e-4 floor -- so the floor, not E32, is what the GPU tests hold the kernel to.  If the last
    assertion fails, the recipe has drifted to where the floor no longer governs."""
    for Sa, Sn, beta in backward_cases():
        ref, clean = backward_reference(Sa, Sn, beta)
        assert clean >= MIN_CLEAN, (Sa, Sn, beta, clean)
        for name in UPSTREAM:
            r = ref[name]
            print(f"composite backward Sa={Sa} Sn={Sn} beta={beta} {name}: clean {clean:.3f}, E32 {r['e32']:.2e}, E32_beta {r['e32_beta']:.2e}, "
                  f"largest |d_rgba| {r['scale_ray'].max().item():.2e}, |d_beta| {r['scale_case']:.2e}")
            assert all(torch.isfinite(t).all() for t in r["want"] if t is not None), (Sa, Sn, beta, name)
            assert 4.0 * r["e32"] <= GRAD_FLOOR and 4.0 * r["e32_beta"] <= GRAD_FLOOR, (Sa, Sn, beta, name, r["e32"], r["e32_beta"])


# ------------------------------------------------------------------------------------------------
# 1. forward composite against the fp64 oracle, every instantiation
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("S", COMPOSITE_S)
def test_composite_against_fp64_at_every_width(R, S, beta):
    """Largest |HIP - fp64 oracle| per output on the MI355X over all 42 cases (bar 2e-5: 4 E32 stays below the floor on the held rays):
    see DESIGN.md section 5."""
    rgba, z, msdf = composite_inputs(S)
    want64, held, e32, clean = composite_reference(S, beta)
    assert clean >= MIN_CLEAN
    got = dict(zip(OUTPUTS, R.composite(dev(rgba), dev(z), dev(msdf), beta)))
    failed = []
    for k in OUTPUTS:
        bar = max(FLOOR, 4.0 * e32[k])
        err = (got[k].cpu().double() - want64[k])[held[k]].abs().max().item()
        print(f"composite S={S} beta={beta} {k}: E32 {e32[k]:.3e} bar {bar:.3e} |HIP - fp64| {err:.3e} (clean rays {clean:.3f})")
        if not err <= bar:  # a NaN fails
            failed.append((k, err, bar))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------
# 2. bit-exact properties of the composite
# ------------------------------------------------------------------------------------------------
def _two_tables(Sa, Sn, seed, rays=RAYS):
    g = torch.Generator().manual_seed(seed)
    def table(S):
        q = torch.rand(rays, S, 5, generator=g)
        q[..., 0] = torch.relu(torch.randn(rays, S, generator=g)) * 0.05
        return q.contiguous(), (torch.randn(rays, S, generator=g) * 0.02).contiguous()
    return table(Sa) + table(Sn) + (g,)


def _gathered(ra, ma, rn, mn, src):
    """The one table that the origin map names, gathered on the host."""
    take = torch.where(src >= 0, src.long(), ra.shape[1] + (-src.long() - 1))
    rgba = torch.gather(torch.cat([ra, rn], 1), 1, take[..., None].expand(-1, -1, 5)).contiguous()
    return rgba, torch.gather(torch.cat([ma, mn], 1), 1, take).contiguous()


def _assert_same_bits(got, want, what):
    for k, a, b in zip(OUTPUTS, got, want):
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            assert torch.equal(bits(a), bits(b)), (what, k)


@gpu
@pytest.mark.parametrize("Sa,Sn", [(40, 24), (64, 64), (100, 93), (128, 128), (200, 57)])  # 64, 128, 193, 256 and 257 (serial kernel) samples
def test_two_tables_give_the_bits_of_one_table(R, Sa, Sn):
    """'Identical arithmetic for one table and for the merged order of two tables on the same samples': the composite through a random origin
    map (a permutation of both tables per ray, both signs) gives the bits of the composite of the table gathered through it on the host."""
    ra, ma, rn, mn, g = _two_tables(Sa, Sn, 100 * Sa + Sn)
    St = Sa + Sn
    z = torch.sort(torch.rand(RAYS, St, generator=g) * 0.3 + 0.8, -1)[0].contiguous()
    perm = torch.argsort(torch.rand(RAYS, St, generator=g), dim=1)  # merged position -> table entry
    src = torch.where(perm < Sa, perm, -(perm - Sa) - 1).to(torch.int32).contiguous()
    assert (src >= 0).any() and (src < 0).any() and torch.equal(torch.sort(perm, -1)[0], torch.arange(St).expand(RAYS, -1))
    rgba, msdf = _gathered(ra, ma, rn, mn, src)
    for beta in (0.05, 1e-3):
        merged = R.composite_merged(dev(ra), dev(ma), dev(rn), dev(mn), dev(src), dev(z), beta, want_contrib=True)
        single = R.composite(dev(rgba), dev(z), dev(msdf), beta)
        _assert_same_bits(merged, single, (Sa, Sn, beta))
        assert all(torch.isfinite(t).all() for t in single)


@gpu
@pytest.mark.parametrize("Sc,Sf", [(64, 64), (40, 30)])
def test_merge_then_composite(R, Sc, Sf):
    """The origin map and merged depths that importance_merge writes, fed to composite_merged, against composite on the gathered table."""
    contrib, z, _ = importance_inputs(Sc, Sf)
    rays = z.shape[0]
    ra, ma, rn, mn, _ = _two_tables(Sc, Sf, 7000 + 100 * Sc + Sf, rays=rays)
    z_new, z_fine, src = R.importance_merge(dev(contrib), dev(z), Sf)
    merged = R.composite_merged(dev(ra), dev(ma), dev(rn), dev(mn), src, z_fine, 0.05, want_contrib=True)
    rgba, msdf = _gathered(ra, ma, rn, mn, src.cpu())
    single = R.composite(dev(rgba), z_fine, dev(msdf), 0.05)
    _assert_same_bits(merged, single, (Sc, Sf))


@gpu
@pytest.mark.parametrize("S", [64, 129, 257])
def test_composite_without_the_contribution_output(R, S):
    """contrib == NULL (what render_pass runs outside debug) changes no bit of the other outputs."""
    rgba, z, msdf = (dev(t) for t in composite_inputs(S))
    for beta in (0.05, 1e-3):
        with_c = R.composite(rgba, z, msdf, beta, want_contrib=True)
        without = R.composite(rgba, z, msdf, beta, want_contrib=False)
        assert without[3] is None and with_c[3] is not None
        for k, a, b in zip(OUTPUTS, without, with_c):
            if k != "contrib":
                assert torch.equal(bits(a), bits(b)), (S, beta, k)


@gpu
def test_composite_handle_equals_the_number(R):
    """vanerf_composite_handle reads sigmoid_beta from the handle's device copy: the bits of vanerf_composite with the same number, above and
    below the 2e-3 clamp of sdf_activation and after an update on the device."""
    from vanerf_amd import synth
    sd = synth.make_full_weights(0)

    def check(w, beta):
        assert w.beta == max(torch.tensor(beta).item(), 2e-3)
        for S in (65, 257):  # a wave kernel and the serial kernel
            rgba, z, msdf = (dev(t) for t in composite_inputs(S))
            _assert_same_bits(R.composite(rgba, z, msdf, w), R.composite(rgba, z, msdf, w.beta), (S, beta))
            _assert_same_bits(R.composite(rgba, z, msdf, w, want_contrib=False), R.composite(rgba, z, msdf, w.beta, want_contrib=False), (S, beta))

    for beta in (0.05, 1e-4):
        sd["sigmoid_beta"] = torch.tensor([beta])
        check(R.PackedWeights(sd, mode="fp32"), beta)
    w = R.PackedWeights(sd, mode="fp32")  # sigmoid_beta 1e-4
    on_dev = {k: v.cuda() for k, v in sd.items()}
    on_dev["sigmoid_beta"] = torch.tensor([0.03], device="cuda")
    before = R.composite(*(dev(t) for t in composite_inputs(65)), w)
    w.update(on_dev)
    check(w, 0.03)
    after = R.composite(*(dev(t) for t in composite_inputs(65)), w)
    assert not torch.equal(bits(before[2]), bits(after[2]))  # the update reached the composite


SENTINEL = 0x5A5AC3C3  # the bits the output buffers are pre-filled with


@gpu
@pytest.mark.parametrize("S", [64, 200, 257])
def test_a_rays_result_does_not_depend_on_the_ray_count(R, S):
    """The C entry on the first R' rays of one input set: rows below R' equal the 37-ray call's rows, and every element past row R' of the
    (longer) output buffers still holds what it was filled with -- a retiring tail wave or thread writes nothing."""
    from vanerf_amd._ffi import check, lib
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rgba, z, msdf = (dev(t) for t in composite_inputs(S))
    beta = 0.05
    pad = 65 if S > 256 else 4  # a whole block more than any correct access (every call here, the 37-ray one included, has them)
    widths = dict(zip(OUTPUTS, ((3,), (), (), (S,), ())))
    want = None
    for n in (RAYS, 1, 2, 3, 4, 5):
        out = {k: torch.full((n + pad,) + widths[k], SENTINEL, dtype=torch.int32, device="cuda") for k in OUTPUTS}
        check(lib.vanerf_composite(P(rgba), P(z), P(msdf), S, None, None, 0, None, n, beta, P(out["color"]), P(out["depth"]), P(out["alpha"]),
                                   P(out["sdf"]), P(out["contrib"]), R._stream()))
        out = {k: v.cpu() for k, v in out.items()}
        if want is None:
            want = out
            assert all((v[:n] != SENTINEL).any() for v in want.values())  # something was written
        for k in OUTPUTS:
            assert torch.equal(out[k][:n], want[k][:n]), (S, n, k)
            assert (out[k][n:] == SENTINEL).all(), (S, n, k)


# ------------------------------------------------------------------------------------------------
# 3. importance merge and the mid-point form
# ------------------------------------------------------------------------------------------------
def _check_draws(z_new, idx, Sc, Sf, uniform, what):
    want, want_idx, decided, _, _ = importance_reference(Sc, Sf, uniform)
    assert decided.float().mean().item() >= MIN_DECIDED
    err = (z_new.cpu() - want).abs().max().item()
    d = (idx.cpu().long() - want_idx).abs()
    print(f"{what} Sc={Sc} Sf={Sf} {'uniform' if uniform else 'random'}: |z_new - oracle| {err:.3e} (bar {Z_NEW_BAR:.0e}), "
          f"{int((~decided).sum())} of {decided.numel()} draws undecided, index differs at {int((d != 0).sum())}")
    assert err <= Z_NEW_BAR
    assert (d[decided] == 0).all() and (d <= 1).all()


@gpu
@pytest.mark.parametrize("Sc,Sf", IMPORTANCE_SHAPES)
def test_importance_merge_at_every_width(R, Sc, Sf):
    contrib, z, u = importance_inputs(Sc, Sf)
    rays = z.shape[0]
    for uniform in (True, False):
        kw = {} if uniform else {"u": dev(u)}
        z_new, z_fine, src, idx = R.importance_merge(dev(contrib), dev(z), Sf, want_idx=True, **kw)
        _check_draws(z_new, idx, Sc, Sf, uniform, "importance_merge")
        zn, zf, s = z_new.cpu(), z_fine.cpu(), src.cpu().long()
        both = torch.cat([z, zn], -1)
        assert torch.equal(zf, torch.sort(both, -1)[0])  # the merge is the sort of [z | its own draws]
        col = torch.where(s >= 0, s, Sc + (-s - 1))
        assert torch.equal(torch.sort(col, -1)[0], torch.arange(Sc + Sf).expand(rays, -1))  # each coarse sample and each draw once
        assert torch.equal(torch.gather(both, 1, col), zf)
        tie = zf[:, 1:] == zf[:, :-1]
        assert (col[:, 1:][tie] > col[:, :-1][tie]).all()  # stable: coarse first on ties, equal draws in draw order
        assert tie[1].any()  # (the degenerate ray has ties)


@gpu
@pytest.mark.parametrize("Sc,Sf", IMPORTANCE_SHAPES)
def test_importance_from_midpoints_at_every_width(R, Sc, Sf):
    """vanerf_importance_sample (the serial template's mid-point form) on contrib[1:-1] and the mid-points; above 256 samples importance_merge
    runs the same template and gives the same bits."""
    contrib, z, u = importance_inputs(Sc, Sf)
    for uniform in (True, False):
        kw = {} if uniform else {"u": dev(u)}
        _, _, _, inner, z_mid = importance_reference(Sc, Sf, uniform)
        z_new, idx = R.importance_from_midpoints(dev(inner), dev(z_mid), Sf, want_idx=True, **kw)
        _check_draws(z_new, idx, Sc, Sf, uniform, "importance_from_midpoints")
        if max(Sc, Sf) > 256:
            zn, _, _, ix = R.importance_merge(dev(contrib), dev(z), Sf, want_idx=True, **kw)
            assert torch.equal(bits(z_new), bits(zn)) and torch.equal(idx.cpu(), ix.cpu())


# ------------------------------------------------------------------------------------------------
# 4. composite backward against fp64 autograd of the oracle, every instantiation
# ------------------------------------------------------------------------------------------------
# Bars, per ray r (module docstring of the forward bars applies to the clean rays): |HIP - fp64|_max,r <= max(2e-4, 4 E32) scale_r + 1e-6 with
# scale_r = max |fp64 gradient of ray r| over d_rgba and d_rgba_n together (they are one ray's gradient: the one-table call on the gathered
# table has the same bits), and |d_beta_r - fp64| <= max(2e-4, 4 E32_beta) scale_case + 1e-6 with scale_case = max |fp64 d_beta| over the held
# rays.  2e-4 and 1e-6 are test_autograd.py::test_composite_backward_against_autograd's, applied per ray instead of per tensor.
_HANDLES = {}


def _handle(R, beta):
    """A weight handle whose device copy of sigmoid_beta is `beta`, clamped (only that copy is read by the composite backward)."""
    if beta not in _HANDLES:
        from vanerf_amd import synth
        sd = synth.make_full_weights(0)
        sd["sigmoid_beta"] = torch.tensor([beta])
        _HANDLES[beta] = R.PackedWeights(sd, mode="fp32")
    return _HANDLES[beta]


def _backward(R, w, Sa, Sn, ups):
    ra, z, ma, rn, mn, src, _ = backward_inputs(Sa, Sn)
    d = lambda t: None if t is None else dev(t)
    return R.composite_backward(w, dev(ra), dev(z), dev(ma), *(d(g) for g in ups), rgba_n=d(rn), sdf_n=d(mn), src=d(src))


def _hold_backward(R, Sa, Sn, beta):
    ref, clean = backward_reference(Sa, Sn, beta)
    assert clean >= MIN_CLEAN
    ups = backward_inputs(Sa, Sn)[-1]
    failed = []
    for name in UPSTREAM:
        r = ref[name]
        d_a, d_n, d_b = _backward(R, _handle(R, beta), Sa, Sn, ups[name])
        assert (d_n is None) == (Sn == 0)
        assert all(torch.isfinite(t).all() for t in (d_a, d_n, d_b) if t is not None), (Sa, Sn, beta, name)  # every ray, held or not
        held = r["held"]
        bar = max(GRAD_FLOOR, 4.0 * r["e32"])
        excess = _ray_errors((d_a, d_n), r["want"][:2]) - (bar * r["scale_ray"] + GRAD_ABS)
        rel = ((_ray_errors((d_a, d_n), r["want"][:2]) - GRAD_ABS).clamp_min(0.0) / r["scale_ray"].clamp_min(1e-300))[held].max().item()
        bar_b = max(GRAD_FLOOR, 4.0 * r["e32_beta"])
        err_b = (d_b.cpu().double() - r["want"][2]).abs()
        rel_b = (err_b - GRAD_ABS).clamp_min(0.0)[held].max().item() / max(r["scale_case"], 1e-300)
        print(f"composite backward Sa={Sa} Sn={Sn} beta={beta} {name}: d_rgba E32 {r['e32']:.3e} bar {bar:.3e} (|HIP - fp64| - 1e-6)+ / scale_ray "
              f"{rel:.3e}; d_beta E32 {r['e32_beta']:.3e} bar {bar_b:.3e} (|HIP - fp64| - 1e-6)+ / scale_case {rel_b:.3e} "
              f"(scale_case {r['scale_case']:.3e}, held rays {int(held.sum())} of {RAYS})")
        if not (excess[held] <= 0.0).all():  # a NaN fails
            worst = int(torch.where(held, excess, torch.full_like(excess, -1.0)).argmax())
            failed.append((name, "d_rgba", "ray", worst, rel, bar))
        if not (err_b[held] <= bar_b * r["scale_case"] + GRAD_ABS).all():
            failed.append((name, "d_beta", rel_b, bar_b))
    assert not failed, failed


@gpu
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("S", BACKWARD_S)
def test_composite_backward_against_fp64_at_every_width(R, S, beta):
    """One table, composite_backward_kernel<1|2|3|4> on both sides of every threshold.  Largest measured errors on the MI355X: DESIGN.md section 5."""
    _hold_backward(R, S, 0, beta)


@gpu
@pytest.mark.parametrize("beta", BACKWARD_TABLE_BETAS)
@pytest.mark.parametrize("Sa,Sn", BACKWARD_TABLES)
def test_composite_backward_of_two_tables_against_fp64(R, Sa, Sn, beta):
    """Two tables through a random origin map: the gradients scattered back into both tables, each held to the bars of the ray."""
    _hold_backward(R, Sa, Sn, beta)


# ------------------------------------------------------------------------------------------------
# 5. bit-exact properties of the composite backward
# ------------------------------------------------------------------------------------------------
def _assert_same_gradients(got, want, what):
    for k, a, b in zip(("d_rgba", "d_rgba_n", "d_beta"), got, want):
        assert (a is None) == (b is None), (what, k)
        if a is not None:
            assert torch.equal(bits(a), bits(b)), (what, k)


@gpu
@pytest.mark.parametrize("Sa,Sn", BACKWARD_TABLES)
def test_backward_of_two_tables_gives_the_bits_of_one_table(R, Sa, Sn):
    """The merged call's d_rgba / d_rgba_n, gathered through the origin map on the host, have the bits of the one-table call on the gathered
    table, and d_beta has equal bits: the same arithmetic, only the addresses differ."""
    ra, z, ma, rn, mn, src, ups = backward_inputs(Sa, Sn)
    rgba, msdf = _gathered(ra, ma, rn, mn, src)
    for beta in BACKWARD_TABLE_BETAS:
        w = _handle(R, beta)
        for name in UPSTREAM:
            g = tuple(None if t is None else dev(t) for t in ups[name])
            d_a, d_n, d_b = _backward(R, w, Sa, Sn, ups[name])
            one, none, b_one = R.composite_backward(w, dev(rgba), dev(z), dev(msdf), *g)
            assert none is None
            both, _ = _gathered(d_a.cpu(), ma, d_n.cpu(), mn, src)
            assert torch.equal(bits(both), bits(one)), (Sa, Sn, beta, name)
            assert torch.equal(bits(d_b), bits(b_one)), (Sa, Sn, beta, name)
            assert torch.isfinite(one).all() and torch.isfinite(b_one).all()


@gpu
@pytest.mark.parametrize("Sa,Sn", [(65, 0), (192, 0), (100, 93)])
def test_a_missing_upstream_gradient_is_a_zero_one(R, Sa, Sn):
    """None for an upstream gradient gives the bits of a tensor of zeros in its place, whichever of the four is missing."""
    ups = backward_inputs(Sa, Sn)[-1]["full"]
    w = _handle(R, 0.01)
    for missing in ((1, 3), (0, 2), (0,), (1,), (2,), (3,), (0, 1, 2, 3)):
        with_none = tuple(None if i in missing else t for i, t in enumerate(ups))
        with_zeros = tuple(torch.zeros_like(t) if i in missing else t for i, t in enumerate(ups))
        _assert_same_gradients(_backward(R, w, Sa, Sn, with_none), _backward(R, w, Sa, Sn, with_zeros), (Sa, Sn, missing))


def _c_backward(R, w, Sa, Sn, n, ups, d_a, d_n, d_b):
    """vanerf_composite_backward itself on the first n rays of a case, into the caller's buffers -> the return code."""
    from vanerf_amd._ffi import lib
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    ra, z, ma, rn, mn, src, _ = (None if t is None or isinstance(t, dict) else dev(t) for t in backward_inputs(Sa, Sn))
    g = [None if t is None else dev(t) for t in ups]
    rc = lib.vanerf_composite_backward(w.handle, P(ra), P(z), P(ma), Sa, P(rn), P(mn), Sn, P(src), n, *(P(t) for t in g), P(d_a), P(d_n), P(d_b), R._stream())
    torch.cuda.synchronize()  # (the inputs above live until the kernel has run)
    return rc


def _sentinel_buffers(Sa, Sn, rows):
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")
    return full(rows, Sa, 5), (full(rows, Sn, 5) if Sn else None), full(rows)


@gpu
@pytest.mark.parametrize("Sa,Sn", [(64, 0), (129, 0), (100, 93)])
def test_backward_without_d_beta(R, Sa, Sn):
    """d_beta == NULL through the C entry changes no bit of d_rgba / d_rgba_n."""
    ups = backward_inputs(Sa, Sn)[-1]["full"]
    w = _handle(R, 0.01)
    with_b, without = _sentinel_buffers(Sa, Sn, RAYS), _sentinel_buffers(Sa, Sn, RAYS)
    assert _c_backward(R, w, Sa, Sn, RAYS, ups, *with_b) == 0
    assert _c_backward(R, w, Sa, Sn, RAYS, ups, without[0], without[1], None) == 0
    _assert_same_gradients(without[:2], with_b[:2], (Sa, Sn))
    assert (with_b[2] != SENTINEL).all() and (without[2] == SENTINEL).all()
    _assert_same_gradients(with_b, _backward(R, w, Sa, Sn, ups), (Sa, Sn, "C entry against the wrapper"))


@gpu
@pytest.mark.parametrize("Sa,Sn", [(64, 0), (129, 0), (200, 0), (100, 29)])
def test_a_rays_gradient_does_not_depend_on_the_ray_count(R, Sa, Sn):
    """The C entry on the first R' rays: rows below R' equal the 37-ray call's rows, and every element past row R' of the (longer) d_rgba,
    d_rgba_n and d_beta still holds what it was filled with -- a retiring tail wave writes nothing."""
    ups = backward_inputs(Sa, Sn)[-1]["full"]
    w = _handle(R, 0.05)
    want = None
    for n in (RAYS, 1, 2, 3, 4, 5):
        out = _sentinel_buffers(Sa, Sn, n + 4)  # a whole block more than any correct access
        assert _c_backward(R, w, Sa, Sn, n, ups, *out) == 0
        out = [None if t is None else t.cpu() for t in out]
        if want is None:
            want = out
            assert all((t[:n] != SENTINEL).any() for t in want if t is not None)  # something was written
        for k, a, b in zip(("d_rgba", "d_rgba_n", "d_beta"), out, want):
            if a is not None:
                assert torch.equal(a[:n], b[:n]), (Sa, Sn, n, k)
                assert (a[n:] == SENTINEL).all(), (Sa, Sn, n, k)


@gpu
@pytest.mark.parametrize("Sa,Sn", [(257, 0), (200, 57)])
def test_backward_refuses_more_than_256_samples(R, Sa, Sn):
    """-22 and a message that names the limit; no output buffer is touched."""
    from vanerf_amd._ffi import lib
    ups = backward_inputs(Sa, Sn)[-1]["full"]
    out = _sentinel_buffers(Sa, Sn, RAYS)
    assert _c_backward(R, _handle(R, 0.05), Sa, Sn, RAYS, ups, *out) == -22
    assert b"at most 256" in lib.vanerf_last_error()
    assert all((t == SENTINEL).all() for t in out if t is not None)


@gpu
def test_backward_reads_sigmoid_beta_from_the_device(R):
    """A handle packed at 1e-4 (clamped to 2e-3) and then updated from a device sigmoid_beta of 0.03 gives the bits of a fresh handle at 0.03,
    and other bits than before the update."""
    from vanerf_amd import synth
    sd = synth.make_full_weights(0)
    sd["sigmoid_beta"] = torch.tensor([1e-4])
    w = R.PackedWeights(sd, mode="fp32")
    on_dev = {k: v.cuda() for k, v in sd.items()}
    on_dev["sigmoid_beta"] = torch.tensor([0.03], device="cuda")
    for Sa, Sn in ((65, 0), (100, 29)):
        ups = backward_inputs(Sa, Sn)[-1]["full"]
        _assert_same_gradients(_backward(R, w, Sa, Sn, ups), _backward(R, _handle(R, 1e-4), Sa, Sn, ups), (Sa, Sn, "before"))
    before = _backward(R, w, 65, 0, backward_inputs(65)[-1]["full"])
    w.update(on_dev)
    for Sa, Sn in ((65, 0), (100, 29)):
        ups = backward_inputs(Sa, Sn)[-1]["full"]
        _assert_same_gradients(_backward(R, w, Sa, Sn, ups), _backward(R, _handle(R, 0.03), Sa, Sn, ups), (Sa, Sn, "after"))
    after = _backward(R, w, 65, 0, backward_inputs(65)[-1]["full"])
    assert not torch.equal(bits(before[0]), bits(after[0])) and not torch.equal(bits(before[2]), bits(after[2]))  # the update reached the kernel


@gpu
@pytest.mark.parametrize("Sa,Sn", [(64, 0), (129, 0), (256, 0), (100, 92)])
def test_backward_gives_the_same_bits_twice(R, Sa, Sn):
    """No atomics: every table entry is stored once, d_beta is one butterfly per wave."""
    ups = backward_inputs(Sa, Sn)[-1]["full"]
    w = _handle(R, 1e-3)
    _assert_same_gradients(_backward(R, w, Sa, Sn, ups), _backward(R, w, Sa, Sn, ups), (Sa, Sn))
