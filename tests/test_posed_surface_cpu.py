"""What tests/test_posed_surface.py rests on, checked without a GPU: the numpy restatement of
vanerf_volume_surface_posed (`restate`; fp64 is the yardstick, fp32 gives E32) on cases worked out by hand, the inputs the GPU tests use
(`case_inputs`) with the condition their bars assume -- at least 90 % of the hit rays of every case are clean -- and the entry's argument
checks, which run before anything touches a device.

The restatement is section 0h's (tests/test_baked_surface.py: restate) with section 0i's warp and rule for empty samples
(tests/test_posed_volume_cpu.py: restate_march, empty_of): the trilinear interpolation, the cameras, grids, voxels and the drawn (T, face, sdf)
are imported from there, not restated.

A hit ray is CLEAN iff every non-empty sample's fp64 g lies at least 1e-6 from iso, the fp64 ga of a crossing (the near end re-evaluated under
the inside end's face) lies at least 1e-6 from iso, and the fp32 and fp64 restatements agree on `found` and on the coarse interval k: on the
other rays a last bit decides which crossing is the first, or whether it is found = 1 or 3, and no bar can hold."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import test_baked_surface as SF
from tests import test_baked_volume as B
from tests import test_posed_volume_cpu as P
from tests.test_baked_volume_cpu import oracle_rays

MIN_CLEAN = 0.9
ISO_MARGIN = 1e-6
SAMPLES = [1, 2, 3, 63, 64, 65, 129]
ISOS = [0.0, 0.012]
REFINES = [0, 1, 2]
KINDS = ("draw", "runs")
KEYS = ("depth", "normal", "color")
INF = float("inf")


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def _pick(a, j):
    return np.take_along_axis(a, j[..., None], -1)[..., 0]


def restate(voxels, origin, spacing, iso, refine, T, face, sdf, reach, rays_d, cam_pos, z, hit, dtype=np.float64):
    """vanerf_volume_surface_posed in numpy: voxels (nz, ny, nx, 4) fp32, origin / spacing (3,) and iso fp32 values, T (nf, 12) fp32, face, sdf
    (V, R, S), reach, rays_d (V, R, 3), cam_pos (V, 4), z (V, R, S), hit (V, R) -> {"depth" (V, R), "normal" (V, R, 4), "color" (V, R, 3),
    "found" (V, R) uint8, "k" (V, R): the coarse interval (z_k, z_k+1) of a crossing (found 1 or 3), -1 without one, "g" (V, R, S): the
    per-sample values, +inf where a sample is empty, "ga" (V, R): the near end re-evaluated under the inside end's face, +inf without a
    crossing}, every operation in `dtype`."""
    t = np.dtype(dtype).type
    vox = np.asarray(voxels, dtype=np.float32).astype(t)
    f_only = vox[..., :1]
    d, o4, zz = (np.asarray(a, dtype=np.float32).astype(t) for a in (rays_d, cam_pos, z))
    o = np.broadcast_to(o4[:, None, :3], d.shape)
    org, spc = [t(np.float32(v)) for v in origin], [t(np.float32(v)) for v in spacing]
    iso = t(np.float32(iso))
    rec_all = np.asarray(T, dtype=np.float32).astype(t)
    nz, ny, nx = vox.shape[:3]
    S = zz.shape[-1]
    empty = P.empty_of(face, sdf, len(rec_all), reach)
    fsafe = np.where(empty, 0, np.asarray(face)).astype(np.int64)

    def warp(rec, at):  # rec (V, R, n, 12) or (V, R, 1, 12), at (V, R, n) depths -> q = A p + t (V, R, n, 3), restate_march's expression
        p = o[..., None, :] + d[..., None, :] * at[..., None]
        return np.stack([((rec[..., 3 * i] * p[..., 0] + rec[..., 3 * i + 1] * p[..., 1]) + rec[..., 3 * i + 2] * p[..., 2]) + rec[..., 9 + i] for i in range(3)], -1)

    def g(rec, at):
        return B.trilinear(f_only, org, spc, warp(rec, at))[..., 0]

    with np.errstate(all="ignore"):  # (rays without a crossing run through the same arithmetic and are zeroed at the end)
        gs = np.where(empty, t(np.inf), g(rec_all[fsafe], zz))
        inside = ~empty & (gs < iso)
        cross = ~inside[..., :-1] & inside[..., 1:]
        k = cross.argmax(-1) if S > 1 else np.zeros(inside.shape[:-1], dtype=np.int64)
        crossed = cross.any(-1)
        k1 = np.minimum(k + 1, S - 1)
        starts = inside[..., 0]
        F = np.where(starts, fsafe[..., 0], _pick(fsafe, k1))  # the face of the INSIDE end carries the whole bracket
        rec = rec_all[F][..., None, :]
        zk, zb, gb = _pick(zz, k), _pick(zz, k1), _pick(gs, k1)
        ga = g(rec, zk[..., None])[..., 0]  # the near end under F's map, whatever sample k was
        held = ga < iso
        found = np.where(np.asarray(hit) != 0, np.where(starts, 2, np.where(crossed, np.where(held, 3, 1), 0)), 0).astype(np.uint8)
        za, ga_r = zk, ga
        frac = (np.arange(64) + 1).astype(t) / t(65)
        for _ in range(int(refine)):  # a, t_0 .. t_63, b: the first adjacent (outside, inside) pair
            tl = za[..., None] + frac * (zb - za)[..., None]
            seq_z = np.concatenate([za[..., None], tl, zb[..., None]], -1)
            seq_g = np.concatenate([ga_r[..., None], g(rec, tl), gb[..., None]], -1)
            ins = seq_g < iso
            j = (~ins[..., :-1] & ins[..., 1:]).argmax(-1)
            za, zb, ga_r, gb = _pick(seq_z, j), _pick(seq_z, j + 1), _pick(seq_g, j), _pick(seq_g, j + 1)
        w = np.fmin(np.fmax((iso - ga_r) / (gb - ga_r), t(0)), t(1))
        zs = np.where(found == 2, zz[..., 0], np.where(found == 3, zk, za + w * (zb - za)))
        q = warp(rec, zs[..., None])[..., 0, :]
        top = np.array([nx - 1, ny - 1, nz - 1]).astype(t)
        u = np.stack([np.fmin(np.fmax((q[..., a] - org[a]) / spc[a], t(0)), top[a]) for a in range(3)], -1)
        color = SF.field_at(vox, u)[..., 1:]
        G = []
        for a in range(3):
            up, um = np.fmin(u[..., a] + t(1), top[a]), np.fmax(u[..., a] - t(1), t(0))
            hi, lo = u.copy(), u.copy()
            hi[..., a], lo[..., a] = up, um
            G.append((SF.field_at(f_only, hi)[..., 0] - SF.field_at(f_only, lo)[..., 0]) / ((up - um) * spc[a]))
        A = rec[..., 0, :]
        N = [(A[..., j] * G[0] + A[..., 3 + j] * G[1]) + A[..., 6 + j] * G[2] for j in range(3)]  # A^T G: the gradient of f(A p + t) in p
        m = np.fmax(np.fmax(np.abs(N[0]), np.abs(N[1])), np.abs(N[2]))
        ok = (m > 0) & np.isfinite(m)
        hx, hy, hz = N[0] / m, N[1] / m, N[2] / m
        ln = np.sqrt(hx * hx + hy * hy + hz * hz)
        n = np.stack([hx / ln, hy / ln, hz / ln], -1)
        dlen = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        ndotv = np.fmax(t(0), -((n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1] + n[..., 2] * d[..., 2]) / dlen))
        normal = np.where(ok[..., None], np.concatenate([n, ndotv[..., None]], -1), t(0))
    seen = found != 0
    bracket = (found == 1) | (found == 3)
    return {"depth": np.where(seen, zs, t(0)), "normal": np.where(seen[..., None], normal, t(0)), "color": np.where(seen[..., None], color, t(0)),
            "found": found, "k": np.where(bracket, k, -1), "g": gs, "ga": np.where(bracket, ga, t(np.inf))}


def reference(voxels, origin, spacing, iso, refine, T, face, sdf, reach, rays):
    """The fp64 yardstick, the clean rays, E32 per output over the clean found rays, and the clean share of the hit rays."""
    args = (voxels, origin, spacing, iso, refine, T, face, sdf, reach, rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    want, have = restate(*args, dtype=np.float64), restate(*args, dtype=np.float32)
    h = np.asarray(rays["hit"]) != 0
    level = np.float64(np.float32(iso))
    with np.errstate(invalid="ignore"):
        away = (np.abs(want["g"] - level) >= ISO_MARGIN).all(-1) & (np.abs(want["ga"] - level) >= ISO_MARGIN)  # (+inf: an empty sample, no crossing)
    clean = h & away & (want["found"] == have["found"]) & (want["k"] == have["k"])
    held = clean & (want["found"] != 0)
    e32 = {key: float(np.abs(have[key].astype(np.float64) - want[key])[held].max(initial=0.0)) for key in KEYS}
    return want, clean, e32, float(clean.sum()) / max(int(h.sum()), 1)


# ------------------------------------------------------------------------------------------------
# the inputs of the GPU tests (seeded, made on the CPU)
# ------------------------------------------------------------------------------------------------
# A case of the table below that the restatement finds under 90 % clean rays gets another draw here: (kind, name, S) -> round.  None needs one.
SEED_ROUND = {}


def case_inputs(kind, name, S):
    """(T of the bent sphere, face, sdf, reach) of the case (kind, grid name, S).  "draw": tests/test_posed_volume_cpu.py's march_inputs, faces
    and sdf independent per sample (10 % bad faces, three eighths beyond reach, NaN / inf among the sdf).  "runs": every sample live, the
    face constant over runs of 8 samples along the ray, sdf = 0."""
    T, face, sdf = P.march_inputs(name, S)
    nf, shape = len(T), (len(B.CAMERAS), B.NX * B.NY, S)
    rnd = SEED_ROUND.get((kind, name, S), 0)
    if kind == "draw":
        if rnd:
            face, sdf = P.draw_face_sdf(nf, shape, seed=1000 * rnd + 17 * S + len(name))
        return T, face, sdf, P.REACH
    runs = np.random.RandomState(1000 * rnd + 7 * S + len(name)).randint(0, nf, (*shape[:2], math.ceil(S / 8)))
    return T, np.ascontiguousarray(np.repeat(runs, 8, axis=-1)[..., :S]).astype(np.int32), np.zeros(shape, dtype=np.float32), P.REACH


def expected_kinds(kind, S, iso):
    """The values `found` takes among the clean rays of a case, by construction of the inputs (asserted here and on the GPU)."""
    if iso > 0 and kind == "draw" and S >= 63:
        return {0, 1, 2, 3}
    if iso > 0 and kind == "runs" and S >= 2:
        return {1, 2}
    return set()


# ------------------------------------------------------------------------------------------------
# by hand
# ------------------------------------------------------------------------------------------------
ORIGIN, SPACING = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
EYE = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def _column(f_of_z):
    """A 2 x 2 column whose f depends on z alone (the given values at z = 0, 1, ...) and whose colour is the position (x, y, z)."""
    nz = len(f_of_z)
    v = np.zeros((nz, 2, 2, 4), dtype=np.float32)
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(2), np.arange(2), indexing="ij")
    v[..., 0] = np.asarray(f_of_z, dtype=np.float32)[:, None, None]
    v[..., 1], v[..., 2], v[..., 3] = xx, yy, zz
    return v


def _one(vox, iso, refine, T, face, z, dtype, sdf=None, reach=INF, d=(0.0, 0.0, 1.0), o=(0.25, 0.5, -1.0), hit=1):
    sdf = np.zeros(len(z)) if sdf is None else sdf
    out = restate(vox, ORIGIN, SPACING, iso, refine, np.float32(T), np.int32([[face]]), np.float32([[sdf]]), reach, np.float32([[d]]),
                  np.float32([[[*o, 0.0]]])[0], np.float32([[z]]), np.uint8([[hit]]), dtype=dtype)
    return {k: v[0, 0] for k, v in out.items()}


DTYPES = [(np.float64, 1e-12), (np.float32, 1e-6)]
FALLING = [1.5, 0.5, -0.5, -1.5]  # f = 1.5 - z: inside behind z = 1.5.  The ray runs along +z from z = -1: depth zz is at p.z = zz - 1


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_the_face_of_the_inside_end_carries_the_bracket(dtype, tol):
    vox = _column(FALLING)
    z = [1.0, 2.0, 3.0, 3.5]  # p.z = 0, 1, 2, 2.5
    shift = lambda tz: [[*EYE, 0, 0, 0], [*EYE, 0, 0, tz]]  # face 1 reads the column tz further along it
    # every sample on face 0: f = 1.5, 0.5, -0.5: the crossing at p.z = 1.5
    o = _one(vox, 0.0, 0, shift(0.25), [0, 0, 0, 0], z, dtype)
    assert o["found"] == 1 and o["k"] == 1 and abs(o["depth"] - 2.5) <= tol and abs(o["ga"] - 0.5) <= tol
    # the inside sample on face 1: the whole bracket moves by ITS translation: ga = f(1.25) = 0.25, gb = f(2.25) = -0.75, q.z = 1.5 at p.z = 1.25
    for refine in (0, 2):
        o = _one(vox, 0.0, refine, shift(0.25), [0, 0, 1, 1], z, dtype)
        assert o["found"] == 1 and o["k"] == 1 and abs(o["depth"] - 2.25) <= 2 * tol, refine
        assert abs(o["ga"] - 0.25) <= tol and abs(o["g"][1] - 0.5) <= tol and abs(o["g"][2] + 0.75) <= tol
        assert np.abs(o["color"] - [0.25, 0.5, 1.5]).max() <= 2 * tol and np.abs(o["normal"] - [0, 0, -1, 1]).max() <= tol
    # the face of the OUTSIDE end does not matter: sample 1 on face 1 is still outside (f(1.25) = 0.25), the bracket is face 0's
    o = _one(vox, 0.0, 0, shift(0.25), [0, 1, 0, 0], z, dtype)
    assert o["found"] == 1 and o["k"] == 1 and abs(o["depth"] - 2.5) <= tol and abs(o["ga"] - 0.5) <= tol and abs(o["g"][1] - 0.25) <= tol
    # a translation under which sample k is inside as well: ga = f(1.75) = -0.25 < iso: found = 3 and the depth is z_k exactly, whatever `refine`
    for refine in (0, 1, 4):
        o = _one(vox, 0.0, refine, shift(0.75), [0, 0, 1, 1], z, dtype)
        assert o["found"] == 3 and o["k"] == 1 and o["depth"] == 2.0 and abs(o["ga"] + 0.25) <= tol
        assert np.abs(o["color"] - [0.25, 0.5, 1.75]).max() <= tol and np.abs(o["normal"] - [0, 0, -1, 1]).max() <= tol
    # ga == iso is outside: found = 1 with w = 0
    o = _one(vox, 0.0, 0, shift(0.5), [0, 0, 1, 1], z, dtype)
    assert o["found"] == 1 and o["depth"] == 2.0 and o["ga"] == 0.0


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_an_empty_sample_in_front_of_an_inside_one(dtype, tol):
    vox = _column(FALLING)
    T = [[*EYE, 0, 0, 0]]
    # sample 1 is empty (each of the four rules): ga comes from F's map at z_1: f(1.25) = 0.25, gb = f(2) = -0.5, the crossing at p.z = 1.5
    for face, sdf, reach in (([0, -1, 0], [0, 0, 0], INF), ([0, 1, 0], [0, 0, 0], INF), ([0, 0, 0], [0, np.nan, 0], INF), ([0, 0, 0], [0, 0.04, 0.03], 0.03)):
        o = _one(vox, 0.0, 0, T, face, [1.0, 2.25, 3.0], dtype, sdf=sdf, reach=reach)
        assert o["found"] == 1 and o["k"] == 1 and o["g"][1] == INF and abs(o["ga"] - 0.25) <= tol and abs(o["depth"] - 2.5) <= 2 * tol, (face, sdf)
    # an empty sample that F's map puts inside: found = 3, held at it
    o = _one(vox, 0.0, 2, T, [0, -1, 0], [1.0, 2.75, 3.0], dtype)
    assert o["found"] == 3 and o["depth"] == 2.75 and abs(o["ga"] + 0.25) <= tol
    # an empty FIRST sample is outside: no found = 2 although the volume is inside there; the bracket is (z_0, z_1) and F's map holds it at z_0
    o = _one(vox, 0.0, 0, T, [-1, 0], [2.75, 3.0], dtype)
    assert o["found"] == 3 and o["k"] == 0 and o["depth"] == 2.75
    # an empty sample BEHIND an inside one ends nothing and starts nothing: inside, empty, inside is found = 2
    o = _one(vox, 0.0, 0, T, [0, -1, 0], [2.75, 3.0, 3.25], dtype)
    assert o["found"] == 2 and o["k"] == -1 and o["depth"] == 2.75 and o["ga"] == INF


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_a_quarter_turn_gives_the_transposed_matrix_times_the_gradient(dtype, tol):
    vox = _column([-1.5, -0.5, 0.5, 1.5])  # f = z - 1.5: the source gradient is +z, inside below z = 1.5
    A = [0, 1, 0, 0, 0, 1, 1, 0, 0]        # q = (p.y, p.z, p.x): source z is posed x, so the posed normal is A^T e_z = +x (A e_z would be +y)
    o = _one(vox, 0.0, 1, [[*A, 0, 0, 0]], [0, 0, 0], [1.0, 2.0, 3.0], dtype, d=(-1.0, 0.0, 0.0), o=(4.0, 0.25, 0.5))  # p.x = 3, 2, 1
    assert o["found"] == 1 and o["k"] == 1 and abs(o["depth"] - 2.5) <= 2 * tol
    assert np.abs(o["normal"] - [1, 0, 0, 1]).max() <= tol and np.abs(o["color"] - [0.25, 0.5, 1.5]).max() <= 2 * tol
    # a record that stretches: q.z = 2 p.x: the crossing at p.x = 0.75 and the gradient twice as long, the unit normal the same
    B2 = [0, 1, 0, 0, 0, 1, 2, 0, 0]
    o = _one(vox, 0.0, 1, [[*B2, 0, 0, 0]], [0, 0], [3.0, 3.5], dtype, d=(-1.0, 0.0, 0.0), o=(4.0, 0.25, 0.5))  # p.x = 1, 0.5: f = 0.5, -0.5
    assert o["found"] == 1 and abs(o["depth"] - 3.25) <= 2 * tol and np.abs(o["normal"] - [1, 0, 0, 1]).max() <= tol
    # an oblique ray: n . v is the cosine to the POSED ray
    d = np.float32([-0.8, 0.0, 0.6]).astype(np.float64)
    o = _one(vox, 0.0, 0, [[*A, 0, 0, 0]], [0, 0], [2.0, 3.0], dtype, d=d, o=(3.6, 0.25, 0.0))  # p.x = 2, 1.2
    assert o["found"] == 1 and np.abs(o["normal"] - [1, 0, 0, -d[0] / np.linalg.norm(d)]).max() <= 10 * tol


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_one_sample_two_crossings_and_a_ray_of_empty_samples(dtype, tol):
    vox, T = _column(FALLING), [[*EYE, 0, 0, 0]]
    o = _one(vox, 0.0, 1, T, [0], [2.75], dtype)  # S == 1: found only when the one sample is inside
    assert o["found"] == 2 and o["depth"] == 2.75 and o["k"] == -1 and np.abs(o["color"] - [0.25, 0.5, 1.75]).max() <= tol
    o = _one(vox, 0.0, 1, T, [0], [2.25], dtype)
    assert o["found"] == 0 and not o["depth"] and not o["normal"].any() and not o["color"].any()
    o = _one(vox, 0.0, 1, T, [-1], [2.75], dtype)
    assert o["found"] == 0
    two = _column([0.5, -0.5, 0.5, -0.5, 0.5])  # inside around z = 1 and around z = 3
    z = [1.0 + 0.5 * i for i in range(9)]
    o = _one(two, 0.0, 0, T, [0] * 9, z, dtype)
    assert o["found"] == 1 and o["k"] == 1 and abs(o["depth"] - 1.5) <= tol  # f == 0 at z = 0.5 is outside: the pair is (0.5, 1)
    o = _one(two, 0.0, 0, T, [0, 0, -1, 0, 0, 0, 0, 0, 0], z, dtype)       # the first region's only inside sample is empty: the second is found
    assert o["found"] == 1 and o["k"] == 5 and abs(o["depth"] - 3.5) <= tol
    for face, sdf, reach in (([-1] * 9, [0] * 9, INF), ([1] * 9, [0] * 9, INF), ([0] * 9, [np.inf] * 9, INF), ([0] * 9, [0] * 9, -INF)):
        o = _one(two, 0.0, 2, T, face, z, dtype, sdf=sdf, reach=reach)
        assert o["found"] == 0 and o["k"] == -1
        for key in KEYS:  # +0 exactly
            assert not o[key].any() and not np.signbit(o[key]).any(), key
    o = _one(two, 0.0, 0, T, [0] * 9, z, dtype, hit=0)
    assert o["found"] == 0 and not o["depth"] and not np.signbit(o["depth"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("S", [1, 3, 65])
def test_identity_records_and_no_reach_give_section_0hs_restatement(S, dtype):
    vox, grid = B.random_voxels("large").numpy(), B.GRIDS["large"]
    rays = {k: v for k, v in oracle_rays("large", S).items() if k in ("rays_d", "cam_pos", "z", "hit")}
    face = np.zeros(rays["z"].shape, dtype=np.int32)
    sdf = np.zeros(rays["z"].shape, dtype=np.float32)
    for iso in ISOS:
        for refine in (0, 2):
            got = restate(vox, grid["origin"], grid["spacing"], iso, refine, P.IDENTITY, face, sdf, np.inf, **rays, dtype=dtype)
            want = SF.restate(vox, grid["origin"], grid["spacing"], iso, refine, **rays, dtype=dtype)
            for key in ("depth", "normal", "color", "found", "k", "g"):
                assert np.array_equal(got[key], want[key]), (iso, refine, key)
            assert not (got["found"] == 3).any()


# ------------------------------------------------------------------------------------------------
# the conditions of the GPU tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(B.GRIDS))
def test_the_inputs_of_the_gpu_tests_are_clean(name, kind):
    grid, vox = B.GRIDS[name], B.random_voxels(name).numpy()
    worst, worst_e = 1.0, {k: 0.0 for k in KEYS}
    for S in SAMPLES:
        rays = oracle_rays(name, S)
        T, face, sdf, reach = case_inputs(kind, name, S)
        for iso in ISOS:
            for refine in REFINES:
                want, clean, e32, share = reference(vox, grid["origin"], grid["spacing"], iso, refine, T, face, sdf, reach, rays)
                what = (kind, name, S, iso, refine)
                worst = min(worst, share)
                worst_e = {k: max(worst_e[k], e32[k]) for k in e32}
                assert share >= MIN_CLEAN, (what, share)
                assert all(np.isfinite(want[k]).all() for k in KEYS) and max(e32.values()) < 1e-3, (what, e32)  # the bars 4 E32 stay bars
                assert expected_kinds(kind, S, iso) <= set(want["found"][clean].tolist()), (what, np.bincount(want["found"][clean], minlength=4))
                if S == 1:
                    assert not ((want["found"] == 1) | (want["found"] == 3)).any(), what
                length = np.linalg.norm(want["normal"][..., :3], axis=-1)
                assert ((np.abs(length - 1) <= 1e-12) | (length == 0)).all(), what
    print(f"{kind} {name}: smallest share of clean rays {worst:.3f}; largest E32: " + ", ".join(f"{k} {v:.2e}" for k, v in worst_e.items()))


def closed_form(rays, S):
    """Item 3 of the GPU tests: section 0h's affine field f = a . x + b seen through ONE rigid map, with the per-face records of
    restate_transforms (equal up to the rounding of the posed vertices).  Samples whose image leaves the grid are made empty (face = -1), so
    every value read is the affine function.  Under the record (A, t) of the bracket's face F, f along the ray is affine in the depth:
    a . (A (o + d z) + t) + b = iso has the root z = (iso - b - a . (A o + t)) / (a . A d); the normal is A^T a / |A^T a| and the colour is
    affine in q*.  Everything in fp64 from the sample points.  -> kind per ray (found, or -1: too close to call -- a sample within 1e-5 of
    the level, or a bracket whose near end leaves the grid under F), depth, normal (4), colour, and the inputs (T, face, sdf)."""
    grid = B.GRIDS["large"]
    a, b = SF.AFFINE_F
    iso = np.float64(np.float32(SF.AFFINE_ISO))
    vs, fs = P.sphere_mesh()
    T = P.restate_transforms(vs, P.rigid(vs)[0], fs)
    A, t = T[:, :9].reshape(-1, 3, 3).astype(np.float64), T[:, 9:].astype(np.float64)
    og, sg, ng = (np.asarray(grid[k], dtype=np.float64) for k in ("origin", "spacing", "dims"))
    o = np.broadcast_to(rays["cam_pos"][:, None, :3], rays["rays_d"].shape).astype(np.float64)
    d, z = rays["rays_d"].astype(np.float64), rays["z"].astype(np.float64)
    face = P.draw_face_sdf(len(fs), z.shape, 5 * S, odd=False)[0].clip(0, len(fs) - 1)

    def image(F, at):  # q_F(at): F (V, R, n) faces, at (V, R, n) depths
        p = o[..., None, :] + d[..., None, :] * at[..., None]
        return np.einsum("...ij,...j->...i", A[F], p) + t[F]

    within = lambda q: ((q >= og + 1e-4) & (q <= og + sg * (ng - 1) - 1e-4)).all(-1)  # noqa: E731
    live = within(image(face, z))
    face = np.where(live, face, -1).astype(np.int32)
    f = np.where(live, image(np.maximum(face, 0), z) @ a + b, np.inf)
    inside = f < iso
    near = (np.abs(f - iso) < 1e-5).any(-1)
    cross = ~inside[..., :-1] & inside[..., 1:]
    k = cross.argmax(-1) if S > 1 else np.zeros(inside.shape[:-1], dtype=np.int64)
    k1 = np.minimum(k + 1, S - 1)
    starts = inside[..., 0]
    F = np.maximum(np.where(starts, face[..., 0], _pick(face, k1)), 0)
    zk = _pick(z, k)
    qk = image(F[..., None], zk[..., None])[..., 0, :]
    ga = qk @ a + b
    zc = (iso - b - (np.einsum("...ij,...j->...i", A[F], o) + t[F]) @ a) / (np.einsum("...ij,...j->...i", A[F], d) @ a)
    h = rays["hit"] != 0
    kind = np.where(starts, 2, np.where(cross.any(-1), np.where(ga < iso, 3, 1), 0))
    unsure = near | ((kind % 2 == 1) & (~within(qk) | (np.abs(ga - iso) < 1e-5)))
    kind = np.where(h, np.where(unsure, -1, kind), 0)
    zs = np.where(kind == 2, z[..., 0], np.where(kind == 3, zk, zc))
    q = image(F[..., None], zs[..., None])[..., 0, :]
    N = np.einsum("...ji,j->...i", A[F], a)
    n = N / np.linalg.norm(N, axis=-1, keepdims=True)
    ndotv = np.maximum(0.0, -(n * d).sum(-1) / np.linalg.norm(d, axis=-1))
    return kind, zs, np.concatenate([n, ndotv[..., None]], -1), SF.AFFINE_C[0] + q @ SF.AFFINE_C[1].T, (T, face, np.zeros(z.shape, dtype=np.float32))


def test_the_closed_form_case_of_the_gpu_tests():
    """The closed form agrees with the restatement on the oracle's rays, and the three cameras see the plane as the GPU test asserts."""
    grid = B.GRIDS["large"]
    vox = SF.affine_voxels(grid).numpy()
    seen_kinds = set()
    for S in (2, 3, 64, 129):
        rays = oracle_rays("large", S)
        kind, zs, normal, color, (T, face, sdf) = closed_form(rays, S)
        sure, seen = kind >= 0, kind > 0
        assert sure.mean() >= 0.9 and (kind == 1).any() and (kind == 2).any(), (S, sure.mean(), np.bincount(kind[sure], minlength=4))
        seen_kinds |= set(kind[sure].tolist())
        for refine in (0, 2):
            for dtype, bars in ((np.float64, (1e-6, 1e-6, 1e-6)), (np.float32, (2e-5, 1e-4, 2e-5))):  # (fp64: the voxels are the plane rounded to fp32; fp32: the GPU test's floors)
                o = restate(vox, grid["origin"], grid["spacing"], SF.AFFINE_ISO, refine, T, face, sdf, np.inf, rays["rays_d"], rays["cam_pos"], rays["z"],
                            rays["hit"], dtype=dtype)
                assert np.array_equal(o["found"][sure], kind[sure]), (S, refine)
                errs = (np.abs(o["depth"] - zs)[seen].max(), np.abs(o["normal"] - normal)[seen].max(), np.abs(o["color"] - color)[seen].max())
                assert all(e <= bar for e, bar in zip(errs, bars)), (S, refine, dtype, errs)
    print("kinds over the four sample counts:", sorted(seen_kinds))


# ------------------------------------------------------------------------------------------------
# argument checks: before any device call
# ------------------------------------------------------------------------------------------------
def entry_refusals(lib, good):
    """Every refusal of vanerf_volume_surface_posed, against a dict of good arguments in the entry's order; returns how many were tried."""
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    tried = []

    def refused(msg, **change):
        rc = lib.vanerf_volume_surface_posed(*dict(good, **change).values())
        assert rc == -22 and msg in lib.vanerf_last_error().decode(), (change, rc, lib.vanerf_last_error())
        tried.append(change)

    for k in ("voxels", "origin", "spacing", "rays_d", "cam_pos", "z", "hit", "T", "face", "sdf", "depth", "normal", "color", "found"):
        refused("null argument", **{k: None})
    for k in ("voxels", "T", "normal"):
        refused("16-byte aligned", **{k: ctypes.c_void_p(good[k].value + 4)})
        refused("16-byte aligned", **{k: ctypes.c_void_p(good[k].value + 8)})
    refused("at least 1", S=0)
    refused("at least 1", nf=0)
    refused("at least 1", nf=-3)
    refused("reach must not be NaN", reach=float("nan"))
    for bad in (float("nan"), float("inf"), float("-inf")):
        refused("iso must be finite", iso=bad)
    for bad in (-1, 5):
        refused("refine", refine=bad)
    refused("whole number of views", R=5)
    refused("whole number of rows", row_rays=3)
    refused("at most 65535", R=65536 * 4)
    for k in ("nx", "ny", "nz"):
        refused("at least 2", **{k: 1})
    refused("below 2^31", nx=1024, ny=1024, nz=293)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("spacing must be finite and positive", spacing=f3(1, bad, 1))
    refused("origin must be finite", origin=f3(0, 0, float("nan")))
    return len(tried)


def test_the_entry_checks_its_arguments_before_any_device_call():
    from vanerf_amd import _ffi
    p = ctypes.c_void_p(64)
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    good = dict(voxels=p, origin=f3(0, 0, 0), spacing=f3(1, 1, 1), nx=3, ny=3, nz=3, iso=0.0, refine=1, rays_d=p, cam_pos=p, z=p, hit=p, R=4, rays_per_view=4,
                row_rays=2, S=2, T=p, nf=5, face=p, sdf=p, reach=0.03, depth=p, normal=p, color=p, found=p, stream=None)
    assert entry_refusals(_ffi.lib, good) > 35
    assert _ffi.lib.vanerf_volume_surface_posed(*dict(good, R=0).values()) == 0  # no rays: a no-op
    assert _ffi.ABI_VERSION == 12 and "vanerf_volume_surface_posed" in _ffi.EXPORTS


def test_the_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from vanerf_amd import baked, posed
    from vanerf_amd.model import VANeRF
    new = {"PosedSamples", "posed_samples", "march_surface_posed", "render_posed_surface", "render_posed_surface_views", "posed_surface_sequence",
           "mano_surface_sequence"}
    assert new <= set(posed.__all__) and all(hasattr(posed, k) for k in posed.__all__)
    assert hasattr(VANeRF, "render_posed_surface_views") and hasattr(VANeRF, "mano_surface_sequence")
    v, f = P.sphere_mesh()
    vol = baked.BakedVolume(torch.zeros(2, 2, 2, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), torch.tensor([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9]]), 0.1,
                            verts=torch.from_numpy(v))
    cams = [B.cam_tar(B.CAMERAS[0])]
    mesh = (torch.from_numpy(f), torch.from_numpy(v))
    T = torch.from_numpy(P.IDENTITY)
    rays = (torch.zeros(1, 4, 3), torch.zeros(1, 4), torch.zeros(1, 4, 2), torch.ones(1, 4, dtype=torch.uint8))
    warp = (T, torch.zeros(1, 4, 2, dtype=torch.int32), torch.zeros(1, 4, 2))
    with pytest.raises(ValueError, match="no CPU fallback"):
        posed.march_surface_posed(vol, *warp, *rays)
    for fn in (posed.posed_samples, posed.render_posed_surface, posed.render_posed_surface_views):
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(vol, *mesh, cams, samples=4)
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="refine"):
            posed.march_surface_posed(vol, *warp, *rays, refine=bad)
        with pytest.raises(ValueError, match="refine"):
            posed.render_posed_surface(vol, *mesh, cams, samples=4, refine=bad)
        with pytest.raises(ValueError, match="refine"):
            posed.posed_surface_sequence(None, {}, [], cams[0], refine=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="iso"):
            posed.march_surface_posed(vol, *warp, *rays, iso=bad)
        with pytest.raises(ValueError, match="iso"):
            posed.render_posed_surface_views(vol, *mesh, cams, samples=4, iso=bad)
    with pytest.raises(ValueError, match="NaN"):
        posed.march_surface_posed(vol, *warp, *rays, reach=float("nan"))
    with pytest.raises(ValueError, match="NaN"):
        posed.render_posed_surface(vol, *mesh, cams, samples=4, reach=float("nan"))
    with pytest.raises(ValueError, match="mode"):
        posed.render_posed_surface_views(vol, *mesh, cams, samples=4, mode="wireframe")
    with pytest.raises(ValueError, match="mode"):
        posed.posed_surface_sequence(None, {}, [], cams[0], mode="wireframe")
    with pytest.raises(ValueError, match="one per pose"):
        posed.posed_surface_sequence(None, {}, [torch.from_numpy(v)] * 3, cams * 2)
    with pytest.raises(ValueError, match="prepared"):
        posed.render_posed_surface(vol, *mesh, cams, samples=4, prepared=object())
    with pytest.raises(ValueError, match="prepared"):
        posed.render_posed_volume(vol, *mesh, cams, samples=4, prepared={"T": T})
