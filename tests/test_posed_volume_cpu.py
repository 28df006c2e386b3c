"""What tests/test_posed_volume.py rests on, checked without a GPU: the numpy restatement of vanerf_pose_transforms
(`restate_transforms`) and of vanerf_volume_render_posed (`restate_march`, fp64 the yardstick, fp32 for E32) on cases worked out by hand, the
inputs the GPU tests draw (`sphere_mesh`, `bent`, `draw_face_sdf`) with the condition their bars assume -- at least 80 % of the hit rays of
every case are clean -- and the two entries' argument checks, which run before anything touches a device.

The trilinear interpolation and the cameras, grids and voxels are those of tests/test_baked_volume.py (section 0g), imported, not restated."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_baked_volume as B
from vanerf_amd import synth

MIN_AREA2 = 1e-30
REACH = 0.03
SAMPLES = [1, 2, 3, 63, 64, 65, 129]
BETAS = [0.1, 1e-3]  # the second is clamped to 2e-3 by both sides


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def _frame(X, f):
    x0, x1, x2 = X[f[:, 0]], X[f[:, 1]], X[f[:, 2]]
    a, b = x1 - x0, x2 - x0
    c = _cross(a, b)
    c2 = _dot(c, c)
    return x0, a, b, c / np.sqrt(c2)[:, None], c2, ((x0 + x1) + x2) / X.dtype.type(3)


def restate_transforms(verts_src, verts_pose, faces, dtype=np.float64):
    """vanerf_pose_transforms in numpy, in the kernel's order of operations: (nv, 3) fp32 twice and (nf, 3) integers -> T (nf, 12) fp32 =
    (A row-major, t) per face, computed in `dtype` and rounded once.  A = M_src M_pose^-1 with M = [a b n], n the unit normal;
    t = x0_src - A x0_pose.  |a x b|^2 <= 1e-30 in either mesh or a non-finite fp32 value: A = I, t = centroid_src - centroid_pose; a vertex
    index outside [0, nv): A = I, t = 0."""
    S, P = (np.asarray(v, dtype=np.float32).astype(dtype) for v in (verts_src, verts_pose))
    faces = np.asarray(faces).astype(np.int64)
    named = ((faces >= 0) & (faces < len(S))).all(1)
    f = np.where(named[:, None], faces, 0)
    with np.errstate(all="ignore"):
        xs, as_, bs, ns, c2s, cens = _frame(S, f)
        xp, ap, bp, npn, c2p, cenp = _frame(P, f)
        bn, na = _cross(bp, npn), _cross(npn, ap)
        det = _dot(ap, bn)
        r = [bn / det[:, None], na / det[:, None], npn]
        A = np.stack([np.stack([(as_[:, i] * r[0][:, j] + bs[:, i] * r[1][:, j]) + ns[:, i] * r[2][:, j] for j in range(3)], 1) for i in range(3)], 1)
        t = np.stack([xs[:, i] - ((A[:, i, 0] * xp[:, 0] + A[:, i, 1] * xp[:, 1]) + A[:, i, 2] * xp[:, 2]) for i in range(3)], 1)
        T = np.concatenate([A.reshape(-1, 9), t], 1).astype(np.float32)
        ok = (c2s > MIN_AREA2) & (c2p > MIN_AREA2) & np.isfinite(T).all(1)
        eye = np.concatenate([np.eye(3, dtype=np.float32).reshape(1, 9).repeat(len(f), 0), (cens - cenp).astype(np.float32)], 1)
    T = np.where(ok[:, None], T, eye)
    T[~named] = np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    return T


def empty_of(face, sdf, nf, reach):
    face, sdf = np.asarray(face), np.asarray(sdf, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (face < 0) | (face >= nf) | ~np.isfinite(sdf) | (sdf > np.float32(reach))


def composite(f, rgb, z, beta, empty, dtype):
    """Section 0g's composite (tests/test_baked_volume.py: composite) with the one new rule: an empty sample has c = 0, so it contributes nothing
    and leaves the transmittance as it is.  dist is 1e10 for the last sample whether or not it is empty.  beta already clamped."""
    t = dtype
    beta = t(beta)
    with np.errstate(over="ignore", invalid="ignore"):
        sg = (t(1) / (t(1) + np.exp(f / beta))) / beta
        dist = np.concatenate([z[..., 1:] - z[..., :-1], np.full_like(z[..., :1], 1e10)], -1)
        c = np.where(empty, t(0), t(1) - np.exp(-sg * dist))
    rgb = np.where(empty[..., None], t(0), rgb)
    T = np.concatenate([np.ones_like(c[..., :1]), np.cumprod((t(1) - c)[..., :-1], -1, dtype=dtype)], -1)
    w = c * T
    color = (rgb * w[..., None]).astype(np.float64).sum(-2).astype(dtype)
    acc = w.astype(np.float64).sum(-1).astype(dtype)
    depth = (z * w).astype(np.float64).sum(-1).astype(dtype) / (acc + t(1e-8))
    return color, depth, acc


def restate_march(voxels, origin, spacing, beta, T, face, sdf, reach, rays_d, cam_pos, z, hit, dtype=np.float64):
    """vanerf_volume_render_posed in numpy: section 0g's restatement with T (nf, 12) fp32, face, sdf (V, R, S) and reach.  p = o + d z;
    q = ((A00 px + A01 py) + A02 pz) + tx ... with the sample's face's record; the trilinear interpolation at q; the composite with the empty
    rule.  -> color (V, R, 3), depth, alpha (V, R)."""
    dtype = np.dtype(dtype).type
    beta = max(np.float32(beta), np.float32(2e-3))
    vox = np.asarray(voxels, dtype=np.float32).astype(dtype)
    d, o, zz = (np.asarray(a, dtype=np.float32).astype(dtype) for a in (rays_d, cam_pos, z))
    T = np.asarray(T, dtype=np.float32).astype(dtype)
    empty = empty_of(face, sdf, len(T), reach)
    rec = T[np.where(empty, 0, np.asarray(face))]  # (V, R, S, 12)
    p = o[:, None, None, :3] + d[:, :, None, :] * zz[..., None]
    q = np.stack([((rec[..., 3 * i] * p[..., 0] + rec[..., 3 * i + 1] * p[..., 1]) + rec[..., 3 * i + 2] * p[..., 2]) + rec[..., 9 + i] for i in range(3)], -1)
    v = B.trilinear(vox, [np.float32(x) for x in origin], [np.float32(x) for x in spacing], q)
    color, depth, acc = composite(v[..., 0], v[..., 1:], zz, beta, empty, dtype)
    h = np.asarray(hit) != 0
    return np.where(h[..., None], color, 0), np.where(h, depth, 0), np.where(h, acc, 0)


def reference(voxels, origin, spacing, beta, T, face, sdf, reach, rays):
    """fp64 yardstick, the rays each output is held on, E32 per output (depth: over the clean rays) and the clean share of the hit rays."""
    args = (voxels, origin, spacing, beta, T, face, sdf, reach, rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    want = dict(zip(("color", "depth", "alpha"), restate_march(*args, dtype=np.float64)))
    have = dict(zip(("color", "depth", "alpha"), restate_march(*args, dtype=np.float32)))
    return (want, *bars(want, have, rays["hit"]))


def bars(want, have, hit):
    h = np.asarray(hit) != 0
    clean = h & ((want["alpha"] > 0.05) | (want["alpha"] < 1e-13))
    held = {"color": h, "alpha": h, "depth": clean}
    e32 = {k: float(np.abs(have[k].astype(np.float64) - want[k])[held[k]].max(initial=0.0)) for k in want}
    return held, e32, float(clean.sum()) / max(int(h.sum()), 1)


# ------------------------------------------------------------------------------------------------
# the inputs of the GPU tests (seeded, made on the CPU)
# ------------------------------------------------------------------------------------------------
def sphere_mesh():
    """synth.uv_sphere(5, 6), radius 5 cm about the centre of section 0g's boxes: (32, 3) fp32, (60, 3) int32."""
    v, f = synth.uv_sphere(rings=5, segs=6)
    return (np.asarray(B.CENTRE) + 0.05 * np.asarray(v, dtype=np.float64)).astype(np.float32), np.asarray(f).astype(np.int32)


def rotation(axis, angle):
    k = np.asarray(axis, dtype=np.float64)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


RIGID = (rotation((0.3, 1.0, -0.2), 0.35), np.array([0.012, -0.007, 0.009]))  # about the mesh's centre, then a shift


def rigid(verts, bend=0.0):
    """The pose of the GPU tests: the source under a smooth bend (x += bend (z - cz)^2 / extent, y likewise with the other sign) and then a rigid
    map about its centre -> (nv, 3) fp32 and the map (Rg, tg) with pose = Rg x + tg for bend = 0."""
    x = np.asarray(verts, dtype=np.float64)
    c = x.mean(0)
    ext = np.ptp(x, axis=0).max()
    u = (x - c) / ext
    x = x + bend * ext * np.stack([u[:, 2] ** 2, -u[:, 0] * u[:, 2], 0.5 * u[:, 0] * u[:, 1]], 1)
    Rg, shift = RIGID
    return ((x - c) @ Rg.T + c + shift).astype(np.float32), (Rg, c - Rg @ c + shift)


def draw_face_sdf(nf, shape, seed, odd=True):
    """The per-sample inputs of the march tests, shares fixed by construction: 10 % of the faces are -1 or nf, the rest uniform in [0, nf);
    sdf uniform in [-0.02, 0.06] (against reach = 0.03: three eighths are beyond it); odd: one sample in 50 has a NaN or infinite sdf."""
    g = np.random.RandomState(seed)
    face = g.randint(0, nf, size=shape).astype(np.int32)
    out = g.rand(*shape) < 0.1
    face[out] = np.where(g.rand(*shape) < 0.5, -1, nf)[out]
    sdf = (g.rand(*shape) * 0.08 - 0.02).astype(np.float32)
    if odd:
        bad = g.rand(*shape) < 0.02
        sdf[bad] = g.choice(np.float32([np.nan, np.inf, -np.inf]), size=shape)[bad]
    return face, sdf


# A ray whose last sample is empty has no 1e10 step to make it opaque, so with 45 % of the samples empty a fifth of the rays of the coarse grid
# end with 1e-13 < alpha < 0.05.  The bars need 80 % clean rays per case; these draws have at least 85 % (found with the restatement alone,
# test_the_inputs_of_the_gpu_tests_are_clean holds every case to the 80 %).
SEED_ROUND = {("small", 2): 2, ("small", 3): 15, ("small", 63): 5, ("small", 64): 4, ("small", 65): 15}


def march_inputs(name, S):
    """(T of the bent sphere, face, sdf) of the case (grid name, S)."""
    vs, f = sphere_mesh()
    T = restate_transforms(vs, rigid(vs, bend=0.3)[0], f)
    face, sdf = draw_face_sdf(len(f), (len(B.CAMERAS), B.NX * B.NY, S), seed=1000 * SEED_ROUND.get((name, S), 0) + 17 * S + len(name))
    return T, face, sdf


# ------------------------------------------------------------------------------------------------
# transforms by hand
# ------------------------------------------------------------------------------------------------
def test_one_right_triangle_under_a_known_rigid_map():
    src = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    pose = np.float32([[1, 2, 3], [1, 3, 3], [0, 2, 3]])  # a quarter turn about z, (x, y, z) -> (-y, x, z), then + (1, 2, 3)
    T = restate_transforms(src, pose, [[0, 1, 2]])
    # posed -> source: A = R^T = ((0, 1, 0), (-1, 0, 0), (0, 0, 1)), t = -R^T (1, 2, 3) = (-2, 1, -3)
    assert T.dtype == np.float32 and T.shape == (1, 12)
    assert np.array_equal(T[0], np.float32([0, 1, 0, -1, 0, 0, 0, 0, 1, -2, 1, -3]))
    for x, p in zip(src, pose):  # and it carries the posed vertices onto the source's
        assert np.array_equal(T[0, :9].reshape(3, 3) @ p + T[0, 9:], x)
    # a point 0.25 above the posed face lands 0.25 above the source face although the posed triangle is twice as large: the unit normal
    big = np.float32([[1, 2, 3], [1, 4, 3], [-1, 2, 3]])
    T2 = restate_transforms(src, big, [[0, 1, 2]])[0]
    assert np.allclose(T2[:9].reshape(3, 3) @ np.float32([1, 2, 3.25]) + T2[9:], [0, 0, 0.25], atol=1e-7)
    assert np.allclose(T2[:9].reshape(3, 3) @ np.float32([1, 4, 3]) + T2[9:], [1, 0, 0], atol=1e-7)


def test_a_pose_equal_to_the_source_is_the_identity():
    v, f = synth.fingered_hand()
    T = restate_transforms(v, v, f)
    assert np.abs(T[:, :9].reshape(-1, 3, 3) - np.eye(3)).max() <= 1e-12 and np.abs(T[:, 9:]).max() <= 1e-12
    vs, fs = sphere_mesh()
    pose, (Rg, tg) = rigid(vs)
    T = restate_transforms(vs, pose, fs)  # a rigid pose: every face carries (Rg^T, -Rg^T tg), up to the fp32 rounding of the posed vertices
    assert np.abs(T[:, :9].reshape(-1, 3, 3) - Rg.T).max() <= 2e-5 and np.abs(T[:, 9:] + Rg.T @ tg).max() <= 2e-5


def test_a_face_without_a_frame_gets_the_centroid_rule():
    src = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 5]])
    pose = src + np.float32([0.5, 0, 0])
    pose[4] = [np.nan, 0, 5]
    faces = [[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 7], [-1, 1, 2]]  # fine; collinear (zero area); a NaN vertex; two that name no vertex
    T = restate_transforms(src, pose, faces)
    eye = np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1])
    assert np.array_equal(T[0], np.float32([*eye, -0.5, 0, 0]))
    assert np.array_equal(T[1], np.float32([*eye, -0.5, 0, 0]))  # centroid_src - centroid_pose
    assert np.array_equal(T[2, :9], eye) and np.isnan(T[2, 9]) and np.array_equal(T[2, 10:], [0, 0])
    assert np.array_equal(T[3], np.float32([*eye, 0, 0, 0])) and np.array_equal(T[4], T[3])
    squashed = src.copy()
    squashed[2] = [0.5, 0, 0]  # zero area in the POSE only
    assert np.array_equal(restate_transforms(src, squashed, [[0, 1, 2]])[0], np.float32([*eye, (1 - 1.5) / 3, 1 / 3, 0]))


# ------------------------------------------------------------------------------------------------
# the march by hand
# ------------------------------------------------------------------------------------------------
def _two_cells():
    """Three points along x, two along y and z: f = 0 everywhere (sigma = 0.5 / beta), red = x / 2."""
    v = np.zeros((2, 2, 3, 4), dtype=np.float32)
    v[..., 1] = np.float32([0.0, 0.5, 1.0])
    return v


def _one_ray(z):
    return dict(rays_d=np.float32([[[1, 0, 0]]]), cam_pos=np.float32([[-1, 0.5, 0.5, 0]]), z=np.float32([[z]]), hit=np.uint8([[1]]))


IDENTITY = np.float32([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_ray_whose_samples_are_all_empty_sees_nothing(dtype):
    rays = _one_ray([1.25, 1.75, 2.5])
    for face, sdf, reach in (([-1, -1, -1], [0, 0, 0], REACH), ([1, 1, 1], [0, 0, 0], REACH), ([0, 0, 0], [0.031, np.nan, np.inf], REACH),
                             ([0, 0, 0], [-1, -1, -1], -np.inf), ([0, 0, 0], [-np.inf] * 3, np.inf)):
        out = restate_march(_two_cells(), (0, 0, 0), (1, 1, 1), 0.1, IDENTITY, np.int32([[face]]), np.float32([[sdf]]), reach, **rays, dtype=dtype)
        assert all((a == 0).all() for a in out), (face, sdf, reach)


def test_one_ray_through_two_cells_with_an_empty_sample_in_the_middle():
    rays = _one_ray([1.25, 1.75, 2.5])  # p.x = 0.25, 0.75, 1.5: red = 0.125, 0.375, 0.75
    sdf = np.float32([[[0.0, 0.0, 0.03]]])  # sdf == reach is not beyond it
    march = lambda face: restate_march(_two_cells(), (0, 0, 0), (1, 1, 1), 0.1, IDENTITY, np.int32([[face]]), sdf, REACH, **rays)
    b = float(np.float32(0.1))
    sg = 0.5 / b
    c0, c1 = 1 - np.exp(-sg * 0.5), 1 - np.exp(-sg * 0.75)
    # the middle sample empty: T_2 = 1 - c0, as if it were not there, and the last sample's 1e10 makes the ray opaque
    color, depth, alpha = march([0, -1, 0])
    w0, w2 = c0, 1 - c0
    assert abs(alpha[0, 0] - 1.0) <= 1e-14 and abs(color[0, 0, 0] - (0.125 * w0 + 0.75 * w2)) <= 1e-12 and (color[0, 0, 1:] == 0).all()
    assert abs(depth[0, 0] - (1.25 * w0 + 2.5 * w2) / (1 + 1e-8)) <= 1e-12
    # nothing empty: the middle sample takes its share
    color, depth, alpha = march([0, 0, 0])
    w1, w2 = (1 - c0) * c1, (1 - c0) * (1 - c1)
    assert abs(alpha[0, 0] - 1.0) <= 1e-14 and abs(color[0, 0, 0] - (0.125 * c0 + 0.375 * w1 + 0.75 * w2)) <= 1e-12
    # the LAST sample empty: its 1e10 does not count, alpha = 1 - (1 - c0)(1 - c1)
    color, depth, alpha = march([0, 0, 1])
    assert abs(alpha[0, 0] - (1 - np.exp(-sg * 1.25))) <= 1e-12 and abs(color[0, 0, 0] - (0.125 * c0 + 0.375 * w1)) <= 1e-12
    # a record that is not the identity: q = A p + t with A = diag(2, 1, 1), t = (-0.5, 0, 0) reads red at x = 0, 1, 2 (2.5 clamped)
    T = np.float32([[2, 0, 0, 0, 1, 0, 0, 0, 1, -0.5, 0, 0]])
    color, _, alpha = restate_march(_two_cells(), (0, 0, 0), (1, 1, 1), 0.1, T, np.int32([[[0, 0, 0]]]), sdf, REACH, **rays)
    assert abs(color[0, 0, 0] - (0.0 * c0 + 0.5 * w1 + 1.0 * w2)) <= 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("S", [1, 3, 65])
def test_identity_transforms_and_no_reach_give_section_0gs_restatement(S, dtype):
    from tests.test_baked_volume_cpu import oracle_rays
    vox, grid = B.random_voxels("large").numpy(), B.GRIDS["large"]
    rays = {k: v for k, v in oracle_rays("large", S).items() if k in ("rays_d", "cam_pos", "z", "hit")}
    face = draw_face_sdf(7, rays["z"].shape, S, odd=False)[0].clip(0, 6)
    sdf = np.zeros(rays["z"].shape, dtype=np.float32)
    got = restate_march(vox, grid["origin"], grid["spacing"], 0.01, IDENTITY.repeat(7, 0), face, sdf, np.inf, **rays, dtype=dtype)
    want = B.restate(vox, grid["origin"], grid["spacing"], 0.01, **rays, dtype=dtype)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------
# the conditions of the GPU tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.GRIDS))
def test_the_inputs_of_the_gpu_tests_are_clean(name):
    from tests.test_baked_volume_cpu import oracle_rays
    grid, vox = B.GRIDS[name], B.random_voxels(name).numpy()
    worst = 1.0
    for S in SAMPLES:
        rays = oracle_rays(name, S)
        T, face, sdf = march_inputs(name, S)
        empty = empty_of(face, sdf, len(T), REACH)
        assert 0.38 < empty.mean() < 0.52 or S < 3  # 10 % by face, three eighths of the rest by reach, 2 % odd: 0.45
        for beta in BETAS:
            want, held, e32, share = reference(vox, grid["origin"], grid["spacing"], beta, T, face, sdf, REACH, rays)
            worst = min(worst, share)
            assert share >= B.MIN_CLEAN, (name, S, beta, share)
            assert all(np.isfinite(v).all() for v in want.values()) and max(e32.values()) < 1e-3, (name, S, beta, e32)
    print(f"{name}: smallest share of clean rays over all cases {worst:.3f}")


def test_the_closed_form_case_is_clean():
    from tests.test_baked_volume_cpu import oracle_rays
    for S in (1, 3, 64, 129):
        rays = oracle_rays("large", S)
        for beta in (0.1, 0.01):
            want, held, e32, share, kept, _ = closed_form(rays, S, beta)
            assert share >= B.MIN_CLEAN and kept > 0.5, (S, beta, share, kept)


def closed_form(rays, S, beta):
    """Item 3 of the GPU tests: section 0g's affine field seen through ONE rigid map (pose = Rg x + tg, so every record is (Rg^T, -Rg^T tg)).
    The expectation comes from the sample points: f = a . Rg^T (p - tg) + b, colour likewise, composited in fp64; samples whose image leaves
    the grid are made empty (face = -1).  -> (want, held, E32 of the restatement on the affine voxels, clean share, share of samples kept,
    the inputs (verts_src, verts_pose, faces, face, sdf))."""
    grid = B.GRIDS["large"]
    vox = B.affine_voxels(grid).numpy()
    vs, fs = sphere_mesh()
    pose, (Rg, tg) = rigid(vs)
    o, s, n = (np.asarray(grid[k], dtype=np.float64) for k in ("origin", "spacing", "dims"))
    pts = rays["cam_pos"][:, None, None, :3].astype(np.float64) + rays["rays_d"][:, :, None, :].astype(np.float64) * rays["z"][..., None].astype(np.float64)
    q = (pts - tg) @ Rg  # Rg^T (p - tg), row vectors
    inside = ((q >= o + 1e-4) & (q <= o + s * (n - 1) - 1e-4)).all(-1)
    face = draw_face_sdf(len(fs), rays["z"].shape, 5 * S, odd=False)[0].clip(0, len(fs) - 1)
    face[~inside] = -1
    sdf = np.zeros(rays["z"].shape, dtype=np.float32)
    f = q @ B.AFFINE_F[0] + B.AFFINE_F[1]
    rgb = B.AFFINE_C[0] + q @ B.AFFINE_C[1].T
    color, depth, acc = composite(f, rgb, rays["z"].astype(np.float64), max(np.float32(beta), np.float32(2e-3)), ~inside, np.float64)
    h = rays["hit"] != 0
    want = {"color": np.where(h[..., None], color, 0), "depth": np.where(h, depth, 0), "alpha": np.where(h, acc, 0)}
    T = restate_transforms(vs, pose, fs)
    args = (vox, grid["origin"], grid["spacing"], beta, T, face, sdf, np.inf, rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    r64 = dict(zip(want, restate_march(*args, dtype=np.float64)))
    r32 = dict(zip(want, restate_march(*args, dtype=np.float32)))
    _, e32, _ = bars(r64, r32, rays["hit"])
    held, _, share = bars(want, want, rays["hit"])
    return want, held, e32, share, float(inside[h].mean()), (vs, pose, fs, face, sdf)


# ------------------------------------------------------------------------------------------------
# argument checks: before any device call
# ------------------------------------------------------------------------------------------------
def march_refusals(lib, good):
    """Every refusal of vanerf_volume_render_posed, against a dict of good arguments in the entry's order; returns how many were tried."""
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    tried = []

    def refused(msg, **change):
        rc = lib.vanerf_volume_render_posed(*dict(good, **change).values())
        assert rc == -22 and msg in lib.vanerf_last_error().decode(), (change, rc, lib.vanerf_last_error())
        tried.append(change)

    for k in ("voxels", "origin", "spacing", "rays_d", "cam_pos", "z", "hit", "T", "face", "sdf", "color", "depth", "alpha"):
        refused("null argument", **{k: None})
    for k in ("nx", "ny", "nz"):
        refused("at least 2", **{k: 1})
    refused("below 2^31", nx=1024, ny=1024, nz=293)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("spacing must be finite and positive", spacing=f3(1, bad, 1))
    refused("origin must be finite", origin=f3(0, 0, float("nan")))
    refused("at least 1", S=0)
    refused("at least 1", nf=0)
    refused("at least 1", nf=-3)
    refused("reach must not be NaN", reach=float("nan"))
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        refused("beta must be finite and positive", beta=bad)
    refused("whole number of views", R=5)
    refused("whole number of rows", row_rays=3)
    refused("16-byte aligned", voxels=ctypes.c_void_p(good["voxels"].value + 4))
    refused("16-byte aligned", T=ctypes.c_void_p(good["T"].value + 8))
    return len(tried)


def transform_refusals(lib, good):
    def refused(msg, **change):
        rc = lib.vanerf_pose_transforms(*dict(good, **change).values())
        assert rc == -22 and msg in lib.vanerf_last_error().decode(), (change, rc, lib.vanerf_last_error())

    for k in ("verts_src", "verts_pose", "faces", "T"):
        refused("null argument", **{k: None})
    for k in ("nv", "nf"):
        refused("at least 1", **{k: 0})
        refused("at least 1", **{k: -1})
    refused("16-byte aligned", T=ctypes.c_void_p(good["T"].value + 4))


def test_the_entries_check_their_arguments_before_any_device_call():
    from vanerf_amd import _ffi
    p = ctypes.c_void_p(64)
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    good = dict(voxels=p, origin=f3(0, 0, 0), spacing=f3(1, 1, 1), nx=3, ny=3, nz=3, w=None, beta=0.1, rays_d=p, cam_pos=p, z=p, hit=p, R=4, rays_per_view=4,
                row_rays=2, S=2, T=p, nf=5, face=p, sdf=p, reach=0.03, color=p, depth=p, alpha=p, stream=None)
    assert march_refusals(_ffi.lib, good) > 30
    assert _ffi.lib.vanerf_volume_render_posed(*dict(good, R=0).values()) == 0  # no rays: a no-op
    transform_refusals(_ffi.lib, dict(verts_src=p, verts_pose=p, nv=3, faces=p, nf=1, T=p, stream=None))
    assert _ffi.ABI_VERSION == 12 and {"vanerf_pose_transforms", "vanerf_volume_render_posed"} <= set(_ffi.EXPORTS)


def test_the_python_layer_refuses_cpu_tensors():
    from vanerf_amd import baked, posed
    v, f = sphere_mesh()
    with pytest.raises(ValueError, match="no CPU fallback"):
        posed.pose_transforms(torch.from_numpy(v), torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(ValueError, match=r"\(nv, 3\)"):
        posed.pose_transforms(torch.zeros(4), torch.zeros(4), torch.from_numpy(f))
    vol = baked.BakedVolume(torch.zeros(2, 2, 2, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), torch.tensor([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9]]), 0.1,
                            verts=torch.from_numpy(v))
    with pytest.raises(ValueError, match="no CPU fallback"):
        posed.render_posed_volume(vol, torch.from_numpy(f), torch.from_numpy(v), [B.cam_tar(B.CAMERAS[0])], samples=4)
