"""What tests/test_baked_surface.py rests on, checked without a GPU: its numpy restatement of vanerf_volume_surface on hand-made cases, and --
with the oracle's own ray setup on the baked-volume tests' cameras and grids -- the conditions its bars assume: at least 90 % of the hit rays
of every case are clean, every case with two samples or more has crossings (found == 1), iso = 0.012 makes rays start inside (found == 2),
and E32 stays far below the bars' floor times 50, so the bars stay bars.  Also the entry's argument checks, which run before anything touches a
device, and the Python layer's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_baked_surface as T
from tests import test_baked_volume as V
from tests.test_baked_volume_cpu import oracle_rays

ORIGIN, SPACING = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def _column(f_of_z, nx=2, ny=2):
    """A volume whose f depends on z alone (the given values at z = 0, 1, ...) and whose colour is the position (x, y, z)."""
    nz = len(f_of_z)
    v = np.zeros((nz, ny, nx, 4), dtype=np.float32)
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v[..., 0] = np.asarray(f_of_z, dtype=np.float32)[:, None, None]
    v[..., 1], v[..., 2], v[..., 3] = xx, yy, zz
    return v


def _ray(z, d=(0.0, 0.0, 1.0), o=(0.25, 0.5, -1.0), hit=1):
    return dict(rays_d=np.array([[d]], dtype=np.float32), cam_pos=np.array([[*o, 0.0]], dtype=np.float32), z=np.array([[z]], dtype=np.float32),
                hit=np.array([[hit]], dtype=np.uint8))


def _one(vox, iso, refine, ray, dtype=np.float64):
    o = T.restate(vox, ORIGIN, SPACING, iso, refine, **ray, dtype=dtype)
    return {k: v[0, 0] for k, v in o.items()}


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_one_plane_crossing_by_hand(dtype, tol):
    vox = _column([0.5, -0.5])  # f = 0.5 - z: inside above z = 0.5
    # the ray runs along +z from z = -1: its samples sit at z = 0, 0.25, 0.75, 1 with f = 0.5, 0.25, -0.25, -0.5
    o = _one(vox, 0.0, 0, _ray([1.0, 1.25, 1.75, 2.0]), dtype)
    assert o["found"] == 1 and o["k"] == 1 and abs(o["depth"] - 1.5) <= tol  # halfway between 1.25 and 1.75
    assert np.abs(o["normal"] - [0.0, 0.0, -1.0, 1.0]).max() <= tol  # towards growing f, which is towards the camera: n . v = 1
    assert np.abs(o["color"] - [0.25, 0.5, 0.5]).max() <= tol
    # another level moves the crossing: f = 0.125 at z = 0.375
    o = _one(vox, 0.125, 0, _ray([1.0, 1.25, 1.75, 2.0]), dtype)
    assert o["found"] == 1 and o["k"] == 1 and abs(o["depth"] - 1.375) <= tol
    # f == iso is outside: the sample at f = 0.25 is not inside at iso = 0.25, the next one is
    o = _one(vox, 0.25, 0, _ray([1.0, 1.25, 1.75, 2.0]), dtype)
    assert o["found"] == 1 and o["k"] == 1 and abs(o["depth"] - 1.25) <= tol
    # an oblique ray: the normal stays, n . v is the cosine
    d = np.float32([0.6, 0.0, 0.8]).astype(np.float64)  # (what the restatement sees of them)
    ox = float(np.float32(0.1))
    o = _one(vox, 0.0, 0, _ray([0.0, 1.0], d=d, o=(ox, 0.5, 0.0)), dtype)
    zc = 0.5 / d[2]
    assert o["found"] == 1 and abs(o["depth"] - zc) <= 10 * tol and np.abs(o["normal"] - [0.0, 0.0, -1.0, d[2] / np.linalg.norm(d)]).max() <= 10 * tol
    assert np.abs(o["color"] - [ox + d[0] * zc, 0.5, 0.5]).max() <= 10 * tol
    # looking at it from inside out: no (outside, inside) pair; and a miss
    o = _one(vox, 0.0, 0, _ray([1.0, 1.5], d=(0.0, 0.0, -1.0), o=(0.25, 0.5, 2.0)), dtype)
    assert o["found"] == 2  # (it starts inside)
    o = _one(vox, 0.0, 0, _ray([1.0, 1.25, 1.75, 2.0], hit=0), dtype)
    assert o["found"] == 0 and o["depth"] == 0 and not o["normal"].any() and not o["color"].any()
    # a constant field has no gradient: found, with a zero normal
    o = _one(_column([-0.5, -0.5]), 0.0, 0, _ray([1.5]), dtype)
    assert o["found"] == 2 and not o["normal"].any()


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_a_ray_that_starts_inside_and_one_sample(dtype, tol):
    vox = _column([0.5, -0.5])
    o = _one(vox, 0.0, 2, _ray([1.75, 2.0]), dtype)
    assert o["found"] == 2 and o["k"] == -1 and abs(o["depth"] - 1.75) <= tol  # the first sample, whatever `refine`
    assert np.abs(o["normal"] - [0.0, 0.0, -1.0, 1.0]).max() <= tol and np.abs(o["color"] - [0.25, 0.5, 0.75]).max() <= tol
    # S == 1: found only when the one sample is inside
    o = _one(vox, 0.0, 1, _ray([1.75]), dtype)
    assert o["found"] == 2 and abs(o["depth"] - 1.75) <= tol
    o = _one(vox, 0.0, 1, _ray([1.25]), dtype)
    assert o["found"] == 0 and o["depth"] == 0 and not o["normal"].any() and not o["color"].any()
    # never inside: nothing
    o = _one(vox, 0.0, 1, _ray([1.0, 1.125, 1.25, 1.375]), dtype)
    assert o["found"] == 0 and o["depth"] == 0


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 1e-6)])
def test_the_first_of_two_crossings_is_taken(dtype, tol):
    vox = _column([0.5, -0.5, 0.5, -0.5, 0.5])  # inside around z = 1 and around z = 3
    z = [1.0 + 0.5 * i for i in range(9)]       # samples at z = 0, 0.5, ..., 4: f = 0.5, 0, -0.5, 0, 0.5, 0, -0.5, 0, 0.5
    o = _one(vox, 0.0, 0, _ray(z), dtype)
    assert o["found"] == 1 and o["k"] == 1  # f == 0 at z = 0.5 is outside: the pair is (0.5, 1)
    assert abs(o["depth"] - 1.5) <= tol and np.abs(o["color"] - [0.25, 0.5, 0.5]).max() <= tol
    # the gradient there is one-sided: u- = 0 (clamped), u+ = 1.5: (f(1.5) - f(0)) / 1.5 = (0 - 0.5) / 1.5
    assert np.abs(o["normal"] - [0.0, 0.0, -1.0, 1.0]).max() <= tol
    o = _one(vox, -0.25, 0, _ray(z), dtype)
    assert o["found"] == 1 and o["k"] == 1 and abs(o["depth"] - 1.75) <= tol
    # samples that step over the first inside region find the second
    o = _one(vox, -0.25, 0, _ray([1.0, 3.0, 3.5, 4.0]), dtype)
    assert o["found"] == 1 and o["k"] == 2 and abs(o["depth"] - 3.75) <= tol


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 2e-6)])
def test_a_refinement_round_finds_the_sub_interval(dtype, tol):
    vox = _column([0.5, 0.25, -0.75], nx=3, ny=3)  # piecewise linear along z: f = 0 at z = 1.25
    ray = _ray([1.0, 3.0])                         # two samples, at z = 0 and z = 2
    o = _one(vox, 0.0, 0, ray, dtype)
    assert o["found"] == 1 and o["k"] == 0 and abs(o["depth"] - (1.0 + 2.0 * 0.5 / 1.25)) <= tol  # the chord of (0.5, -0.75): off by 0.45
    # one round: t_l = 1 + 2 (l + 1) / 65 -- z = 1.25 lies between l = 39 (z = 80 / 65) and l = 40 (z = 82 / 65), where f is linear
    for refine in (1, 2, 4):
        o = _one(vox, 0.0, refine, ray, dtype)
        assert o["found"] == 1 and o["k"] == 0 and abs(o["depth"] - 2.25) <= tol, refine
        assert np.abs(o["color"] - [0.25, 0.5, 1.25]).max() <= tol
    # the crossing inside the first and inside the last of the 65 pieces: (a, t_0) and (t_63, b)
    first = _column([0.5, -63.5], nx=3, ny=3)   # one cell, f linear in it: f = 0 at z = 1 / 128 < 1 / 65
    o = _one(first, 0.0, 1, _ray([1.0, 2.0]), dtype)
    assert o["found"] == 1 and abs(o["depth"] - (1.0 + 1.0 / 128.0)) <= tol
    last = _column([63.5, -0.5], nx=3, ny=3)    # f = 0 at z = 127 / 128 > 64 / 65
    o = _one(last, 0.0, 1, _ray([1.0, 2.0]), dtype)
    assert o["found"] == 1 and abs(o["depth"] - (1.0 + 127.0 / 128.0)) <= tol


def test_the_axes_of_the_gradient():
    nx, ny, nz = 4, 3, 5
    a, b = np.array([0.3, -0.2, -0.7]), 1.8
    origin, spacing = (-1.0, 0.5, 2.0), (0.5, 0.25, 0.125)
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    xyz = np.asarray(origin) + np.stack([xx, yy, zz], -1) * np.asarray(spacing)
    vox = np.concatenate([(xyz @ a + b)[..., None], xyz], -1).astype(np.float32)
    d = np.array([0.0, 0.0, 1.0])
    for start in ((-0.9, 0.55, 1.0), (0.4, 0.95, 1.0), (-0.3, 0.7, 1.0)):  # next to the lower and upper x / y borders, and in the middle
        o = T.restate(vox, origin, spacing, 0.0, 1, **_ray([1.0, 1.5], d=d, o=start))
        zc = -(b + np.asarray(start) @ a) / (d @ a)
        assert o["found"][0, 0] == 1 and abs(o["depth"][0, 0] - zc) <= 1e-6
        assert np.abs(o["normal"][0, 0, :3] - a / np.linalg.norm(a)).max() <= 1e-5 and abs(o["normal"][0, 0, 3] - 0.7 / np.linalg.norm(a)) <= 1e-5
        assert np.abs(o["color"][0, 0] - (np.asarray(start) + d * zc)).max() <= 1e-6


@pytest.mark.parametrize("name", list(V.GRIDS))
def test_the_inputs_of_the_gpu_tests_are_clean(name):
    g = V.GRIDS[name]
    vox = V.random_voxels(name).numpy()
    worst, worst_e = 1.0, {k: 0.0 for k in ("depth", "normal", "color")}
    for S in V.SAMPLES:
        rays = oracle_rays(name, S)
        for iso in T.ISOS:
            for refine in T.REFINES:
                want, clean, e32, share = T.reference(vox, g["origin"], g["spacing"], iso, refine, rays)
                what = (name, S, iso, refine)
                worst = min(worst, share)
                worst_e = {k: max(worst_e[k], e32[k]) for k in e32}
                assert share >= T.MIN_CLEAN, (what, share)
                assert all(np.isfinite(want[k]).all() for k in ("depth", "normal", "color")) and max(e32.values()) < 1e-3, (what, e32)  # the bars 4 E32 stay bars
                if S >= 2:
                    assert (want["found"][clean] == 1).any(), what
                else:
                    assert not (want["found"] == 1).any(), what
                if iso > 0:
                    assert (want["found"][clean] == 2).any(), what
                length = np.linalg.norm(want["normal"][..., :3], axis=-1)
                assert ((np.abs(length - 1) <= 1e-12) | (length == 0)).all(), what
    print(f"{name}: smallest share of clean rays {worst:.3f}; largest E32: " + ", ".join(f"{k} {v:.2e}" for k, v in worst_e.items()))


def test_the_affine_case_of_the_gpu_tests():
    """The closed form of the affine test agrees with the restatement on the oracle's rays, and its cameras see the plane as that test asserts."""
    g = V.GRIDS["large"]
    vox = T.affine_voxels(g).numpy()
    for S in (2, 3, 64, 129):
        rays = oracle_rays("large", S)
        kind, zs, normal, color, _ = T.affine_expectation(g, rays)
        h = rays["hit"] != 0
        assert (kind == 1).sum() > 0.5 * h.sum() and (kind == 2).any() and (kind >= 0).sum() >= 0.9 * kind.size, (S, (kind == 1).sum(), (kind == 2).sum(), h.sum())
        for refine in (0, 2):
            for dtype, bars in ((np.float64, (1e-6, 1e-6, 1e-6)), (np.float32, (2e-5, 1e-4, 2e-5))):  # (fp64: the voxels are the plane rounded to fp32; fp32: the GPU test's bars)
                o = T.restate(vox, g["origin"], g["spacing"], T.AFFINE_ISO, refine, rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"], dtype=dtype)
                sure, seen = kind >= 0, kind > 0
                assert np.array_equal(o["found"][sure], kind[sure]), (S, refine)
                errs = (np.abs(o["depth"] - zs)[seen].max(), np.abs(o["normal"] - normal)[seen].max(), np.abs(o["color"] - color)[seen].max())
                assert all(e <= b for e, b in zip(errs, bars)), (S, refine, dtype, errs)


def test_the_entry_checks_its_arguments_before_any_device_call():
    from vanerf_amd import _ffi
    lib = _ffi.lib
    p = ctypes.c_void_p(64)
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    #       0  1             2             3  4  5  6    7  8  9  10 11 12 13 14 15 16 17 18 19 20
    good = [p, f3(0, 0, 0), f3(1, 1, 1), 3, 3, 3, 0.0, 1, p, p, p, p, 4, 4, 2, 2, p, p, p, p, None]

    def refused(msg, at, value):
        args = list(good)
        args[at] = value
        assert lib.vanerf_volume_surface(*args) == -22 and msg in lib.vanerf_last_error().decode(), (at, value, lib.vanerf_last_error())

    for at in (0, 1, 2, 8, 9, 10, 11, 16, 17, 18, 19):
        refused("null argument", at, None)
    for at in (3, 4, 5):
        refused("at least 2", at, 1)
    refused("below 2^31", 3, 2 ** 27)
    refused("spacing must be finite and positive", 2, f3(1, 0, 1))
    refused("spacing must be finite and positive", 2, f3(float("inf"), 1, 1))
    refused("spacing must be finite and positive", 2, f3(1, 1, float("nan")))
    refused("origin must be finite", 1, f3(0, float("nan"), 0))
    refused("origin must be finite", 1, f3(float("inf"), 0, 0))
    refused("at least 1", 15, 0)
    for bad in (float("nan"), float("inf"), float("-inf")):
        refused("iso must be finite", 6, bad)
    for bad in (-1, 5):
        refused("refine", 7, bad)
    refused("voxels must be 16-byte aligned", 0, ctypes.c_void_p(68))
    refused("normal must be 16-byte aligned", 17, ctypes.c_void_p(72))
    refused("whole number of views", 12, 5)
    refused("whole number of rows", 14, 3)
    refused("at most 65535", 12, 65536 * 4)
    args = list(good)
    args[12] = 0
    assert lib.vanerf_volume_surface(*args) == 0  # no rays: a no-op
    assert _ffi.ABI_VERSION == 12 and "vanerf_volume_surface" in _ffi.EXPORTS


def test_the_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from vanerf_amd import baked
    assert {"march_surface", "render_volume_surface", "render_baked_surface_views", "surface_views_fn"} <= set(baked.__all__)
    vol = baked.BakedVolume(torch.zeros(2, 2, 2, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), torch.tensor([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9]]), 0.1)
    cams = [V.cam_tar(V.CAMERAS[0])]
    rays = (torch.zeros(1, 4, 3), torch.zeros(1, 4), torch.zeros(1, 4, 2), torch.ones(1, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU fallback"):
        baked.march_surface(vol, *rays)
    with pytest.raises(ValueError, match="no CPU fallback"):
        baked.render_volume_surface(vol, cams, samples=4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        baked.render_baked_surface_views(vol, cams, samples=4)
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="refine"):
            baked.march_surface(vol, *rays, refine=bad)
        with pytest.raises(ValueError, match="refine"):
            baked.render_volume_surface(vol, cams, samples=4, refine=bad)
        with pytest.raises(ValueError, match="refine"):
            baked.surface_views_fn(32, 32, refine=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="iso"):
            baked.march_surface(vol, *rays, iso=bad)
        with pytest.raises(ValueError, match="iso"):
            baked.render_baked_surface_views(vol, cams, samples=4, iso=bad)
    with pytest.raises(ValueError, match="mode"):
        baked.render_baked_surface_views(vol, cams, samples=4, mode="wireframe")
    with pytest.raises(ValueError, match="mode"):
        baked.surface_views_fn(32, 32, mode="wireframe")
    with pytest.raises(ValueError, match="samples"):
        baked.render_volume_surface(vol, cams, samples=0)
    with pytest.raises(TypeError):
        baked.render_volume_surface(vol.voxels, cams)
