"""What tests/test_baked_volume.py rests on, checked without a GPU: its numpy restatement of vanerf_volume_render on hand-made cases, and --
with the oracle's own ray setup on that file's cameras and grids -- the conditions its bars assume: at least 80 % of the hit rays of every
case are clean (fp64 acc > 0.05 or < 1e-13), camera 1's frame partly misses the box, camera 2's samples are bounded by znear / zfar rather
than by the box, and every sample of a hit ray lies inside the grid (which the affine test needs).  Also the two entries' argument checks,
which run before anything touches a device."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import vanerf_oracle as orc
from tests import test_baked_volume as T


def _voxels_2x2x2():
    v = np.zeros((2, 2, 2, 4), dtype=np.float32)
    for z in range(2):
        for y in range(2):
            for x in range(2):
                v[z, y, x] = [1 * x + 10 * y + 100 * z, x, y, z]
    return v


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_trilinear_at_a_corner_at_the_centre_and_outside(dtype):
    v = _voxels_2x2x2().astype(dtype)
    origin, spacing = (1.0, 2.0, 3.0), (0.5, 0.25, 2.0)
    at = lambda *p: T.trilinear(v, origin, spacing, np.array([p], dtype=dtype))[0]
    assert np.array_equal(at(1.0, 2.0, 3.0), v[0, 0, 0]) and np.array_equal(at(1.5, 2.25, 5.0), v[1, 1, 1])  # corners: the voxel itself
    assert np.array_equal(at(1.5, 2.0, 3.0), v[0, 0, 1]) and np.array_equal(at(1.0, 2.25, 3.0), v[0, 1, 0]) and np.array_equal(at(1.0, 2.0, 5.0), v[1, 0, 0])
    assert np.allclose(at(1.25, 2.125, 4.0), v.reshape(8, 4).mean(0), rtol=1e-6)  # the centre of the cell: the mean of the eight
    # outside: border padding, per axis
    assert np.array_equal(at(9.0, 2.0, 3.0), v[0, 0, 1]) and np.array_equal(at(-9.0, 2.25, 5.0), v[1, 1, 0])
    assert np.array_equal(at(1.0, 99.0, -99.0), v[0, 1, 0]) and np.array_equal(at(9.0, 9.0, 9.0), v[1, 1, 1])
    assert np.allclose(at(9.0, 2.125, 3.0), 0.5 * (v[0, 0, 1] + v[0, 1, 1]))
    assert np.array_equal(at(np.nan, 2.25, 5.0), v[1, 1, 0])  # a NaN coordinate clamps to 0
    i0, w = T.cell_of(np.array([0.9, 1.0, 1.26, 1.5, 1.6, np.nan], dtype=dtype), 1.0, 0.5, 2)
    assert i0.tolist() == [0] * 6 and np.allclose(w, [0.0, 0.0, 0.52, 1.0, 1.0, 0.0])
    i0, w = T.cell_of(np.array([0.0, 3.0, 3.5, 4.0, 7.0], dtype=dtype), 0.0, 1.0, 5)
    assert i0.tolist() == [0, 3, 3, 3, 3] and w.tolist() == [0.0, 0.0, 0.5, 1.0, 1.0]  # the last point belongs to the last cell, weight 1


def test_the_axes_are_x_then_y_then_z():
    nx, ny, nz = 4, 3, 5
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.stack([1.0 * xx + 10.0 * yy + 100.0 * zz, xx, yy, zz], -1).astype(np.float64)
    origin, spacing = (-1.0, 0.5, 2.0), (0.5, 0.25, 0.125)
    u = np.array([[2.25, 0.5, 3.75], [0.0, 1.75, 0.25], [2.999, 0.001, 1.5]])
    got = T.trilinear(v, origin, spacing, np.asarray(origin) + u * np.asarray(spacing))
    assert np.allclose(got[:, 0], u @ [1.0, 10.0, 100.0], atol=1e-9) and np.allclose(got[:, 1:], u, atol=1e-9)
    # 1e30 entries never meet a difference or an infinity: a cell with one outside corner stays finite, and weight 0 ignores it
    w = np.full((2, 2, 2, 4), 0.25, dtype=np.float32)
    w[1, 1, 1, 0] = 1e30
    q = T.trilinear(w, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), np.array([[0.5, 0.5, 0.5], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0]], dtype=np.float32))
    assert np.isfinite(q).all() and q[0, 0] > 1e29 and q[1, 0] == np.float32(0.25) and q[2, 0] == np.float32(1e30)


def test_one_ray_of_one_sample():
    v = np.zeros((2, 2, 2, 4), dtype=np.float32)
    v[..., 0], v[..., 1:] = 0.55, [0.2, 0.4, 0.8]
    rays = dict(rays_d=np.array([[[0.0, 0.0, 1.0]]], dtype=np.float32), cam_pos=np.array([[0.5, 0.5, -1.0, 0.0]], dtype=np.float32),
                z=np.array([[[1.25]]], dtype=np.float32), hit=np.array([[1]], dtype=np.uint8))
    beta = 0.02
    color, depth, alpha = T.restate(v, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), beta, **rays)
    b = float(np.float32(beta))
    sg = 1.0 / (1.0 + np.exp(float(np.float32(0.55)) / b)) / b
    want = 1.0 - np.exp(-sg * 1e10)  # the one sample's dist is 1e10
    assert 0.3 < want < 0.6 and abs(alpha[0, 0] - want) <= 1e-12
    assert np.allclose(color[0, 0], np.float32([0.2, 0.4, 0.8]).astype(np.float64) * want, atol=1e-12) and abs(depth[0, 0] - 1.25 * want / (want + 1e-8)) <= 1e-12
    miss = T.restate(v, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), beta, **dict(rays, hit=np.array([[0]], dtype=np.uint8)))
    assert all((a == 0).all() for a in miss)
    # an outside voxel: exactly nothing, in both dtypes and at the clamped beta
    v[..., 0] = 1e30
    for dtype in (np.float64, np.float32):
        for bb in (0.1, 1e-3):
            out = T.restate(v, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), bb, **rays, dtype=dtype)
            assert all((a == 0).all() and np.isfinite(a).all() for a in out)


@pytest.mark.parametrize("S", [1, 2, 7, 65])
def test_the_composite_of_the_restatement_is_the_oracles(S):
    g = torch.Generator().manual_seed(S)
    f = (torch.rand(5, S, generator=g, dtype=torch.float64) * 0.07 - 0.02)
    rgb = torch.rand(5, S, 3, generator=g, dtype=torch.float64)
    z = torch.sort(torch.rand(5, S, generator=g, dtype=torch.float64) * 0.3 + 0.8, -1)[0]
    for beta in (0.1, 0.01, 1e-3):
        rgba = torch.cat([f[..., None], torch.zeros_like(f[..., None]), rgb], -1)
        want = orc.rgba2out({"sigmoid_beta": torch.tensor([beta], dtype=torch.float64)}, rgba[None], z[None], torch.zeros(1, 5, S, 1, dtype=torch.float64))
        got = T.composite(f.numpy(), rgb.numpy(), z.numpy(), max(beta, 2e-3), np.float64)
        for a, b in zip(got, (want[0][0], want[1][0], want[2][0])):
            assert np.abs(a - b.numpy()).max() <= 1e-12


def oracle_rays(name, S):
    """The oracle's ray setup (generate_rays, uniform depths) for the three cameras of the GPU tests on the 7 x 5 pixel grid, laid out as
    ray_setup_views lays its outputs out, and the box's own entry / exit depths."""
    bounds = T.grid_bounds(T.GRIDS[name])
    out = {k: [] for k in ("rays_d", "cam_pos", "z", "hit", "z1", "z2", "near", "far")}
    for spec in T.CAMERAS:
        cam = T.cam_tar(spec)
        d, o, near, far, hit = orc.generate_rays(T.pixel_grids(), cam, bounds, cam["znear"], cam["zfar"])
        z1, z2, _ = orc.ray_bbox_intersection(bounds, o, d)
        t = torch.linspace(0.0, 1.0, steps=S)[None, None, :]
        out["rays_d"].append(d[0]); out["cam_pos"].append(torch.cat([o[0, 0], torch.zeros(1)])); out["z"].append((near + (far - near) * t)[0])
        out["hit"].append(hit[0, :, 0].to(torch.uint8)); out["z1"].append(z1[0, :, 0]); out["z2"].append(z2[0, :, 0])
        out["near"].append(near[0, :, 0]); out["far"].append(far[0, :, 0])
    return {k: torch.stack(v).numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", list(T.GRIDS))
def test_the_cameras_are_what_the_gpu_tests_say_they_are(name):
    r = oracle_rays(name, 9)
    h = r["hit"] != 0
    assert r["hit"].shape == (3, T.NX * T.NY) and h.any(1).all()
    assert 0 < (~h[1]).sum() < h[1].size  # camera 1: part of the frame misses the box
    by_near, by_far = h[2] & (r["near"][2] > r["z1"][2]), h[2] & (r["far"][2] < r["z2"][2])
    print(f"{name}: camera 2: {int(h[2].sum())} hit rays, {int(by_near.sum())} start at znear, {int(by_far.sum())} end at zfar, {int((by_near & by_far).sum())} both")
    assert (by_near | by_far).sum() >= 0.8 * h[2].sum() and (by_near & by_far).sum() >= 5  # camera 2: znear / zfar, not the box, bound the samples
    for v in (0, 1):
        assert (r["near"][v][h[v]] == r["z1"][v][h[v]]).all() and (r["far"][v][h[v]] == r["z2"][v][h[v]]).all()  # the others: the box does
    assert (r["far"][h] > r["near"][h]).all()
    # every sample of a hit ray lies inside the grid's box, up to the rounding of the clip
    g = T.GRIDS[name]
    o, s, n = (np.asarray(g[k], dtype=np.float64) for k in ("origin", "spacing", "dims"))
    pts = r["cam_pos"][:, None, None, :3].astype(np.float64) + r["rays_d"][:, :, None, :].astype(np.float64) * r["z"][..., None].astype(np.float64)
    assert (pts[h] >= o - 1e-5).all() and (pts[h] <= o + s * (n - 1) + 1e-5).all()


@pytest.mark.parametrize("name", list(T.GRIDS))
def test_the_inputs_of_the_gpu_tests_are_clean(name):
    g = T.GRIDS[name]
    volumes = {"random": T.random_voxels(name).numpy()}
    if name == "large":
        volumes["affine"] = T.affine_voxels(g).numpy()
    worst = 1.0
    for S in T.SAMPLES:
        rays = oracle_rays(name, S)
        for what, vox in volumes.items():
            for beta in T.BETAS:
                want, held, e32, share = T.reference(vox, g["origin"], g["spacing"], beta, rays)
                worst = min(worst, share)
                assert share >= T.MIN_CLEAN, (name, what, S, beta, share)
                assert all(np.isfinite(v).all() for v in want.values()) and all(np.isfinite(e) for e in e32.values())
                assert max(e32.values()) < 1e-3, (name, what, S, beta, e32)  # the bars 4 E32 stay bars
    print(f"{name}: smallest share of clean rays over all cases {worst:.3f}")


def test_the_entries_check_their_arguments_before_any_device_call():
    from vanerf_amd import _ffi
    lib = _ffi.lib
    p = ctypes.c_void_p(64)
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    good = [p, f3(0, 0, 0), f3(1, 1, 1), 3, 3, 3, None, 0.1, p, p, p, p, 4, 4, 2, 2, p, p, p, None]

    def refused(msg, at, value):
        args = list(good)
        args[at] = value
        assert lib.vanerf_volume_render(*args) == -22 and msg in lib.vanerf_last_error().decode(), (at, value, lib.vanerf_last_error())

    for at in (0, 1, 2, 8, 9, 10, 11, 16, 17, 18):
        refused("null argument", at, None)
    for at in (3, 4, 5):
        refused("at least 2", at, 1)
    refused("below 2^31", 3, 2 ** 27)
    refused("spacing must be finite and positive", 2, f3(1, 0, 1))
    refused("spacing must be finite and positive", 2, f3(float("inf"), 1, 1))
    refused("origin must be finite", 1, f3(0, float("nan"), 0))
    refused("at least 1", 15, 0)
    refused("beta must be finite and positive", 7, 0.0)
    refused("beta must be finite and positive", 7, float("nan"))
    refused("16-byte aligned", 0, ctypes.c_void_p(68))
    args = list(good)
    args[12] = 0
    assert lib.vanerf_volume_render(*args) == 0  # no rays: a no-op
    assert lib.vanerf_volume_pack(None, p, 4, p, None) == -22 and "null argument" in lib.vanerf_last_error().decode()
    assert lib.vanerf_volume_pack(p, p, -1, p, None) == -22 and lib.vanerf_volume_pack(p, p, 0, p, None) == 0
    assert _ffi.ABI_VERSION == 12 and {"vanerf_volume_pack", "vanerf_volume_render"} <= set(_ffi.EXPORTS)


def test_the_python_layer_refuses_cpu_tensors():
    from vanerf_amd import baked
    with pytest.raises(ValueError, match="no CPU fallback"):
        baked.pack_volume(torch.zeros(4), torch.zeros(4, 3))
    vol = baked.BakedVolume(torch.zeros(2, 2, 2, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), torch.tensor([[0.1, 0.1, 0.1], [0.9, 0.9, 0.9]]), 0.1)
    with pytest.raises(ValueError, match="no CPU fallback"):
        baked.render_volume(vol, [T.cam_tar(T.CAMERAS[0])], samples=4)
    with pytest.raises(ValueError, match="samples"):
        baked.render_volume(vol, [T.cam_tar(T.CAMERAS[0])], samples=0)
