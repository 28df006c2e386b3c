"""The baked volume (vanerf_amd/baked.py, vanerf_amd/csrc/volume_render.hip) on a real MI355X: the packer bit for bit, the
ray march against its fp64 restatement at every sample count on both sides of a round of 64, an affine field against its closed form, 1e30
entries, determinism, the end-to-end path on the synthetic two-hand frame and the argument checks.

The restatement (`restate`) is numpy code that evaluates the header's definition of vanerf_volume_render in a chosen dtype; fp64 is the
yardstick and the same function in fp32 gives E32 = max |fp32 - fp64| per output.  tests/test_baked_volume_cpu.py checks the restatement on
hand-made cases and shows, with the oracle's own ray setup, that the cameras and grids used here satisfy the `clean` condition.

Bars: the composite's own (tests/test_composite_widths.py).  Colour and alpha within max(2e-5, 4 E32); depth, a sum divided by acc + 1e-8,
under the same bar on CLEAN rays only (fp64 acc > 0.05 or acc < 1e-13, E32 over those rays), and at least 80 % of the hit rays of every case
must be clean.  Rays with hit == 0 are exactly zero in every output.

Shapes: grids of (5, 4, 3) and (9, 8, 7) points with unequal spacings; three cameras of an orbit (CAMERAS) on a 7 x 5 pixel grid (35 rays per
view: no multiple of the four rays of a block, odd in both directions of the 2 x 2 tile)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from vanerf_amd import synth

pytestmark = pytest.mark.gpu

FLOOR = 2e-5
MIN_CLEAN = 0.8
SAMPLES = [1, 2, 3, 63, 64, 65, 128, 129, 257]
BETAS = [0.1, 0.01, 1e-3]  # the last one is clamped to 2e-3 by both sides
GRIDS = {"small": dict(dims=(5, 4, 3), origin=(-0.11, -0.08, 0.9), spacing=(0.055, 0.06, 0.07)),
         "large": dict(dims=(9, 8, 7), origin=(-0.12, -0.1, 0.88), spacing=(0.03, 0.028, 0.035))}
WIDTH, HEIGHT, X0, Y0, STEP, NX, NY = 64, 48, 1, 2, 9, 7, 5
CENTRE = (0.0, 0.01, 0.99)
# yaw (degrees) about the box, what the camera looks at relative to the box centre, distance, znear, zfar:
#   0: every ray of its frame hits the box; 1: aims beside it, so part of its frame misses the box; 2: close, and its znear / zfar cut the samples inside the box
CAMERAS = [dict(yaw=0.0, aim=(0.0, 0.0, 0.0), dist=1.0, znear=0.5, zfar=1.5),
           dict(yaw=55.0, aim=(0.12, 0.05, 0.0), dist=1.1, znear=0.5, zfar=1.8),
           dict(yaw=-120.0, aim=(0.0, 0.0, 0.0), dist=0.6, znear=0.56, zfar=0.69)]
PAD = 0.01  # the ray clip's


# ------------------------------------------------------------------------------------------------
# the restatement (no GPU): vanerf_volume_render's definition in numpy
# ------------------------------------------------------------------------------------------------
def cell_of(p, origin, spacing, n):
    """Per axis: u = (p - origin) / spacing clamped to [0, n - 1] (a NaN clamps to 0), i0 = min(floor(u), n - 2), w = u - i0, in p's dtype."""
    t = p.dtype.type
    u = (p - t(origin)) / t(spacing)
    u = np.fmin(np.fmax(u, t(0)), t(n - 1))
    i0 = np.minimum(np.floor(u).astype(np.int64), n - 2)
    return i0, u - i0.astype(p.dtype)


def trilinear(voxels, origin, spacing, pts):
    """voxels (nz, ny, nx, C), pts (..., 3) of the working dtype -> (..., C): (1 - w) a + w b along x, then y, then z."""
    nz, ny, nx = voxels.shape[:3]
    ix, wx = cell_of(pts[..., 0], origin[0], spacing[0], nx)
    iy, wy = cell_of(pts[..., 1], origin[1], spacing[1], ny)
    iz, wz = cell_of(pts[..., 2], origin[2], spacing[2], nz)
    one = pts.dtype.type(1)

    def mix(w, a, b):
        return (one - w)[..., None] * a + w[..., None] * b

    def corner(dx, dy, dz):
        return voxels[iz + dz, iy + dy, ix + dx]

    lo = mix(wy, mix(wx, corner(0, 0, 0), corner(1, 0, 0)), mix(wx, corner(0, 1, 0), corner(1, 1, 0)))
    hi = mix(wy, mix(wx, corner(0, 0, 1), corner(1, 0, 1)), mix(wx, corner(0, 1, 1), corner(1, 1, 1)))
    return mix(wz, lo, hi)


def composite(f, rgb, z, beta, dtype):
    """composite_kernel's arithmetic with a = f: f (..., S), rgb (..., S, 3), z (..., S) in `dtype`; beta already clamped.  Products in
    `dtype`, sums in fp64, results in `dtype` -> color (..., 3), depth, alpha (...,)."""
    t = dtype
    beta = t(beta)
    with np.errstate(over="ignore"):
        sg = (t(1) / (t(1) + np.exp(f / beta))) / beta
    dist = np.concatenate([z[..., 1:] - z[..., :-1], np.full_like(z[..., :1], 1e10)], -1)
    c = t(1) - np.exp(-sg * dist)
    T = np.concatenate([np.ones_like(c[..., :1]), np.cumprod((t(1) - c)[..., :-1], -1, dtype=dtype)], -1)
    w = c * T
    color = (rgb * w[..., None]).astype(np.float64).sum(-2).astype(dtype)
    acc = w.astype(np.float64).sum(-1).astype(dtype)
    depth = (z * w).astype(np.float64).sum(-1).astype(dtype) / (acc + t(1e-8))
    return color, depth, acc


def restate(voxels, origin, spacing, beta, rays_d, cam_pos, z, hit, dtype=np.float64):
    """vanerf_volume_render in numpy: voxels (nz, ny, nx, 4) fp32, origin / spacing (3,) fp32 values, beta a number (clamped at 2e-3 here, in
    fp32, as the library clamps it), rays_d (V, R, 3), cam_pos (V, 4), z (V, R, S), hit (V, R) -> color (V, R, 3), depth, alpha (V, R)."""
    dtype = np.dtype(dtype).type
    beta = max(np.float32(beta), np.float32(2e-3))
    vox = np.asarray(voxels, dtype=np.float32).astype(dtype)
    d, o, zz = (np.asarray(a, dtype=np.float32).astype(dtype) for a in (rays_d, cam_pos, z))
    pts = o[:, None, None, :3] + d[:, :, None, :] * zz[..., None]
    q = trilinear(vox, [np.float32(v) for v in origin], [np.float32(v) for v in spacing], pts)
    color, depth, acc = composite(q[..., 0], q[..., 1:], zz, beta, dtype)
    h = np.asarray(hit) != 0
    return np.where(h[..., None], color, 0), np.where(h, depth, 0), np.where(h, acc, 0)


def reference(voxels, origin, spacing, beta, rays):
    """fp64 yardstick, E32 per output (depth: over the clean rays), the clean hit rays and their share of the hit rays."""
    args = (voxels, origin, spacing, beta, rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    want = dict(zip(("color", "depth", "alpha"), restate(*args, dtype=np.float64)))
    have = dict(zip(("color", "depth", "alpha"), restate(*args, dtype=np.float32)))
    h = np.asarray(rays["hit"]) != 0
    clean = h & ((want["alpha"] > 0.05) | (want["alpha"] < 1e-13))
    held = {"color": h, "alpha": h, "depth": clean}
    e32 = {k: float(np.abs(have[k].astype(np.float64) - want[k])[held[k]].max(initial=0.0)) for k in want}
    return want, held, e32, float(clean.sum()) / max(int(h.sum()), 1)


# ------------------------------------------------------------------------------------------------
# inputs (seeded, made on the CPU)
# ------------------------------------------------------------------------------------------------
def grid_bounds(grid):
    """The bounds whose clip box (widened by PAD) is the grid's own box: (1, 2, 3) fp32."""
    o, s, n = (np.asarray(grid[k], dtype=np.float64) for k in ("origin", "spacing", "dims"))
    return torch.tensor(np.stack([o + PAD, o + s * (n - 1) - PAD])[None], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def random_voxels(name, seed=0):
    nx, ny, nz = GRIDS[name]["dims"]
    g = torch.Generator().manual_seed(1000 + seed + nx)
    vox = torch.rand(nz, ny, nx, 4, generator=g)
    vox[..., 0] = vox[..., 0] * 0.07 - 0.02  # f in about [-0.02, 0.05]; colours in [0, 1]
    return vox.contiguous()


def cam_tar(spec):
    """One target-camera dict (host tensors) of the synthetic orbit."""
    c = np.asarray(CENTRE, dtype=np.float64)
    a = np.radians(spec["yaw"])
    eye = c + spec["dist"] * np.array([np.sin(a), -0.15, -np.cos(a)])
    E = torch.from_numpy(synth.look_at_extrinsic(eye, c + np.asarray(spec["aim"])))
    K = torch.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 260.0 * spec["dist"], 275.0 * spec["dist"], WIDTH / 2.0 - 1.5, HEIGHT / 2.0 - 4.0
    return {"K": K[None], "RT": E[None], "KRT": (K @ E)[None], "width": WIDTH, "height": HEIGHT, "znear": spec["znear"], "zfar": spec["zfar"]}


def pixel_grids():
    """The (1, R, 2) int64 pixel list of the 7 x 5 grid, row-major: what ray_setup_views marches with (X0, Y0, STEP, NX, NY)."""
    yg, xg = torch.meshgrid(torch.arange(NY) * STEP + Y0, torch.arange(NX) * STEP + X0, indexing="ij")
    return torch.stack([xg, yg], -1).view(1, -1, 2)


# ------------------------------------------------------------------------------------------------
# GPU fixtures
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


_RAYS = {}


def device_rays(R, name, S):
    """ray_setup_views on the device for the three cameras (S = 1: the first column of S = 2), and host copies: computed once per case."""
    key = (name, S)
    if key not in _RAYS:
        cams = [cam_tar(c) for c in CAMERAS]
        o = R.ray_setup_views(cams, grid_bounds(GRIDS[name]).cuda(), X0, Y0, STEP, NX, NY, max(S, 2))
        z = o["z"] if S >= 2 else o["z"][..., :1].contiguous()
        dev = dict(rays_d=o["rays_d"], cam_pos=o["cam_pos"], z=z, hit=o["hit"])
        _RAYS[key] = (dev, {k: v.cpu().numpy() for k, v in dev.items()})
    return _RAYS[key]


_HANDLES = {}


def handle_with(R, beta):
    """A weight handle whose sigmoid_beta is `beta` (packed once per value)."""
    if beta not in _HANDLES:
        sd = dict(synth.make_full_weights(0))
        sd["sigmoid_beta"] = torch.tensor([beta])
        _HANDLES[beta] = R.PackedWeights(sd, mode="fp32")
    return _HANDLES[beta]


def volume_of(vox, grid, beta):
    from vanerf_amd import baked
    return baked.BakedVolume(voxels=vox.cuda().contiguous(), origin=tuple(float(np.float32(v)) for v in grid["origin"]),
                             spacing=tuple(float(np.float32(v)) for v in grid["spacing"]), dims=tuple(grid["dims"]), bounds=grid_bounds(grid), beta=beta)


def check_against(got, want, held, e32, clean_share, what):
    """The module's bars; prints every figure before it asserts."""
    errs = {}
    for k, g in zip(("color", "depth", "alpha"), got):
        g = g.detach().cpu().numpy().astype(np.float64)
        errs[k] = float(np.abs(g - want[k])[held[k]].max(initial=0.0))
    print(f"{what}: " + ", ".join(f"{k} err {errs[k]:.3e} (E32 {e32[k]:.3e}, bar {max(FLOOR, 4 * e32[k]):.3e})" for k in errs) + f"; clean {clean_share:.3f}")
    assert clean_share >= MIN_CLEAN, what
    for k in errs:
        assert errs[k] <= max(FLOOR, 4 * e32[k]), (what, k, errs[k], e32[k])


def check_missed_rays(got, hit, what):
    miss = torch.from_numpy(np.asarray(hit) == 0)
    for k, g in zip(("color", "depth", "alpha"), got):
        assert (bits(g)[miss] == 0).all(), (what, k)  # +0.0 exactly


# ------------------------------------------------------------------------------------------------
# 1. pack
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_pack_interleaves_bit_for_bit_and_cleans_non_finite_values(R, n):
    from vanerf_amd import baked
    g = torch.Generator().manual_seed(n)
    f, rgb = torch.randn(n, generator=g), torch.randn(n, 3, generator=g)
    f[0] = -0.0
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")])
    if n > 16:
        f[3:6] = bad
        rgb[7, :] = bad
        rgb[9, 1] = float("nan")
        f[n - 1] = float("inf")
        f[10], rgb[10, 2] = 3e38, -3e38  # large but finite: copied
    else:
        rgb[0, 1] = float("nan")
    vox = baked.pack_volume(f.cuda(), rgb.cuda())
    assert vox.shape == (n, 4) and vox.dtype == torch.float32
    want = torch.cat([torch.where(torch.isfinite(f), f, torch.tensor(1e30))[:, None], torch.where(torch.isfinite(rgb), rgb, torch.tensor(0.0))], 1)
    assert torch.equal(bits(vox), bits(want))
    assert torch.isfinite(vox).all()
    grid = baked.pack_volume(f.cuda().view(1, n, 1), rgb.cuda().view(1, n, 1, 3))  # any leading shape
    assert grid.shape == (1, n, 1, 4) and torch.equal(bits(grid).view(n, 4), bits(vox))


# ------------------------------------------------------------------------------------------------
# 2. the march against fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("name", list(GRIDS))
def test_render_against_fp64(R, name, S, beta):
    from vanerf_amd import baked
    vox, grid = random_voxels(name), GRIDS[name]
    dev, host = device_rays(R, name, S)
    assert host["hit"].any(1).all() and 0 < (host["hit"][1] == 0).sum()  # every camera sees the box; camera 1's frame misses part of it
    want, held, e32, share = reference(vox.numpy(), grid["origin"], grid["spacing"], beta, host)
    got = baked.march_volume(volume_of(vox, grid, beta), dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"], row_rays=NX)
    check_against(got, want, held, e32, share, f"{name} S={S} beta={beta} by value")
    check_missed_rays(got, host["hit"], "by value")
    # sigmoid_beta from a weight handle's device copy (clamped there): the same bits
    by_handle = baked.march_volume(volume_of(vox, grid, handle_with(R, beta)), dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"], row_rays=NX)
    for a, b in zip(got, by_handle):
        assert torch.equal(bits(a), bits(b))
    # the tile only decides which rays share a block
    flat = baked.march_volume(volume_of(vox, grid, beta), dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"])
    for a, b in zip(got, flat):
        assert torch.equal(bits(a), bits(b))


def test_render_volume_marches_the_rays_of_ray_setup_views(R):
    """render_volume = ray_setup_views + one march: its outputs are march_volume's on those rays, bit for bit, for S = 1 too."""
    from vanerf_amd import baked
    vox, grid = random_voxels("large"), GRIDS["large"]
    vol = volume_of(vox, grid, 0.05)
    cams = [cam_tar(c) for c in CAMERAS]
    for S in (1, 70):
        dev, _ = device_rays(R, "large", S)
        o = baked.render_volume(vol, cams, samples=S, x0=X0, y0=Y0, step=STEP, nx=NX, ny=NY)
        want = baked.march_volume(vol, dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"], row_rays=NX)
        for k, t in zip(("color", "depth", "alpha"), want):
            assert torch.equal(bits(o[k]), bits(t)), (S, k)
        assert torch.equal(o["hit"], dev["hit"]) and o["index"].shape == (3, NX * NY) and o["index"].dtype == torch.int64
        assert int(o["index"][0, 0]) == X0 + Y0 * WIDTH and int(o["index"][2, -1]) == X0 + (NX - 1) * STEP + (Y0 + (NY - 1) * STEP) * WIDTH


# ------------------------------------------------------------------------------------------------
# 3. an affine field: the expectation comes from the sample points, not from the grid
# ------------------------------------------------------------------------------------------------
AFFINE_F = (np.array([0.31, -0.23, 0.17]), -0.155)  # f = a . x + b: crosses zero inside the box
AFFINE_C = (np.array([0.5, 0.4, 0.3]), np.array([[1.1, -0.7, 0.2], [-0.5, 0.9, 0.3], [0.6, 0.25, -0.8]]))  # colour = c0 + C x


def affine_voxels(grid):
    nx, ny, nz = grid["dims"]
    o, s = (np.asarray(grid[k], dtype=np.float32).astype(np.float64) for k in ("origin", "spacing"))
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    xyz = o + np.stack([xx, yy, zz], -1) * s
    f = xyz @ AFFINE_F[0] + AFFINE_F[1]
    rgb = AFFINE_C[0] + xyz @ AFFINE_C[1].T
    return torch.from_numpy(np.concatenate([f[..., None], rgb], -1).astype(np.float32)).contiguous()


@pytest.mark.parametrize("beta", [0.1, 0.01])
@pytest.mark.parametrize("S", [1, 3, 64, 129])
def test_affine_field_against_its_closed_form(R, S, beta):
    from vanerf_amd import baked
    grid = GRIDS["large"]
    vox = affine_voxels(grid)
    dev, host = device_rays(R, "large", S)
    # every sample of a hit ray lies inside the grid's box (up to the rounding of the clip), so the interpolation is exact up to rounding
    o, s, n = (np.asarray(grid[k], dtype=np.float64) for k in ("origin", "spacing", "dims"))
    pts = host["cam_pos"][:, None, None, :3].astype(np.float64) + host["rays_d"][:, :, None, :].astype(np.float64) * host["z"][..., None].astype(np.float64)
    h = host["hit"] != 0
    assert (pts[h] >= o - 1e-5).all() and (pts[h] <= o + s * (n - 1) + 1e-5).all()
    _, held, e32, share = reference(vox.numpy(), grid["origin"], grid["spacing"], beta, host)
    f = pts @ AFFINE_F[0] + AFFINE_F[1]
    rgb = AFFINE_C[0] + pts @ AFFINE_C[1].T
    color, depth, acc = composite(f, rgb, host["z"].astype(np.float64), max(np.float32(beta), np.float32(2e-3)), np.float64)
    want = {"color": np.where(h[..., None], color, 0), "depth": np.where(h, depth, 0), "alpha": np.where(h, acc, 0)}
    clean = h & ((want["alpha"] > 0.05) | (want["alpha"] < 1e-13))
    held = dict(held, depth=held["depth"] & clean)
    got = baked.march_volume(volume_of(vox, grid, beta), dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"], row_rays=NX)
    check_against(got, want, held, e32, share, f"affine S={S} beta={beta}")
    assert np.ptp(want["color"][h], axis=0).min() > 0.05  # the colours do vary over the frame


# ------------------------------------------------------------------------------------------------
# 4. 1e30 entries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 64, 130])
def test_no_nan_comes_out_of_a_volume_with_outside_entries(R, S):
    from vanerf_amd import baked
    grid = GRIDS["large"]
    nx, ny, nz = grid["dims"]
    dev, host = device_rays(R, "large", S)
    g = torch.Generator().manual_seed(77)
    f_clean, rgb = random_voxels("large")[..., 0].clone(), random_voxels("large")[..., 1:].clone()
    scattered = f_clean.clone()
    scattered[torch.rand(nz, ny, nx, generator=g) < 0.3] = float("nan")
    scattered[:, :, 0] = float("inf")   # whole slabs
    scattered[nz - 2:] = float("-inf")
    slabs = f_clean.clone()
    slabs[:, :, 3:] = float("inf")      # the upper two thirds of x: rays that stay there see nothing
    empty = torch.full_like(f_clean, float("nan"))
    some_blind = 0
    for name, f in (("scattered", scattered), ("slabs", slabs), ("empty", empty)):
        vox = baked.pack_volume(f.cuda(), rgb.cuda())
        assert torch.isfinite(vox).all() and int((vox[..., 0] == 1e30).sum()) == int((~torch.isfinite(f)).sum())
        for beta in (0.1, 1e-3):
            got = baked.march_volume(volume_of(vox.cpu(), grid, beta), dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"], row_rays=NX)
            for k, t in zip(("color", "depth", "alpha"), got):
                assert torch.isfinite(t).all(), (name, beta, k)
            # rays all of whose samples have eight outside corners
            pts = host["cam_pos"][:, None, None, :3] + host["rays_d"][:, :, None, :] * host["z"][..., None]
            o32, s32 = np.asarray(grid["origin"], dtype=np.float32), np.asarray(grid["spacing"], dtype=np.float32)
            idx = [cell_of(pts[..., a], o32[a], s32[a], n)[0] for a, n in enumerate((nx, ny, nz))]
            out = vox.cpu().numpy()[..., 0] == np.float32(1e30)
            blind = np.ones(pts.shape[:-1], dtype=bool)
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        blind &= out[idx[2] + dz, idx[1] + dy, idx[0] + dx]
            blind = blind.all(-1) & (host["hit"] != 0)
            some_blind += int(blind.sum())
            a = got[2].cpu().numpy()
            assert (a[blind] == 0).all() and (got[0].cpu().numpy()[blind] == 0).all(), (name, beta)
            if name == "empty":
                assert blind.sum() == (host["hit"] != 0).sum()
            want, held, e32, _ = reference(vox.cpu().numpy(), grid["origin"], grid["spacing"], beta, host)
            for k, t in zip(("color", "alpha"), (got[0], got[2])):  # (depth: a ray that sees next to nothing is not clean)
                assert np.abs(t.cpu().numpy() - want[k]).max() <= max(FLOOR, 4 * e32[k]), (name, beta, k)
    assert some_blind > 0


# ------------------------------------------------------------------------------------------------
# 5. determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 129])
def test_the_same_bits_every_call(R, S):
    from vanerf_amd import baked
    vox, grid = random_voxels("large"), GRIDS["large"]
    dev, _ = device_rays(R, "large", S)
    vol = volume_of(vox, grid, 0.01)
    args = (vol, dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"])
    first = baked.march_volume(*args, row_rays=NX)
    again = baked.march_volume(*args, row_rays=NX)
    V, Rn = dev["hit"].shape
    filled = (torch.full((V, Rn, 3), float("nan"), device="cuda"), torch.full((V, Rn), float("nan"), device="cuda"), torch.full((V, Rn), float("nan"), device="cuda"))
    into = baked.march_volume(*args, row_rays=NX, out=filled)
    assert all(a is b for a, b in zip(into, filled))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = baked.march_volume(*args, row_rays=NX)
    side.synchronize()
    for k, a, b, c, d in zip(("color", "depth", "alpha"), first, again, into, on_side):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c)) and torch.equal(bits(a), bits(d)), k
    p1 = baked.pack_volume(vox[..., 0].contiguous().cuda(), vox[..., 1:].contiguous().cuda())
    p2 = baked.pack_volume(vox[..., 0].contiguous().cuda(), vox[..., 1:].contiguous().cuda())
    assert torch.equal(bits(p1), bits(p2)) and torch.equal(bits(p1), bits(vox))


# ------------------------------------------------------------------------------------------------
# 6. end to end on the synthetic two-hand frame
# ------------------------------------------------------------------------------------------------
def _net(precision):
    from vanerf_amd.config import default_config
    from vanerf_amd.model import VANeRF
    torch.manual_seed(0)
    cfg = default_config()
    cfg["models"]["VANeRF"]["mfma_precision"] = precision
    cfg["models"]["VANeRF"]["dr_kwargs"].update(sample_per_ray_c=16, sample_per_ray_f=16)
    net = VANeRF(cfg).cuda().eval()
    net.load_state_dict(synth.make_full_weights(0), strict=False)
    return net


def _orbit(frame_cpu, n_frames, size=16):
    from vanerf_amd.model import get_360cameras
    headpose = torch.eye(4)
    headpose[:3, 3] = frame_cpu["targets"]["vert_world"][0].mean(0)
    return get_360cameras(headpose[:3, :4].cuda(), 64.0 * size / 16, 1.0, 1.0, size, size, 0.71, 1.42, n_frames=n_frames)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_end_to_end_on_the_synthetic_frame(R, precision, monkeypatch):
    from vanerf_amd import baked, surface
    from vanerf_amd.novel_views import camera_to_cam_tar, render_novel_views
    net = _net(precision)
    frame_cpu = synth.make_frame(seed=3, tar_h=16, tar_w=16)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    S = 32

    # the volume is field_on_grid on the widened bounds, packed, bit for bit; the method returns the same
    vol = baked.bake_volume(net, trb, resolution=32)
    nx, ny, nz = vol.dims
    assert max(vol.dims) == 32 and vol.voxels.shape == (nz, ny, nx, 4) and vol.voxels.is_cuda and vol.voxels.dtype == torch.float32
    b = frame_cpu["bounds"][0].double()
    wide = torch.stack([b[0] - 0.01, b[1] + 0.01])
    voxel = float((wide[1] - wide[0]).max()) / 31
    origin, spacing, dims = surface.grid_spec(wide, voxel_size=voxel)
    assert (origin, spacing, dims) == (vol.origin, vol.spacing, vol.dims)
    f, rgb = surface.field_on_grid(net, trb, bounds=wide, voxel_size=voxel, want_rgb=True)
    want_vox = torch.cat([torch.where(torch.isfinite(f), f, torch.full_like(f, 1e30))[..., None], torch.where(torch.isfinite(rgb), rgb, torch.zeros_like(rgb))], -1)
    assert torch.equal(bits(vol.voxels), bits(want_vox))
    assert torch.equal(bits(net.bake_volume(trb, resolution=32).voxels), bits(vol.voxels))
    assert torch.equal(vol.bounds.cpu().reshape(2, 3), frame_cpu["bounds"][0]) and vol.beta is net.packed_weights()
    lo = torch.tensor(vol.origin, dtype=torch.float64)
    hi = lo + torch.tensor(vol.spacing, dtype=torch.float64) * (torch.tensor(vol.dims) - 1)
    assert (lo <= wide[0] + 1e-7).all() and (hi >= wide[1] - 1e-7).all()  # the grid covers the clip box
    inside = float((vol.voxels[..., 0] < 0).float().mean())
    assert 0.005 < inside < 0.9  # the volume holds the hands

    # render_volume against the chain of existing stages on the same rays
    cams = [camera_to_cam_tar(c) for c in _orbit(frame_cpu, 8)[:3]]
    o = baked.render_volume(vol, cams, samples=S)
    V, Rn = 3, 16 * 16
    rays = R.ray_setup_views(cams, vol.bounds, 0, 0, 1, 16, 16, S)
    assert torch.equal(o["hit"], rays["hit"]) and torch.equal(o["index"], rays["index"]) and o["color"].shape == (V, Rn, 3)
    pts = R.sample_points(rays["rays_d"].view(-1, 3), rays["cam_pos"], rays["z"].view(-1, S), rays_per_view=Rn)
    u = (pts.double() - torch.tensor(vol.origin, dtype=torch.float64, device="cuda")) / torch.tensor(vol.spacing, dtype=torch.float64, device="cuda")
    top = torch.tensor([nx - 1, ny - 1, nz - 1], dtype=torch.float64, device="cuda")
    u = torch.minimum(torch.clamp(u, min=0.0), top)
    i0 = torch.minimum(u.floor().long(), top.long() - 1)
    w = u - i0
    vox64 = vol.voxels.double()
    corner = lambda dx, dy, dz: vox64[i0[:, 2] + dz, i0[:, 1] + dy, i0[:, 0] + dx]
    mix = lambda t, a, c: (1.0 - t)[:, None] * a + t[:, None] * c
    q = mix(w[:, 2], mix(w[:, 1], mix(w[:, 0], corner(0, 0, 0), corner(1, 0, 0)), mix(w[:, 0], corner(0, 1, 0), corner(1, 1, 0))),
            mix(w[:, 1], mix(w[:, 0], corner(0, 0, 1), corner(1, 0, 1)), mix(w[:, 0], corner(0, 1, 1), corner(1, 1, 1)))).float()
    rgba = torch.cat([q[:, :1], torch.zeros_like(q[:, :1]), q[:, 1:]], 1).view(V * Rn, S, 5).contiguous()
    color, depth, alpha, _, _ = R.composite(rgba, rays["z"].view(-1, S), torch.zeros(V * Rn, S, device="cuda"), net.packed_weights(), want_contrib=False)
    host = {k: rays[k].cpu().numpy() for k in ("rays_d", "cam_pos", "z", "hit")}
    beta = float(net.state_dict()["sigmoid_beta"].reshape(-1)[0])
    _, held, e32, share = reference(vol.voxels.cpu().numpy(), vol.origin, vol.spacing, beta, host)
    h = host["hit"] != 0
    chain = {"color": np.where(h[..., None], color.view(V, Rn, 3).cpu().numpy().astype(np.float64), 0),
             "depth": np.where(h, depth.view(V, Rn).cpu().numpy().astype(np.float64), 0), "alpha": np.where(h, alpha.view(V, Rn).cpu().numpy().astype(np.float64), 0)}
    assert h.mean() > 0.2 and float(o["alpha"].max()) > 0.5  # the views see the hands
    check_against((o["color"], o["depth"], o["alpha"]), chain, held, e32, share, f"{precision}: render_volume against the chain of stages")
    check_missed_rays((o["color"], o["depth"], o["alpha"]), host["hit"], precision)

    # whole frames, laid out as render_pifu_nerf_views lays them out
    views = baked.render_baked_views(vol, cams, samples=S)
    assert len(views) == 3
    for v, d in enumerate(views):
        assert d["tex_fg"].shape == (3, 16, 16) and d["depth"].shape == (1, 16, 16) and d["alpha"].shape == (1, 16, 16) and d["tex_fg_fine"] is d["tex_fg"]
        assert torch.equal(d["tex_fg"], o["color"][v].view(16, 16, 3).permute(2, 0, 1)) and torch.equal(d["alpha"].view(-1), o["alpha"][v])
        assert d["vert_xy"].shape == (1, 1558, 2)
    exact = net.render_pifu_nerf_views(trb["im"], trb["cam"], trb["hand_type"], trb["targets"], cams, sp_data=dict(trb["sp_data"]), fine=True, uniform=True,
                                       sample_per_ray_c=16, sample_per_ray_f=16, src_foreground_mask=trb["src_foreground_mask"], bounds=trb["dr_data"]["bounds"])
    for v in range(3):
        assert torch.equal(views[v]["vert_xy"], exact[v]["vert_xy"])
        mse = float(((views[v]["tex_fg"].clamp(0, 1) - exact[v]["tex_fg_fine"].clamp(0, 1)) ** 2).mean())
        print(f"{precision}: view {v}: baked (32 points, {S} samples) against the exact pass (16 + 16 samples): PSNR {-10 * np.log10(max(mse, 1e-30)):.1f} dB")

    # the orbit driver: one bake for the whole orbit, a new one for a new batch
    bakes = []
    real = baked.bake_volume
    monkeypatch.setattr(baked, "bake_volume", lambda *a, **k: bakes.append(1) or real(*a, **k))
    fn = baked.baked_views_fn(32, S)
    orbit = _orbit(frame_cpu, 6)
    frames, src = render_novel_views(net, orbit, trb, only_renderings=True, views_per_pass=4, render_views_fn=fn)
    assert frames.shape == (6, 16, 16, 3) and frames.dtype == np.uint8 and len(bakes) == 1
    assert frames.max() > 0 and not np.array_equal(frames[0], frames[3])  # something is seen, and the orbit moves
    first = (views[0]["tex_fg"].clamp(0, 1).permute(1, 2, 0) * 255.0).to(torch.uint8).cpu().numpy()
    again, _ = render_novel_views(net, orbit[:2], trb, only_renderings=True, render_views_fn=fn)
    assert len(bakes) == 1 and np.array_equal(again, frames[:2])
    assert np.array_equal(render_novel_views(net, _orbit(frame_cpu, 8)[:1], trb, only_renderings=True, render_views_fn=fn)[0][0], first)
    render_novel_views(net, orbit[:1], dict(trb), only_renderings=True, render_views_fn=fn)  # another batch object
    assert len(bakes) == 2


# ------------------------------------------------------------------------------------------------
# 7. argument checks: refused with the library's message, nothing launched
# ------------------------------------------------------------------------------------------------
def test_the_entries_refuse_bad_arguments(R):
    from vanerf_amd import _ffi
    lib = _ffi.lib
    vox = torch.zeros(3, 3, 3, 4, device="cuda")
    rd, cp, z, hit = torch.zeros(4, 3, device="cuda"), torch.zeros(1, 4, device="cuda"), torch.zeros(4, 2, device="cuda"), torch.ones(4, dtype=torch.uint8, device="cuda")
    color, depth, alpha = torch.full((4, 3), 7.0, device="cuda"), torch.full((4,), 7.0, device="cuda"), torch.full((4,), 7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    good = dict(voxels=p(vox), origin=f3(0, 0, 0), spacing=f3(1, 1, 1), nx=3, ny=3, nz=3, w=None, beta=0.1, rays_d=p(rd), cam_pos=p(cp), z=p(z), hit=p(hit), R=4,
                rays_per_view=4, row_rays=2, S=2, color=p(color), depth=p(depth), alpha=p(alpha), stream=None)

    def refused(msg, **change):
        rc = lib.vanerf_volume_render(*dict(good, **change).values())
        assert rc == -22 and msg in lib.vanerf_last_error().decode(), (change, rc, lib.vanerf_last_error())

    for k in ("voxels", "origin", "spacing", "rays_d", "cam_pos", "z", "hit", "color", "depth", "alpha"):
        refused("null argument", **{k: None})
    for k in ("nx", "ny", "nz"):
        refused("at least 2", **{k: 1})
    refused("below 2^31", nx=1024, ny=1024, nz=293)
    refused("below 2^31", nx=40000, ny=40000, nz=2)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("spacing must be finite and positive", spacing=f3(1, bad, 1))
    for bad in (float("nan"), float("-inf")):
        refused("origin must be finite", origin=f3(0, 0, bad))
    refused("at least 1", S=0)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        refused("beta must be finite and positive", beta=bad)
    refused("whole number of views", R=5)
    refused("whole number of rows", row_rays=3)
    refused("16-byte aligned", voxels=ctypes.c_void_p(vox.data_ptr() + 4))
    assert lib.vanerf_volume_render(*dict(good, R=0).values()) == 0  # no rays: a no-op
    torch.cuda.synchronize()
    assert (color == 7.0).all() and (depth == 7.0).all() and (alpha == 7.0).all()  # nothing was launched by any of the above
    assert lib.vanerf_volume_render(*good.values()) == 0
    torch.cuda.synchronize()
    assert (alpha == 1.0).all() and (color == 0.0).all() and (depth == 0.0).all()  # f = 0 at z = 0: the last sample's 1e10 makes the ray opaque
    out = torch.full((5, 4), 7.0, device="cuda")
    f, rgb = torch.zeros(5, device="cuda"), torch.zeros(5, 3, device="cuda")
    assert lib.vanerf_volume_pack(None, p(rgb), 5, p(out), None) == -22 and "null argument" in lib.vanerf_last_error().decode()
    assert lib.vanerf_volume_pack(p(f), None, 5, p(out), None) == -22 and lib.vanerf_volume_pack(p(f), p(rgb), 5, None, None) == -22
    assert lib.vanerf_volume_pack(p(f), p(rgb), -1, p(out), None) == -22 and "outside" in lib.vanerf_last_error().decode()
    assert lib.vanerf_volume_pack(p(f), p(rgb), 0, p(out), None) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_the_python_layer_refuses_bad_arguments(R):
    from vanerf_amd import baked
    vox, grid = random_voxels("small"), GRIDS["small"]
    vol = volume_of(vox, grid, 0.1)
    cams = [cam_tar(c) for c in CAMERAS]
    with pytest.raises(ValueError, match="samples"):
        baked.render_volume(vol, cams, samples=0)
    with pytest.raises(ValueError, match="one width / height"):
        baked.render_volume(vol, [cams[0], dict(cams[1], width=32)], samples=4)
    with pytest.raises(ValueError, match="at least one target camera"):
        baked.render_volume(vol, [], samples=4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        baked.render_volume(baked.BakedVolume(vox, vol.origin, vol.spacing, vol.dims, vol.bounds, 0.1), cams, samples=4)
    with pytest.raises(ValueError, match="no CPU fallback"):
        baked.pack_volume(torch.zeros(4), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="expected a tensor"):
        baked.render_volume(baked.BakedVolume(vol.voxels, vol.origin, vol.spacing, (4, 4, 4), vol.bounds, 0.1), cams, samples=4)
    dev, _ = device_rays(R, "small", 4)
    with pytest.raises(ValueError, match="volume's device"):
        baked.march_volume(vol, dev["rays_d"].cpu(), dev["cam_pos"], dev["z"], dev["hit"])
    with pytest.raises(ValueError, match="hit: expected"):
        baked.march_volume(vol, dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"][:, :-1])
    with pytest.raises(_ffi_error(), match="beta must be finite and positive"):
        baked.march_volume(volume_of(vox, grid, 0.0), dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"])
    if torch.cuda.device_count() > 1:
        other = {k: (v.to("cuda:1") if torch.is_tensor(v) else v) for k, v in cams[0].items()}
        with pytest.raises(ValueError, match="the volume on"):
            baked.render_volume(vol, [other], samples=4)
    with pytest.raises(TypeError):
        baked.render_volume(vox, cams)
    frame = synth.make_frame(seed=3, tar_h=16, tar_w=16)
    fd = synth.to_device(frame, "cuda")
    sd = synth.make_full_weights(0)
    sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
    fdat = R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
    with pytest.raises(ValueError, match="resolution"):
        baked.bake_volume(handle_with(R, 0.1), fdat, resolution=1)
    with pytest.raises(TypeError):
        baked.bake_volume(handle_with(R, 0.1), synth.to_tr_batch(fd))
    with pytest.raises(ValueError, match="no CPU fallback"):
        baked.bake_volume(_cpu_net(), synth.to_tr_batch(frame))


def _cpu_net():
    from vanerf_amd.config import default_config
    from vanerf_amd.model import VANeRF
    return VANeRF(default_config()).eval()


def _ffi_error():
    from vanerf_amd import _ffi
    return _ffi.VanerfError
