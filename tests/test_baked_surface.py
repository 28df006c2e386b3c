"""The surface of the baked volume as a camera sees it (vanerf_amd/baked.py, vanerf_amd/csrc/volume_surface.hip) on a real
MI355X: the march against its fp64 restatement at every sample count on both sides of a round of 64 and every number of refinement rounds, an
affine field against its closed form, 1e30 entries, determinism and the end-to-end path on the synthetic two-hand frame.

The restatement (`restate`) is numpy code that evaluates the header's definition of vanerf_volume_surface in a chosen dtype; fp64 is the
yardstick and the same function in fp32 gives E32 = max |fp32 - fp64| per output over the clean, found rays.  A ray is CLEAN iff it hits the
box, its S fp64 sample values all lie at least 1e-6 from iso, and the fp32 and fp64 restatements agree on `found` and on the coarse interval:
on the other rays a last bit decides which crossing is the first, and no bar can hold.  tests/test_baked_surface_cpu.py checks the
restatement on hand-made cases and shows, with the oracle's own ray setup, that at least 90 % of the hit rays of every case here are clean.

Bars: on clean rays `found` is equal exactly, depth and colour are within max(2e-5, 4 E32) (the composite's bars), the normal's four channels
within max(1e-4, 4 E32).  On every ray the outputs are finite, found is 0, 1 or 2, |n| is 1 within 1e-5 or exactly 0, and hit == 0 gives exact
zeros.  Shapes, cameras, grids and the pixel grid are tests/test_baked_volume.py's."""
import numpy as np
import pytest
import torch

from tests.test_baked_volume import CAMERAS, GRIDS, NX, NY, SAMPLES, STEP, X0, Y0, bits, cam_tar, cell_of, device_rays, random_voxels, trilinear, volume_of
from vanerf_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


FLOOR = {"depth": 2e-5, "color": 2e-5, "normal": 1e-4}
MIN_CLEAN = 0.9
ISO_MARGIN = 1e-6
ISOS = [0.0, 0.012]
REFINES = [0, 1, 2]
KEYS = ("depth", "normal", "color", "found")


# ------------------------------------------------------------------------------------------------
# the restatement (no GPU): vanerf_volume_surface's definition in numpy
# ------------------------------------------------------------------------------------------------
def field_at(voxels, u):
    """voxels (nz, ny, nx, C) at CLAMPED grid coordinates u (..., 3): the trilinear interpolation of tests/test_baked_volume.py on the grid
    with origin 0 and spacing 1, where (u - 0) / 1 is u itself."""
    return trilinear(voxels, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), u)


def restate(voxels, origin, spacing, iso, refine, rays_d, cam_pos, z, hit, dtype=np.float64):
    """vanerf_volume_surface in numpy: voxels (nz, ny, nx, 4) fp32, origin / spacing (3,) and iso fp32 values, rays_d (V, R, 3), cam_pos
    (V, 4), z (V, R, S), hit (V, R) -> {"depth" (V, R), "normal" (V, R, 4), "color" (V, R, 3), "found" (V, R) uint8, "k" (V, R): the coarse
    interval (z_k, z_k+1) of a crossing, -1 without one}, every operation in `dtype`."""
    t = np.dtype(dtype).type
    vox = np.asarray(voxels, dtype=np.float32).astype(t)
    f_only = vox[..., :1]
    d, o4, zz = (np.asarray(a, dtype=np.float32).astype(t) for a in (rays_d, cam_pos, z))
    o = np.broadcast_to(o4[:, None, :3], d.shape)
    org, spc = [t(np.float32(v)) for v in origin], [t(np.float32(v)) for v in spacing]
    iso = t(np.float32(iso))
    nz, ny, nx = vox.shape[:3]
    S = zz.shape[-1]

    def g(at):  # at (V, R, n) depths -> f there
        return trilinear(f_only, org, spc, o[..., None, :] + d[..., None, :] * at[..., None])[..., 0]

    def pick(a, j):
        return np.take_along_axis(a, j[..., None], -1)[..., 0]

    with np.errstate(all="ignore"):  # (rays without a crossing run through the same arithmetic and are zeroed at the end)
        gs = g(zz)
        inside = gs < iso
        cross = ~inside[..., :-1] & inside[..., 1:]
        k = cross.argmax(-1) if S > 1 else np.zeros(inside.shape[:-1], dtype=np.int64)
        crossed = cross.any(-1)
        found = np.where(np.asarray(hit) != 0, np.where(inside[..., 0], 2, np.where(crossed, 1, 0)), 0).astype(np.uint8)
        k1 = np.minimum(k + 1, S - 1)
        za, zb, ga, gb = pick(zz, k), pick(zz, k1), pick(gs, k), pick(gs, k1)
        frac = (np.arange(64) + 1).astype(t) / t(65)
        for _ in range(int(refine)):  # a, t_0 .. t_63, b: the first adjacent (outside, inside) pair
            tl = za[..., None] + frac * (zb - za)[..., None]
            seq_z = np.concatenate([za[..., None], tl, zb[..., None]], -1)
            seq_g = np.concatenate([ga[..., None], g(tl), gb[..., None]], -1)
            ins = seq_g < iso
            j = (~ins[..., :-1] & ins[..., 1:]).argmax(-1)
            za, zb, ga, gb = pick(seq_z, j), pick(seq_z, j + 1), pick(seq_g, j), pick(seq_g, j + 1)
        w = np.fmin(np.fmax((iso - ga) / (gb - ga), t(0)), t(1))
        zs = np.where(found == 2, zz[..., 0], za + w * (zb - za))
        p = o + d * zs[..., None]
        top = np.array([nx - 1, ny - 1, nz - 1]).astype(t)
        u = np.stack([np.fmin(np.fmax((p[..., a] - org[a]) / spc[a], t(0)), top[a]) for a in range(3)], -1)
        color = field_at(vox, u)[..., 1:]
        G = []
        for a in range(3):
            up, um = np.fmin(u[..., a] + t(1), top[a]), np.fmax(u[..., a] - t(1), t(0))
            hi, lo = u.copy(), u.copy()
            hi[..., a], lo[..., a] = up, um
            G.append((field_at(f_only, hi)[..., 0] - field_at(f_only, lo)[..., 0]) / ((up - um) * spc[a]))
        m = np.fmax(np.fmax(np.abs(G[0]), np.abs(G[1])), np.abs(G[2]))
        ok = (m > 0) & np.isfinite(m)
        hx, hy, hz = G[0] / m, G[1] / m, G[2] / m
        ln = np.sqrt(hx * hx + hy * hy + hz * hz)
        n = np.stack([hx / ln, hy / ln, hz / ln], -1)
        dlen = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        ndotv = np.fmax(t(0), -((n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1] + n[..., 2] * d[..., 2]) / dlen))
        normal = np.where(ok[..., None], np.concatenate([n, ndotv[..., None]], -1), t(0))
    seen = found != 0
    return {"depth": np.where(seen, zs, t(0)), "normal": np.where(seen[..., None], normal, t(0)), "color": np.where(seen[..., None], color, t(0)),
            "found": found, "k": np.where(found == 1, k, -1), "g": gs}


def reference(voxels, origin, spacing, iso, refine, rays):
    """The fp64 yardstick, the clean rays, E32 per output over the clean found rays, and the clean share of the hit rays."""
    args = (voxels, origin, spacing, iso, refine, rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    want, have = restate(*args, dtype=np.float64), restate(*args, dtype=np.float32)
    h = np.asarray(rays["hit"]) != 0
    away = (np.abs(want["g"] - np.float64(np.float32(iso))) >= ISO_MARGIN).all(-1)
    clean = h & away & (want["found"] == have["found"]) & (want["k"] == have["k"])
    held = clean & (want["found"] != 0)
    e32 = {key: float(np.abs(have[key].astype(np.float64) - want[key])[held].max(initial=0.0)) for key in ("depth", "normal", "color")}
    return want, clean, e32, float(clean.sum()) / max(int(h.sum()), 1)


# ------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------
def check_every_ray(got, hit, what):
    """What holds on every ray, clean or not."""
    depth, normal, color, found = (x.detach().cpu() for x in got)
    for key, x in zip(KEYS[:3], (depth, normal, color)):
        assert torch.isfinite(x).all(), (what, key)
    assert found.dtype == torch.uint8 and int(found.max()) <= 2, what
    length = normal[..., :3].double().norm(dim=-1)
    assert (((length - 1).abs() <= 1e-5) | (normal[..., :3] == 0).all(-1)).all(), (what, float((length - 1).abs().min()))
    assert (normal[..., 3] >= 0).all() and (normal[..., 3] <= 1 + 1e-6).all(), what
    gone = found == 0
    assert not found[torch.from_numpy(np.asarray(hit) == 0)].any(), what
    for key, x in zip(KEYS[:3], (depth, normal, color)):
        assert (bits(x)[gone] == 0).all(), (what, key)  # +0.0 exactly: a miss, or no crossing


def check_against(got, want, clean, e32, share, what):
    """The module's bars on the clean rays; prints every figure before it asserts."""
    errs = {}
    held = clean & (want["found"] != 0)
    for key, x in zip(KEYS[:3], got):
        errs[key] = float(np.abs(x.detach().cpu().numpy().astype(np.float64) - want[key])[held].max(initial=0.0))
    found = got[3].cpu().numpy()
    print(f"{what}: " + ", ".join(f"{key} err {errs[key]:.3e} (E32 {e32[key]:.3e}, bar {max(FLOOR[key], 4 * e32[key]):.3e})" for key in errs)
          + f"; clean {share:.3f}; found 1: {int((found == 1).sum())}, 2: {int((found == 2).sum())}, 0: {int((found == 0).sum())}")
    assert share >= MIN_CLEAN, what
    assert np.array_equal(found[clean], want["found"][clean]), what
    for key in errs:
        assert errs[key] <= max(FLOOR[key], 4 * e32[key]), (what, key, errs[key], e32[key])
    return errs


# ------------------------------------------------------------------------------------------------
# 1. random volumes against fp64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", REFINES)
@pytest.mark.parametrize("iso", ISOS)
@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("name", list(GRIDS))
def test_surface_against_fp64(R, name, S, iso, refine):
    from vanerf_amd import baked
    vox, grid = random_voxels(name), GRIDS[name]
    dev, host = device_rays(R, name, S)
    want, clean, e32, share = reference(vox.numpy(), grid["origin"], grid["spacing"], iso, refine, host)
    vol = volume_of(vox, grid, 0.1)
    got = baked.march_surface(vol, dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"], iso=iso, refine=refine, row_rays=NX)
    what = f"{name} S={S} iso={iso} refine={refine}"
    check_every_ray(got, host["hit"], what)
    check_against(got, want, clean, e32, share, what)
    found = got[3].cpu().numpy()
    if S >= 2:
        assert (found == 1).any(), what
    if iso > 0:
        assert (found == 2).any(), what
    if S == 1:
        assert not (found == 1).any(), what
    flat = baked.march_surface(vol, dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"], iso=iso, refine=refine)  # the tile only decides which rays share a block
    for a, b in zip(got, flat):
        assert torch.equal(a, b), what


# ------------------------------------------------------------------------------------------------
# 2. an affine field against its closed form
# ------------------------------------------------------------------------------------------------
# f = a . x + b.  No plane faces all three cameras (0 and 2 look at the box from opposite sides): this one falls along the view of cameras 0 and 1, whose
# rays cross it from outside, and camera 2's rays start inside it
AFFINE_F = (np.array([0.28, -0.09, -0.4]), 0.4)
AFFINE_C = (np.array([0.5, 0.4, 0.3]), np.array([[1.1, -0.7, 0.2], [-0.5, 0.9, 0.3], [0.6, 0.25, -0.8]]))  # colour = c0 + C x
AFFINE_ISO = 0.004


def affine_voxels(grid):
    nx, ny, nz = grid["dims"]
    o, s = (np.asarray(grid[k], dtype=np.float32).astype(np.float64) for k in ("origin", "spacing"))
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    xyz = o + np.stack([xx, yy, zz], -1) * s
    return torch.from_numpy(np.concatenate([(xyz @ AFFINE_F[0] + AFFINE_F[1])[..., None], AFFINE_C[0] + xyz @ AFFINE_C[1].T], -1).astype(np.float32)).contiguous()


def affine_expectation(grid, host):
    """Per ray, from the closed form alone (fp64): kind (1 a crossing strictly inside the sampled range from outside, 2 the first sample well
    inside, 0 neither, -1 too close to call: a hit ray whose first sample or crossing lies within the margins), depth, normal (4) and colour."""
    a, b = AFFINE_F
    iso = np.float64(np.float32(AFFINE_ISO))
    o = np.broadcast_to(host["cam_pos"][:, None, :3], host["rays_d"].shape).astype(np.float64)
    d, z = host["rays_d"].astype(np.float64), host["z"].astype(np.float64)
    f0 = (o + d * z[..., :1]) @ a + b
    f1 = (o + d * z[..., -1:]) @ a + b
    zc = (iso - b - o @ a) / (d @ a)
    h = host["hit"] != 0
    kind = np.full(h.shape, -1)
    kind[h & (f0 < iso - 1e-5)] = 2
    kind[h & (f0 > iso + 1e-5) & (f1 < iso - 1e-5)] = 1
    kind[h & (f0 > iso + 1e-5) & (f1 > iso + 1e-5)] = 0
    kind[~h] = 0
    zs = np.where(kind == 2, z[..., 0], zc)
    p = o + d * zs[..., None]
    n = a / np.linalg.norm(a)
    ndotv = np.maximum(0.0, -(d @ n) / np.linalg.norm(d, axis=-1))
    normal = np.concatenate([np.broadcast_to(n, d.shape), ndotv[..., None]], -1)
    return kind, zs, normal, AFFINE_C[0] + p @ AFFINE_C[1].T, p


@pytest.mark.parametrize("refine", [0, 2])
@pytest.mark.parametrize("S", [2, 3, 64, 129])
def test_affine_field_against_its_closed_form(R, S, refine):
    from vanerf_amd import baked
    grid = GRIDS["large"]
    vox = affine_voxels(grid)
    dev, host = device_rays(R, "large", S)
    kind, zs, normal, color, p = affine_expectation(grid, host)
    got = baked.march_surface(volume_of(vox, grid, 0.1), dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"], iso=AFFINE_ISO, refine=refine, row_rays=NX)
    what = f"affine S={S} refine={refine}"
    check_every_ray(got, host["hit"], what)
    depth_g, normal_g, color_g, found_g = (x.cpu().numpy() for x in got)
    sure = kind >= 0
    h = host["hit"] != 0
    assert np.array_equal(found_g[sure], kind[sure]), what
    assert (kind == 1).sum() > 0.5 * h.sum() and (kind == 2).any() and sure.sum() >= 0.9 * sure.size, (what, (kind == 1).sum(), (kind == 2).sum(), h.sum())
    seen = kind > 0
    errs = {"depth": np.abs(depth_g - zs)[seen].max(), "normal": np.abs(normal_g - normal)[seen].max(), "color": np.abs(color_g - color)[seen].max()}
    # crossings next to the grid's border, where the central difference is one-sided
    o, s, n = (np.asarray(grid[k], dtype=np.float64) for k in ("origin", "spacing", "dims"))
    u = (p - o) / s
    near_border = seen & ((u < 1.0) | (u > n - 2.0)).any(-1)
    print(f"{what}: depth err {errs['depth']:.3e}, normal err {errs['normal']:.3e}, colour err {errs['color']:.3e}; found 1: {int((kind == 1).sum())}, "
          f"2: {int((kind == 2).sum())}, 0: {int((kind == 0).sum())}, too close to call: {int((~sure).sum())}; within a cell of the border: {int(near_border.sum())}")
    assert near_border.sum() >= 5, what
    assert errs["depth"] <= 2e-5 and errs["color"] <= 2e-5 and errs["normal"] <= 1e-4, (what, errs)


# ------------------------------------------------------------------------------------------------
# 3. 1e30 entries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 64, 130])
def test_no_nan_comes_out_of_a_volume_with_outside_entries(R, S):
    from vanerf_amd import baked
    grid = GRIDS["large"]
    nx, ny, nz = grid["dims"]
    dev, host = device_rays(R, "large", S)
    g = torch.Generator().manual_seed(77)
    base = random_voxels("large")
    scattered = base.clone()
    scattered[..., 0][torch.rand(nz, ny, nx, generator=g) < 0.3] = 1e30
    scattered[:, :, 0, 0] = 1e30  # whole slabs
    scattered[nz - 2:, :, :, 0] = 1e30
    slabs = base.clone()
    slabs[:, :, 3:, 0] = 1e30      # the upper two thirds of x: rays that stay there see nothing
    empty = base.clone()
    empty[..., 0] = 1e30
    some_blind = some_found = 0
    for name, vox in (("scattered", scattered), ("slabs", slabs), ("empty", empty)):
        for iso in ISOS:
            for refine in (0, 2):
                what = f"{name} S={S} iso={iso} refine={refine}"
                got = baked.march_surface(volume_of(vox, grid, 0.1), dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"], iso=iso, refine=refine, row_rays=NX)
                check_every_ray(got, host["hit"], what)  # finite; |n| is 1 or 0
                # rays all of whose samples have eight outside corners
                pts = host["cam_pos"][:, None, None, :3] + host["rays_d"][:, :, None, :] * host["z"][..., None]
                o32, s32 = np.asarray(grid["origin"], dtype=np.float32), np.asarray(grid["spacing"], dtype=np.float32)
                idx = [cell_of(pts[..., a], o32[a], s32[a], n)[0] for a, n in enumerate((nx, ny, nz))]
                out = vox.numpy()[..., 0] == np.float32(1e30)
                blind = np.ones(pts.shape[:-1], dtype=bool)
                for dz in (0, 1):
                    for dy in (0, 1):
                        for dx in (0, 1):
                            blind &= out[idx[2] + dz, idx[1] + dy, idx[0] + dx]
                blind = blind.all(-1) & (host["hit"] != 0)
                found = got[3].cpu().numpy()
                assert not found[blind].any(), what
                some_blind += int(blind.sum())
                some_found += int((found != 0).sum())
                if name == "empty":
                    assert blind.sum() == (host["hit"] != 0).sum() and not found.any()
                # `found` as the restatement's on the clean rays.  No bar on the other outputs here: inside a cell with a 1e30 corner the field is
                # below iso only where that corner's weight is exactly 0, so which piece of a refinement round crosses hangs on a last bit
                want, clean, _, _ = reference(vox.numpy(), grid["origin"], grid["spacing"], iso, refine, host)
                assert np.array_equal(found[clean], want["found"][clean]), what
    assert some_blind > 0 and some_found > 0


# ------------------------------------------------------------------------------------------------
# 4. determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 129])
def test_the_same_bits_every_call(R, S):
    from vanerf_amd import baked
    vox, grid = random_voxels("large"), GRIDS["large"]
    dev, _ = device_rays(R, "large", S)
    vol = volume_of(vox, grid, 0.1)
    args = (vol, dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"])
    kw = dict(iso=0.012, refine=2, row_rays=NX)
    first = baked.march_surface(*args, **kw)
    again = baked.march_surface(*args, **kw)
    V, Rn = dev["hit"].shape
    nan = float("nan")
    filled = (torch.full((V, Rn), nan, device="cuda"), torch.full((V, Rn, 4), nan, device="cuda"), torch.full((V, Rn, 3), nan, device="cuda"),
              torch.full((V, Rn), 255, dtype=torch.uint8, device="cuda"))
    into = baked.march_surface(*args, **kw, out=filled)
    assert all(a is b for a, b in zip(into, filled))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = baked.march_surface(*args, **kw)
    side.synchronize()
    for key, a, b, c, d in zip(KEYS, first, again, into, on_side):
        a, b, c, d = (x.cpu().contiguous().view(torch.uint8) for x in (a, b, c, d))
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d), key
    assert (first[3] == 1).any() and (first[3] == 2).any()


# ------------------------------------------------------------------------------------------------
# 5. end to end on the synthetic two-hand frame
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_end_to_end_on_the_synthetic_frame(R, precision, monkeypatch):
    from tests.test_baked_volume import _net, _orbit
    from vanerf_amd import baked
    from vanerf_amd.novel_views import camera_to_cam_tar, render_novel_views
    net = _net(precision)
    frame_cpu = synth.make_frame(seed=3, tar_h=16, tar_w=16)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    S, H, W = 32, 16, 16
    vol = baked.bake_volume(net, trb, resolution=32)
    cams = [camera_to_cam_tar(c) for c in _orbit(frame_cpu, 8)[:3]]
    rays = R.ray_setup_views(cams, vol.bounds, 0, 0, 1, W, H, S)
    host = {k: rays[k].cpu().numpy() for k in ("rays_d", "cam_pos", "z", "hit")}
    vox_host = vol.voxels.cpu().numpy()
    colour = baked.render_volume(vol, cams, samples=S)

    # render_volume_surface = ray_setup_views + one march, and the march is the restatement's on the read-back voxels
    for refine in REFINES:
        o = baked.render_volume_surface(vol, cams, samples=S, refine=refine)
        want_bits = baked.march_surface(vol, rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"], iso=0.0, refine=refine, row_rays=W)
        for key, x in zip(KEYS, want_bits):
            assert torch.equal(o[key].cpu().contiguous().view(torch.uint8), x.cpu().contiguous().view(torch.uint8)), (refine, key)
        assert torch.equal(o["hit"], rays["hit"]) and torch.equal(o["index"], rays["index"]) and o["normal"].shape == (3, H * W, 4)
        got = tuple(o[key] for key in KEYS)
        want, clean, e32, share = reference(vox_host, vol.origin, vol.spacing, 0.0, refine, host)
        check_every_ray(got, host["hit"], f"{precision} refine={refine}")
        check_against(got, want, clean, e32, share, f"{precision}: render_volume_surface, refine={refine}")
        seen = o["found"].cpu().numpy() != 0
        assert seen.mean() > 0.05  # the views see the hands
        # how far the field at the surface point is from the level (fp64, on the found == 1 rays), and how the found pixels sit in the colour render's alpha
        one = o["found"].cpu().numpy() == 1
        p = host["cam_pos"][:, None, :3].astype(np.float64) + host["rays_d"].astype(np.float64) * o["depth"].cpu().numpy().astype(np.float64)[..., None]
        f_star = trilinear(vox_host[..., :1].astype(np.float64), [np.float32(v) for v in vol.origin], [np.float32(v) for v in vol.spacing], p)[..., 0]
        opaque = (colour["alpha"].cpu().numpy() > 0.5)[seen].mean() if seen.any() else float("nan")
        print(f"{precision}: refine={refine}: {int(seen.sum())} found pixels of {seen.size} ({int(one.sum())} crossings), |f64(p*) - iso| max "
              f"{np.abs(f_star[one]).max(initial=0.0):.3e} mean {np.abs(f_star[one]).mean() if one.any() else 0.0:.3e}; render_volume's alpha > 0.5 on {opaque:.3f} of them")
    assert torch.equal(baked.render_volume_surface(vol, cams, samples=1)["depth"], baked.march_surface(vol, rays["rays_d"], rays["cam_pos"], rays["z"][..., :1].contiguous(), rays["hit"])[0])

    # whole frames: the images follow from the kernel's outputs by the documented formulas
    o = baked.render_volume_surface(vol, cams, samples=S, refine=1)
    ambient, background = 0.3, 0.125
    by_mode = {mode: baked.render_baked_surface_views(vol, cams, samples=S, mode=mode, ambient=ambient, background=background) for mode in baked.SURFACE_MODES}
    for v in range(3):
        seen = (o["found"][v] != 0).view(1, H, W)
        n4 = o["normal"][v].view(H, W, 4).permute(2, 0, 1).double()
        rot = cams[v]["RT"].reshape(-1, 4, 4)[0, :3, :3].double().cuda()
        n_cam = torch.einsum("ij,jhw->ihw", rot, n4[:3])
        normal_img = 0.5 + 0.5 * n_cam * torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64, device="cuda").view(3, 1, 1)
        shade = ambient + (1.0 - ambient) * n4[3:]
        col = o["color"][v].view(H, W, 3).permute(2, 0, 1).double()
        depth = o["depth"][v].view(1, H, W).double()
        znear, zfar = float(cams[v]["znear"]), float(cams[v]["zfar"])
        tex = {"shaded": col * shade, "clay": (0.8 * shade).expand(3, H, W), "normal": normal_img, "depth": ((zfar - depth) / (zfar - znear)).expand(3, H, W)}
        bg = torch.full((), background, dtype=torch.float64, device="cuda")
        for mode, views in by_mode.items():
            d = views[v]
            assert len(views) == 3 and d["tex_fg_fine"] is d["tex_fg"] and d["vert_xy"].shape == (1, 1558, 2)
            assert d["depth"].shape == (1, H, W) and d["found"].shape == (1, H, W) and d["normal"].shape == (3, H, W) and d["tex_fg"].shape == (3, H, W)
            assert torch.equal(d["depth"].reshape(-1), o["depth"][v]) and torch.equal(d["found"].reshape(-1), o["found"][v]) and torch.equal(d["normal"], n4[:3].float())
            for key, want_img in (("normal_img", normal_img), ("shade", shade), ("tex_fg", tex[mode])):
                want_img = torch.where(seen, want_img, bg)
                assert (d[key].double() - want_img).abs().max() <= 1e-6, (mode, v, key)
                assert (d[key][(~seen).expand_as(d[key])] == background).all(), (mode, v, key)
        assert (~seen).any() and seen.any()
    via_model = net.render_surface_views(trb, cams, resolution=32, samples=S, mode="clay", ambient=ambient, background=background)
    for v in range(3):
        assert torch.equal(via_model[v]["tex_fg"], by_mode["clay"][v]["tex_fg"])

    # the orbit driver: one bake for the whole orbit
    bakes = []
    real = baked.bake_volume
    monkeypatch.setattr(baked, "bake_volume", lambda *a, **k: bakes.append(1) or real(*a, **k))
    orbit = _orbit(frame_cpu, 6)
    frames, _ = render_novel_views(net, orbit, trb, only_renderings=True, views_per_pass=4, render_views_fn=baked.surface_views_fn(32, 32))
    assert frames.shape == (6, 16, 16, 3) and frames.dtype == np.uint8 and len(bakes) == 1
    assert frames.max() > 0 and not np.array_equal(frames[0], frames[3])  # something is seen, and the orbit moves


def test_the_python_layer_refuses_bad_arguments(R):
    from vanerf_amd import baked
    vox, grid = random_voxels("small"), GRIDS["small"]
    vol = volume_of(vox, grid, 0.1)
    dev, _ = device_rays(R, "small", 4)
    args = (vol, dev["rays_d"], dev["cam_pos"], dev["z"], dev["hit"])
    cams = [cam_tar(c) for c in CAMERAS]
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="refine"):
            baked.march_surface(*args, refine=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="iso"):
            baked.march_surface(*args, iso=bad)
    with pytest.raises(ValueError, match="mode"):
        baked.render_baked_surface_views(vol, cams, samples=4, mode="wireframe")
    with pytest.raises(ValueError, match="volume's device"):
        baked.march_surface(vol, dev["rays_d"].cpu(), dev["cam_pos"], dev["z"], dev["hit"])
    with pytest.raises(ValueError, match="out normal"):
        baked.march_surface(*args, out=(torch.empty(3, 35, device="cuda"), torch.empty(3, 35, 3, device="cuda"), torch.empty(3, 35, 3, device="cuda"),
                                        torch.empty(3, 35, dtype=torch.uint8, device="cuda")))
    with pytest.raises(ValueError, match="samples"):
        baked.render_volume_surface(vol, cams, samples=0)
    o = baked.render_volume_surface(vol, cams, samples=4, x0=X0, y0=Y0, step=STEP, nx=NX, ny=NY)
    assert o["found"].shape == (3, NX * NY) and o["found"].dtype == torch.uint8
