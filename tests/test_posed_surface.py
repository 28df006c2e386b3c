"""Depth, normal and shaded views of the hand in another pose (vanerf_amd/posed.py, vanerf_amd/csrc/volume_surface.hip) on
a real MI355X: the march against its fp64 restatement at every sample count on both sides of a round of 64, for independent and for run-wise
faces, identity records against baked.march_surface bit for bit, an affine field through one rigid map against its closed form, the empty
rules, determinism, the end-to-end path on the synthetic two-hand frame and the argument checks.

The restatement (`restate`), the clean condition, the drawn inputs (`case_inputs`) and the closed form are those of
tests/test_posed_surface_cpu.py, which checks them on cases worked out by hand and shows that at least 90 % of the hit rays of every case
here are clean.

Bars: section 0h's own.  On clean rays `found` is equal exactly, depth and colour are within max(2e-5, 4 E32), the normal's four channels
within max(1e-4, 4 E32), E32 = max |fp32 - fp64| of the restatement over the clean found rays.  On every ray the outputs are finite, found is
at most 3, |n| is 1 within 1e-5 or exactly 0, n . v lies in [0, 1 + 1e-6], the outputs are +0 wherever found == 0, and found == 0 wherever
hit == 0."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import test_baked_surface as SF
from tests import test_baked_volume as B
from tests import test_posed_surface_cpu as C
from tests import test_posed_volume as PV
from tests import test_posed_volume_cpu as P
from vanerf_amd import synth

pytestmark = pytest.mark.gpu

R = B.R  # the module fixture: the renderer, or a failure without a GPU
bits = B.bits
dev = PV.dev
INF = float("inf")
KEYS = ("depth", "normal", "color", "found")
FLOOR = SF.FLOOR


def check_every_ray(got, hit, what):
    """What holds on every ray, clean or not."""
    depth, normal, color, found = (x.detach().cpu() for x in got)
    for key, x in zip(KEYS[:3], (depth, normal, color)):
        assert torch.isfinite(x).all(), (what, key)
    assert found.dtype == torch.uint8 and int(found.max()) <= 3, what
    length = normal[..., :3].double().norm(dim=-1)
    assert (((length - 1).abs() <= 1e-5) | (normal[..., :3] == 0).all(-1)).all(), (what, float((length - 1).abs().min()))
    assert (normal[..., 3] >= 0).all() and (normal[..., 3] <= 1 + 1e-6).all(), what
    gone = found == 0
    assert not found[torch.from_numpy(np.asarray(hit) == 0)].any(), what
    for key, x in zip(KEYS[:3], (depth, normal, color)):
        assert (bits(x)[gone] == 0).all(), (what, key)  # +0.0 exactly: a miss, or no crossing


def check_against(got, want, clean, e32, share, what, need_clean=True):
    """The module's bars on the clean rays; prints every figure before it asserts."""
    errs = {}
    held = clean & (want["found"] != 0)
    for key, x in zip(KEYS[:3], got):
        errs[key] = float(np.abs(x.detach().cpu().numpy().astype(np.float64) - want[key])[held].max(initial=0.0))
    found = got[3].cpu().numpy()
    print(f"{what}: " + ", ".join(f"{key} err {errs[key]:.3e} (E32 {e32[key]:.3e}, bar {max(FLOOR[key], 4 * e32[key]):.3e})" for key in errs)
          + f"; clean {share:.3f}; found 0 / 1 / 2 / 3: " + " / ".join(str(int((found == v).sum())) for v in range(4)))
    if need_clean:
        assert share >= C.MIN_CLEAN, what
    assert np.array_equal(found[clean], want["found"][clean]), what
    for key in errs:
        assert errs[key] <= max(FLOOR[key], 4 * e32[key]), (what, key, errs[key], e32[key])
    return errs


def zero_bits(got, what):
    for key, t in zip(KEYS, got):
        assert (bits(t) == 0).all() if t.dtype != torch.uint8 else not t.any(), (what, key)


# ------------------------------------------------------------------------------------------------
# 1. the march against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", C.REFINES)
@pytest.mark.parametrize("iso", C.ISOS)
@pytest.mark.parametrize("S", C.SAMPLES)
@pytest.mark.parametrize("name", list(B.GRIDS))
@pytest.mark.parametrize("kind", C.KINDS)
def test_march_against_fp64(R, kind, name, S, iso, refine):
    from vanerf_amd import posed
    vox, grid = B.random_voxels(name), B.GRIDS[name]
    rays, host = B.device_rays(R, name, S)
    T, face, sdf, reach = C.case_inputs(kind, name, S)
    want, clean, e32, share = C.reference(vox.numpy(), grid["origin"], grid["spacing"], iso, refine, T, face, sdf, reach, host)
    vol = B.volume_of(vox, grid, 0.1)
    args = (vol, dev(T), dev(face), dev(sdf), rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    got = posed.march_surface_posed(*args, iso=iso, refine=refine, reach=reach, row_rays=B.NX)
    what = f"{kind} {name} S={S} iso={iso} refine={refine}"
    check_every_ray(got, host["hit"], what)
    check_against(got, want, clean, e32, share, what)
    found = got[3].cpu().numpy()
    assert C.expected_kinds(kind, S, iso) <= set(found[clean].tolist()), what
    if S == 1:
        assert not ((found == 1) | (found == 3)).any(), what
    flat = posed.march_surface_posed(*args, iso=iso, refine=refine, reach=reach)  # the tile only decides which rays share a block
    for key, a, b in zip(KEYS, got, flat):
        assert torch.equal(bits(a), bits(b)) if a.dtype != torch.uint8 else torch.equal(a, b), (what, key)


# ------------------------------------------------------------------------------------------------
# 2. identity records: march_surface's bits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 64, 130])
def test_identity_records_give_the_bits_of_march_surface(R, S):
    """Both kernels are one search over a point map and differ by that map alone.  With every record exactly [I | 0], face = 0, sdf = 0 and
    reach = inf no sample is empty, the warp is exact -- for finite p, ((1 px + 0 py) + 0 pz) + 0 is px -- the near end re-evaluated under F
    is the sample's own value, and A^T G is G: march_surface_posed must return march_surface's bits.  tests/test_posed_volume.py's host-made
    inputs: 2 views of 5 x 3 rays (odd in both directions of the 2 x 2 tile) through a 7 x 6 x 5 grid, one ray with hit = 0."""
    from vanerf_amd import baked, posed
    rng = np.random.default_rng(40 + S)
    grid = PV.IDENTITY_GRID
    (nx, ny, nz), o, s = grid["dims"], np.array(grid["origin"]), np.array(grid["spacing"])
    vox = rng.random((nz, ny, nx, 4), dtype=np.float32)
    vox[..., 0] = vox[..., 0] * 0.07 - 0.02
    V, row_rays, rows = 2, 5, 3
    Rn = row_rays * rows
    eyes = np.array([[0.01, -0.02, 0.0], [0.95, 0.03, 1.01]])
    aims = o + rng.random((V, Rn, 3)) * s * (np.array([nx, ny, nz]) - 1)  # points of the grid's box
    d = aims - eyes[:, None]
    rays_d = dev((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32))
    cam_pos = dev(np.concatenate([eyes, np.zeros((V, 1))], 1).astype(np.float32))
    z = dev(np.sort(0.75 + 0.5 * rng.random((V, Rn, S), dtype=np.float32), axis=-1))  # from in front of the box to behind it
    hit = np.ones((V, Rn), dtype=np.uint8)
    hit[1, 4] = 0
    vol = B.volume_of(torch.from_numpy(vox), grid, 0.05)
    T = dev(np.tile(P.IDENTITY, (3, 1)))
    face, sdf = torch.zeros(V, Rn, S, dtype=torch.int32, device="cuda"), torch.zeros(V, Rn, S, device="cuda")
    kinds = set()
    for refine in (0, 2):
        for iso in (0.0, 0.012):
            plain = baked.march_surface(vol, rays_d, cam_pos, z, dev(hit), iso=iso, refine=refine, row_rays=row_rays)
            warped = posed.march_surface_posed(vol, T, face, sdf, rays_d, cam_pos, z, dev(hit), iso=iso, refine=refine, reach=INF, row_rays=row_rays)
            for key, a, b in zip(KEYS, plain, warped):
                assert torch.equal(a.cpu().contiguous().view(torch.uint8), b.cpu().contiguous().view(torch.uint8)), (S, refine, iso, key)
            kinds |= set(plain[3].cpu().numpy().ravel().tolist())
    assert {0, 2} <= kinds and (S == 1 or 1 in kinds)  # the rays do see the volume


# ------------------------------------------------------------------------------------------------
# 3. an affine field through one rigid map, T from the library's own pose_transforms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [0, 2])
@pytest.mark.parametrize("S", [2, 3, 64, 129])
def test_affine_field_through_a_rigid_map_against_its_closed_form(R, S, refine):
    from vanerf_amd import posed
    grid = B.GRIDS["large"]
    vox = SF.affine_voxels(grid)
    rays, host = B.device_rays(R, "large", S)
    kind, zs, normal, color, (T_np, face, sdf) = C.closed_form(host, S)
    vs, fs = P.sphere_mesh()
    T = posed.pose_transforms(dev(vs), dev(P.rigid(vs)[0]), dev(fs))  # the library's own transforms: direction, transposition and stride are under test
    assert np.abs(T.cpu().numpy() - T_np).max() <= 1e-6  # (2 ulp: tests/test_posed_volume.py)
    _, clean, e32, _ = C.reference(vox.numpy(), grid["origin"], grid["spacing"], SF.AFFINE_ISO, refine, T_np, face, sdf, INF, host)
    got = posed.march_surface_posed(B.volume_of(vox, grid, 0.1), T, dev(face), dev(sdf), rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"],
                                    iso=SF.AFFINE_ISO, refine=refine, reach=INF, row_rays=B.NX)
    what = f"rigid S={S} refine={refine}"
    check_every_ray(got, host["hit"], what)
    depth_g, normal_g, color_g, found_g = (x.cpu().numpy() for x in got)
    sure, seen = kind >= 0, kind > 0
    errs = {"depth": np.abs(depth_g - zs)[seen].max(), "normal": np.abs(normal_g - normal)[seen].max(), "color": np.abs(color_g - color)[seen].max()}
    print(f"{what}: " + ", ".join(f"{k} err {errs[k]:.3e} (E32 {e32[k]:.3e}, bar {max(FLOOR[k], 4 * e32[k]):.3e})" for k in errs)
          + "; found 0 / 1 / 2 / 3: " + " / ".join(str(int((kind == v).sum())) for v in range(4)) + f", too close to call: {int((~sure).sum())}")
    assert np.array_equal(found_g[sure], kind[sure]), what
    assert (kind == 1).any() and (kind == 2).any() and sure.mean() >= 0.9, what  # over the three cameras
    for k in errs:
        assert errs[k] <= max(FLOOR[k], 4 * e32[k]), (what, k, errs[k], e32[k])
    h = host["hit"] != 0
    assert np.ptp(color[seen & h], axis=0).min() > 0.05  # the colours do vary over the frame


# ------------------------------------------------------------------------------------------------
# 4. the empty rules
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 64, 130])
def test_empty_samples_are_outside(R, S):
    from vanerf_amd import baked, posed
    grid, vox = B.GRIDS["large"], B.random_voxels("large")
    rays, host = B.device_rays(R, "large", S)
    vs, fs = P.sphere_mesh()
    T = dev(P.restate_transforms(vs, P.rigid(vs, bend=0.3)[0], fs))
    face, sdf = P.draw_face_sdf(len(fs), host["z"].shape, S, odd=False)
    face = face.clip(0, len(fs) - 1)
    tail = (rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    vol = B.volume_of(vox, grid, 0.1)
    kw = dict(iso=0.012, refine=2, row_rays=B.NX)
    seen = posed.march_surface_posed(vol, T, dev(face), dev(sdf), *tail, reach=INF, **kw)
    assert (seen[3] != 0).any()  # the same inputs with nothing empty do see the volume
    cases = {"all faces -1": (np.full_like(face, -1), sdf, P.REACH), "all faces nf": (np.full_like(face, len(fs)), sdf, INF), "reach = -inf": (face, sdf, -INF),
             "all sdf NaN": (face, np.full_like(sdf, np.nan), INF)}
    for what, (fc, sd, reach) in cases.items():
        zero_bits(posed.march_surface_posed(vol, T, dev(fc), dev(sd), *tail, reach=reach, **kw), what)  # found = 0 and +0.0 exactly, on every ray
    # a volume of 1e30 voxels: finite outputs
    outside = baked.pack_volume(torch.full((grid["dims"][2], grid["dims"][1], grid["dims"][0]), float("nan")).cuda(), vox[..., 1:].contiguous().cuda())
    assert (outside[..., 0] == 1e30).all()
    for iso in C.ISOS:
        got = posed.march_surface_posed(B.volume_of(outside.cpu(), grid, 0.1), T, dev(face), dev(sdf), *tail, reach=INF, iso=iso, refine=2, row_rays=B.NX)
        check_every_ray(got, host["hit"], f"1e30 iso={iso}")
        assert not got[3].any()


# ------------------------------------------------------------------------------------------------
# 5. determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 129])
def test_the_same_bits_every_call(R, S):
    from vanerf_amd import posed
    vox, grid = B.random_voxels("large"), B.GRIDS["large"]
    rays, _ = B.device_rays(R, "large", S)
    T, face, sdf, reach = C.case_inputs("draw", "large", S)
    args = (B.volume_of(vox, grid, 0.1), dev(T), dev(face), dev(sdf), rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    kw = dict(iso=0.012, refine=2, reach=reach, row_rays=B.NX)
    first = posed.march_surface_posed(*args, **kw)
    again = posed.march_surface_posed(*args, **kw)
    V, Rn = rays["hit"].shape
    nan = float("nan")
    filled = (torch.full((V, Rn), nan, device="cuda"), torch.full((V, Rn, 4), nan, device="cuda"), torch.full((V, Rn, 3), nan, device="cuda"),
              torch.full((V, Rn), 255, dtype=torch.uint8, device="cuda"))
    into = posed.march_surface_posed(*args, **kw, out=filled)
    assert all(a is b for a, b in zip(into, filled))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = posed.march_surface_posed(*args, **kw)
    side.synchronize()
    for key, a, b, c, d in zip(KEYS, first, again, into, on_side):
        a, b, c, d = (x.cpu().contiguous().view(torch.uint8) for x in (a, b, c, d))
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d), key
    assert {0, 1, 2, 3} <= set(first[3].cpu().numpy().ravel().tolist())


# ------------------------------------------------------------------------------------------------
# 6. end to end on the synthetic two-hand frame
# ------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


FRAME_KEYS = {"depth", "found", "normal", "normal_img", "shade", "tex_fg", "tex_fg_fine", "vert_xy"}


def same_frames(a, b):
    return len(a) == len(b) and all(set(x) == set(y) == FRAME_KEYS and all(same_bits(x[k], y[k]) for k in FRAME_KEYS) for x, y in zip(a, b))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_end_to_end_on_the_synthetic_frame(R, precision, monkeypatch):
    from vanerf_amd import baked, mano, posed
    from vanerf_amd.novel_views import camera_to_cam_tar
    net = B._net(precision)
    frame_cpu = synth.make_frame(seed=3, tar_h=16, tar_w=16)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    S, V, H, W = 32, 3, 16, 16
    Rn = H * W
    vol = baked.bake_volume(net, trb, resolution=32)
    faces = posed._frame_faces(trb, vol.voxels.device)
    nf = faces.shape[0]
    cams = [camera_to_cam_tar(c) for c in B._orbit(frame_cpu, 8)[:3]]
    vox_host = vol.voxels.cpu().numpy()

    # (a) the hands moved by a centimetre: the wrapper is its stages, bit for bit, and the stages are the restatement
    pose = (vol.verts + torch.tensor([0.01, 0.0, 0.0], device="cuda")).contiguous()
    o = posed.render_posed_surface(vol, faces, pose, cams, samples=S)
    prep = posed.posed_samples(vol, faces, pose, cams, samples=S)
    assert isinstance(prep, posed.PosedSamples) and prep.T.shape == (nf, 12) and prep.face.shape == (V, Rn, S) and prep.row_rays == W
    staged = posed.march_surface_posed(vol, prep.T, prep.face, prep.sdf, prep.rays_d, prep.cam_pos, prep.z, prep.hit, row_rays=prep.row_rays)
    assert set(o) == {"depth", "normal", "color", "found", "hit", "index", "face", "sdf"} and o["normal"].shape == (V, Rn, 4) and o["found"].dtype == torch.uint8
    for key, t in zip(KEYS, staged):
        assert same_bits(o[key], t), key
    for key in ("hit", "index", "face", "sdf"):
        assert same_bits(o[key], getattr(prep, key)), key
    reused = posed.render_posed_surface(vol, faces, pose, cams, samples=S, accel=R.MeshAccel(pose, faces))
    handed = posed.render_posed_surface(vol, faces, pose, cams, samples=S, prepared=prep)
    assert all(same_bits(o[key], reused[key]) and same_bits(o[key], handed[key]) for key in o) and handed["face"] is prep.face
    colour = posed.render_posed_volume(vol, faces, pose, cams, samples=S)
    colour_handed = posed.render_posed_volume(vol, faces, pose, cams, samples=S, prepared=prep)
    assert set(colour) == set(colour_handed) and all(same_bits(colour[key], colour_handed[key]) for key in colour)
    host = {k: getattr(prep, k).cpu().numpy() for k in ("rays_d", "cam_pos", "z", "hit")}
    T_np, face_np, sdf_np = prep.T.cpu().numpy(), o["face"].cpu().numpy(), o["sdf"].cpu().numpy()
    for refine in (0, 1, 2):
        got = posed.march_surface_posed(vol, prep.T, prep.face, prep.sdf, prep.rays_d, prep.cam_pos, prep.z, prep.hit, refine=refine, row_rays=W)
        want, clean, e32, share = C.reference(vox_host, vol.origin, vol.spacing, 0.0, refine, T_np, face_np, sdf_np, posed.REACH, host)
        what = f"{precision}: moved pose against the restatement, refine={refine}"
        check_every_ray(got, host["hit"], what)
        check_against(got, want, clean, e32, share, what, need_clean=False)  # (the share is printed, not capped: section 0i's end-to-end does not cap it)
    found = o["found"].cpu().numpy()
    empty = P.empty_of(face_np, sdf_np, nf, posed.REACH)
    print(f"{precision}: moved pose: {100 * empty.mean():.1f} % of the samples are empty, {int((found != 0).sum())} of {found.size} rays found, "
          f"found == 3 on {int((found == 3).sum())} of them ({100 * (found == 3).sum() / max((found != 0).sum(), 1):.1f} %)")
    assert (found != 0).mean() > 0.05  # the views see the hands

    # (b) the identity pose on the volume's own bounds with no reach, against render_volume_surface
    base = baked.render_volume_surface(vol, cams, samples=S)
    same = posed.render_posed_surface(vol, faces, vol.verts, cams, samples=S, reach=INF, bounds=vol.bounds)
    assert torch.equal(same["hit"], base["hit"]) and torch.equal(same["index"], base["index"])
    identical = all(same_bits(same[key], base[key]) for key in KEYS)
    agree = (same["found"] == base["found"]).cpu().numpy()
    both = agree & (base["found"].cpu().numpy() != 0)
    gap = (same["depth"] - base["depth"]).abs().cpu().numpy()[both].max(initial=0.0)
    print(f"{precision}: identity pose against render_volume_surface: bit-identical = {identical}, found equal on {agree.mean():.4f} of the rays, "
          f"largest depth difference on them {gap:.3e}")

    # (c) frames: the images follow from the march's outputs by render_baked_surface_views' formulas
    ambient, background = 0.3, 0.125
    by_mode = {mode: posed.render_posed_surface_views(vol, faces, pose, cams, samples=S, mode=mode, ambient=ambient, background=background, prepared=prep)
               for mode in baked.SURFACE_MODES}
    assert same_frames(by_mode["shaded"], posed.render_posed_surface_views(vol, faces, pose, cams, samples=S, ambient=ambient, background=background))
    KRT = lambda c: c["KRT"].to("cuda").float()  # noqa: E731
    for v in range(V):
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
        vimg = pose[None] @ KRT(cams[v])[:, :3, :3].transpose(1, 2) + KRT(cams[v])[:, :3, 3][:, None]
        for mode, views in by_mode.items():
            d = views[v]
            assert len(views) == V and set(d) == FRAME_KEYS and d["tex_fg_fine"] is d["tex_fg"] and d["vert_xy"].shape == (1, 1558, 2)
            assert d["depth"].shape == (1, H, W) and d["found"].shape == (1, H, W) and d["normal"].shape == (3, H, W) and d["tex_fg"].shape == (3, H, W)
            assert torch.equal(d["depth"].reshape(-1), o["depth"][v]) and torch.equal(d["found"].reshape(-1), o["found"][v]) and torch.equal(d["normal"], n4[:3].float())
            assert torch.equal(d["vert_xy"], vimg[..., :2] / (vimg[..., 2:3] + 1e-8))  # the POSED vertices
            for key, want_img in (("normal_img", normal_img), ("shade", shade), ("tex_fg", tex[mode])):
                want_img = torch.where(seen, want_img, bg)
                assert (d[key].double() - want_img).abs().max() <= 1e-6, (mode, v, key)
                assert (d[key][(~seen).expand_as(d[key])] == background).all(), (mode, v, key)
        assert (~seen).any() and seen.any()
    # a pixel with found == 3 is shaded, not background.  One by construction: the sample behind a clean crossing gets a record of its own that
    # maps every point of the ray onto that sample's source point, so both ends of the bracket read its value, inside: found = 3, a zero
    # normal (A = 0), and the shade is the ambient term
    want, clean, _, _ = C.reference(vox_host, vol.origin, vol.spacing, 0.0, 1, T_np, face_np, sdf_np, posed.REACH, host)
    k1 = np.clip(want["k"] + 1, 0, S - 1)
    g1 = np.take_along_axis(want["g"], k1[..., None], -1)[..., 0]
    v0, r0 = np.argwhere(clean & (want["found"] == 1) & (g1 < -1e-4))[0]
    kk = int(k1[v0, r0])
    rec = T_np[face_np[v0, r0, kk]].astype(np.float64)
    p = host["cam_pos"][v0, :3].astype(np.float64) + host["rays_d"][v0, r0].astype(np.float64) * float(host["z"][v0, r0, kk])
    q = rec[:9].reshape(3, 3) @ p + rec[9:]
    T2 = torch.cat([prep.T, dev(np.float32([[0] * 9 + list(q)]))])
    face2 = prep.face.clone()
    face2[v0, r0, kk] = nf
    held = posed.render_posed_surface_views(vol, faces, pose, cams, samples=S, ambient=ambient, background=background,
                                            prepared=dataclasses.replace(prep, T=T2, face=face2))[v0]
    y0, x0 = divmod(int(r0), W)
    assert int(held["found"][0, y0, x0]) == 3 and float(held["depth"][0, y0, x0]) == float(host["z"][v0, r0, kk - 1])
    assert float(held["shade"][0, y0, x0]) == pytest.approx(ambient, abs=1e-7) and not held["normal"][:, y0, x0].any()
    assert (held["tex_fg"][:, y0, x0] != background).all() and (held["normal_img"][:, y0, x0] == 0.5).all()
    via_model = net.render_posed_surface_views(trb, pose, cams, volume=vol, samples=S, mode="clay", ambient=ambient, background=background)
    assert same_frames(via_model, by_mode["clay"])

    # (d) sequences: one bake, one camera or one per pose, render_posed_surface_views' bits
    bakes = []
    real = baked.bake_volume
    monkeypatch.setattr(baked, "bake_volume", lambda *a, **k: bakes.append(1) or real(*a, **k))
    poses = [vol.verts, pose, (vol.verts + torch.tensor([0.0, 0.005, 0.0], device="cuda")).contiguous()]
    frames = list(posed.posed_surface_sequence(net, trb, poses, cams[0], resolution=32, samples=S, mode="clay", ambient=ambient, background=background))
    assert len(frames) == 3 and len(bakes) == 1
    assert same_frames(frames[1:2], [by_mode["clay"][0]]) and not torch.equal(frames[0]["depth"], frames[1]["depth"])
    per_pose = list(posed.posed_surface_sequence(net, trb, poses, cams, volume=vol, samples=S, mode="normal", ambient=ambient, background=background))
    assert len(per_pose) == 3 and len(bakes) == 1 and same_frames(per_pose[1:2], [by_mode["normal"][1]])
    with pytest.raises(ValueError, match="one per pose"):
        posed.posed_surface_sequence(net, trb, poses, cams[:2])
    if precision == "fp32":  # (the pose track does not depend on the networks' arithmetic)
        frame_verts = frame_cpu["targets"]["vert_world"][0].numpy()
        hands = [mano.ManoModel.from_arrays(**dict(synth.mano_like_model(20 + h, nv=779), v_template=frame_verts[779 * h:779 * (h + 1)])) for h in range(2)]
        rng = np.random.default_rng(11)
        track = (dev((rng.standard_normal((3, 2, 48)) * 0.03).astype(np.float32)), dev((rng.standard_normal((3, 2, 10)) * 0.3).astype(np.float32)),
                 dev(rng.uniform(-0.005, 0.005, (3, 2, 3)).astype(np.float32)))
        kw = dict(flat_hand_mean=True, seal=False)
        skins = []
        real_skin = mano.skin_two_hands
        monkeypatch.setattr(mano, "skin_two_hands", lambda *a, **k: skins.append(1) or real_skin(*a, **k))
        by_track = list(posed.mano_surface_sequence(net, trb, *hands, *track, cams[0], resolution=32, samples=S, mode="depth", **kw))
        assert len(by_track) == 3 and len(bakes) == 2 and len(skins) == 1
        verts, _ = real_skin(*hands, *track, **kw)
        assert same_frames(by_track, [posed.render_posed_surface_views(vol, faces, verts[i].contiguous(), [cams[0]], samples=S, mode="depth")[0] for i in range(3)])
        by_method = net.mano_surface_sequence(trb, *hands, *track, cams, volume=vol, samples=S, mode="depth", **kw)  # one camera per pose
        assert isinstance(by_method, list) and len(bakes) == 2 and len(skins) == 2
        assert same_frames(by_method, [posed.render_posed_surface_views(vol, faces, verts[i].contiguous(), [cams[i]], samples=S, mode="depth")[0] for i in range(3)])
    baked_here = len(bakes)
    assert same_frames(net.render_posed_surface_views(trb, pose, cams, resolution=32, samples=S, mode="clay", ambient=ambient, background=background), by_mode["clay"])
    assert len(bakes) == baked_here + 1


# ------------------------------------------------------------------------------------------------
# 7. argument checks: refused with the library's message, nothing launched
# ------------------------------------------------------------------------------------------------
def test_the_entry_refuses_bad_arguments(R):
    import ctypes

    from vanerf_amd import _ffi
    lib = _ffi.lib
    vox = torch.zeros(3, 3, 3, 4, device="cuda")
    vox[..., 0] = -1.0
    rd, cp, z, hit = torch.zeros(4, 3, device="cuda"), torch.zeros(1, 4, device="cuda"), torch.zeros(4, 2, device="cuda"), torch.ones(4, dtype=torch.uint8, device="cuda")
    T = dev(np.tile(P.IDENTITY, (5, 1)))
    face, sdf = torch.zeros(4, 2, dtype=torch.int32, device="cuda"), torch.zeros(4, 2, device="cuda")
    depth, normal, color, found = torch.full((4,), 7.0, device="cuda"), torch.full((4, 4), 7.0, device="cuda"), torch.full((4, 3), 7.0, device="cuda"), \
        torch.full((4,), 7, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    good = dict(voxels=p(vox), origin=f3(0, 0, 0), spacing=f3(1, 1, 1), nx=3, ny=3, nz=3, iso=0.0, refine=1, rays_d=p(rd), cam_pos=p(cp), z=p(z), hit=p(hit), R=4,
                rays_per_view=4, row_rays=2, S=2, T=p(T), nf=5, face=p(face), sdf=p(sdf), reach=0.03, depth=p(depth), normal=p(normal), color=p(color),
                found=p(found), stream=None)
    assert C.entry_refusals(lib, good) > 35
    assert lib.vanerf_volume_surface_posed(*dict(good, R=0).values()) == 0  # no rays: a no-op
    torch.cuda.synchronize()
    assert (depth == 7.0).all() and (normal == 7.0).all() and (color == 7.0).all() and (found == 7).all()  # nothing was launched by any of the above
    assert lib.vanerf_volume_surface_posed(*good.values()) == 0
    torch.cuda.synchronize()
    assert (found == 2).all() and (depth == 0.0).all() and (normal == 0.0).all() and (color == 0.0).all()  # f = -1 at z = 0: every ray starts inside a constant field
    assert lib.vanerf_volume_surface_posed(*dict(good, reach=-INF).values()) == 0  # -inf is a reach: everything is empty
    torch.cuda.synchronize()
    assert (found == 0).all()


def test_the_python_layer_refuses_bad_arguments(R):
    from vanerf_amd import posed
    vox, grid = B.random_voxels("small"), B.GRIDS["small"]
    vol = B.volume_of(vox, grid, 0.1)
    rays, _ = B.device_rays(R, "small", 4)
    T, face, sdf = (dev(a) for a in P.march_inputs("small", 4))
    tail = (rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    V, Rn = rays["hit"].shape
    posed.march_surface_posed(vol, T, face, sdf, *tail)  # the good call
    with pytest.raises(ValueError, match="volume's device"):
        posed.march_surface_posed(vol, T.cpu(), face, sdf, *tail)
    with pytest.raises(ValueError, match="volume's device"):
        posed.march_surface_posed(vol, T, face, sdf, rays["rays_d"].cpu(), *tail[1:])
    with pytest.raises(ValueError, match="contiguous"):
        posed.march_surface_posed(vol, T.t().contiguous().t(), face, sdf, *tail)
    with pytest.raises(ValueError, match=r"\(nf, 12\)"):
        posed.march_surface_posed(vol, T[:, :9].contiguous(), face, sdf, *tail)
    with pytest.raises(ValueError, match="face: expected"):
        posed.march_surface_posed(vol, T, face[..., :-1].contiguous(), sdf, *tail)
    with pytest.raises(ValueError, match="sdf: expected"):
        posed.march_surface_posed(vol, T, face, sdf[:, :-1].contiguous(), *tail)
    with pytest.raises(ValueError, match="contiguous"):
        posed.march_surface_posed(vol, T, face.long(), sdf, *tail)  # int32 faces
    with pytest.raises(ValueError, match="NaN"):
        posed.march_surface_posed(vol, T, face, sdf, *tail, reach=float("nan"))
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="refine"):
            posed.march_surface_posed(vol, T, face, sdf, *tail, refine=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="iso"):
            posed.march_surface_posed(vol, T, face, sdf, *tail, iso=bad)
    with pytest.raises(ValueError, match="out normal"):
        posed.march_surface_posed(vol, T, face, sdf, *tail, out=(torch.empty(V, Rn, device="cuda"), torch.empty(V, Rn, 3, device="cuda"),
                                                                 torch.empty(V, Rn, 3, device="cuda"), torch.empty(V, Rn, dtype=torch.uint8, device="cuda")))
    v, f = P.sphere_mesh()
    cams = [B.cam_tar(c) for c in B.CAMERAS]
    with pytest.raises(ValueError, match="no source vertices"):
        posed.render_posed_surface(vol, dev(f), dev(v), cams, samples=4)
    with_verts = dataclasses.replace(vol, verts=dev(v))
    with pytest.raises(ValueError, match="accel"):
        posed.render_posed_surface(with_verts, dev(f), dev(v), cams, samples=4, accel=object())
    with pytest.raises(ValueError, match="samples"):
        posed.posed_samples(with_verts, dev(f), dev(v), cams, samples=0)
    with pytest.raises(ValueError, match="prepared"):
        posed.render_posed_surface(with_verts, dev(f), dev(v), cams, samples=4, prepared=object())
    with pytest.raises(ValueError, match="mode"):
        posed.render_posed_surface_views(with_verts, dev(f), dev(v), cams, samples=4, mode="wireframe")
    o = posed.render_posed_surface(with_verts, dev(f), dev(v), cams, samples=4, x0=B.X0, y0=B.Y0, step=B.STEP, nx=B.NX, ny=B.NY)  # and the good call on a pixel grid
    assert o["found"].shape == (3, B.NX * B.NY) and o["found"].dtype == torch.uint8 and o["face"].shape == (3, B.NX * B.NY, 4)
