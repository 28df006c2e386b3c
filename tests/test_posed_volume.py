"""The baked hand in another pose (vanerf_amd/posed.py, vanerf_amd/csrc/pose_warp.hip) on a real MI355X: the per-face
transforms against fp64, the march against its restatement at every sample count on both sides of a round of 64, the identity pose against
march_volume bit for bit, an affine field seen through a
rigid map against its closed form, the empty rules, determinism, the end-to-end path on the synthetic two-hand frame and the argument checks.

The restatements (`restate_transforms`, `restate_march`) and the drawn inputs are those of tests/test_posed_volume_cpu.py, which checks them on
cases worked out by hand and shows that the draws satisfy the `clean` condition.  The march takes (face, sdf) as INPUTS, so the tests draw them:
10 % of the faces are -1 or nf, sdf is uniform in [-0.02, 0.06] against reach = 0.03, one sample in 50 carries a NaN or an infinity.

Bars: section 0g's own (tests/test_baked_volume.py).  Colour and alpha within max(2e-5, 4 E32), E32 = max |fp32 - fp64| of the restatement; depth
under the same bar on CLEAN rays (fp64 acc > 0.05 or < 1e-13), at least 80 % of the hit rays of every drawn case.  Transforms: every value
within 2 ulp (fp32) of the fp64 numpy result rounded to fp32 -- the kernel works in fp64, where conditioning of up to 1e4 leaves 1e-12, enough
to move a rounding by one step and no more."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_baked_volume as B
from tests import test_posed_volume_cpu as P
from vanerf_amd import synth

pytestmark = pytest.mark.gpu

R = B.R  # the module fixture: the renderer, or a failure without a GPU
bits = B.bits
INF = float("inf")


def check_against(got, want, held, e32, share, what, need_clean=True):
    """Section 0g's bars; prints every figure before it asserts."""
    errs = {}
    for k, g in zip(("color", "depth", "alpha"), got):
        g = g.detach().cpu().numpy().astype(np.float64)
        errs[k] = float(np.abs(g - want[k])[held[k]].max(initial=0.0))
    print(f"{what}: " + ", ".join(f"{k} err {errs[k]:.3e} (E32 {e32[k]:.3e}, bar {max(B.FLOOR, 4 * e32[k]):.3e})" for k in errs) + f"; clean {share:.3f}")
    if need_clean:
        assert share >= B.MIN_CLEAN, what
    for k in errs:
        assert errs[k] <= max(B.FLOOR, 4 * e32[k]), (what, k, errs[k], e32[k])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------
# 1. transforms
# ------------------------------------------------------------------------------------------------
def _mesh(which):
    if which == "sphere":
        return P.sphere_mesh()
    v, f = synth.fingered_hand()
    return np.asarray(v, dtype=np.float32), np.asarray(f).astype(np.int32)


@pytest.mark.parametrize("which", ["sphere", "hand"])
def test_transforms_against_fp64(R, which):
    from vanerf_amd import posed
    v, f = _mesh(which)
    pose, _ = P.rigid(v, bend=0.3)
    want = P.restate_transforms(v, pose, f)
    assert np.isfinite(want).all() and np.abs(want[:, :9].reshape(-1, 3, 3) - np.eye(3)).max() > 0.1  # a real pose, every face with a frame
    T = posed.pose_transforms(dev(v), dev(pose), dev(f))
    assert T.shape == (len(f), 12) and T.dtype == torch.float32 and T.is_cuda
    got = T.cpu().numpy()
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print(f"{which}: {len(f)} faces, largest difference {ulps.max():.2f} ulp, {int((ulps > 0).sum())} of {ulps.size} values differ")
    assert ulps.max() <= 2.0
    # what the record is for: it carries the face's posed vertices onto its source vertices
    A, t = got[:, :9].reshape(-1, 3, 3).astype(np.float64), got[:, 9:].astype(np.float64)
    for k in range(3):
        back = np.einsum("fij,fj->fi", A, pose[f[:, k]].astype(np.float64)) + t
        assert np.abs(back - v[f[:, k]]).max() <= 1e-6
    assert torch.equal(bits(posed.pose_transforms(dev(v), dev(pose), dev(f))), bits(T))


def test_faces_without_a_frame_get_the_fallback_exactly(R):
    from vanerf_amd import posed
    v, f = P.sphere_mesh()
    pose, _ = P.rigid(v, bend=0.3)
    pose[7] = [np.nan, 0.5, 1.0]                       # one NaN vertex: every face around it
    f = np.concatenate([f, [[3, 3, 9], [2, 40, 5], [-1, 2, 5]]]).astype(np.int32)  # one zero-area face; two that name no vertex
    want = P.restate_transforms(v, pose, f)
    got = posed.pose_transforms(dev(v), dev(pose), dev(f)).cpu().numpy()
    eye = np.eye(3, dtype=np.float32).reshape(9)
    fallen = (want[:, :9] == eye).all(1)
    around = (f == 7).any(1)
    assert fallen.sum() == around.sum() + 3 and fallen[around].all() and fallen[-3:].all() and np.isnan(want[around, 9]).all()
    assert (want[-2:, 9:] == 0).all() and np.isfinite(want[-3]).all()
    assert np.array_equal(got[fallen], want[fallen], equal_nan=True)  # exactly
    ulps = np.abs(got[~fallen].astype(np.float64) - want[~fallen]) / np.spacing(np.abs(want[~fallen])).astype(np.float64)
    assert ulps.max() <= 2.0


# ------------------------------------------------------------------------------------------------
# 2. the march against the restatement
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", P.BETAS)
@pytest.mark.parametrize("S", P.SAMPLES)
@pytest.mark.parametrize("name", list(B.GRIDS))
def test_march_against_fp64(R, name, S, beta):
    from vanerf_amd import posed
    vox, grid = B.random_voxels(name), B.GRIDS[name]
    rays, host = B.device_rays(R, name, S)
    T, face, sdf = P.march_inputs(name, S)
    want, held, e32, share = P.reference(vox.numpy(), grid["origin"], grid["spacing"], beta, T, face, sdf, P.REACH, host)
    args = (dev(T), dev(face), dev(sdf), rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    got = posed.march_volume_posed(B.volume_of(vox, grid, beta), *args, reach=P.REACH, row_rays=B.NX)
    check_against(got, want, held, e32, share, f"{name} S={S} beta={beta} by value")
    B.check_missed_rays(got, host["hit"], "by value")
    by_handle = posed.march_volume_posed(B.volume_of(vox, grid, B.handle_with(R, beta)), *args, reach=P.REACH, row_rays=B.NX)
    flat = posed.march_volume_posed(B.volume_of(vox, grid, beta), *args, reach=P.REACH)  # the tile only decides which rays share a block
    for a, b, c in zip(got, by_handle, flat):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c))


IDENTITY_GRID = dict(dims=(7, 6, 5), origin=(-0.12, -0.1, 0.9), spacing=(0.04, 0.04, 0.05))


@pytest.mark.parametrize("S", [1, 64, 130])
def test_the_identity_pose_gives_the_bits_of_march_volume(R, S):
    """Both marches are wave_ray.h's march_rounds on volume_field.h's field and differ by their sample functor alone.  With every record
    exactly [I | 0], face = 0, sdf = 0 and reach = inf no sample is empty and the warp is exact -- for finite p, ((1 px + 0 py) + 0 pz) + 0
    is px -- so march_volume_posed must return march_volume's bits.  Host-made inputs: 2 views of 5 x 3 rays (odd in both directions of the
    2 x 2 tile) through a 7 x 6 x 5 grid, one ray with hit = 0, sample counts on both sides of a round of 64."""
    from vanerf_amd import baked, posed
    rng = np.random.default_rng(40 + S)
    grid = IDENTITY_GRID
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
    T = dev(np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32), (3, 1)))
    face, sdf = torch.zeros(V, Rn, S, dtype=torch.int32, device="cuda"), torch.zeros(V, Rn, S, device="cuda")
    plain = baked.march_volume(vol, rays_d, cam_pos, z, dev(hit), row_rays=row_rays)
    warped = posed.march_volume_posed(vol, T, face, sdf, rays_d, cam_pos, z, dev(hit), reach=INF, row_rays=row_rays)
    assert float(plain[2].max()) > 0.1 and torch.isfinite(plain[1]).all()  # the rays do see the volume
    for k, a, b in zip(("color", "depth", "alpha"), plain, warped):
        assert torch.equal(bits(a), bits(b)), k


# ------------------------------------------------------------------------------------------------
# 3. an affine field through one rigid map: the expectation comes from the sample points
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.1, 0.01])
@pytest.mark.parametrize("S", [1, 3, 64, 129])
def test_affine_field_through_a_rigid_map_against_its_closed_form(R, S, beta):
    from vanerf_amd import posed
    grid = B.GRIDS["large"]
    rays, host = B.device_rays(R, "large", S)
    want, held, e32, share, kept, (vs, pose, fs, face, sdf) = P.closed_form(host, S, beta)
    T = posed.pose_transforms(dev(vs), dev(pose), dev(fs))  # the library's own transforms: direction, transposition and stride are under test
    got = posed.march_volume_posed(B.volume_of(B.affine_voxels(grid), grid, beta), T, dev(face), dev(sdf), rays["rays_d"], rays["cam_pos"], rays["z"],
                                   rays["hit"], reach=INF, row_rays=B.NX)
    assert kept > 0.5
    check_against(got, want, held, e32, share, f"rigid S={S} beta={beta} ({100 * kept:.0f} % of the samples kept)")
    h = host["hit"] != 0
    assert np.ptp(want["color"][h], axis=0).min() > 0.05  # the colours do vary over the frame


# ------------------------------------------------------------------------------------------------
# 4. the empty rules
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 64, 130])
def test_empty_samples_contribute_exactly_nothing(R, S):
    from vanerf_amd import baked, posed
    grid, vox = B.GRIDS["large"], B.random_voxels("large")
    rays, host = B.device_rays(R, "large", S)
    vs, fs = P.sphere_mesh()
    T = dev(P.restate_transforms(vs, P.rigid(vs, bend=0.3)[0], fs))
    face, sdf = P.draw_face_sdf(len(fs), host["z"].shape, S, odd=False)
    face = face.clip(0, len(fs) - 1)
    tail = (rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    vol = B.volume_of(vox, grid, 0.1)
    seen = posed.march_volume_posed(vol, T, dev(face), dev(sdf), *tail, reach=INF, row_rays=B.NX)
    assert float(seen[2].max()) > 0.5  # the same inputs with nothing empty do see the volume
    cases = {"all faces -1": (np.full_like(face, -1), sdf, P.REACH), "all faces nf": (np.full_like(face, len(fs)), sdf, INF), "reach = -inf": (face, sdf, -INF),
             "all sdf NaN": (face, np.full_like(sdf, np.nan), INF)}
    for what, (fc, sd, reach) in cases.items():
        got = posed.march_volume_posed(vol, T, dev(fc), dev(sd), *tail, reach=reach, row_rays=B.NX)
        for k, t in zip(("color", "depth", "alpha"), got):
            assert (bits(t) == 0).all(), (what, k)  # +0.0 exactly, on every ray
    # a volume of 1e30 voxels: finite outputs and alpha exactly 0
    outside = baked.pack_volume(torch.full((grid["dims"][2], grid["dims"][1], grid["dims"][0]), float("nan")).cuda(), vox[..., 1:].contiguous().cuda())
    assert (outside[..., 0] == 1e30).all()
    for beta in (0.1, 1e-3):
        got = posed.march_volume_posed(B.volume_of(outside.cpu(), grid, beta), T, dev(face), dev(sdf), *tail, reach=INF, row_rays=B.NX)
        for k, t in zip(("color", "depth", "alpha"), got):
            assert torch.isfinite(t).all(), (beta, k)
        assert (bits(got[2]) == 0).all() and (bits(got[0]) == 0).all()


# ------------------------------------------------------------------------------------------------
# 5. determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 129])
def test_the_same_bits_every_call(R, S):
    from vanerf_amd import posed
    vox, grid = B.random_voxels("large"), B.GRIDS["large"]
    rays, host = B.device_rays(R, "large", S)
    T, face, sdf = P.march_inputs("large", S)
    args = (B.volume_of(vox, grid, 0.01), dev(T), dev(face), dev(sdf), rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    first = posed.march_volume_posed(*args, reach=P.REACH, row_rays=B.NX)
    again = posed.march_volume_posed(*args, reach=P.REACH, row_rays=B.NX)
    V, Rn = rays["hit"].shape
    filled = (torch.full((V, Rn, 3), float("nan"), device="cuda"), torch.full((V, Rn), float("nan"), device="cuda"), torch.full((V, Rn), float("nan"), device="cuda"))
    into = posed.march_volume_posed(*args, reach=P.REACH, row_rays=B.NX, out=filled)
    assert all(a is b for a, b in zip(into, filled))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = posed.march_volume_posed(*args, reach=P.REACH, row_rays=B.NX)
    side.synchronize()
    for k, a, b, c, d in zip(("color", "depth", "alpha"), first, again, into, on_side):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c)) and torch.equal(bits(a), bits(d)), k


# ------------------------------------------------------------------------------------------------
# 6. end to end on the synthetic two-hand frame
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_end_to_end_on_the_synthetic_frame(R, precision, monkeypatch):
    from vanerf_amd import baked, posed
    from vanerf_amd.mask_at_box import frame_bounds
    from vanerf_amd.novel_views import camera_to_cam_tar
    net = B._net(precision)
    frame_cpu = synth.make_frame(seed=3, tar_h=16, tar_w=16)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    S, V, Rn = 32, 3, 16 * 16
    vol = baked.bake_volume(net, trb, resolution=32)
    faces = posed._frame_faces(trb, vol.voxels.device)
    assert faces.shape == (3108, 3) and faces.dtype == torch.int32 and vol.verts.shape == (1558, 3)
    cams = [camera_to_cam_tar(c) for c in B._orbit(frame_cpu, 8)[:3]]
    beta = float(net.state_dict()["sigmoid_beta"].reshape(-1)[0])
    vox_host = vol.voxels.cpu().numpy()

    # (a) the identity pose on the volume's own bounds with no reach: render_volume
    base = baked.render_volume(vol, cams, samples=S)
    same = posed.render_posed_volume(vol, faces, vol.verts, cams, samples=S, reach=INF, bounds=vol.bounds)
    assert torch.equal(same["hit"], base["hit"]) and torch.equal(same["index"], base["index"])
    assert same["face"].shape == (V, Rn, S) and same["face"].dtype == torch.int32 and same["sdf"].shape == (V, Rn, S) and same["sdf"].dtype == torch.float32
    assert int(same["face"].min()) >= 0 and int(same["face"].max()) < 3108 and torch.isfinite(same["sdf"]).all()
    rays = R.ray_setup_views(cams, vol.bounds, 0, 0, 1, 16, 16, S)
    host = {k: rays[k].cpu().numpy() for k in ("rays_d", "cam_pos", "z", "hit")}
    _, held, e32, share = B.reference(vox_host, vol.origin, vol.spacing, beta, host)
    want = {k: base[k].cpu().numpy().astype(np.float64) for k in ("color", "depth", "alpha")}
    identical = all(torch.equal(bits(same[k]), bits(base[k])) for k in ("color", "depth", "alpha"))
    print(f"{precision}: identity pose against render_volume: bit-identical = {identical}")
    check_against((same["color"], same["depth"], same["alpha"]), want, held, e32, share, f"{precision}: identity pose against render_volume", need_clean=False)
    assert float(base["alpha"].max()) > 0.5  # the views see the hands

    # (b) the hands moved by a centimetre: the wrapper is its stages, bit for bit, and the stages are the restatement
    pose = (vol.verts + torch.tensor([0.01, 0.0, 0.0], device="cuda")).contiguous()
    o = posed.render_posed_volume(vol, faces, pose, cams, samples=S)
    T = posed.pose_transforms(vol.verts, pose, faces)
    accel = R.MeshAccel(pose, faces)
    rays = R.ray_setup_views(cams, frame_bounds(pose), 0, 0, 1, 16, 16, S)
    pts = R.sample_points(rays["rays_d"].view(-1, 3), rays["cam_pos"], rays["z"].view(-1, S), rays_per_view=Rn)
    sdf, _, face = R.mesh_query_accel(accel, pose, faces, torch.zeros(1558, device="cuda"), pts, want_face=True, want_knn=False)
    staged = posed.march_volume_posed(vol, T, face.view(V, Rn, S), sdf.view(V, Rn, S), rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"], row_rays=16)
    assert torch.equal(o["face"].view(-1), face) and torch.equal(bits(o["sdf"].view(-1)), bits(sdf)) and torch.equal(o["hit"], rays["hit"]) and torch.equal(o["index"], rays["index"])
    for k, t in zip(("color", "depth", "alpha"), staged):
        assert torch.equal(bits(o[k]), bits(t)), k
    reused = posed.render_posed_volume(vol, faces, pose, cams, samples=S, accel=accel)
    assert all(torch.equal(bits(o[k]), bits(reused[k])) for k in ("color", "depth", "alpha"))
    host = {k: rays[k].cpu().numpy() for k in ("rays_d", "cam_pos", "z", "hit")}
    T_np = P.restate_transforms(vol.verts.cpu().numpy(), pose.cpu().numpy(), faces.cpu().numpy())
    face_np, sdf_np = o["face"].cpu().numpy(), o["sdf"].cpu().numpy()
    want, held, e32, share = P.reference(vox_host, vol.origin, vol.spacing, beta, T_np, face_np, sdf_np, posed.REACH, host)
    empty = P.empty_of(face_np, sdf_np, 3108, posed.REACH)
    print(f"{precision}: moved pose: {100 * empty.mean():.1f} % of the samples are empty, {100 * float((host['hit'] != 0).mean()):.1f} % of the rays hit the box")
    check_against((o["color"], o["depth"], o["alpha"]), want, held, e32, share, f"{precision}: moved pose against the restatement", need_clean=False)
    B.check_missed_rays((o["color"], o["depth"], o["alpha"]), host["hit"], precision)
    assert 0.3 < empty.mean() < 1.0 and float(o["alpha"].max()) > 0.5 and not torch.equal(o["alpha"], base["alpha"])

    # (c) the animation loop bakes once; the module's method returns frames laid out as render_baked_views lays them out
    bakes = []
    real = baked.bake_volume
    monkeypatch.setattr(baked, "bake_volume", lambda *a, **k: bakes.append(1) or real(*a, **k))
    poses = [vol.verts, pose, (vol.verts + torch.tensor([0.0, 0.005, 0.0], device="cuda")).contiguous()]
    frames = list(posed.posed_sequence(net, trb, poses, cams[0], resolution=32, samples=S))
    assert len(frames) == 3 and len(bakes) == 1
    assert torch.equal(bits(frames[1]["tex_fg"]), bits(o["color"][0].view(16, 16, 3).permute(2, 0, 1))) and not torch.equal(frames[0]["alpha"], frames[1]["alpha"])
    per_pose = list(posed.posed_sequence(net, trb, poses, cams, volume=vol, samples=S))  # one camera per pose, a volume handed in: no bake
    assert len(per_pose) == 3 and len(bakes) == 1 and torch.equal(bits(per_pose[1]["alpha"].view(-1)), bits(posed.render_posed_volume(vol, faces, pose, [cams[1]], samples=S)["alpha"].view(-1)))
    with pytest.raises(ValueError, match="one per pose"):
        posed.posed_sequence(net, trb, poses, cams[:2])
    views = net.render_posed_views(trb, pose, cams, resolution=32, samples=S)
    assert len(views) == 3 and len(bakes) == 2
    KRT = lambda c: c["KRT"].to("cuda").float()  # noqa: E731
    for v, d in enumerate(views):
        assert set(d) == {"tex_fg", "depth", "alpha", "tex_fg_fine", "vert_xy"} and d["tex_fg_fine"] is d["tex_fg"]
        assert d["tex_fg"].shape == (3, 16, 16) and d["depth"].shape == (1, 16, 16) and d["alpha"].shape == (1, 16, 16) and d["vert_xy"].shape == (1, 1558, 2)
        assert torch.equal(bits(d["alpha"].view(-1)), bits(o["alpha"][v])) and torch.equal(bits(d["tex_fg"]), bits(o["color"][v].view(16, 16, 3).permute(2, 0, 1)))
        vimg = pose[None] @ KRT(cams[v])[:, :3, :3].transpose(1, 2) + KRT(cams[v])[:, :3, 3][:, None]
        assert torch.equal(d["vert_xy"], vimg[..., :2] / (vimg[..., 2:3] + 1e-8))  # the POSED vertices
        src = vol.verts[None] @ KRT(cams[v])[:, :3, :3].transpose(1, 2) + KRT(cams[v])[:, :3, 3][:, None]
        assert not torch.equal(d["vert_xy"], src[..., :2] / (src[..., 2:3] + 1e-8))
    given = net.render_posed_views(trb, pose, cams[:1], volume=vol, samples=S)
    assert len(bakes) == 2 and torch.equal(bits(given[0]["tex_fg"]), bits(views[0]["tex_fg"]))


# ------------------------------------------------------------------------------------------------
# 7. argument checks: refused with the library's message, nothing launched
# ------------------------------------------------------------------------------------------------
def test_the_entries_refuse_bad_arguments(R):
    from vanerf_amd import _ffi
    lib = _ffi.lib
    vox = torch.zeros(3, 3, 3, 4, device="cuda")
    rd, cp, z, hit = torch.zeros(4, 3, device="cuda"), torch.zeros(1, 4, device="cuda"), torch.zeros(4, 2, device="cuda"), torch.ones(4, dtype=torch.uint8, device="cuda")
    T = torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]] * 5, dtype=torch.float32, device="cuda")
    face, sdf = torch.zeros(4, 2, dtype=torch.int32, device="cuda"), torch.zeros(4, 2, device="cuda")
    color, depth, alpha = torch.full((4, 3), 7.0, device="cuda"), torch.full((4,), 7.0, device="cuda"), torch.full((4,), 7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    good = dict(voxels=p(vox), origin=f3(0, 0, 0), spacing=f3(1, 1, 1), nx=3, ny=3, nz=3, w=None, beta=0.1, rays_d=p(rd), cam_pos=p(cp), z=p(z), hit=p(hit), R=4,
                rays_per_view=4, row_rays=2, S=2, T=p(T), nf=5, face=p(face), sdf=p(sdf), reach=0.03, color=p(color), depth=p(depth), alpha=p(alpha), stream=None)
    assert P.march_refusals(lib, good) > 30
    assert lib.vanerf_volume_render_posed(*dict(good, R=0).values()) == 0  # no rays: a no-op
    verts, tri = torch.rand(6, 3, device="cuda"), torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device="cuda")
    rec = torch.full((2, 12), 7.0, device="cuda")
    tgood = dict(verts_src=p(verts), verts_pose=p(verts), nv=6, faces=p(tri), nf=2, T=p(rec), stream=None)
    P.transform_refusals(lib, tgood)
    torch.cuda.synchronize()
    assert (color == 7.0).all() and (depth == 7.0).all() and (alpha == 7.0).all() and (rec == 7.0).all()  # nothing was launched by any of the above
    assert lib.vanerf_volume_render_posed(*good.values()) == 0 and lib.vanerf_pose_transforms(*tgood.values()) == 0
    torch.cuda.synchronize()
    assert (alpha == 1.0).all() and (color == 0.0).all() and (depth == 0.0).all()  # f = 0 at z = 0: the last sample's 1e10 makes the ray opaque
    assert (rec[:, :9].view(2, 3, 3) - torch.eye(3, device="cuda")).abs().max() <= 1e-6 and rec[:, 9:].abs().max() <= 1e-6
    assert lib.vanerf_volume_render_posed(*dict(good, reach=-INF).values()) == 0  # -inf is a reach: everything is empty
    torch.cuda.synchronize()
    assert (alpha == 0.0).all()


def test_the_python_layer_refuses_bad_arguments(R):
    from vanerf_amd import posed
    vox, grid = B.random_voxels("small"), B.GRIDS["small"]
    vol = B.volume_of(vox, grid, 0.1)
    rays, _ = B.device_rays(R, "small", 4)
    T, face, sdf = P.march_inputs("small", 4)
    T, face, sdf = dev(T), dev(face), dev(sdf)
    tail = (rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"])
    posed.march_volume_posed(vol, T, face, sdf, *tail)  # the good call
    with pytest.raises(ValueError, match="volume's device"):
        posed.march_volume_posed(vol, T.cpu(), face, sdf, *tail)
    with pytest.raises(ValueError, match="volume's device"):
        posed.march_volume_posed(vol, T, face, sdf.cpu(), *tail)
    with pytest.raises(ValueError, match="contiguous"):
        posed.march_volume_posed(vol, T.t().contiguous().t(), face, sdf, *tail)
    with pytest.raises(ValueError, match="contiguous"):
        posed.march_volume_posed(vol, T, face.transpose(0, 1).contiguous().transpose(0, 1), sdf, *tail)
    for bad in (T[:, :9].contiguous(), T.view(-1), T.view(-1, 6)):
        with pytest.raises(ValueError, match=r"\(nf, 12\)"):
            posed.march_volume_posed(vol, bad, face, sdf, *tail)
    with pytest.raises(ValueError, match="face: expected"):
        posed.march_volume_posed(vol, T, face[..., :-1].contiguous(), sdf, *tail)
    with pytest.raises(ValueError, match="sdf: expected"):
        posed.march_volume_posed(vol, T, face, sdf[:, :-1].contiguous(), *tail)
    with pytest.raises(ValueError, match="contiguous"):
        posed.march_volume_posed(vol, T, face.long(), sdf, *tail)  # int32 faces
    with pytest.raises(ValueError, match="NaN"):
        posed.march_volume_posed(vol, T, face, sdf, *tail, reach=float("nan"))
    v, f = P.sphere_mesh()
    with pytest.raises(ValueError, match="topology"):
        posed.pose_transforms(dev(v), dev(v[:-1]), dev(f))
    with pytest.raises(ValueError, match="device of verts_src"):
        posed.pose_transforms(dev(v), torch.from_numpy(v), dev(f))
    with pytest.raises(ValueError, match="contiguous"):
        posed.pose_transforms(dev(v), dev(v), dev(f).long())
    cams = [B.cam_tar(c) for c in B.CAMERAS]
    with pytest.raises(ValueError, match="no source vertices"):
        posed.render_posed_volume(vol, dev(f), dev(v), cams, samples=4)
    import dataclasses
    with_verts = dataclasses.replace(vol, verts=dev(v))
    with pytest.raises(ValueError, match="accel"):
        posed.render_posed_volume(with_verts, dev(f), dev(v), cams, samples=4, accel=object())
    with pytest.raises(ValueError, match="samples"):
        posed.render_posed_volume(with_verts, dev(f), dev(v), cams, samples=0)
    o = posed.render_posed_volume(with_verts, dev(f), dev(v), cams, samples=4, x0=B.X0, y0=B.Y0, step=B.STEP, nx=B.NX, ny=B.NY)  # and the good call on a pixel grid
    assert o["color"].shape == (3, B.NX * B.NY, 3) and o["face"].shape == (3, B.NX * B.NY, 4)
