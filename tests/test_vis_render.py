"""render_vis (src/render_vis.py:181-226) on the GPU: vanerf_render_vis against an fp64 restatement of pytorch3d 0.7.5's semantics.

The restatement (`ref_render` below) follows DESIGN.md section 0b: PerspectiveCameras(in_ndc=False), rasterisation with blur_radius 0 and
faces_per_pixel 1, both windings drawn, perspective-correct barycentrics, SoftPhongShader with the default Materials and a point light at
(0, 0, -3), softmax_rgb_blend with sigma = gamma = 1e-4, then the reference's threshold.  pytorch3d itself is not a dependency: parity
against it is unpinned.  The CPU tests check the ABI's argument validation and the restatement on hand-made scenes; the GPU tests hold the
kernel to the restatement on the two-hand synthetic mesh."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from vanerf_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------------------
# fp64 restatement
# ------------------------------------------------------------------------------------------------------------------------------------
def _normalize(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-6)


def project(verts, R, T, focal, princpt, H, W):
    """-> view-space positions (NV,3), NDC (NV,2): u = px - fx Xv/Zv, x_ndc = (W - 2u) / min(H, W) (and y alike)."""
    Xv = verts @ R + T
    u = princpt[0] - focal[0] * Xv[:, 0] / Xv[:, 2]
    v = princpt[1] - focal[1] * Xv[:, 1] / Xv[:, 2]
    m = float(min(H, W))
    return Xv, np.stack([(W - 2.0 * u) / m, (H - 2.0 * v) / m], 1)


def vertex_normals(verts, faces):
    """Meshes.verts_normals_packed: cross(v2 - v1, v0 - v1) summed into the three corners, normalised with eps 1e-6."""
    v0, v1, v2 = (verts[faces[:, k]] for k in range(3))
    nf = np.cross(v2 - v1, v0 - v1)
    n = np.zeros_like(verts)
    for k in range(3):
        np.add.at(n, faces[:, k], nf)
    return _normalize(n)


def pixel_centres(H, W):
    m = float(min(H, W))
    return (W - 2.0 * np.arange(W) - 1.0) / m, (H - 2.0 * np.arange(H) - 1.0) / m  # x per column, y per row


def face_bary(ndc, z, face, x, y):
    """Perspective-corrected barycentrics (..., 3) and depth of `face` at NDC points (x, y); nan where the face draws nothing there
    (zero area, zero denominator)."""
    a, b, c = (ndc[face[k]] for k in range(3))
    za, zb, zc = (z[face[k]] for k in range(3))
    area = (c[0] - a[0]) * (b[1] - a[1]) - (c[1] - a[1]) * (b[0] - a[0])
    if abs(area) <= 1e-8:
        nan = np.full(np.broadcast(x, y).shape, np.nan)
        return np.stack([nan, nan, nan], -1), nan
    w0 = ((x - b[0]) * (c[1] - b[1]) - (y - b[1]) * (c[0] - b[0])) / area
    w1 = ((x - c[0]) * (a[1] - c[1]) - (y - c[1]) * (a[0] - c[0])) / area
    w2 = ((x - a[0]) * (b[1] - a[1]) - (y - a[1]) * (b[0] - a[0])) / area
    t = np.stack([w0 * (zb * zc), w1 * (za * zc), w2 * (za * zb)], -1)
    den = t.sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        bary = np.where(den != 0.0, t / den, np.nan)
    pz = bary[..., 0] * za + bary[..., 1] * zb + bary[..., 2] * zc
    return bary, pz


def _seg_dist2(px, py, a, b):
    d = b - a
    l2 = d @ d
    if l2 <= 1e-8:
        return (px - b[0]) ** 2 + (py - b[1]) ** 2
    t = np.clip((d[0] * (px - a[0]) + d[1] * (py - a[1])) / l2, 0.0, 1.0)
    return (px - (a[0] + t * d[0])) ** 2 + (py - (a[1] + t * d[1])) ** 2


def ref_render(verts, faces, vert_vis, R, T, focal, princpt, H, W):
    """fp64 render_vis -> dict(rgb (3,H,W), vis (H,W), pix_to_face (H,W), zbuf (H,W), bary (H,W,3), normals (NV,3), mean255 (H,W))."""
    verts, R, T, focal, princpt = (np.asarray(a, np.float64) for a in (verts, R, T, focal, princpt))
    faces = np.asarray(faces, np.int64)
    tex = np.asarray(vert_vis, np.float64).reshape(-1)
    Xv, ndc = project(verts, R, T, focal, princpt, H, W)
    z = Xv[:, 2]
    normals = vertex_normals(verts, faces)
    xs, ys = pixel_centres(H, W)
    m = float(min(H, W))
    zbuf = np.full((H, W), np.inf)
    p2f = np.full((H, W), -1, np.int64)
    bary = np.zeros((H, W, 3))
    for f in range(faces.shape[0]):
        fz = z[faces[f]]
        fx, fy = ndc[faces[f], 0], ndc[faces[f], 1]
        if np.all(fz > 0):  # the covered pixel centres lie in the face's box: test only those
            c_lo = max(int(np.floor((W - 1 - m * fx.max()) / 2.0)) - 1, 0)
            c_hi = min(int(np.ceil((W - 1 - m * fx.min()) / 2.0)) + 1, W - 1)
            r_lo = max(int(np.floor((H - 1 - m * fy.max()) / 2.0)) - 1, 0)
            r_hi = min(int(np.ceil((H - 1 - m * fy.min()) / 2.0)) + 1, H - 1)
            if c_lo > c_hi or r_lo > r_hi:
                continue
        else:
            c_lo, c_hi, r_lo, r_hi = 0, W - 1, 0, H - 1
        X, Y = np.meshgrid(xs[c_lo:c_hi + 1], ys[r_lo:r_hi + 1])
        b, pz = face_bary(ndc, z, faces[f], X, Y)
        with np.errstate(invalid="ignore"):
            cov = (pz >= 0) & np.all(b > 0, -1)
            zb = zbuf[r_lo:r_hi + 1, c_lo:c_hi + 1]
            win = cov & (pz < zb)  # ascending face order: the lower index keeps a tie
        zb[win] = pz[win]
        p2f[r_lo:r_hi + 1, c_lo:c_hi + 1][win] = f
        bary[r_lo:r_hi + 1, c_lo:c_hi + 1][win] = b[win]
    rgb = np.ones((3, H, W))
    C = -T @ R.T
    rr, cc = np.nonzero(p2f >= 0)
    for r, c in zip(rr, cc):
        fc = faces[p2f[r, c]]
        bw = bary[r, c]
        t = bw @ tex[fc]
        p = bw @ verts[fc]
        n = _normalize(bw @ normals[fc])
        lt = _normalize(np.array([0.0, 0.0, -3.0]) - p)
        e = _normalize(C - p)
        nl = n @ lt
        diffuse = 0.3 * max(nl, 0.0)
        spec = 0.2 * (max(e @ (2.0 * nl * n - lt), 0.0) * (nl > 0)) ** 64
        col = (0.5 + diffuse) * t + spec
        d2 = min(_seg_dist2(xs[c], ys[r], ndc[fc[k]], ndc[fc[(k + 1) % 3]]) for k in range(3))
        prob = 1.0 / (1.0 + np.exp(-d2 / 1e-4))
        z_inv = (100.0 - zbuf[r, c]) / 99.0
        z_inv_max = max(z_inv, 1e-10)
        wnum = prob * np.exp((z_inv - z_inv_max) / 1e-4)
        delta = max(np.exp((1e-10 - z_inv_max) / 1e-4), 1e-10)
        rgb[:, r, c] = (wnum * col + delta) / (wnum + delta)
    mean255 = (rgb * 255.0).mean(0)
    zbuf[p2f < 0] = -1.0
    return {"rgb": rgb, "vis": (mean255 >= 50.0).astype(np.float64), "pix_to_face": p2f, "zbuf": zbuf, "bary": bary, "normals": normals,
            "mean255": mean255, "ndc": ndc, "z": z}


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the ABI and the restatement
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ffi():
    from vanerf_amd import build
    build.build()
    from vanerf_amd import _ffi
    return _ffi


def test_render_vis_is_declared_and_exported(ffi):
    hdr = open(os.path.join(REPO, "include", "vanerf_hip.h")).read()
    assert re.search(r"\bint\s+vanerf_render_vis\s*\(", hdr)
    assert "vanerf_render_vis" in ffi.EXPORTS
    assert hasattr(ffi.lib, "vanerf_render_vis")
    assert ffi.lib.vanerf_abi_version() == 12


def test_render_vis_rejects_bad_arguments_without_a_gpu(ffi):
    p = ctypes.c_void_p(256)  # never dereferenced: validation comes first
    args = dict(verts=p, nv=4, faces=p, nf=2, vert_vis=p, R=p, T=p, focal=p, princpt=p, H=8, W=8, scratch=p, scratch_bytes=4 * 16 * 4, rgb=p, vis=p,
                p2f=None, zbuf=None, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return ffi.lib.vanerf_render_vis(*a.values()), ffi.lib.vanerf_last_error().decode()

    for k in ("verts", "faces", "vert_vis", "R", "T", "focal", "princpt", "scratch", "rgb", "vis"):
        rc, msg = call(**{k: None})
        assert rc == -22 and "null" in msg, k
    for kw, word in (({"nv": 0}, "nv=0"), ({"nf": -1}, "nf=-1"), ({"H": 0}, "H=0"), ({"W": 5000}, "W=5000"), ({"scratch_bytes": 255}, "scratch"),
                     ({"scratch": ctypes.c_void_p(260)}, "aligned")):
        rc, msg = call(**kw)
        assert rc == -22 and word in msg, (kw, msg)


def _one_face_scene(H=32, W=32, zs=(2.0, 2.0, 2.0)):
    # view space == world space (R = I, T = 0); screen vertices away from every pixel centre
    focal, princpt = np.array([40.0, 40.0]), np.array([W / 2.0, H / 2.0])
    uv = np.array([[5.3, 4.7], [26.1, 9.2], [12.6, 27.9]])
    z = np.asarray(zs, np.float64)
    X = (princpt[0] - uv[:, 0]) * z / focal[0]
    Y = (princpt[1] - uv[:, 1]) * z / focal[1]
    verts = np.stack([X, Y, z], 1)
    return verts, uv, np.eye(3), np.zeros(3), focal, princpt, H, W


def _inside_screen(uv, H, W):
    """Pixel centres (c + 0.5, r + 0.5) strictly inside the screen triangle uv (either winding)."""
    cc, rr = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    e = [(uv[(k + 1) % 3, 0] - uv[k, 0]) * (rr - uv[k, 1]) - (uv[(k + 1) % 3, 1] - uv[k, 1]) * (cc - uv[k, 0]) for k in range(3)]
    return (e[0] > 0) & (e[1] > 0) & (e[2] > 0) | (e[0] < 0) & (e[1] < 0) & (e[2] < 0)


def test_restatement_one_face_covers_the_expected_pixel_centres_in_either_winding():
    verts, uv, R, T, focal, princpt, H, W = _one_face_scene()
    expect = _inside_screen(uv, H, W)
    assert 50 < expect.sum() < H * W - 50
    a = ref_render(verts, np.array([[0, 1, 2]]), np.ones(3), R, T, focal, princpt, H, W)
    assert np.array_equal(a["pix_to_face"] >= 0, expect)
    assert np.allclose(a["zbuf"][expect], 2.0) and np.all(a["zbuf"][~expect] == -1.0)
    b = ref_render(verts, np.array([[0, 2, 1]]), np.ones(3), R, T, focal, princpt, H, W)
    assert np.array_equal(a["pix_to_face"], b["pix_to_face"]) and np.allclose(a["zbuf"], b["zbuf"], rtol=0.0, atol=1e-12)
    # visible texels give a lit face (>= 0.5 on every channel: vis 1), the background is white
    assert np.all(a["rgb"][:, expect] >= 0.5) and np.all(a["vis"][expect] == 1.0)


def test_restatement_nearer_face_wins_in_either_order():
    verts, uv, R, T, focal, princpt, H, W = _one_face_scene()
    far = verts * 1.5  # same screen triangle, 1.5x the depth
    V = np.concatenate([verts, far], 0)
    for faces, near_id in ((np.array([[0, 1, 2], [3, 4, 5]]), 0), (np.array([[3, 4, 5], [0, 1, 2]]), 1)):
        o = ref_render(V, faces, np.ones(6), R, T, focal, princpt, H, W)
        cov = o["pix_to_face"] >= 0
        assert np.array_equal(cov, _inside_screen(uv, H, W)) and np.all(o["pix_to_face"][cov] == near_id)
        assert np.allclose(o["zbuf"][cov], 2.0)


def test_restatement_faces_behind_the_camera_or_of_zero_area_draw_nothing():
    verts, uv, R, T, focal, princpt, H, W = _one_face_scene()
    behind = verts * np.array([1.0, 1.0, -1.0])
    o = ref_render(behind, np.array([[0, 1, 2]]), np.ones(3), R, T, focal, princpt, H, W)
    assert np.all(o["pix_to_face"] == -1)
    flat = verts.copy()
    flat[2] = 0.5 * (flat[0] + flat[1])  # collinear: zero area
    o = ref_render(flat, np.array([[0, 1, 2]]), np.ones(3), R, T, focal, princpt, H, W)
    assert np.all(o["pix_to_face"] == -1)
    # the background: rgb 1 on every channel, vis 1
    assert np.all(o["rgb"] == 1.0) and np.all(o["vis"] == 1.0)


def test_restatement_invisible_texels_fall_below_the_threshold():
    verts, uv, R, T, focal, princpt, H, W = _one_face_scene()
    o = ref_render(verts, np.array([[0, 1, 2]]), np.zeros(3), R, T, focal, princpt, H, W)
    cov = o["pix_to_face"] >= 0
    assert cov.any() and np.all(o["vis"][cov] == 0.0) and np.all(o["vis"][~cov] == 1.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the restatement
# ------------------------------------------------------------------------------------------------------------------------------------
CASES = [(0, 8.0, 256, 256), (1, -25.0, 256, 256), (2, 40.0, 256, 256), (3, 15.0, 200, 256)]


def _scene(seed, orbit, H, W):
    """Two-hand mesh, its vertex visibility from the source view (FrameData, as the model computes it), the target camera in pytorch3d's
    convention (synth.p3d_tar_cam) for an H x W target."""
    from vanerf_amd import renderer
    frame = synth.make_frame(seed=seed, tar_h=H, tar_w=W, orbit_deg=orbit)
    fd = synth.to_device(frame, "cuda")
    sd = {k: v.cuda() for k, v in synth.make_texframe_weights().items()}
    fdat = renderer.FrameData(sd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
    cam = synth.p3d_tar_cam(frame["cam_tar"])
    return frame, fdat, cam


def _gpu_render(fdat, cam, H, W):
    """vanerf_render_vis through the C ABI -> rgb, vis, pix_to_face, zbuf, scratch (all on the host)."""
    from vanerf_amd import _ffi
    f32 = torch.float32
    nv, nf = fdat.verts3.shape[0], fdat.faces.shape[0]
    Rm, T = cam["tar_R"][0].cuda().contiguous(), cam["tar_T"][0].cuda().contiguous()
    focal, pp = cam["tar_focal"][0].cuda().contiguous(), cam["tar_princpt"][0].cuda().contiguous()
    scratch = torch.full((nv, 16), float("nan"), device="cuda")
    rgb = torch.empty(3, H, W, device="cuda")
    vis = torch.empty(H, W, device="cuda")
    p2f = torch.empty(H, W, dtype=torch.int32, device="cuda")
    zb = torch.empty(H, W, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _ffi.check(_ffi.lib.vanerf_render_vis(ptr(fdat.verts3), nv, ptr(fdat.faces), nf, ptr(fdat.vert_vis), ptr(Rm), ptr(T), ptr(focal), ptr(pp), H, W,
                                          ptr(scratch), scratch.numel() * 4, ptr(rgb), ptr(vis), ptr(p2f), ptr(zb),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert all(t.dtype == f32 for t in (rgb, vis, zb))
    return rgb.cpu(), vis.cpu(), p2f.cpu(), zb.cpu(), scratch.cpu()


def _inputs(fdat, cam):
    return (fdat.verts3.cpu().double().numpy(), fdat.faces.cpu().long().numpy(), fdat.vert_vis.cpu().double().numpy(),
            cam["tar_R"][0].double().numpy(), cam["tar_T"][0].double().numpy(), cam["tar_focal"][0].double().numpy(),
            cam["tar_princpt"][0].double().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("seed,orbit,H,W", CASES)
def test_kernel_matches_the_fp64_restatement(seed, orbit, H, W):
    frame, fdat, cam = _scene(seed, orbit, H, W)
    rgb, vis, p2f, zb, scratch = _gpu_render(fdat, cam, H, W)
    V, F, tex, Rm, T, focal, pp = _inputs(fdat, cam)
    ref = ref_render(V, F, tex, Rm, T, focal, pp, H, W)
    g = p2f.numpy().astype(np.int64)
    r = ref["pix_to_face"]
    xs, ys = pixel_centres(H, W)

    def at(face, row, col):  # fp64 smallest barycentric and depth of `face` at the pixel centre
        if face < 0:
            return np.inf, np.nan
        b, pz = face_bary(ref["ndc"], ref["z"], F[face], np.float64(xs[col]), np.float64(ys[row]))
        return np.min(b), pz

    diff = np.argwhere(g != r)
    ties = np.zeros((H, W), bool)
    for row, col in diff:
        bg, zg = at(g[row, col], row, col)
        br, zr = at(r[row, col], row, col)
        near_edge = abs(bg) < 1e-5 or abs(br) < 1e-5
        near_depth = np.isfinite(zg) and np.isfinite(zr) and abs(zg - zr) < 1e-6 * abs(zr)
        assert near_edge or near_depth, (row, col, g[row, col], r[row, col], bg, br, zg, zr)
        ties[row, col] = True
    same = g == r
    covered = same & (r >= 0)
    rgb_err = np.abs(rgb.numpy() - ref["rgb"])[:, same].max()
    z_err = np.abs(zb.numpy()[covered] - ref["zbuf"][covered]).max()
    vis_diff = vis.numpy() != ref["vis"]
    vis_ok = ties | (np.abs(ref["mean255"] - 50.0) < 1e-3)
    print(f"seed {seed} orbit {orbit} {H}x{W}: {covered.sum()} covered pixels, {len(diff)} pix_to_face near-ties, max |rgb - fp64| = {rgb_err:.2e}, "
          f"max |zbuf - fp64| = {z_err:.2e}, {vis_diff.sum()} vis differences ({(vis_diff & ~ties).sum()} off the ties)")
    assert covered.sum() > 0.02 * H * W
    assert len(diff) <= 0.002 * H * W
    assert rgb_err <= 2e-5
    assert z_err <= 1e-5 * np.abs(ref["zbuf"][covered]).max()
    assert not np.any(vis_diff & ~vis_ok)
    # background: rgb 1, vis 1, zbuf -1
    bg = (g < 0) & same
    assert np.all(rgb.numpy()[:, bg] == 1.0) and np.all(vis.numpy()[bg] == 1.0) and np.all(zb.numpy()[bg] == -1.0)


@pytest.mark.gpu
def test_vertex_normals_match_fp64():
    frame, fdat, cam = _scene(1, -25.0, 256, 256)
    *_, scratch = _gpu_render(fdat, cam, 256, 256)
    V, F = fdat.verts3.cpu().double().numpy(), fdat.faces.cpu().long().numpy()
    vt = torch.from_numpy(V)
    nf = torch.cross(vt[F[:, 2]] - vt[F[:, 1]], vt[F[:, 0]] - vt[F[:, 1]], dim=1)
    n = torch.zeros_like(vt)
    for k in range(3):
        n.index_add_(0, torch.from_numpy(F[:, k]), nf)
    n = torch.nn.functional.normalize(n, dim=1, eps=1e-6)
    err = (scratch[:, 12:15].double() - n).abs().max().item()
    print(f"max |vertex normal - fp64| = {err:.2e}")
    assert err <= 1e-6
    # the world positions and the texel are stored as given
    assert torch.equal(scratch[:, 8:11], fdat.verts3.cpu()) and torch.equal(scratch[:, 7], fdat.vert_vis.cpu())


@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    frame, fdat, cam = _scene(2, 40.0, 256, 256)
    a = _gpu_render(fdat, cam, 256, 256)
    b = _gpu_render(fdat, cam, 256, 256)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,orbit,H,W", [(0, 8.0, 256, 256), (3, 15.0, 200, 256)])
def test_silhouette_registers_with_the_target_camera(seed, orbit, H, W):
    frame, fdat, cam = _scene(seed, orbit, H, W)
    _, vis, p2f, _, _ = _gpu_render(fdat, cam, H, W)
    KRT = frame["cam_tar"]["KRT"][0, :3].double()
    p = fdat.verts3.cpu().double() @ KRT[:, :3].T + KRT[:, 3]
    uv = p[:, :2] / p[:, 2:3]
    rows, cols = torch.nonzero(p2f >= 0, as_tuple=True)
    box = [cols.min().item() + 0.5, cols.max().item() + 0.5, rows.min().item() + 0.5, rows.max().item() + 0.5]
    proj = [uv[:, 0].min().item(), uv[:, 0].max().item(), uv[:, 1].min().item(), uv[:, 1].max().item()]
    proj = [min(max(x, 0.5), lim - 0.5) for x, lim in zip(proj, (W, W, H, H))]  # clipped to the pixel centres of the image
    print(f"silhouette box {box}, projected-vertex box {proj}")
    assert all(abs(a - b) <= 1.0 for a, b in zip(box, proj)), (box, proj)
    # not trivial: inside the silhouette the visibility image holds both values (the synthetic frame has visible and hidden vertices)
    inside = vis[p2f >= 0]
    assert 0.0 < fdat.vert_vis.mean().item() < 1.0
    assert (inside == 0.0).any() and (inside == 1.0).any()


def _model(on):
    from vanerf_amd.config import default_config
    from vanerf_amd.model import VANeRF
    torch.manual_seed(0)
    cfg = default_config()
    cfg["models"]["VANeRF"].update(train_out_h=8, train_out_w=8, render_vis=on)
    cfg["models"]["VANeRF"]["dr_kwargs"].update(sample_per_ray_c=8, sample_per_ray_f=8, rand_noise_std=0.0, uniform=False, fine=True)
    net = VANeRF(cfg).cuda()
    net.load_state_dict(synth.make_full_weights(0), strict=False)
    return net


def _model_frame():
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64, orbit_deg=12.0)
    frame["targets"]["tar_cam"] = synth.p3d_tar_cam(frame["cam_tar"])
    return synth.to_device(frame, "cuda")


def _batch_render(net, f):
    # level 3 on a 64x64 target: 16x16 rays at stride 4, offset (x 1, y 2)
    return net.batch_render_pifu_nerf(net, f["img_in"], f["cam_in"], f["hand_type"], f["targets"], 1, f["cam_tar"], 3,
                                      torch.tensor([[1, 2]]), None, f["feat_geo"], f["feat_tex"], None, dict(f["sp_data"]), None, fine=True,
                                      uniform=True, sample_per_ray_c=8, sample_per_ray_f=8, src_foreground_mask=f["src_foreground_mask"],
                                      bounds=f["bounds"])


@pytest.mark.gpu
def test_model_switch_fills_vis_img_with_render_vis():
    from vanerf_amd.render_vis import render_vis
    net = _model(True).eval()
    assert net.render_vis is True
    f = _model_frame()
    with torch.no_grad():
        out = _batch_render(net, f)
    tc = f["targets"]["tar_cam"]
    _, vis_all = render_vis(f["targets"]["vert_world"], f["targets"]["face_world"].long(), out["vert_vis"], tc["tar_R"], tc["tar_T"],
                            tc["tar_focal"][:, 0], tc["tar_focal"][:, 1], tc["tar_princpt"][:, 0], tc["tar_princpt"][:, 1])
    assert out["vis_img_all"].shape == (1, 1, 256, 256)
    assert torch.equal(out["vis_img_all"], vis_all)
    assert (vis_all == 0.0).any() and (vis_all == 1.0).any()
    ys, xs = torch.meshgrid(torch.arange(16) * 4 + 2, torch.arange(16) * 4 + 1, indexing="ij")
    index = (ys * 64 + xs).reshape(-1).cuda()
    assert out["vis_img"].shape == (1, 1, 16, 16)
    assert torch.equal(out["vis_img"].reshape(-1), vis_all.reshape(-1)[index])
    # switched off on the same module: zeros, as before
    net.render_vis = False
    with torch.no_grad():
        off = _batch_render(net, f)
    assert torch.equal(off["vis_img_all"], torch.zeros(1, 1, 256, 256, device="cuda"))
    assert torch.equal(off["vis_img"], torch.zeros(1, 1, 16, 16, device="cuda"))


@pytest.mark.gpu
def test_model_default_is_off_and_training_forward_runs_with_the_switch_on():
    assert _model(False).render_vis is False
    net = _model(True).train()
    f = _model_frame()
    dr = {"img": f["img_in"], "cam": f["cam_in"], "cam_tar": f["cam_tar"], "tar": torch.rand(1, 3, 64, 64, device="cuda"),
          "msk": torch.ones(1, 1, 64, 64, device="cuda")}
    res = net(f["img_in"], f["cam_in"], f["hand_type"], f["targets"], None, None, n_views=1, sp_data=dict(f["sp_data"]), dr_data=dr,
              src_foreground_mask=f["src_foreground_mask"], bounds=f["bounds"])
    out = res["out"]["nerf"]
    assert torch.isfinite(res["loss"]).all()
    res["loss"].backward()
    assert out["vis_img_all"].shape == (1, 1, 256, 256) and out["vis_img"].shape == (1, 1, 8, 8)
    assert (out["vis_img_all"] == 0.0).any() and (out["vis_img_all"] == 1.0).any()
