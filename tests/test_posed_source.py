"""The HIP path under posed, off-centre SOURCE cameras.  Needs a real MI355X: `pytest -m gpu`.

Everywhere else the source camera is make_frame's: identity extrinsic, principal point at the image centre, fx == fy.  There VanerfFrame.extrin
holds R == R^T and t == 0, KRT[3] = KRT[7] = KRT[11] = 0, kpt_cam == kpt3d and x / y are interchangeable, so a transposed rotation, a dropped
translation, a row / column mix-up of the kernel's camera-space transform or an x / y swap in a projection passes every other test.  Here the
per-frame tables, the per-sample forward kernels (fp32, bf16x3, hoisted bf16x3), the validity partition, whole passes, the module interface
and the fused backward run on the two poses of synth.SOURCE_POSES (tests/test_oracle_posed.py has the table) against the oracle in fp64
-- same discrete inputs on both sides, bars as in the tests each part is modelled on -- and against the reference's own numbers on pose A
(tests/golden/query_posed.npz, pass_16x16_s16_posed.npz).  tests/test_oracle_posed.py proves the pose is visible in that reference."""
import pytest
import torch

from oracle import vanerf_oracle as orc
from tests.conftest import assert_close_frac
from tests.test_backward_per_sample import VARIANTS, check_block_against_fp64
from tests.test_hip_injected import COARSE, FINE, _compare, _inject
from tests.test_hip_parity import R, _frame_data, dev, net, sd_full  # noqa: F401  (R, sd_full, net: that module's fixtures)
from tests.test_oracle_fp64 import cast, reference
from tests.test_oracle_posed import N_POINTS, POSES, border_band_points, decision_margins, mesh_queries, near_mesh_points, posed_frame
from vanerf_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4
KERNELS = {"fp32": ("fp32", None), "bf16x3": ("bf16x3", None), "bf16x3_hoisted": ("bf16x3", "auto")}  # name -> (weights mode, vertex_products)
_CASES = {}


def _case(R, sd, pose):
    """Per pose, built once: the frame, its FrameData, N_POINTS points near the mesh (off-image and on-vertex ones among them), the oracle's
    q_sdf / q_vis, the device's 1-NN, and the fp64 oracle's per-sample pass with the DEVICE's vert_vis (so that a visibility mismatch fails in
    test_per_frame_tables and nowhere else)."""
    if pose not in _CASES:
        frame = posed_frame(pose, dict(POSES)[pose])
        fdat = _frame_data(R, sd, frame)
        pts = near_mesh_points(frame, N_POINTS, seed=2)
        q_sdf, q_vis, vert_vis = mesh_queries(frame, pts)
        knn = R.knn1(fdat.verts4, dev(pts))
        r64 = reference(sd, frame, pts, q_sdf, q_vis, fdat.vert_vis.cpu())
        sd64 = cast(sd, torch.float64)
        want = orc.eval_func(sd64, r64["raw"][None], r64["valid"][None, :, None], frame["cam_in"]["nml_scale"])[0]
        _CASES[pose] = dict(frame=frame, fdat=fdat, pts=pts, q_sdf=q_sdf, q_vis=q_vis, vert_vis=vert_vis, knn=knn, r64=r64, want=want)
    return _CASES[pose]


def _run_kernel(R, sd, c, kernel, pts=None, q_sdf=None, q_vis=None, knn=None):
    mode, vp = KERNELS[kernel]
    w = R.PackedWeights(sd, mode=mode)
    pts = c["pts"] if pts is None else pts
    q_sdf, q_vis = (c["q_sdf"], c["q_vis"]) if q_sdf is None else (q_sdf, q_vis)
    knn = c["knn"] if knn is None else knn
    got, valid = R.query_samples(w, c["fdat"], dev(pts), dev(q_sdf.contiguous()), dev(q_vis.to(torch.uint8).contiguous()), knn, want_valid=True,
                                 vertex_products=vp)
    if vp is not None:
        assert c["fdat"].vertex_products(w) is not None  # the hoisted kernel really ran
    return got.cpu(), valid.cpu().bool()


def _within_the_bar(got, want, what, beta=0.1, tol=TOL, sigma_tol=None):
    """All five outputs [alpha, sdf, r, g, b] within `tol` (a number, or one per output) of the fp64 reference, and sigma within `sigma_tol`
    (default: tol) relative to its scale 1 / beta, beta the handle's clamped sigmoid_beta
    (tests/test_hip_parity.py::test_query_samples_vs_oracle has the reasoning)."""
    err = (got.double() - want).abs()
    sig = (torch.sigmoid(-got[:, 0].double() / beta) / beta - torch.sigmoid(-want[:, 0] / beta) / beta).abs().max().item()
    print(f"{what}: max |HIP - fp64| [alpha, sdf, r, g, b] = {[f'{e:.2e}' for e in err.max(0)[0].tolist()]}, sigma {sig:.2e} (scale 1/beta = {1.0 / beta:g})")
    assert (err.max(0)[0] <= torch.as_tensor(tol, dtype=torch.float64)).all(), (what, err.max(0)[0].tolist())
    assert sig * beta <= (tol if sigma_tol is None else sigma_tol), (what, sig)


# ---------------------------------------------------------------------------------------------------------------------
# a. per-frame tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", [p for p, _ in POSES])
def test_per_frame_tables(R, sd_full, pose):
    """FrameData's host-side tables on a posed camera.  vert_xy01 / vert_z01 / kpt_cam against the fp64 projection within 1e-6 (values <= 1
    behind fewer than eight fp32 roundings of <= 1.2e-7 each); the three per-vertex feature tables against the fp64 oracle's feat_sample x
    vert_vis within 1e-4; vert_vis EQUAL to the oracle's (it does not move under +-1 ulp of the projected vertices on these poses)."""
    c = _case(R, sd_full, pose)
    frame, fdat = c["frame"], c["fdat"]
    f64 = cast(frame, torch.float64)
    verts = f64["targets"]["vert_world"]
    xy01, z01 = orc.source_vert_xyz01(verts, f64["cam_in"])
    ext = f64["sp_data"]["extrin"]
    kpt_cam = f64["sp_data"]["kpt3d"] @ ext[:, :3, :3].transpose(1, 2) + ext[:, :3, 3][:, None]
    e_xy = (fdat.vert_xy01.cpu().double() - xy01[0]).abs().max().item()
    e_z = (fdat.vert_z01.cpu().double() - z01[0, :, 0]).abs().max().item()
    e_k = (fdat.kpt_cam.cpu().double()[:, :3] - kpt_cam[0]).abs().max().item()
    assert 0.0 < xy01.min() and xy01.max() < 1.0 and 0.3 < z01.min() and z01.max() < 0.7  # the mesh is inside the posed view
    assert (kpt_cam[0] - f64["sp_data"]["kpt3d"][0]).abs().max() > 1e-2  # the identity camera's kpt_cam is kpt3d: 1e4 bars away from it here
    assert torch.equal(fdat.kpt_cam.cpu()[:, 3], torch.zeros(42))
    same_vis = torch.equal(fdat.vert_vis.cpu(), c["vert_vis"])
    vis = c["vert_vis"].double()[None, :, None]
    vxy = orc.project_verts(verts, f64["cam_in"])
    e_f = {"vfeat0": (fdat.vfeat0.cpu().double() - (orc.feat_sample(f64["feat_geo"][0], vxy) * vis)[0]).abs().max().item(),
           "vfeat1": (fdat.vfeat1.cpu().double() - (orc.feat_sample(f64["feat_geo"][1], vxy) * vis)[0]).abs().max().item()}
    sd64 = {k: v.double() for k, v in sd_full.items() if k.startswith("tex_vis_fusion.")}
    vt = orc.tex_vertex_features(sd64, vxy, f64["feat_tex"], f64["img_in"]) * vis
    e_f["vfeat_tex"] = (fdat.vfeat_tex.cpu().double()[:, :29] - vt[0]).abs().max().item()
    print(f"pose {pose}: |vert_xy01| {e_xy:.2e} |vert_z01| {e_z:.2e} |kpt_cam| {e_k:.2e}; vertex features {e_f}; vert_vis equal {same_vis} "
          f"(mean {c['vert_vis'].mean().item():.3f})")
    assert e_xy <= 1e-6 and e_z <= 1e-6 and e_k <= 1e-6
    assert same_vis, f"{int((fdat.vert_vis.cpu() != c['vert_vis']).sum())} vertices differ in visibility"
    assert 0.2 < c["vert_vis"].mean() < 0.8
    assert max(e_f.values()) <= TOL
    assert torch.equal(fdat.vfeat_tex.cpu()[:, 29:], torch.zeros(1558, 3))


# ---------------------------------------------------------------------------------------------------------------------
# b. per-sample forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("pose", [p for p, _ in POSES])
def test_query_samples_on_posed_cameras(R, sd_full, pose, kernel):
    """vanerf_query_samples (fp32, bf16x3) and its hoisted form with vertex_products (bf16x3) against the fp64 oracle.  First the inputs are
    proved safe: in fp64 no point lies within 1e-5 of a validity decision (|x|, |y| <= 1.01, z >= -1, fg > 0.1), so none is excluded and the
    validity flags must be equal."""
    c = _case(R, sd_full, pose)
    margin = decision_margins(c["frame"], c["pts"])[0]
    assert margin.min() > 1e-5, margin.min().item()
    got, valid = _run_kernel(R, sd_full, c, kernel)
    want_valid = c["r64"]["valid"]
    assert torch.equal(c["knn"].cpu().long(), orc.knn1(c["pts"], c["frame"]["targets"]["vert_world"][0]))  # 1-NN index: bit-exact
    assert torch.equal(valid, want_valid), f"{int((valid != want_valid).sum())} validity flags differ"
    assert 0.05 < want_valid.float().mean() < 0.95
    _within_the_bar(got, c["want"], f"pose {pose} [{kernel}] valid {want_valid.float().mean().item():.3f}")


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_query_samples_vs_posed_reference_golden(R, sd_full, golden, kernel):
    """The same points against the reference's own VANeRF.query on pose A (tests/golden/query_posed.npz)."""
    g = golden("query_posed")
    c = _case(R, sd_full, "A")
    assert torch.equal(c["pts"], g["pts"][0]) and torch.equal(c["q_sdf"], g["q_sdf"][0]) and torch.equal(c["q_vis"], g["q_vis"][0, :, 0])
    got, valid = _run_kernel(R, sd_full, c, kernel)
    want = orc.eval_func(sd_full, g["out"], g["valid"], 100.0)[0]
    assert torch.equal(valid, g["valid"][0, :, 0])
    _within_the_bar(got, want.double(), f"pose A [{kernel}] vs reference golden")


# ---------------------------------------------------------------------------------------------------------------------
# c. border band
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_border_band(R, sd_full, kernel):
    """32 points un-projected through the fp64 pose-A camera to x or y in (1.0, 1.01) and (-1.01, -1.0): beyond the last pixel centre, inside
    the validity test's eps band, where the foreground mask and every feature map are sampled with border clamping.  All valid (whole source
    view in the foreground), all within the bar."""
    if "band" not in _CASES:
        frame = posed_frame("A", 3, half=False)
        fdat = _frame_data(R, sd_full, frame)
        pts = border_band_points(frame)
        q_sdf, q_vis, _ = mesh_queries(frame, pts)
        r64 = reference(sd_full, frame, pts, q_sdf, q_vis, fdat.vert_vis.cpu())
        want = orc.eval_func(cast(sd_full, torch.float64), r64["raw"][None], r64["valid"][None, :, None], 100.0)[0]
        _CASES["band"] = dict(frame=frame, fdat=fdat, pts=pts, q_sdf=q_sdf, q_vis=q_vis, knn=R.knn1(fdat.verts4, dev(pts)), r64=r64, want=want)
    c = _CASES["band"]
    margin, xy, z, fg = decision_margins(c["frame"], c["pts"])
    big = xy.abs().max(-1)[0]
    assert margin.min() > 1e-5 and ((big > 1.0 + 1e-5) & (big < 1.01 - 1e-5)).all() and (z.abs() < 0.5).all()
    assert c["r64"]["valid"].all()
    got, valid = _run_kernel(R, sd_full, c, kernel)
    assert torch.equal(c["knn"].cpu().long(), orc.knn1(c["pts"], c["frame"]["targets"]["vert_world"][0]))
    assert torch.equal(valid, c["r64"]["valid"])
    _within_the_bar(got, c["want"], f"border band [{kernel}]")


# ---------------------------------------------------------------------------------------------------------------------
# d. validity partition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("pose", [p for p, _ in POSES])
def test_validity_partition_on_posed_cameras(R, sd_full, pose, precision):
    """vanerf_query_order projects with the posed KRT on its own: a permutation, the valid samples first and then the others, each group in
    its order; vanerf_query_samples gives the same bits with and without it.  Samples on real rays of the target view."""
    c = _case(R, sd_full, pose)
    frame, fdat = c["frame"], c["fdat"]
    w = R.PackedWeights(sd_full, mode=precision)
    rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 0, 0, 1, 64, 64, 24, device="cuda")
    pts_all = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"])
    for n in (24 * 1000 + 7, 33, 1):
        pts = pts_all[24 * 1200: 24 * 1200 + n].contiguous()
        q_sdf, q_vis, knn = R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts)
        ref, valid = R.query_samples(w, fdat, pts, q_sdf, q_vis, knn, want_valid=True)
        order = R.query_order(fdat, pts)
        o = order.long().cpu()
        assert torch.equal(torch.sort(o)[0], torch.arange(n))
        v = valid.bool().cpu()
        nv = int(v.sum())
        assert v[o[:nv]].all() and not v[o[nv:]].any()
        assert (o[:nv][1:] > o[:nv][:-1]).all() and (o[nv:][1:] > o[nv:][:-1]).all()  # stable
        got, valid2 = R.query_samples(w, fdat, pts, q_sdf, q_vis, knn, want_valid=True, order=order)
        assert torch.equal(got, ref) and torch.equal(valid2, valid)
        if n > 10000:
            assert 0.05 < v.float().mean() < 0.95
            # and the flags are the fp64 decisions wherever fp64 puts the point clear of every one of them
            margin, xy, z, fg = decision_margins(frame, pts.cpu())
            want = (xy.abs() <= 1.01).all(-1) & (z >= -1.0) & (fg > 0.1)
            clear = margin > 1e-5
            assert clear.float().mean() > 0.99 and torch.equal(v[clear], want[clear])


# ---------------------------------------------------------------------------------------------------------------------
# e. whole pass with injected rays
# ---------------------------------------------------------------------------------------------------------------------
def _images_fp64(sd, frame, ref):
    """The seven images of the oracle's pass `ref` with the per-sample networks and the composite in fp64 at the SAME (fp32) sample
    positions, depths and mesh queries: {tex_fg, depth, alpha, tex_fg_fine, depth_fine, alpha_fine, sdf} shaped as batch_render's."""
    sd64 = cast(sd, torch.float64)
    n_y, n_x = ref["depth"].shape[-2:]
    out = {}
    for part, z, suffix in ((ref["coarse"], ref["z"], ""), (ref["fine"], ref["z_fine"], "_fine")):
        S = z.shape[-1]
        pts = part["pts"][0]
        r = reference(sd, frame, pts, part["q_sdf"].reshape(-1), part["q_vis"].reshape(-1), part["vert_vis"].reshape(-1))
        rgba = orc.eval_func(sd64, r["raw"][None], r["valid"][None, :, None], frame["cam_in"]["nml_scale"]).view(1, -1, S, 5)
        color, depth, alpha, _, sdf = orc.rgba2out(sd64, rgba, z.double(), part["q_sdf"].double().view(1, -1, S, 1))
        out["tex_fg" + suffix] = color.view(1, n_y, n_x, 3).permute(0, 3, 1, 2)
        out["depth" + suffix], out["alpha" + suffix] = depth.view(1, n_y, n_x), alpha.view(1, n_y, n_x)
        if suffix:
            out["sdf"] = sdf.view(1, n_y, n_x)
    return out


@pytest.fixture(scope="module")
def posed_pass(sd_full):
    """The oracle's pass of pass_16x16_s16_posed.npz (pose A, 16 x 16 rays, 16 + 16 samples) and its fp64 images."""
    frame = posed_frame("A", 3)
    ref = orc.batch_render(sd_full, frame, 3, torch.tensor([[[1, 2]]]), 16, 16)
    return frame, ref, _images_fp64(sd_full, frame, ref)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_whole_pass_with_injected_rays(R, sd_full, golden, posed_pass, precision):
    """The oracle's rays and depths injected (renderer.render_pass(inject=...)): zero elements of the seven images above 1e-4 against the
    oracle evaluated in fp64, the coarse images also against the reference's own (the fine ones are behind importance_sample's u = 1.0
    tie there: allowance as in tests/test_hip_injected.py); and the same pass through the one-call C entry point gives render_pass's bits."""
    frame, ref, ref64 = posed_pass
    g = golden("pass_16x16_s16_posed")
    c = _case(R, sd_full, "A")
    assert c["frame"]["cam_in"]["KRT"].equal(frame["cam_in"]["KRT"])
    fdat = c["fdat"]
    w = R.PackedWeights(sd_full, mode=precision)
    out = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], 1, 2, 4, 16, 16, 16, 16, inject=_inject(ref))
    assert torch.equal(out["index"].cpu(), ref["index"][0])
    worst = _compare(out, ref64, 16, 16, TOL, f"posed pass [{precision}] vs fp64 oracle")
    worst32 = max((ref[k].double() - ref64[k]).abs().max().item() for k in ref64)
    worst_c = _compare(out, g, 16, 16, TOL, f"posed pass [{precision}] vs reference golden", COARSE)
    print(f"posed pass [{precision}] injected rays: max |HIP - fp64 oracle| = {worst:.3e} (fp32 oracle: {worst32:.3e}); max |HIP - reference| coarse = {worst_c:.3e}")
    for k, gk, ch in FINE:
        got = out[k].cpu().view(16, 16, 3).permute(2, 0, 1) if ch == 3 else out[k].cpu().view(16, 16)
        assert_close_frac(got, g[gk][0], TOL, 1e-3, gk)
    assert ref["depth_fine"].std() > 1e-3 and 0.05 < ref["coarse"]["rgba"][..., 0].gt(0).float().mean() < 0.95
    own = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], 1, 2, 4, 16, 16, 16, 16)
    one = R.render_pass_c(w, fdat, frame["cam_tar"], frame["bounds"], 1, 2, 4, 16, 16, 16, 16)
    for k in ("index", "hit", "z", "color", "depth", "alpha", "color_fine", "depth_fine", "alpha_fine", "sdf", "z_fine"):
        assert torch.equal(own[k], one[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# f. module interface
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_transf", [False, True])
def test_model_batch_render_on_a_posed_camera(net, sd_full, with_transf):
    """VANeRF.batch_render_pifu_nerf with the posed cam_in, plain and with the 2-D affine cam_in['transf'] folded into the (now full) KRT
    (VANeRF.fold_transf; the oracle applies it behind the projection), 16 x 16 rays, 16 + 16 samples, with the allowance of
    tests/test_hip_parity.py::test_model_cam_transf_is_folded_into_the_projection."""
    frame_cpu = synth.pose_source_camera(synth.make_frame(seed=3, tar_h=16, tar_w=16), **synth.SOURCE_POSES["A"])
    if with_transf:
        frame_cpu["cam_in"] = dict(frame_cpu["cam_in"], transf=torch.tensor([[[0.97, 0.02, 3.0], [-0.015, 1.03, -2.0]]]))
    f = synth.to_device(frame_cpu, "cuda")
    S = 16
    ref = orc.batch_render(sd_full, frame_cpu, 1, torch.tensor([[[0, 0]]]), S, S)
    if with_transf:
        plain = orc.batch_render(sd_full, dict(frame_cpu, cam_in={k: v for k, v in frame_cpu["cam_in"].items() if k != "transf"}), 1,
                                 torch.tensor([[[0, 0]]]), S, S)
        assert (ref["tex_fg_fine"] - plain["tex_fg_fine"]).abs().max() > 1e-2  # the affine matters
    out = net.batch_render_pifu_nerf(net, f["img_in"], f["cam_in"], f["hand_type"], f["targets"], 1, f["cam_tar"], 1, 0, None, f["feat_geo"],
                                     f["feat_tex"], None, dict(f["sp_data"]), None, fine=True, uniform=True, sample_per_ray_c=S, sample_per_ray_f=S,
                                     src_foreground_mask=f["src_foreground_mask"], bounds=f["bounds"], mask_at_box=None)
    for k in ("tex_fg", "depth", "alpha", "tex_fg_fine", "depth_fine", "alpha_fine"):
        assert out[k].shape == ref[k].shape, k
        assert_close_frac(out[k].cpu(), ref[k], TOL, 2e-2, k)
    assert ref["depth_fine"].std() > 1e-3


def test_frame_cache_sees_a_change_of_extrin_alone(net):
    """VANeRF.frame_data keeps the per-frame tables while its inputs are the same tensors: with the same image, maps, mesh and KRT but another
    sp_data['extrin'] (another tensor, or the same one written in place) the tables are rebuilt -- kpt_cam follows the new extrinsic."""
    base = synth.to_device(synth.make_frame(seed=3, tar_h=16, tar_w=16), "cuda")
    f = synth.pose_source_camera(base, **synth.SOURCE_POSES["A"])
    args = lambda sp: (f["img_in"], f["cam_in"], f["targets"], f["feat_geo"], f["feat_tex"], sp, f["src_foreground_mask"])
    kpt = f["sp_data"]["kpt3d"][0]
    with torch.no_grad():
        fd0 = net.frame_data(*args(base["sp_data"]))  # posed KRT, un-posed extrin
        assert fd0 is net.frame_data(*args(base["sp_data"]))
        assert torch.equal(fd0.kpt_cam[:, :3], kpt)
        fd1 = net.frame_data(*args(f["sp_data"]))
        assert fd1 is not fd0 and fd1 is net.frame_data(*args(f["sp_data"]))
        E = f["sp_data"]["extrin"][0].double()
        want = kpt.double() @ E[:3, :3].t() + E[:3, 3]
        assert (fd1.kpt_cam[:, :3].double() - want).abs().max() <= 1e-6 and (fd1.kpt_cam[:, :3] - kpt).abs().max() > 1e-2
        assert list(fd1.c.extrin) == f["sp_data"]["extrin"][0, :3, :4].reshape(-1).tolist()
        sp = dict(f["sp_data"], extrin=f["sp_data"]["extrin"].clone())
        fd2 = net.frame_data(*args(sp))
        sp["extrin"][0, :3, 3] += 0.01  # in place: same address, another version
        fd3 = net.frame_data(*args(sp))
        assert fd3 is not fd2 and (fd3.kpt_cam[:, :3] - fd2.kpt_cam[:, :3] - 0.01).abs().max() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# g. fused backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def posed_env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import hip_backward as HB, renderer as R
    sd = synth.make_full_weights(0)
    frame = posed_frame("A", 3)
    fdat = _frame_data(R, sd, frame)
    return HB, R, sd, frame, fdat, R.PackedWeights(sd, mode="fp32")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_backward_on_a_posed_camera(posed_env, variant):
    """vanerf_query_forward_spill + vanerf_query_backward on pose A against fp64 autograd with the helpers and bounds of
    tests/test_backward_per_sample.py: every layer's output gradient, the nine IG tensors, every operand slot and the parameter gradients
    through vanerf_weight_products.  600 points: 568 near the mesh and the 32 border-band points, where the bilinear taps clamp (half of the
    source view is masked here, so the band points that project into its masked columns are invalid samples)."""
    HB, R, sd, frame, fdat, w0 = posed_env
    band = border_band_points(frame)
    pts = torch.cat([near_mesh_points(frame, 568, seed=4), band]).contiguous()
    assert pts.shape[0] == 600 and decision_margins(frame, pts)[0].min() > 1e-5
    valid, knn, q_vis, flip, _ = check_block_against_fp64(posed_env, pts, variant)
    assert 0.05 < valid[:568].float().mean() < 0.95 and bool(q_vis.any()) and not bool(q_vis.all())
    assert 8 <= int(valid[568:].sum()) < 32 and not flip[568:].all()
