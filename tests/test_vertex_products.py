"""The per-vertex half of three first layers, hoisted out of the bf16x3 per-sample kernel (vanerf_amd/csrc/vertex_products.hip, layer_spec.h).

geo_vis_fusion.fconv_at.0, geo_vis_fusion.fconv_ated.0 and tex_vis_fusion.fconv_at.0 multiply rows of the per-frame vertex tables that depend
only on a sample's 1-NN vertex; vanerf_vertex_products evaluates those products once per frame and the hoisted kernel starts its accumulators
from the gathered table rows.  Checked here: the split of the layers is an identity (CPU, fp64), the table against fp64 at the fp32 summation
bound, the hoisted kernel against the un-hoisted one and the fp32 kernel, against the reference's golden vector, after a weight update, through
the one-call pass and through the multi-view pass."""
import pytest
import torch

from oracle import vanerf_oracle as orc
from vanerf_amd import synth

TOL = 1e-4  # the bar of tests/test_hip_parity.py on per-sample outputs


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def sd_full(golden, hot_weights):
    from tests.test_oracle_golden import _texframe_weights
    sd = dict(hot_weights)
    sd.update(_texframe_weights(golden))
    return sd


def _frame_data(R, sd, frame):
    fd = synth.to_device(frame, "cuda")
    sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
    return R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])


def test_split_of_the_three_layers_is_an_identity():
    """fp64, random weights and inputs in the reference's concatenation order: (the layer on its per-sample columns) + (table rows x gates) is the
    whole layer.  Pins which columns are per-vertex and the [img3 | tex8 | gf18] <-> 11 / 18 regrouping of a vfeat_tex row."""
    from vanerf_amd import renderer as R
    g = torch.Generator().manual_seed(0)
    f64 = torch.float64
    rnd = lambda *s: torch.randn(*s, dtype=f64, generator=g)
    w_at, w_ated, w_tex = rnd(10, 196), rnd(64, 196), rnd(96, 96)
    vfeat0, vfeat_tex = rnd(R.NV, 64), rnd(R.NV, 32)
    tab = R.vertex_products_reference(w_at, w_ated, w_tex, vfeat0, vfeat_tex)
    n = 500
    i = torch.randint(0, R.NV, (n,), generator=g)
    i[:4] = torch.tensor([0, R.NV_HAND - 1, R.NV_HAND, R.NV - 1])
    tw = R.twin_vertex(i)
    assert torch.equal(tw[:4], torch.tensor([R.NV_HAND, R.NV - 1, 0, R.NV_HAND - 1]))
    pix, scal = rnd(n, 64), rnd(n, 4)  # scal = [sdf | qvis | vis_nn | vis_tw]
    a = torch.rand(n, 3, dtype=f64, generator=g)
    geo_rest = list(range(64)) + list(range(192, 196))
    # fconv_at.0 on [pix | nn | twin | scalars]
    whole = torch.cat([pix, vfeat0[i], vfeat0[tw], scal], 1) @ w_at.T
    split = torch.cat([pix, scal], 1) @ w_at[:, geo_rest].T + tab["A0"][i]
    assert (whole - split).abs().max() <= 1e-12
    # fconv_ated.0 on [a0 pix | a1 nn | a2 twin | scalars]
    whole = torch.cat([a[:, :1] * pix, a[:, 1:2] * vfeat0[i], a[:, 2:3] * vfeat0[tw], scal], 1) @ w_ated.T
    split = torch.cat([a[:, :1] * pix, scal], 1) @ w_ated[:, geo_rest].T + a[:, 1:2] * tab["N0"][i] + a[:, 2:3] * tab["T0"][i]
    assert (whole - split).abs().max() <= 1e-12
    # tex fconv_at.0 on [img3, tex8 | nn11 | twin11 | gf_nn18 | gf_twin18 | lat24 | qvis | vis_nn | vis_tw]
    q11, lat, vis3 = rnd(n, 11), rnd(n, 24), rnd(n, 3)
    vt_nn, vt_tw = vfeat_tex[i], vfeat_tex[tw]
    whole = torch.cat([q11, vt_nn[:, :11], vt_tw[:, :11], vt_nn[:, 11:29], vt_tw[:, 11:29], lat, vis3], 1) @ w_tex.T
    tex_rest = list(range(11)) + list(range(69, 96))
    split = torch.cat([q11, lat, vis3], 1) @ w_tex[:, tex_rest].T + tab["P"][i]
    assert (whole - split).abs().max() <= 1e-12
    # every column is either per-sample or per-vertex, once
    assert sorted(geo_rest + list(R.GEO_NN_COLS) + list(R.GEO_TWIN_COLS)) == list(range(196))
    assert sorted(tex_rest + list(R.TEX_NN_COLS) + list(R.TEX_TWIN_COLS)) == list(range(96))


def test_hoisted_stream_holds_the_per_sample_columns_once(hot_weights):
    """Host packer: the hoisted bf16x3 stream is the bf16x3 stream with three layers shortened to their per-sample k-pairs -- 8 + 16 + 12 fewer
    (k-step, block) fragments of 512 words -- and its high bf16 parts hold every per-sample column of those layers exactly once, no other."""
    from vanerf_amd import renderer as R
    sd = dict(hot_weights)
    plain, hoisted = R.stream_host(sd, 1), R.stream_host(sd, 3)
    assert plain.numel() - hoisted.numel() == (8 * 1 + 8 * 2 + 4 * 3) * 512
    bf16 = lambda w: (w.contiguous().view(torch.int32) + 0x7fff + ((w.contiguous().view(torch.int32) >> 16) & 1)) >> 16 & 0xffff  # round to nearest even
    geo_rest = list(range(64)) + list(range(192, 196))
    tex_rest = list(range(11)) + list(range(69, 96))
    at = 0
    for layer, key, steps, nb, cols in ((0, "geo_vis_fusion.fconv_at.0.weight", 5, 1, geo_rest), (2, "geo_vis_fusion.fconv_ated.0.weight", 5, 2, geo_rest),
                                        (16, "tex_vis_fusion.fconv_at.0.weight", 3, 3, tex_rest)):
        # offset of the layer: the layers before it are unchanged except the hoisted ones
        off = {0: 0, 2: (5 + 1) * 512, 16: None}[layer]
        if off is None:
            off = hoisted.numel() - 2 * 64 * 4 - (3 * 3 + 6 * 1 + 7 * 3 + 6 * 1) * 512  # tex_at_a, tex_at_b, tex_a, tex_b end the stream (+ slack)
        words = hoisted[off:off + steps * nb * 512].view(steps * nb, 2, 256)[:, 0].reshape(-1)  # the hi parts
        got = torch.cat([words & 0xffff, (words >> 16) & 0xffff])
        w = sd[key].reshape(sd[key].shape[0], -1)[:, cols]
        want = bf16(w.float()).reshape(-1)
        got, want = torch.sort(got[got != 0])[0], torch.sort(want[want != 0])[0]
        assert got.numel() == want.numel() and torch.equal(got, want), layer


@pytest.mark.gpu
def test_hoisted_stream_on_the_device_equals_the_host_packer(R, sd_full):
    """After the pack and after an update in place, the hoisted stream a bf16x3 handle holds is the host packer's, word for word."""
    w = R.PackedWeights(sd_full, mode="bf16x3")
    assert torch.equal(R.stream_device(w, 3), R.stream_host(sd_full, 3))
    other = synth.make_full_weights(7)
    other["sigmoid_beta"] = torch.tensor([0.07])
    w.update({k: v.cuda() for k, v in other.items()})
    assert torch.equal(R.stream_device(w, 3), R.stream_host(other, 3)) and torch.equal(R.stream_device(w, 0), R.stream_host(other, 1))


@pytest.mark.gpu
def test_table_matches_fp64_at_the_fp32_summation_bound(R, sd_full):
    """Every element of the table against the fp64 product of the same fp32 inputs, within K 2^-24 sum |w_k x_k| (K = length of its dot
    product: the bound of an fp32 fmaf chain); rows beyond a layer's outputs are 0; two builds give the same bits."""
    frame = synth.make_frame(seed=5, tar_h=64, tar_w=64, orbit_deg=40.0, half_mask=True)
    fdat = _frame_data(R, sd_full, frame)
    vis = fdat.vert_vis
    assert 0 < int((vis == 0).sum()) < R.NV  # non-trivial visibility: whole rows of the vertex tables are zero
    w = R.PackedWeights(sd_full, mode="bf16x3")
    t1, t2 = R.build_vertex_products(w, fdat), R.build_vertex_products(w, fdat)
    assert torch.equal(t1, t2)
    got, pad = R.vertex_products_unpack(t1)
    assert pad == 0.0
    mats = [sd_full[k].cuda() for k in ("geo_vis_fusion.fconv_at.0.weight", "geo_vis_fusion.fconv_ated.0.weight", "tex_vis_fusion.fconv_at.0.weight")]
    mats = [m.reshape(m.shape[0], m.shape[1]) for m in mats]
    f64 = torch.float64
    ref = R.vertex_products_reference(*(m.to(f64) for m in mats), fdat.vfeat0.to(f64), fdat.vfeat_tex.to(f64))
    mag = R.vertex_products_reference(*(m.to(f64).abs() for m in mats), fdat.vfeat0.to(f64).abs(), fdat.vfeat_tex.to(f64).abs())
    for name, K in (("A0", 128), ("N0", 64), ("T0", 64), ("P", 58)):
        err = (got[name].to(f64) - ref[name]).abs()
        bound = K * 2.0 ** -24 * mag[name]
        print(f"{name}: max |err| {err.max().item():.3e}, max bound {bound.max().item():.3e}, max |value| {ref[name].abs().max().item():.3e}")
        assert (err <= bound).all(), name
        assert ref[name].abs().max() > 1e-3, name
    # a vertex that is invisible, and whose twin is too, has all-zero rows
    dead = (vis == 0) & (vis[R.twin_vertex(torch.arange(R.NV, device="cuda"))] == 0)
    if dead.any():
        assert all(float(got[k][dead].abs().max()) == 0.0 for k in got)
    # argument checks
    from vanerf_amd._ffi import lib
    from ctypes import byref, c_void_p
    assert lib.vanerf_vertex_products(None, None, None, 0, None) == t1.numel()
    assert lib.vanerf_vertex_products(w.handle, byref(fdat.c), c_void_p(t1.data_ptr()), t1.numel() - 1, None) == -22
    w0 = R.PackedWeights(sd_full, mode="fp32")
    assert lib.vanerf_vertex_products(w0.handle, byref(fdat.c), c_void_p(t1.data_ptr()), t1.numel(), None) == -22
    assert fdat.vertex_products(w0) is None


@pytest.fixture(scope="module")
def half_masked(R, sd_full):
    """The 128 x 128 x 24 half-masked frame of test_validity_partition_changes_nothing_but_the_order_of_work: valid, mixed and all-invalid groups.
    Inputs and the fp32 kernel's outputs, computed once (the networks are per-sample functions: a prefix of the samples has the prefix of the outputs)."""
    frame = synth.make_frame(seed=5, tar_h=128, tar_w=128, orbit_deg=40.0, half_mask=True)
    fdat = _frame_data(R, sd_full, frame)
    rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 0, 0, 1, 128, 128, 24, device="cuda")
    pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"])
    q_sdf, q_vis, knn = R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts)
    ref, valid = R.query_samples(R.PackedWeights(sd_full, mode="fp32"), fdat, pts, q_sdf, q_vis, knn, want_valid=True)
    return fdat, pts, q_sdf, q_vis, knn, ref, valid, R.PackedWeights(sd_full, mode="bf16x3")


@pytest.mark.gpu
@pytest.mark.parametrize("with_order", [False, True])
@pytest.mark.parametrize("n", [None, 1000 * 24 + 7, 33, 1])
def test_hoisted_kernel_against_unhoisted_and_fp32(R, half_masked, n, with_order):
    """Same validity flags, outputs within 1e-4 of the fp32 kernel, the same number of groups on the all-invalid short path; prints the largest
    difference between the two bf16x3 variants (summation order only: of the order of 1e-5)."""
    fdat, pts, q_sdf, q_vis, knn, ref, valid, w = half_masked
    n = n or pts.shape[0]
    p, s, v, k = (t[:n].contiguous() for t in (pts, q_sdf, q_vis, knn))
    order = R.query_order(fdat, p) if with_order else None
    table = fdat.vertex_products(w)
    assert table is not None
    c0 = w.short_groups()
    plain, valid_p = R.query_samples(w, fdat, p, s, v, k, want_valid=True, order=order, vertex_products=None)
    c1 = w.short_groups()
    hoisted, valid_h = R.query_samples(w, fdat, p, s, v, k, want_valid=True, order=order)
    c2 = w.short_groups()
    assert torch.equal(valid_h, valid_p) and torch.equal(valid_h, valid[:n])
    assert c2 - c1 == c1 - c0
    if n > 10000:
        assert 0 < c1 - c0 < (n + 31) // 32  # some groups take the short path, some do not
        assert 0.05 < valid[:n].float().mean() < 0.95
    d_var = (hoisted - plain).abs().max().item()
    d_ref = (hoisted - ref[:n]).abs().max().item()
    print(f"n={n} order={with_order}: hoisted vs un-hoisted bf16x3 {d_var:.3e}, hoisted vs fp32 {d_ref:.3e}, un-hoisted vs fp32 {(plain - ref[:n]).abs().max().item():.3e}")
    assert d_ref <= TOL
    assert d_var <= TOL
    assert torch.equal(hoisted, R.query_samples(w, fdat, p, s, v, k, order=order, vertex_products=table))  # the explicit table is the default one


@pytest.mark.gpu
def test_hoisted_kernel_vs_reference_golden(R, sd_full, golden):
    """The golden vector of the reference's own VANeRF.query (tests/golden/query.npz), at the bar of the module test in tests/test_hip_parity.py."""
    g = golden("query")
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64, half_mask=True)
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode="bf16x3")
    assert fdat.vertex_products(w) is not None
    gpts = g["pts"][0].contiguous().cuda()
    got, gvalid = R.query_samples(w, fdat, gpts, g["q_sdf"][0].contiguous().cuda(), g["q_vis"][0, :, 0].to(torch.uint8).contiguous().cuda(),
                                  R.knn1(fdat.verts4, gpts), want_valid=True)
    ref = orc.eval_func(sd_full, g["out"], g["valid"], 100.0)[0]
    assert torch.equal(gvalid.cpu().bool(), g["valid"][0, :, 0])
    err = (got.cpu() - ref).abs().max().item()
    print(f"hoisted bf16x3 vs the reference's query: max abs err {err:.3e}")
    assert err <= TOL


@pytest.mark.gpu
def test_a_changed_weight_rebuilds_the_table(R):
    """PackedWeights.update bumps the handle's version: the next pass rebuilds the frame's table and equals a pass with a freshly built one."""
    sd = synth.make_full_weights(0)
    sd["sigmoid_beta"] = torch.tensor([0.1])
    frame = synth.make_frame(seed=3, tar_h=32, tar_w=32)
    fdat = _frame_data(R, sd, frame)
    w = R.PackedWeights(sd, mode="bf16x3")
    rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 0, 0, 1, 32, 32, 8, device="cuda")
    pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"])
    q_sdf, q_vis, knn = R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts)
    before, valid = R.query_samples(w, fdat, pts, q_sdf, q_vis, knn, want_valid=True)
    assert valid.any()
    old = fdat.vertex_products(w).clone()
    assert fdat.vertex_products(w).data_ptr() == fdat.vertex_products(w).data_ptr()  # kept, not rebuilt
    on_dev = {k: v.clone().cuda() for k, v in sd.items()}
    for key in ("geo_vis_fusion.fconv_at.0.weight", "geo_vis_fusion.fconv_ated.0.weight", "tex_vis_fusion.fconv_at.0.weight"):
        on_dev[key].reshape(on_dev[key].shape[0], -1)[:, 40:70] += 0.25  # per-vertex columns of all three layers (and some per-sample ones)
    w.update(on_dev)
    after = R.query_samples(w, fdat, pts, q_sdf, q_vis, knn)
    fresh = R.build_vertex_products(w, fdat)
    assert torch.equal(fdat.vertex_products(w), fresh) and not torch.equal(fresh, old)
    assert torch.equal(after, R.query_samples(w, fdat, pts, q_sdf, q_vis, knn, vertex_products=fresh))
    assert not torch.equal(after, before)
    # ... and equals a freshly packed handle of the changed weights, whose table is new by construction
    w2 = R.PackedWeights({k: v.cpu() for k, v in on_dev.items()}, mode="bf16x3")
    assert torch.equal(after, R.query_samples(w2, fdat, pts, q_sdf, q_vis, knn))
    assert len(fdat._vertex_products) == 2


@pytest.mark.gpu
def test_one_call_pass_with_the_table_equals_the_python_sequence(R, sd_full):
    """vanerf_render_pass with vertex_products against renderer.render_pass with the same table: 16 x 16 rays, 16 + 16 samples, every output bit for bit -- and
    the table is in use (VANERF_VERTEX_PRODUCTS=0 gives the un-hoisted bits, which differ)."""
    import os
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode="bf16x3")
    cam, b = frame["cam_tar"], frame["bounds"]
    keys = ("index", "hit", "z", "color", "depth", "alpha", "color_fine", "depth_fine", "alpha_fine", "sdf", "z_fine")
    a, c = R.render_pass(w, fdat, cam, b, 0, 0, 4, 16, 16, 16, 16), R.render_pass_c(w, fdat, cam, b, 0, 0, 4, 16, 16, 16, 16)
    for k in keys:
        assert torch.equal(a[k], c[k]), k
    assert a["hit"].any() and a["alpha_fine"].max() > 0
    keep = os.environ.get("VANERF_VERTEX_PRODUCTS")
    os.environ["VANERF_VERTEX_PRODUCTS"] = "0"
    try:
        assert fdat.vertex_products(w) is None
        plain = R.render_pass_c(w, fdat, cam, b, 0, 0, 4, 16, 16, 16, 16)
    finally:
        if keep is None:
            del os.environ["VANERF_VERTEX_PRODUCTS"]
        else:
            os.environ["VANERF_VERTEX_PRODUCTS"] = keep
    assert not torch.equal(plain["color"], c["color"])
    assert (plain["color"] - c["color"]).abs().max() <= TOL


@pytest.mark.gpu
def test_multi_view_pass_with_the_table_equals_single_passes(R, sd_full):
    """vanerf_render_pass over a camera table with vertex_products: 2 views of 40 x 20 rays in one pass hold, view after view, the bits of the single-view passes."""
    from vanerf_amd.model import get_360cameras
    from vanerf_amd.novel_views import camera_to_cam_tar
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode="bf16x3")
    headpose = torch.eye(4)
    headpose[:3, 3] = frame["targets"]["vert_world"][0].mean(0)
    cams = [camera_to_cam_tar(c) for c in get_360cameras(headpose[:3, :4].cuda(), 4.0 * 64, 1.0, 1.0, 64, 64, 0.71, 1.42, n_frames=8)][:2]
    bounds = synth.to_device(frame, "cuda")["bounds"]
    got = R.render_pass_views(w, fdat, cams, bounds, 0, 0, 1, 40, 20, 16, 16)
    assert fdat.vertex_products(w) is not None
    for v, cam in enumerate(cams):
        one = R.render_pass_c(w, fdat, cam, bounds, 0, 0, 1, 40, 20, 16, 16)
        for k in ("index", "hit", "z", "color", "depth", "alpha", "color_fine", "depth_fine", "alpha_fine", "sdf", "z_fine"):
            assert torch.equal(got[k][v], one[k]), (k, v)
    assert got["hit"].any() and got["alpha_fine"].max() > 0
