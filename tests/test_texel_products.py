"""The texel level of the bf16x3 stream and kernel (vanerf_amd/csrc/layer_spec.h, level 3; query_kernel<1, false, 3>).

The pixel feature of geo_vis_fusion.fconv_at.0 / fconv_ated.0 is the bilinear sample of the 64-channel geometry map.  grid_sample is linear in the
tap values and the gate a0 is a scalar, so W[:, 0:64] bilin(geo0) = bilin(W[:, 0:64] geo0): vanerf_vertex_products forms the per-texel products
GA / GM once per frame and weight version behind the per-vertex parts of its table, and the kernel samples them where it sampled the feature;
the two layers keep the one bf16 step of their scalar k-pairs.  Checked here with the criteria of tests/test_vertex_products.py and
tests/test_lean_stream.py: the algebra (CPU, fp64), the host packer, the two parts at the fp32 summation bound, the kernel against the fp32
kernel, the lean level and the reference's golden vector, the map's borders, other map sizes and the capacity rule, a weight update, the
VANERF_TEXEL_PRODUCTS switch through the one-call pass, determinism."""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import vanerf_oracle as orc
from vanerf_amd import synth

TOL = 1e-4       # the bar of tests/test_hip_parity.py on per-sample outputs (against the reference's golden vector)
TOL_FP32 = 3.3e-5  # the bf16x3 kernel against the fp32 kernel, per sample
WAT, WATED = "geo_vis_fusion.fconv_at.0.weight", "geo_vis_fusion.fconv_ated.0.weight"
PASS_KEYS = ("index", "hit", "z", "color", "depth", "alpha", "color_fine", "depth_fine", "alpha_fine", "sdf", "z_fine")


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


@contextlib.contextmanager
def env(name, value):
    """An environment switch for the launches inside (the library reads it at every launch)."""
    keep = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if keep is None:
            del os.environ[name]
        else:
            os.environ[name] = keep


def lean_level():
    return env("VANERF_TEXEL_PRODUCTS", "0")


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_split_into_texel_vertex_and_sample_columns_is_an_identity():
    """fp64.  Both layers on [a0 pix | a1 nn | a2 twin | scalars], pix = grid_sample(geo0) with border clamp, against the sampled per-texel
    products + the table's per-vertex rows + the layer on its four scalar columns -- sample positions inside, on texel centres, on and beyond
    the border."""
    from vanerf_amd import renderer as R
    g = torch.Generator().manual_seed(2)
    f64 = torch.float64
    rnd = lambda *s: torch.randn(*s, dtype=f64, generator=g)
    h0, w0, n = 7, 11, 400
    w_at, w_ated, w_tex = rnd(10, 196), rnd(64, 196), rnd(96, 96)
    vfeat0, vfeat_tex, geo0 = rnd(R.NV, 64), rnd(R.NV, 32), rnd(h0, w0, 64)
    tab = R.vertex_products_reference(w_at, w_ated, w_tex, vfeat0, vfeat_tex, geo0)
    assert tab["GA"].shape == (h0 * w0, 10) and tab["GM"].shape == (h0 * w0, 64)
    uv = torch.rand(n, 2, dtype=f64, generator=g) * 2.4 - 1.2  # a sixth of them beyond the border
    uv[:w0, 0] = torch.arange(w0, dtype=f64) / (w0 - 1) * 2 - 1  # texel centres of a row, the last column among them
    uv[:w0, 1] = 1.0
    sample = lambda m: F.grid_sample(m.permute(2, 0, 1)[None], uv[None, :, None], mode="bilinear", padding_mode="border", align_corners=True)[0, :, :, 0].T
    pix, ga, gm = sample(geo0), sample(tab["GA"].view(h0, w0, 10)), sample(tab["GM"].view(h0, w0, 64))
    i = torch.randint(0, R.NV, (n,), generator=g)
    tw = R.twin_vertex(i)
    scal, a = rnd(n, 4), torch.rand(n, 3, dtype=f64, generator=g)
    whole = torch.cat([pix, vfeat0[i], vfeat0[tw], scal], 1) @ w_at.T
    split = ga + tab["A0"][i] + scal @ w_at[:, 192:].T
    assert (whole - split).abs().max() <= 1e-12 * whole.abs().max()
    whole = torch.cat([a[:, :1] * pix, a[:, 1:2] * vfeat0[i], a[:, 2:3] * vfeat0[tw], scal], 1) @ w_ated.T
    split = a[:, :1] * gm + a[:, 1:2] * tab["N0"][i] + a[:, 2:3] * tab["T0"][i] + scal @ w_ated[:, 192:].T
    assert (whole - split).abs().max() <= 1e-12 * whole.abs().max()
    assert sorted(list(R.GEO_PIX_COLS) + list(R.GEO_NN_COLS) + list(R.GEO_TWIN_COLS) + [192, 193, 194, 195]) == list(range(196))


def test_host_packer_emits_the_texel_stream_behind_unchanged_streams(hot_weights):
    """Stream 8 is the lean stream (4) without the four pixel steps of the two layers: 4 x 1 + 4 x 2 fragments of 512 words shorter, the same
    words everywhere else; the high bf16 parts of the two layers hold their four scalar columns exactly once; stream 9 is the bias table."""
    from vanerf_amd import renderer as R
    sd = dict(hot_weights)
    s4, s8 = R.stream_host(sd, 4), R.stream_host(sd, 8)
    assert s4.numel() - s8.numel() == (4 * 1 + 4 * 2) * 512
    assert torch.equal(R.stream_host(sd, 9), R.stream_host(sd, 5))
    # lean: [at0_a 5 | at0_b 1 | ated0_a 5 x 2 | rest]; texel: [at0_a 1 | at0_b 1 | ated0_a 1 x 2 | rest]
    f = 512
    assert torch.equal(s8[0:f], s4[4 * f:5 * f]) and torch.equal(s8[f:2 * f], s4[5 * f:6 * f])  # the scalar step, then at0_b
    assert torch.equal(s8[2 * f:4 * f], s4[(6 + 8) * f:(6 + 10) * f]) and torch.equal(s8[4 * f:], s4[16 * f:])
    bf16 = lambda w: (w.contiguous().view(torch.int32) + 0x7fff + ((w.contiguous().view(torch.int32) >> 16) & 1)) >> 16 & 0xffff
    for key, off, nb in ((WAT, 0, 1), (WATED, 2 * f, 2)):
        words = s8[off:off + nb * f].view(nb, 2, 256)[:, 0].reshape(-1)  # the hi parts
        got = torch.cat([words & 0xffff, (words >> 16) & 0xffff])
        want = bf16(sd[key].reshape(sd[key].shape[0], -1)[:, 192:196].float()).reshape(-1)
        got, want = torch.sort(got[got != 0])[0], torch.sort(want[want != 0])[0]
        assert got.numel() == want.numel() and torch.equal(got, want), key


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _geo_mats(sd):
    return [sd[k].reshape(sd[k].shape[0], -1).cuda() for k in (WAT, WATED, "tex_vis_fusion.fconv_at.0.weight")]


@pytest.mark.gpu
def test_texel_parts_match_fp64_at_the_fp32_summation_bound(R, sd_full):
    """GA / GM against the fp64 product of the same fp32 inputs within K 2^-24 sum |w_k x_k|, K = 64 (the bound used for A0 / N0); padding rows
    and the rows of texels beyond h0 * w0 are 0; two builds give the same bits; the size query sizes the table; the device stream is the host's."""
    frame = synth.make_frame(seed=5, tar_h=64, tar_w=64, orbit_deg=40.0, half_mask=True)
    frame["feat_geo"][0] = torch.rand(1, 64, 16, 40, generator=torch.Generator().manual_seed(9)) * 2 - 1  # 640 of the 1 024 rows in use
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode="bf16x3")
    t1, t2 = R.build_vertex_products(w, fdat), R.build_vertex_products(w, fdat)
    assert torch.equal(t1.view(torch.int32), t2.view(torch.int32))
    got, pad = R.vertex_products_unpack(t1, texels=16 * 40)
    assert pad == 0.0 and list(got) == ["A0", "N0", "T0", "P", "GA", "GM"]
    first, pad4 = R.vertex_products_unpack(t1)
    assert pad4 == 0.0 and list(first) == ["A0", "N0", "T0", "P"] and all(torch.equal(first[k], got[k]) for k in first)
    f64 = torch.float64
    mats = _geo_mats(sd_full)
    ref = R.vertex_products_reference(*(m.to(f64) for m in mats), fdat.vfeat0.to(f64), fdat.vfeat_tex.to(f64), fdat.geo0.to(f64))
    mag = R.vertex_products_reference(*(m.to(f64).abs() for m in mats), fdat.vfeat0.to(f64).abs(), fdat.vfeat_tex.to(f64).abs(), fdat.geo0.to(f64).abs())
    for name, K in (("GA", 64), ("GM", 64)):
        err = (got[name].to(f64) - ref[name]).abs()
        bound = K * 2.0 ** -24 * mag[name]
        print(f"{name}: max |err| {err.max().item():.3e}, max bound {bound.max().item():.3e}, max |value| {ref[name].abs().max().item():.3e}")
        assert (err <= bound).all(), name
        assert ref[name].abs().max() > 1e-3, name
    from ctypes import byref, c_void_p
    from vanerf_amd._ffi import lib
    assert lib.vanerf_vertex_products(None, None, None, 0, None) == t1.numel()
    assert lib.vanerf_vertex_products(w.handle, byref(fdat.c), c_void_p(t1.data_ptr()), t1.numel() - 1, None) == -22
    assert torch.equal(R.stream_device(w, 8), R.stream_host(sd_full, 8)) and torch.equal(R.stream_device(w, 9), R.stream_host(sd_full, 5))


@pytest.fixture(scope="module")
def half_masked(R, sd_full):
    """The half-masked 128 x 128 frame of tests/test_lean_stream.py at 16 samples per ray (64 * 64 * 64 samples: full, mixed and all-invalid
    groups, several rounds per block).  Inputs and the fp32 kernel's outputs, computed once."""
    frame = synth.make_frame(seed=5, tar_h=128, tar_w=128, orbit_deg=40.0, half_mask=True)
    fdat = _frame_data(R, sd_full, frame)
    rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 0, 0, 1, 128, 128, 16, device="cuda")
    pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"])
    assert pts.shape[0] == 64 * 64 * 64
    q_sdf, q_vis, knn = R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts)
    ref, valid = R.query_samples(R.PackedWeights(sd_full, mode="fp32"), fdat, pts, q_sdf, q_vis, knn, want_valid=True)
    return fdat, pts, q_sdf, q_vis, knn, ref, valid, R.PackedWeights(sd_full, mode="bf16x3")


def _texel_and_lean(R, w, fdat, p, s, v, k, order):
    """-> (texel outputs, flags, short groups), (lean outputs, flags, short groups)"""
    res = []
    for switch in ("1", "0"):
        with env("VANERF_TEXEL_PRODUCTS", switch):
            c0 = w.short_groups()
            out, valid = R.query_samples(w, fdat, p, s, v, k, want_valid=True, order=order)
            res.append((out, valid, w.short_groups() - c0))
    return res


def _all_invalid_samples(valid, order, n):
    """Indices of the samples that sit in a 32-slot group without a valid sample (the slots beyond n repeat sample n - 1)."""
    slots = torch.arange((n + 31) // 32 * 32, device=valid.device).clamp(max=n - 1)
    idx = order.long()[slots] if order is not None else slots
    dead = ~valid.bool()[idx].view(-1, 32).any(1)
    return idx.view(-1, 32)[dead].reshape(-1).unique()


def _check_against_lean_and_fp32(R, w, fdat, p, s, v, k, order, ref, valid, label):
    n = p.shape[0]
    (tex, valid_t, short_t), (lean, valid_l, short_l) = _texel_and_lean(R, w, fdat, p, s, v, k, order)
    assert torch.equal(valid_t, valid_l) and torch.equal(valid_t, valid)
    assert short_t == short_l
    dead = _all_invalid_samples(valid, order, n)
    assert torch.equal(tex[dead].view(torch.int32), lean[dead].view(torch.int32))  # the short path is untouched
    d_lean = (tex - lean).abs().max().item()
    d_ref = (tex - ref).abs().max().item()
    print(f"{label}: texel vs lean {d_lean:.3e}, texel vs fp32 {d_ref:.3e}, lean vs fp32 {(lean - ref).abs().max().item():.3e}, "
          f"short groups {short_t} of {(n + 31) // 32}, samples in all-invalid groups {dead.numel()}")
    assert d_ref <= TOL_FP32
    return tex, lean, short_t


@pytest.mark.gpu
@pytest.mark.parametrize("with_order", [False, True])
@pytest.mark.parametrize("n", [1, 33, 257, 64 * 64 * 64])
def test_texel_kernel_against_lean_and_fp32(R, half_masked, n, with_order):
    """Same validity flags and short-group count as the lean level, every all-invalid group bit-equal to the lean level's, every output within
    3.3e-5 of the fp32 kernel; prints the largest texel-vs-lean difference (summation order: recorded, not asserted)."""
    fdat, pts, q_sdf, q_vis, knn, ref, valid, w = half_masked
    at = 0 if n > 10000 else int(valid.nonzero()[0])  # the frame's first samples are all masked out: the small sets begin at the first valid one
    p, s, v, k = (t[at:at + n].contiguous() for t in (pts, q_sdf, q_vis, knn))
    order = R.query_order(fdat, p) if with_order else None
    assert fdat.vertex_products(w) is not None and valid[at:at + n].any()
    tex, lean, short = _check_against_lean_and_fp32(R, w, fdat, p, s, v, k, order, ref[at:at + n], valid[at:at + n], f"n={n} order={with_order}")
    if n > 10000:
        assert 0 < short < (n + 31) // 32 and 0.05 < valid.float().mean() < 0.95
        assert not torch.equal(tex, lean)  # the switch switches
        again = R.query_samples(w, fdat, p, s, v, k, order=order)
        assert torch.equal(tex.view(torch.int32), again.view(torch.int32))  # two launches: the same bits


@pytest.mark.gpu
def test_texel_kernel_vs_reference_golden(R, sd_full, golden):
    """The golden vector of the reference's own VANeRF.query (tests/golden/query.npz) at 1e-4, equal validity flags."""
    g = golden("query")
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64, half_mask=True)
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode="bf16x3")
    assert fdat.vertex_products(w) is not None and os.environ.get("VANERF_TEXEL_PRODUCTS", "1") != "0"
    gpts = g["pts"][0].contiguous().cuda()
    args = (g["q_sdf"][0].contiguous().cuda(), g["q_vis"][0, :, 0].to(torch.uint8).contiguous().cuda(), R.knn1(fdat.verts4, gpts))
    got, gvalid = R.query_samples(w, fdat, gpts, *args, want_valid=True)
    with lean_level():
        lean = R.query_samples(w, fdat, gpts, *args)
    ref = orc.eval_func(sd_full, g["out"], g["valid"], 100.0)[0]
    assert torch.equal(gvalid.cpu().bool(), g["valid"][0, :, 0]) and gvalid.any()
    err = (got.cpu() - ref).abs().max().item()
    print(f"texel bf16x3 vs the reference's query: max abs err {err:.3e} (lean: {(lean.cpu() - ref).abs().max().item():.3e})")
    assert err <= TOL
    assert not torch.equal(got, lean)


def _border_points(fdat, frame, h0, w0):
    """Points whose projection into the source view lies, at the geo0 scale, on texel centres, in the last column and row, in the +-1e-2 band
    around the border and outside the view: p = M^-1 (d [u, v, 1] - t) for KRT = [M | t], at the mean depth of the mesh."""
    f64 = torch.float64
    KRT = frame["cam_in"]["KRT"][0].to(f64)
    M, t = KRT[:3, :3], KRT[:3, 3]
    W, H = float(fdat.c.width), float(fdat.c.height)
    d = (frame["targets"]["vert_world"][0].to(f64) @ M.T + t)[:, 2].mean()
    ix, iy = [], []
    cx, cy = torch.arange(w0, dtype=f64), torch.arange(h0, dtype=f64)
    gx, gy = torch.meshgrid(cx, cy, indexing="xy")
    ix.append(gx.reshape(-1)); iy.append(gy.reshape(-1))                                   # texel centres, corners included
    fr = torch.linspace(0.0, 1.0, 33, dtype=f64)
    ix.append(w0 - 2 + fr); iy.append(torch.full_like(fr, h0 / 2.0 + 0.3))                  # the last column: x1 = min(x0 + 1, W - 1)
    ix.append(torch.full_like(fr, w0 / 3.0 + 0.2)); iy.append(h0 - 2 + fr)                  # the last row
    ix.append(w0 - 2 + fr); iy.append(h0 - 2 + fr)                                         # the last corner
    band = torch.linspace(-1.5e-2, 1.5e-2, 31, dtype=f64)                                  # normalised units: inside, on and beyond the eps band
    for side in (-1.0, 1.0):
        xs = (side + band * 1.0 + 1.0) / 2.0 * (w0 - 1)
        ix.append(xs); iy.append(torch.full_like(xs, h0 / 2.0))
        ys = (side + band + 1.0) / 2.0 * (h0 - 1)
        ix.append(torch.full_like(ys, w0 / 2.0)); iy.append(ys)
    out = torch.tensor([-0.6, -0.25, 1.25, 1.6], dtype=f64) * (w0 - 1)                       # outside the view
    ix.append(out); iy.append(torch.full_like(out, h0 / 2.0))
    ix.append(torch.full_like(out, w0 / 2.0)); iy.append(out / (w0 - 1) * (h0 - 1))
    ix, iy = torch.cat(ix), torch.cat(iy)
    u, v = ix / (w0 - 1) * (W - 1), iy / (h0 - 1) * (H - 1)
    pix = torch.stack([u * d, v * d, torch.full_like(u, d)], 1)
    return torch.linalg.solve(M, (pix - t).T).T.to(torch.float32).contiguous().cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("h0,w0", [(32, 32), (16, 40), (40, 40)])
def test_borders_and_map_sizes(R, sd_full, h0, w0):
    """Samples on texel centres, in the last column and row, around the border's eps band and outside the view, on the 32 x 32 map, on a
    non-square one inside the capacity and on one above it.  Inside the capacity: the bars of the kernel test.  Above it (40 x 40 = 1 600
    texels): the table's per-texel part stays unwritten and the launch holds the lean level's bits exactly."""
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    frame["feat_geo"][0] = torch.rand(1, 64, h0, w0, generator=torch.Generator().manual_seed(h0 * w0)) * 2 - 1
    frame["src_foreground_mask"] = torch.ones_like(frame["src_foreground_mask"])  # valid wherever the projection is in the view
    fdat = _frame_data(R, sd_full, frame)
    pts = _border_points(fdat, frame, h0, w0)
    q_sdf, q_vis, knn = R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts)
    ref, valid = R.query_samples(R.PackedWeights(sd_full, mode="fp32"), fdat, pts, q_sdf, q_vis, knn, want_valid=True)
    n_out = 8
    assert valid[:h0 * w0].all() and not valid[-n_out:].any() and 0 < int(valid.sum()) < pts.shape[0] - n_out  # the band holds both kinds
    w = R.PackedWeights(sd_full, mode="bf16x3")
    for with_order in (False, True):
        order = R.query_order(fdat, pts) if with_order else None
        tex, lean, _ = _check_against_lean_and_fp32(R, w, fdat, pts, q_sdf, q_vis, knn, order, ref, valid, f"{h0}x{w0} order={with_order}")
        if h0 * w0 > R.TEXELS_MAX:
            assert torch.equal(tex.view(torch.int32), lean.view(torch.int32))
        else:
            assert not torch.equal(tex, lean)


@pytest.mark.gpu
def test_a_changed_pixel_column_is_followed(R):
    """PackedWeights.update with columns 0..63 of both layers changed: the next launch rebuilds the table, its results equal a freshly packed
    handle's and differ from the old ones; the device holds the host packer's texel stream."""
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
    on_dev = {k: v.clone().cuda() for k, v in sd.items()}
    for key in (WAT, WATED):
        on_dev[key].reshape(on_dev[key].shape[0], -1)[:, 0:64] += 0.25
    w.update(on_dev)
    host = {k: v.cpu() for k, v in on_dev.items()}
    assert torch.equal(R.stream_device(w, 8), R.stream_host(host, 8)) and torch.equal(R.stream_device(w, 9), R.stream_host(host, 5))
    after = R.query_samples(w, fdat, pts, q_sdf, q_vis, knn)
    fresh = R.build_vertex_products(w, fdat)
    got_old, _ = R.vertex_products_unpack(old, texels=32 * 32)
    got_new, _ = R.vertex_products_unpack(fresh, texels=32 * 32)
    assert torch.equal(fdat.vertex_products(w), fresh)
    assert not torch.equal(got_new["GA"], got_old["GA"]) and not torch.equal(got_new["GM"], got_old["GM"])
    assert all(torch.equal(got_new[k], got_old[k]) for k in ("A0", "N0", "T0", "P"))  # only the pixel columns changed
    assert not torch.equal(after, before)
    w2 = R.PackedWeights(host, mode="bf16x3")
    assert torch.equal(after, R.query_samples(w2, fdat, pts, q_sdf, q_vis, knn))
    ref = R.query_samples(R.PackedWeights(host, mode="fp32"), fdat, pts, q_sdf, q_vis, knn)
    assert (after - ref).abs().max() <= TOL_FP32


@pytest.mark.gpu
def test_switch_and_one_call_pass(R, sd_full):
    """16 x 16 rays, 16 + 16 samples.  Unset: vanerf_render_pass equals the Python sequence of stages bit for bit.  VANERF_TEXEL_PRODUCTS=0: the
    one-call pass and the Python sequence hold the same bits, the lean level's (tools/query_bits.py holds that level to the previous
    library's bits), and they differ from the texel level's within the per-sample bar."""
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode="bf16x3")
    cam, b = frame["cam_tar"], frame["bounds"]
    args = (w, fdat, cam, b, 0, 0, 4, 16, 16, 16, 16)
    with lean_level():
        off_py, off_c = R.render_pass(*args), R.render_pass_c(*args)
    on_py, on_c = R.render_pass(*args), R.render_pass_c(*args)
    for k in PASS_KEYS:
        assert torch.equal(off_py[k], off_c[k]), k
        assert torch.equal(on_py[k], on_c[k]), k
    assert on_c["hit"].any() and on_c["alpha_fine"].max() > 0
    assert not torch.equal(on_c["color"], off_c["color"])
    assert (on_c["color"] - off_c["color"]).abs().max() <= TOL
