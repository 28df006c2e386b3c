"""The lean level of the bf16x3 stream and kernel (vanerf_amd/csrc/layer_spec.h, level 2; query_kernel<1, false, 2>).

The lean stream is the hoisted stream without work a sample's result does not need: geo_vis_fusion.fconv_ated.2 / fconv_ated1.2 are linear
layers in front of linear layers and are multiplied into mlp_geo.layers1's layers 0 / 2 by the packer; five layers whose bias k-pair opened
a bf16 step of its own start their accumulators from an fp32 bias table instead; TexVisFusion's input holds (qt[2] | vis_tw) in one k-pair;
mlp_geo.layers2's two last layers are resident in LDS.  Checked here: the algebra (CPU, fp64), the host packer, the folded matrices at the
fp32 summation bound, the device packer word for word, the kernel against the hoisted and the fp32 kernel on the half-masked frame, against
the reference's golden vectors, the VANERF_LEAN_STREAM switch through the one-call and the multi-view pass, determinism, another weight
family and a non-finite folded factor."""
import contextlib
import os

import pytest
import torch

from oracle import vanerf_oracle as orc
from vanerf_amd import synth

TOL = 1e-4  # the bar of tests/test_hip_parity.py on per-sample outputs
WATED0, WATED1 = "geo_vis_fusion.fconv_ated.2.weight", "geo_vis_fusion.fconv_ated1.2.weight"
MLP0, MLP2 = "mlp_geo.layers1.layers.0.linear.", "mlp_geo.layers1.layers.2.linear."
# the fragments (k-step, output block) the lean stream saves against the hoisted one, per layer, as they follow from layer_spec.h:
# fconv_ated.2 4 x 2, fconv_ated1.2 1 x 1, layers1.1 1 x 4, layers2.0 1 x 2, layers2.1 1 x 2, layers2.2 1 x 1, ibr_compress 1 x 1, tex fconv.0 1 x 3
SAVED_FRAGMENTS = 8 + 1 + 4 + 2 + 2 + 1 + 1 + 3


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
def lean_stream(value):
    """VANERF_LEAN_STREAM for the launches inside (the library reads it at every launch)."""
    keep = os.environ.get("VANERF_LEAN_STREAM")
    os.environ["VANERF_LEAN_STREAM"] = value
    try:
        yield
    finally:
        if keep is None:
            del os.environ["VANERF_LEAN_STREAM"]
        else:
            os.environ["VANERF_LEAN_STREAM"] = keep


def _effective(sd, prefix):
    """fp32 effective matrix of a weight-normed layer as the packer folds it: v * (g / ||v||), the norm summed in double."""
    v, g = sd[prefix + "weight_v"].float(), sd[prefix + "weight_g"].float().reshape(-1)
    scale = g / v.double().pow(2).sum(1).sqrt().float()
    return v * scale[:, None]


def _mat(sd, key):
    return sd[key].reshape(sd[key].shape[0], -1).float()


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_the_algebra_of_the_lean_level_in_fp64():
    """fp64, random weights and inputs in the reference's concatenation order.  mlp0([PE | W_b relu(m)], bias) is mlp0 with its geo columns
    replaced by W_mlp0[:, geo] W_b on [PE | relu(m)]; the same for mlp2 with scale 1; a layer with a bias equals the layer without, its
    accumulator started at the bias; the merged TexVisFusion k-pair list holds every input column of fconv.0 / fconv_at.0 exactly once."""
    g = torch.Generator().manual_seed(1)
    f64 = torch.float64
    rnd = lambda *s: torch.randn(*s, dtype=f64, generator=g)
    n = 300
    # scale 0: mlp_geo.layers1.0 on [PE294 | g64], g64 = W_b relu(mid)
    w0, b0, wb = rnd(128, 358), rnd(128), rnd(64, 64)
    pe, mid = rnd(n, 294), rnd(n, 64)
    whole = torch.cat([pe, torch.relu(mid) @ wb.T], 1) @ w0.T + b0
    folded = torch.cat([w0[:, :294], w0[:, 294:] @ wb], 1)
    assert (whole - (torch.cat([pe, torch.relu(mid)], 1) @ folded.T + b0)).abs().max() <= 1e-12 * whole.abs().max()
    # scale 1: mlp_geo.layers1.2 on [h128 | g8]
    w2, b2, wb1 = rnd(120, 136), rnd(120), rnd(8, 8)
    h, mid8 = rnd(n, 128), rnd(n, 8)
    whole = torch.cat([h, torch.relu(mid8) @ wb1.T], 1) @ w2.T + b2
    folded = torch.cat([w2[:, :128], w2[:, 128:] @ wb1], 1)
    assert (whole - (torch.cat([h, torch.relu(mid8)], 1) @ folded.T + b2)).abs().max() <= 1e-12 * whole.abs().max()
    # the five layers that lose their bias k-pair: [x | 1] [W | b]^T = b + W x, summed from the bias on
    for nout, kin in ((128, 128), (64, 128), (64, 64), (2, 64), (24, 128)):
        w, b, x = rnd(nout, kin), rnd(nout), rnd(n, kin)
        with_pair = torch.cat([x, torch.ones(n, 1, dtype=f64)], 1) @ torch.cat([w, b[:, None]], 1).T
        acc = b.expand(n, nout).clone()
        for k in range(kin):
            acc += x[:, k:k + 1] * w[:, k]
        assert (with_pair - acc).abs().max() <= 1e-12 * with_pair.abs().max()
    # the merged pair: the k-pairs of TexVisFusion's first layers, lean level, as the packer lists them (weights_pack.cpp: tex_input_pairs)
    def tex_pairs(hoisted):
        p = [] if hoisted else [(11 + t, 22 + t) for t in range(11)] + [(33 + t, 51 + t) for t in range(18)]
        p += [(u, 6 + u) for u in range(5)] + [(5, 95)]
        p += [(69 + (r & 3) + 8 * (r >> 2), 69 + (r & 3) + 8 * (r >> 2) + 4) for r in range(12) if (r & 3) + 8 * (r >> 2) + 4 < 24]
        return p + [(93, 94)]
    from vanerf_amd import renderer as R
    cols = [c for pair in tex_pairs(False) for c in pair]
    assert len(tex_pairs(False)) == 48 and sorted(cols) == list(range(96))  # fconv.0: every input column once
    cols = [c for pair in tex_pairs(True) for c in pair]
    assert len(tex_pairs(True)) == 19 and sorted(cols + list(R.TEX_NN_COLS) + list(R.TEX_TWIN_COLS)) == list(range(96))  # fconv_at.0 + the table's


def test_host_packer_emits_the_lean_stream_behind_unchanged_streams(hot_weights):
    """stream 4 is SAVED_FRAGMENTS (k-step, block) fragments of 512 words shorter than stream 3; the high bf16 parts of L_MLP0's geo k-pairs are
    the bf16 of the fp32 folded product; the bias table holds the five layers' biases in D-register order; streams 1 and 3 are the words they
    were (their own tests pin their content: here they are compared with a second pack and against their sizes)."""
    from vanerf_amd import renderer as R
    sd = dict(hot_weights)
    s1, s3 = R.stream_host(sd, 1), R.stream_host(sd, 3)
    s4 = R.stream_host(sd, 4)
    assert s3.numel() - s4.numel() == SAVED_FRAGMENTS * 512
    # ... word for word what the packer emitted for these weights before it knew a lean level (SHA-256 of the words, recorded then)
    import hashlib
    assert hashlib.sha256(s1.numpy().tobytes()).hexdigest() == "00dd952f89d6bcdd2d0ada7f47aac64b7a48733b73e6bd4f743f5686e82cd8c8"
    assert hashlib.sha256(s3.numpy().tobytes()).hexdigest() == "955f42a4a2b14933e53e73da48637a87b686dd76c88e58227c60a23f561c38a3"
    assert s1.numel() - s3.numel() == (8 * 1 + 8 * 2 + 4 * 3) * 512  # as tests/test_vertex_products.py
    # the fp32 folded product as the packer formed it (test_folded_matrices_match_fp64... holds it against fp64)
    acc = R.folded_matrices(sd)[0]
    bf16 = lambda w: (w.contiguous().view(torch.int32) + 0x7fff + ((w.contiguous().view(torch.int32) >> 16) & 1)) >> 16 & 0xffff
    # L_MLP0 starts behind [at0_a 5 | at0_b 1 | ated0_a 5 x 2 | at1_a 2 | at1_b 1 | ated1_a 2] fragments; its k-pairs 147..178 are the geo pairs:
    # steps 18 (pairs 144..151) to 22 (176..183), 4 blocks each, hi part first
    off = (5 + 1 + 10 + 2 + 1 + 2) * 512
    layer = s4[off:off + 23 * 4 * 512].view(23, 4, 2, 64, 4)[:, :, 0]  # [step][block][lane][word] of the hi parts
    got = torch.zeros(128, 64, dtype=torch.int64)
    for t in range(147, 179):
        s, j = divmod(t, 8)
        word = layer[s, :, :, j // 2]  # [block][lane]
        half = (word >> (16 * (j % 2))) & 0xffff
        r = t - 147
        k0 = 32 * (r // 16) + (r % 16 & 3) + 8 * (r % 16 >> 2)
        for ob in range(4):
            got[32 * ob:32 * ob + 32, k0] = half[ob, :32]
            got[32 * ob:32 * ob + 32, k0 + 4] = half[ob, 32:]
    assert torch.equal(got, bf16(acc).long())
    # the bias table
    tab = R.bias_table(sd)
    assert tab.numel() == 2 * 16 * (4 + 2 + 2 + 1 + 1)
    at = 0
    for key, nb in (("mlp_geo.layers1.layers.1.linear.bias", 4), ("mlp_geo.layers2.layers.0.linear.bias", 2), ("mlp_geo.layers2.layers.1.linear.bias", 2),
                    ("mlp_geo.layers2.layers.2.linear.bias", 1), ("ibr_compress_gfeat.bias", 1)):
        b = sd[key].float().reshape(-1)
        rows = tab[at:at + 2 * nb * 16].view(2, nb, 16)
        at += 2 * nb * 16
        for h in range(2):
            for ob in range(nb):
                for r in range(16):
                    o = 32 * ob + (r & 3) + 8 * (r >> 2) + 4 * h
                    want = b[o].item() if o < b.numel() else 0.0
                    assert rows[h, ob, r].item() == want, (key, h, ob, r)


def test_folded_matrices_match_fp64_at_the_fp32_summation_bound(hot_weights):
    """Every element of both fp32 folded matrices against the fp64 product of the same fp32 factors within K 2^-24 sum |a_k| |b_k| (K = 64 for
    scale 0, 8 for scale 1: the bound of an fp32 fmaf chain); and what the lean stream holds at their k-pairs of L_MLP0 / L_MLP2, hi + lo bf16
    parts, is that fp32 number to the 2^-16 relative two bf16 parts leave of it."""
    from vanerf_amd import renderer as R
    sd = dict(hot_weights)
    s4 = R.stream_host(sd, 4)
    f64 = torch.float64
    bf = lambda half: (half.to(torch.int32) << 16).view(torch.float32)

    def read(off, steps, t_lo, npairs, nout, nreg_rows):
        layer = s4[off:off + steps * 4 * 512].view(steps, 4, 2, 64, 4)
        got = torch.zeros(nout, nreg_rows, dtype=f64)
        for r in range(npairs):
            s, j = divmod(t_lo + r, 8)
            half = (layer[s, :, :, :, j // 2] >> (16 * (j % 2))) & 0xffff  # [block][part][lane]
            val = bf(half[:, 0]).double() + bf(half[:, 1]).double()  # hi + lo
            k0 = 32 * (r // 16) + (r % 16 & 3) + 8 * (r % 16 >> 2)
            for ob in range(4):
                rows = slice(32 * ob, min(32 * ob + 32, nout))
                got[rows, k0] = val[ob, :rows.stop - rows.start]
                got[rows, k0 + 4] = val[ob, 32:32 + rows.stop - rows.start]
        return got

    off0 = (5 + 1 + 10 + 2 + 1 + 2) * 512
    off2 = off0 + (23 * 4 + 8 * 4) * 512  # behind mlp0 (23 steps) and mlp1 (8 steps, lean), 4 blocks each
    f0, f1 = R.folded_matrices(sd)
    for name, f, packed, a, b, K in (("scale 0", f0, read(off0, 23, 147, 32, 128, 64), _effective(sd, MLP0)[:, 294:], _mat(sd, WATED0), 64),
                                     ("scale 1", f1, read(off2, 9, 64, 4, 120, 8), _effective(sd, MLP2)[:, 128:], _mat(sd, WATED1), 8)):
        ref, mag = a.double() @ b.double(), a.double().abs() @ b.double().abs()
        err = (f.double() - ref).abs()
        bound = K * 2.0 ** -24 * mag
        print(f"{name}: max |err| {err.max().item():.3e}, max bound {bound.max().item():.3e}, max |value| {ref.abs().max().item():.3e}")
        assert (err <= bound).all(), name
        assert ref.abs().max() > 1e-3, name
        assert ((packed - f.double()).abs() <= 2.0 ** -16 * f.double().abs()).all(), name


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lean_stream_on_the_device_equals_the_host_packer(R, sd_full):
    """After the pack and after an update in place with other weights, the lean stream and the bias table a bf16x3 handle holds are the host
    packer's, word for word (and the update left streams 1 and 3 what the host packer makes of the new weights)."""
    w = R.PackedWeights(sd_full, mode="bf16x3")
    assert torch.equal(R.stream_device(w, 4), R.stream_host(sd_full, 4))
    assert torch.equal(R.bias_table(w).view(torch.int32), R.bias_table(sd_full).view(torch.int32))
    other = synth.make_full_weights(7)
    other["sigmoid_beta"] = torch.tensor([0.07])
    w.update({k: v.cuda() for k, v in other.items()})
    assert torch.equal(R.stream_device(w, 4), R.stream_host(other, 4))
    assert torch.equal(R.bias_table(w).view(torch.int32), R.bias_table(other).view(torch.int32))
    for dev_f, host_f in zip(R.folded_matrices(w), R.folded_matrices(other)):
        assert torch.equal(dev_f.view(torch.int32), host_f.view(torch.int32))  # host and device run the same fmaf chain
    assert not torch.equal(R.stream_host(other, 4), R.stream_host(sd_full, 4))
    assert torch.equal(R.stream_device(w, 3), R.stream_host(other, 3)) and torch.equal(R.stream_device(w, 0), R.stream_host(other, 1))
    from vanerf_amd._ffi import lib
    from ctypes import byref, c_int64
    n = c_int64()
    w0 = R.PackedWeights(sd_full, mode="fp32")
    assert lib.vanerf_weights_download(w0.handle, 4, None, 0, byref(n)) == -22  # an fp32 handle carries no lean stream


@pytest.fixture(scope="module")
def half_masked(R, sd_full):
    """The half-masked 128 x 128 frame of tests/test_vertex_products.py at 16 samples per ray: 64 * 64 * 64 = 262 144 samples -- on a 256-CU
    device at least three rounds per block, with full, mixed and all-invalid groups (the ring's hand-overs full -> full, full -> short and
    short -> full).  Inputs and the fp32 kernel's outputs, computed once; a prefix of the samples has the prefix of the outputs."""
    frame = synth.make_frame(seed=5, tar_h=128, tar_w=128, orbit_deg=40.0, half_mask=True)
    fdat = _frame_data(R, sd_full, frame)
    rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 0, 0, 1, 128, 128, 16, device="cuda")
    pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"])
    assert pts.shape[0] == 64 * 64 * 64
    q_sdf, q_vis, knn = R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts)
    ref, valid = R.query_samples(R.PackedWeights(sd_full, mode="fp32"), fdat, pts, q_sdf, q_vis, knn, want_valid=True)
    return fdat, pts, q_sdf, q_vis, knn, ref, valid, R.PackedWeights(sd_full, mode="bf16x3")


def _lean_and_hoisted(R, w, fdat, p, s, v, k, order):
    """-> (lean outputs, flags, short groups), (hoisted outputs, flags, short groups)"""
    res = []
    for switch in ("1", "0"):
        with lean_stream(switch):
            c0 = w.short_groups()
            out, valid = R.query_samples(w, fdat, p, s, v, k, want_valid=True, order=order)
            res.append((out, valid, w.short_groups() - c0))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("n,with_order", [(1, False), (31, False), (33, False), (256 + 17, False), (64 * 64 * 64, False), (64 * 64 * 64, True)])
def test_lean_kernel_against_hoisted_and_fp32(R, half_masked, n, with_order):
    """Same validity flags and the same number of groups on the all-invalid short path as the hoisted kernel, every output within 1e-4 of the
    fp32 kernel; prints the largest lean-vs-hoisted difference (summation order: of the order of 1e-5, recorded, not asserted)."""
    fdat, pts, q_sdf, q_vis, knn, ref, valid, w = half_masked
    p, s, v, k = (t[:n].contiguous() for t in (pts, q_sdf, q_vis, knn))
    order = R.query_order(fdat, p) if with_order else None
    assert fdat.vertex_products(w) is not None
    (lean, valid_l, short_l), (hoisted, valid_h, short_h) = _lean_and_hoisted(R, w, fdat, p, s, v, k, order)
    assert torch.equal(valid_l, valid_h) and torch.equal(valid_l, valid[:n])
    assert short_l == short_h
    if n > 10000:
        assert 0 < short_l < (n + 31) // 32  # some groups take the short path, some do not
        assert 0.05 < valid[:n].float().mean() < 0.95
    d_var = (lean - hoisted).abs().max().item()
    d_ref = (lean - ref[:n]).abs().max().item()
    print(f"n={n} order={with_order}: lean vs hoisted bf16x3 {d_var:.3e}, lean vs fp32 {d_ref:.3e}, hoisted vs fp32 {(hoisted - ref[:n]).abs().max().item():.3e}, "
          f"short groups {short_l} of {(n + 31) // 32}")
    assert d_ref <= TOL
    if n > 10000:
        assert not torch.equal(lean, hoisted)  # the switch switches


@pytest.mark.gpu
def test_lean_kernel_is_deterministic(R, half_masked):
    """Two launches of the largest case: the same bits."""
    fdat, pts, q_sdf, q_vis, knn, ref, valid, w = half_masked
    a = R.query_samples(w, fdat, pts, q_sdf, q_vis, knn)
    b = R.query_samples(w, fdat, pts, q_sdf, q_vis, knn)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["query", "query_posed"])
def test_lean_kernel_vs_reference_golden(R, sd_full, golden, name):
    """The golden vectors of the reference's own VANeRF.query (tests/golden/query.npz, query_posed.npz) at the bar of the hoisted kernel's
    golden test (tests/test_vertex_products.py, tests/test_posed_source.py): 1e-4, equal validity flags."""
    g = golden(name)
    if name == "query_posed":  # as tests/test_posed_source.py::test_query_vs_reference_golden_posed, whose case this is
        from tests.test_posed_source import _case, _run_kernel, _within_the_bar
        c = _case(R, sd_full, "A")
        assert torch.equal(c["pts"], g["pts"][0]) and torch.equal(c["q_sdf"], g["q_sdf"][0]) and torch.equal(c["q_vis"], g["q_vis"][0, :, 0])
        assert R.lean_stream_enabled()
        got, valid = _run_kernel(R, sd_full, c, "bf16x3_hoisted")  # a bf16x3 handle with the frame's table: the lean kernel
        assert torch.equal(valid, g["valid"][0, :, 0])
        _within_the_bar(got, orc.eval_func(sd_full, g["out"], g["valid"], 100.0)[0].double(), "pose A [lean bf16x3] vs reference golden")
        return
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64, half_mask=True)
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode="bf16x3")
    assert fdat.vertex_products(w) is not None and R.lean_stream_enabled()
    gpts = g["pts"][0].contiguous().cuda()
    got, gvalid = R.query_samples(w, fdat, gpts, g["q_sdf"][0].contiguous().cuda(), g["q_vis"][0, :, 0].to(torch.uint8).contiguous().cuda(),
                                  R.knn1(fdat.verts4, gpts), want_valid=True)
    ref = orc.eval_func(sd_full, g["out"], g["valid"], 100.0)[0]
    assert torch.equal(gvalid.cpu().bool(), g["valid"][0, :, 0])
    err = (got.cpu() - ref).abs().max().item()
    print(f"lean bf16x3 vs the reference's {name}: max abs err {err:.3e}")
    assert err <= TOL


PASS_KEYS = ("index", "hit", "z", "color", "depth", "alpha", "color_fine", "depth_fine", "alpha_fine", "sdf", "z_fine")


@pytest.mark.gpu
def test_switch_and_one_call_pass(R, sd_full):
    """16 x 16 rays, 16 + 16 samples.  VANERF_LEAN_STREAM=0: the one-call pass holds the bits of the hoisted path (the Python sequence of stages
    under the same switch, whose per-sample launch is the hoisted kernel: its outputs equal an explicit hoisted launch).  Switched on: the
    one-call pass equals the Python sequence bit for bit, and differs from the hoisted bits (the lean kernel really ran)."""
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode="bf16x3")
    cam, b = frame["cam_tar"], frame["bounds"]
    args = (w, fdat, cam, b, 0, 0, 4, 16, 16, 16, 16)
    with lean_stream("0"):
        off_py, off_c = R.render_pass(*args), R.render_pass_c(*args)
    on_py, on_c = R.render_pass(*args), R.render_pass_c(*args)
    for k in PASS_KEYS:
        assert torch.equal(off_py[k], off_c[k]), k
        assert torch.equal(on_py[k], on_c[k]), k
    assert on_c["hit"].any() and on_c["alpha_fine"].max() > 0
    assert not torch.equal(on_c["color"], off_c["color"])
    assert (on_c["color"] - off_c["color"]).abs().max() <= TOL


@pytest.mark.gpu
def test_multi_view_pass_equals_single_passes(R, sd_full):
    """A 2-view camera-table pass on the lean kernel holds, view after view, the bits of its single-view passes."""
    from vanerf_amd.model import get_360cameras
    from vanerf_amd.novel_views import camera_to_cam_tar
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode="bf16x3")
    headpose = torch.eye(4)
    headpose[:3, 3] = frame["targets"]["vert_world"][0].mean(0)
    cams = [camera_to_cam_tar(c) for c in get_360cameras(headpose[:3, :4].cuda(), 4.0 * 64, 1.0, 1.0, 64, 64, 0.71, 1.42, n_frames=8)][:2]
    bounds = synth.to_device(frame, "cuda")["bounds"]
    assert R.lean_stream_enabled()
    got = R.render_pass_views(w, fdat, cams, bounds, 0, 0, 1, 40, 20, 16, 16)
    for v, cam in enumerate(cams):
        one = R.render_pass_c(w, fdat, cam, bounds, 0, 0, 1, 40, 20, 16, 16)
        for k in PASS_KEYS:
            assert torch.equal(got[k][v], one[k]), (k, v)
    assert got["hit"].any() and got["alpha_fine"].max() > 0


@pytest.mark.gpu
def test_gains_family_within_the_bar(R):
    """synth.make_weight_family("gains", 0), the case and the bar of tests/test_weight_families.py::test_forward_kernels_on_every_family for
    the hoisted kernel: equal validity flags, every output within max(1e-4, 4 E32 + 2^-15 A) of the fp64 oracle (E32 = the fp32 oracle's own
    error, A = the largest pre-activation: that module's docstring), sigma with each sigmoid_beta of the family.  The family's outputs reach
    3.6e3, where one fp32 ulp is 2.4e-4: a plain 1e-4 is not a bar any fp32 output can be held to there (lean vs fp32 kernel on the
    half-masked 64 x 64 frame: 1.2e-1 on alpha at |alpha| up to 3.6e3, 3.4e-5 relative), which is why that module derives its bar."""
    from tests.test_posed_source import _run_kernel, _within_the_bar
    from tests.test_weight_families import _bars, _case
    c = _case(R, "gains")
    assert R.lean_stream_enabled()
    got, valid = _run_kernel(R, c["sd"], c, "bf16x3_hoisted")  # a bf16x3 handle with the frame's table: the lean kernel
    assert torch.equal(valid, c["r64"]["valid"]), f"{int((valid != c['r64']['valid']).sum())} validity flags differ"
    with lean_stream("0"):
        hoisted, _ = _run_kernel(R, c["sd"], c, "bf16x3_hoisted")
    assert not torch.equal(got, hoisted)
    bar = _bars(c, "bf16x3_hoisted")
    err = (got.double() - c["want"]).abs().max(0)[0]
    print(f"gains [lean]: max |HIP - fp64| {[f'{e:.2e}' for e in err.tolist()]}, bar {[f'{b:.2e}' for b in bar.tolist()]}, "
          f"hoisted {[f'{e:.2e}' for e in (hoisted.double() - c['want']).abs().max(0)[0].tolist()]}")
    assert torch.isfinite(got).all()
    for b in synth.GAINS_BETAS:
        beta = max(torch.tensor(b).item(), 2e-3)
        _within_the_bar(got, c["want"], f"gains [lean] beta {beta:g}", beta=beta, tol=bar, sigma_tol=bar[0].item() / (4.0 * beta))


@pytest.mark.gpu
def test_a_nan_in_a_folded_factor_gives_non_finite_sdf(R):
    """One NaN in geo_vis_fusion.fconv_ated.2.weight, which the packer multiplies into mlp_geo.layers1.0: sdf is non-finite on every valid
    sample, as in the kernels that run the layer (tests/test_weight_families.py::test_non_finite_weights_give_non_finite_outputs), and the
    device packer holds the host packer's bits of the folded matrix."""
    sd = synth.make_full_weights(0)
    w_bad = sd[WATED0].clone()
    w_bad.view(torch.int32).reshape(64, -1)[5, 7] = 0x7fffffff
    bad = dict(sd, **{WATED0: w_bad})
    frame = synth.make_frame(seed=5, tar_h=64, tar_w=64, orbit_deg=40.0, half_mask=True)
    fdat = _frame_data(R, sd, frame)
    rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 0, 0, 1, 64, 64, 8, device="cuda")
    pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"])
    q_sdf, q_vis, knn = R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts)
    h = R.PackedWeights(sd, mode="bf16x3").update({k: v.cuda() for k, v in bad.items()})
    assert torch.equal(R.stream_device(h, 4), R.stream_host(bad, 4))
    assert fdat.vertex_products(h) is not None and R.lean_stream_enabled()
    got, valid = R.query_samples(h, fdat, pts, q_sdf, q_vis, knn, want_valid=True)
    valid = valid.bool()
    assert valid.any() and not valid.all()
    v = got[valid]
    assert not torch.isfinite(v[:, 1]).any(), int(torch.isfinite(v[:, 1]).sum())
