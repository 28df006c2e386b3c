"""Whole passes of the HIP path with NOTHING left to the last bit of the ray generator: the oracle's own rays and depths are injected
(renderer.render_pass(inject=...)), so every sample position is bit-identical on both sides, and the bar is the north star's 1e-4 with no
outlier allowance.  Plus the training-mode pass of the reference replayed from its recorded random numbers, the values of the GT gathers
(src/model.py:1361-1418) and BASELINE config 3 (128 + 128 samples per ray) on a 16x16 ray grid.  Needs a real MI355X: `pytest -m gpu`.

What the un-injected whole-image tests (tests/test_hip_parity.py) allow as "outliers" is shown here to come from the ray generator's last
bit alone: with injected rays BOTH kernels (fp32 MFMA and split bf16) have ZERO elements above 1e-4 on every case below, coarse and fine
(largest error seen: 9.2e-6)."""
import copy

import pytest
import torch

from oracle import vanerf_oracle as orc
from tests.conftest import assert_close_frac
from tests.test_hip_parity import _frame, _frame_data, dev
from tests.test_oracle_golden import train_draws
from vanerf_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4
# Same bar for the split-bf16 kernel.  Measured with injected rays (MI355X, round 2): fp32 MFMA <= 4.7e-6, split bf16 <= 9.2e-6 over all
# seven images of every case below -- the per-sample 3.3e-5 of the bf16 kernel averages out in the composite.
TOL_BF16X3 = 1e-4


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


def _inject(ref):
    return {"rays_d": dev(ref["cam_rays"][0].contiguous()), "cam_pos": dev(ref["cam_pos"].reshape(3).contiguous()), "z": dev(ref["z"][0].contiguous()),
            "z_fine": dev(ref["z_fine"][0].contiguous())}


COARSE = (("color", "tex_fg", 3), ("depth", "depth", 1), ("alpha", "alpha", 1))
FINE = (("color_fine", "tex_fg_fine", 3), ("depth_fine", "depth_fine", 1), ("alpha_fine", "alpha_fine", 1), ("sdf", "sdf", 1))


def _compare(out, want, n_y, n_x, tol, what, keys=COARSE + FINE):
    """Every element of the (seven) outputs within tol: returns the largest error seen."""
    worst = 0.0
    for k, gk, ch in keys:
        got = out[k].cpu().view(n_y, n_x, 3).permute(2, 0, 1) if ch == 3 else out[k].cpu().view(n_y, n_x)
        err = (got - want[gk][0]).abs()
        n_bad = int((err > tol).sum())
        assert n_bad == 0, f"{what} {gk}: {n_bad}/{err.numel()} elements above {tol} (max {err.max().item():.3e})"
        worst = max(worst, err.max().item())
    return worst


@pytest.mark.parametrize("tag,seed,hw,orbit,half", [("pass_8x8_s16", 3, 64, 8.0, False), ("pass_16x16_s24_bvv", 5, 64, 70.0, True),
                                                     ("pass_64x64_s64", 11, 256, 15.0, False)])
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_reference_goldens_with_injected_rays(R, sd_full, golden, tag, seed, hw, orbit, half, precision):
    """The three whole-pass goldens of the reference (tests/golden/pass_*.npz).  The oracle supplies its rays, coarse depths and merged fine
    depths; the HIP march must then match the oracle's seven images AND the reference's coarse images with no element above the bar.  The
    reference's fine images are behind importance_sample's u = 1.0 tie (searchsorted on cdf[-1] ~ 1 depends on the last bit of the reference's
    float .sum(): the oracle itself is compared to them with a 1e-3 outlier fraction, tests/test_oracle_golden.py::test_whole_pass) -- same
    allowance here."""
    g = golden(tag)
    frame = _frame(seed, hw, orbit, half)
    S, level = int(g["S"]), int(g["level"])
    ref = orc.batch_render(sd_full, frame, level, g["stride_xy"].long()[None, None], S, S)
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode=precision)
    step = 2 ** (level - 1)
    off = g["stride_xy"].long().tolist()
    n = hw // step
    out = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], off[0], off[1], step, n, n, S, S, inject=_inject(ref))
    assert torch.equal(out["index"].cpu(), ref["index"][0])
    tol = TOL if precision == "fp32" else TOL_BF16X3
    worst = _compare(out, ref, n, n, tol, f"{tag} [{precision}] vs oracle")
    worst_c = _compare(out, g, n, n, tol, f"{tag} [{precision}] vs reference golden", COARSE)
    print(f"{tag} [{precision}] injected rays: max |HIP - oracle| over all seven outputs = {worst:.3e}; max |HIP - reference| coarse = {worst_c:.3e}")
    for k, gk, ch in FINE:
        got = out[k].cpu().view(n, n, 3).permute(2, 0, 1) if ch == 3 else out[k].cpu().view(n, n)
        assert_close_frac(got, g[gk][0], tol, 1e-3, gk)
    assert g["depth_fine"].std() > 1e-3  # not an empty view (alpha is ~1 everywhere: the last interval is 1e10 long, src/model.py:1485)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_benchmark_slice_with_injected_rays(R, sd_full, precision):
    """A strided slice of the 512x334 @ 64 + 64 benchmark view (BASELINE config 2; 660 rays, 84 480 network evaluations) against the oracle."""
    frame = _frame(11, 512, 15.0, tar_w=334)
    step, nx, ny = 16, 334 // 16, 512 // 16
    gy, gx = torch.meshgrid(torch.arange(ny) * step + 3, torch.arange(nx) * step + 5, indexing="ij")
    fr = dict(frame)
    fr["out_hw"] = (ny, nx)
    ref = orc.batch_render(sd_full, fr, 1, None, 64, 64, grids=torch.stack([gx, gy], -1).view(1, -1, 2))
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode=precision)
    out = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], 5, 3, step, nx, ny, 64, 64, inject=_inject(ref))
    assert torch.equal(out["index"].cpu(), ref["index"][0])
    worst = _compare(out, ref, ny, nx, TOL if precision == "fp32" else TOL_BF16X3, f"512x334 slice [{precision}]")
    print(f"512x334 slice [{precision}] injected rays: max |HIP - oracle| = {worst:.3e}")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_config3_128_samples_on_16x16_rays(R, sd_full, precision):
    """BASELINE config 3 (128 coarse + 128 importance samples per ray, large view change, half foreground mask) on a 16x16 strided grid of
    the 512x334 view: 256 rays, 98 304 network evaluations on the oracle side.  Injected rays: no element above the bar; and the same pass
    with the HIP path's own rays and its importance kernel (two samples per lane at 128 + 128) within a whole-image allowance (this view --
    70 degree orbit, half mask, 256 samples per ray -- is the flip-richest of the suite: ~5 of 256 pixels)."""
    frame = synth.make_frame(seed=5, tar_h=512, tar_w=334, orbit_deg=70.0, half_mask=True)
    n, sx, sy = 16, 20, 32
    gy, gx = torch.meshgrid(torch.arange(n) * sy + 7, torch.arange(n) * sx + 9, indexing="ij")
    fr = dict(frame)
    fr["out_hw"] = (n, n)
    ref = orc.batch_render(sd_full, fr, 1, None, 128, 128, grids=torch.stack([gx, gy], -1).view(1, -1, 2))
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode=precision)
    px = torch.stack([gx, gy], -1).view(-1, 2).to(torch.int32).cuda().contiguous()
    out = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], 0, 0, 1, n * n, 1, 128, 128, pixels=px, inject=_inject(ref))
    assert torch.equal(out["index"].cpu(), ref["index"][0])
    worst = _compare(out, ref, n, n, TOL if precision == "fp32" else TOL_BF16X3, f"config 3 [{precision}]")
    print(f"config 3 (128+128) [{precision}] injected rays: max |HIP - oracle| = {worst:.3e}")
    assert ref["depth_fine"].std() > 1e-3  # the grid sees hand and background
    own = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], 0, 0, 1, n * n, 1, 128, 128, pixels=px)
    for k, gk in (("color", "tex_fg"), ("color_fine", "tex_fg_fine")):
        err, bad = assert_close_frac(own[k].cpu().view(n, n, 3).permute(2, 0, 1), ref[gk][0], TOL, 3e-2, gk)
        print(f"config 3 [{precision}] own rays {gk}: {bad}/768 elements above 1e-4 (max {err:.2e}): flips behind last-bit differences of the ray generator")
    for k in ("depth", "alpha", "depth_fine", "alpha_fine"):
        assert_close_frac(own[k].cpu().view(n, n), ref[k][0], TOL, 3e-2, k)
    # the full-size shape of config 3 (512x334 rays, 128 + 128 samples: 43.8 M fine samples in one pass) through the C entry point: rays are
    # independent, so the 256 rays above are bit-for-bit the full view's values at their pixels -- which ties the whole view to the oracle
    full = R.render_pass_c(w, fdat, frame["cam_tar"], frame["bounds"], 0, 0, 1, 334, 512, 128, 128)
    torch.cuda.synchronize()
    assert torch.equal(full["index"].cpu(), torch.arange(334 * 512)) and torch.isfinite(full["color_fine"]).all()
    assert (full["z_fine"][:, 1:] >= full["z_fine"][:, :-1]).all()
    at = own["index"]
    for k in ("color", "depth", "alpha", "color_fine", "depth_fine", "alpha_fine", "sdf", "z_fine"):
        assert torch.equal(full[k][at], own[k]), k


def _train_case(golden):
    g = golden("pass_train_16x16_s16")
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    grids, index = orc.train_window(g["msk_in"][0], int(g["pick"].reshape(-1)[0]), 16, 16, 64, 64)
    return g, frame, grids, index


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_training_pass_replayed_from_the_reference_draws(R, sd_full, golden, precision):
    """the reference's training-mode pass (tests/golden/pass_train_16x16_s16.npz: clamped 16x16 window around a random mask
    pixel, stratified depths, random importance draws, rand_noise_std = 0.01 on both marches) on the HIP path with the recorded draws.
    (a) pixel window and index: bit-exact.  (b) stratified depths from the jitter: 1e-6.  (c) everything injected from the oracle: no element
    of the seven images above the bar against the REFERENCE's values.  (d) the HIP path's own rays and importance kernel with the same draws:
    coarse images within the bar everywhere, fine images within the whole-image allowance."""
    g, frame, grids, index = _train_case(golden)
    S = int(g["S"])
    fr = dict(frame)
    fr["out_hw"] = (16, 16)
    ref = orc.batch_render(sd_full, fr, 5, None, S, S, grids=grids, draws=train_draws(g))
    fdat = _frame_data(R, sd_full, frame)
    w = R.PackedWeights(sd_full, mode=precision)
    px = grids[0].to(torch.int32).cuda().contiguous()
    jitter, u = dev(g["jitter"][0].contiguous()), dev(g["u"][0].contiguous())
    noise = (dev(g["noise_c"].reshape(-1)), dev(g["noise_f"].reshape(-1)))
    kw = dict(jitter=jitter, u=u, noise_std=0.01, noise_draws=noise, pixels=px)
    tol = TOL if precision == "fp32" else TOL_BF16X3
    own = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], 0, 0, 1, 256, 1, S, S, **kw)
    assert torch.equal(own["index"].cpu(), index[0])                                        # (a)
    assert (own["z"].cpu() - ref["z"][0]).abs().max() <= 1e-6                               # (b) z = near + (far - near) (lower + rand (upper - lower))
    out = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], 0, 0, 1, 256, 1, S, S, inject=_inject(ref), **kw)
    worst = _compare(out, g, 16, 16, tol, f"training pass [{precision}] vs reference golden")  # (c)
    print(f"training pass [{precision}] injected: max |HIP - reference| = {worst:.3e}")
    for k, gk in (("color", "tex_fg"), ("depth", "depth"), ("alpha", "alpha")):                # (d)
        got = own[k].cpu().view(16, 16, 3).permute(2, 0, 1) if k == "color" else own[k].cpu().view(16, 16)
        assert_close_frac(got, g[gk][0], tol, 5e-3, gk)
    for k, gk in (("color_fine", "tex_fg_fine"), ("depth_fine", "depth_fine"), ("alpha_fine", "alpha_fine"), ("sdf", "sdf")):
        got = own[k].cpu().view(16, 16, 3).permute(2, 0, 1) if k == "color_fine" else own[k].cpu().view(16, 16)
        assert_close_frac(got, g[gk][0], tol, 2e-2, gk)
    # the noise really entered: without it the coarse image differs
    quiet = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], 0, 0, 1, 256, 1, S, S, jitter=jitter, u=u, pixels=px)
    assert (quiet["color"] - own["color"]).abs().max() > 1e-4


def test_model_training_pass_and_gt_gathers_vs_reference(golden, hot_weights):
    """Through the drop-in module in train mode (VANeRF.batch_render_pifu_nerf, src/model.py:1102-1422) with the recorded draws: the GT
    gathers tar_img / tar_alpha / input_mask / img_in equal the reference's values exactly, the rendered patch matches the reference's, and
    forward()'s loss dict matches compute_error on the reference's patch (src/model.py:1023, src/utils.py:159-178)."""
    from tests.test_oracle_golden import _texframe_weights
    from vanerf_amd.config import default_config
    from vanerf_amd.model import VANeRF
    g, frame, grids, index = _train_case(golden)
    cfg = default_config()
    cfg["models"]["VANeRF"].update(train_out_h=16, train_out_w=16)
    net = VANeRF(cfg).cuda()
    sd = dict(hot_weights)
    sd.update(_texframe_weights(golden))
    missing = net.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys
    net.train()
    fd = synth.to_device(frame, "cuda")
    draws = {k: g[k] for k in ("pick", "jitter", "u", "noise_c", "noise_f")}
    S = int(g["S"])
    with torch.no_grad():
        o = net.batch_render_pifu_nerf(net, fd["img_in"], fd["cam_in"], fd["hand_type"], fd["targets"], 1, fd["cam_tar"], 5, torch.tensor([[3, 1]]),
                                       g["tar_img_in"].cuda(), fd["feat_geo"], fd["feat_tex"], None, copy.copy(fd["sp_data"]), None, fine=True,
                                       uniform=False, rand_noise_std=0.01, sample_per_ray_c=S, sample_per_ray_f=S, msk=g["msk_in"].cuda(),
                                       src_foreground_mask=fd["src_foreground_mask"], bounds=fd["bounds"], _draws=draws)
    for k in ("tar_img", "tar_alpha", "input_mask", "img_in"):
        assert o[k].shape == g[k].shape and torch.equal(o[k].cpu().float(), g[k].float()), k
    assert o["vis_img"].shape == (1, 1, 16, 16) and o["vis_img_all"].shape == (1, 1, 256, 256)
    for k in ("tex_fg", "depth", "alpha"):
        assert_close_frac(o[k].cpu(), g[k], TOL, 5e-3, k)
    for k in ("tex_fg_fine", "depth_fine", "alpha_fine", "sdf"):
        assert_close_frac(o[k].cpu(), g[k], TOL, 2e-2, k)
    # forward(): same pass behind the training entry point, loss = compute_error(out_nerf, vggloss=None, lambdas)
    dr = {"img": fd["img_in"], "cam": fd["cam_in"], "cam_tar": fd["cam_tar"], "tar": g["tar_img_in"].cuda(), "msk": g["msk_in"].cuda()}
    net.kwargs["dr_kwargs"].update(sample_per_ray_c=S, sample_per_ray_f=S)
    net.attach_geo_feat = lambda im, return_val=False: fd["feat_geo"]  # the frame's feature maps stand in for the encoders, as in the golden
    net.attach_tex_feat = lambda im, return_val=False: fd["feat_tex"]
    with torch.no_grad():
        r = net(fd["img_in"], fd["cam_in"], fd["hand_type"], fd["targets"], None, None, 1, copy.copy(fd["sp_data"]), dr,
                src_foreground_mask=fd["src_foreground_mask"], bounds=fd["bounds"], _draws=draws)
    want = {k[4:]: float(v) for k, v in g.items() if k.startswith("err_")}
    assert set(r["err_dict"]) == set(want)
    for k, v in want.items():  # L1 means over the 16x16 patch: a few flipped pixels move them by < 1e-3 relative
        assert abs(float(r["err_dict"][k]) - v) <= 2e-3 * max(1.0, abs(v)), (k, float(r["err_dict"][k]), v)
    assert torch.is_tensor(r["loss"]) and abs(float(r["loss"]) - float(g["loss"])) <= 2e-3 * float(g["loss"])
    assert float((r["loss"] + 0.1 * torch.tensor(0.3, device="cuda")).item()) > float(r["loss"])  # training_step's arithmetic, src/model.py:405


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_every_outlier_of_the_uninjected_image_has_a_flipped_decision(R, sd_full, precision):
    """The shipped path (HIP ray generator, no injection) against the oracle on 40 x 40 strided rays of the 512x334 benchmark view, 64 + 64
    samples: whatever pixel exceeds 1e-4 must show a flipped discrete decision at one of its samples -- visibility flag, inside flag,
    validity, a per-sample output jump, a fine sample in another cdf bin (bench.py: explain_outliers, which runs in every bench --full)."""
    import bench
    frame = synth.make_frame(seed=11, tar_h=512, tar_w=334, orbit_deg=15.0)
    fd = synth.to_device(frame, "cuda")
    sdd = {k: v.cuda() for k, v in sd_full.items() if k.startswith("tex_vis_fusion.")}
    fdat = R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
    w = R.PackedWeights(sd_full, mode=precision)
    S, side = 64, 40
    _, ref, grids = bench.cpu_baseline(sd_full, frame, S, side)
    px = grids[0].to(torch.int32).cuda().contiguous()
    out = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], 0, 0, 1, px.shape[0], 1, S, S, pixels=px)
    want = ref["tex_fg_fine"][0].reshape(3, -1).t()
    err = (out["color_fine"].cpu() - want).abs()
    rep = bench.explain_outliers(R, w, fdat, frame, px, S, ref, err)
    print(precision, rep)
    assert rep["pixels_above_1e-4"] == rep["pixels_above_1e-4_with_a_flipped_decision"], rep
    assert rep["pixels_above_1e-4"] <= 0.01 * side * side
