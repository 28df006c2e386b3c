"""The fused backward of the per-sample networks (vanerf_query_forward_spill + vanerf_query_backward, csrc/query_backward.hip, driven by
hip_backward.run_block) sample by sample against the fp64 CPU oracle differentiated by torch.autograd (tests/test_oracle_fp64.py proves the
oracle's hooks mean what is assumed here), and vanerf_scatter_add_taps against an fp64 index_add.

Per-sample bound, row by row (one sample's vector of every IG tensor, every layer's Ys and Xs), relative to row max + 1e-3 tensor max:
TOL = 1e-4, or three times what the plain fp32 evaluation of the same networks (the CPU oracle in fp32, same samples) reaches against fp64
where that is more -- and no more rows above TOL than twice as many as plain fp32 has (+ 2).  A fixed bound cannot hold for any fp32
implementation: a gate's gradient is a sum of input x gradient products that cancel, and on GeoVisFusion's 8-channel scale plain fp32 itself
is 5e-3 off in a few rows.  The block's parameter gradients are held to TOL of the tensor's max (or 3x plain fp32).  A wiring error is O(1).
Decision flips: the kernel makes its ReLU and `rad + noise > 0` decisions on fp32 values, so a pre-activation within fp32 noise of zero can
take the other branch than in fp64 and change that sample's gradient by O(1).  A threshold on |pre-activation| would exclude far too many
samples (1e-4 of the layer's largest value: ~25 %, 3e-5: ~7 %; the fp32 error of a pre-activation reaches 1.4e-5 of it), so the decisions
are compared directly: the kernel's read from its spilled operands (the next layer's Xs is relu(Y) as the kernel computed it; raw + noise
from its raw output), plain fp32's and fp64's from the oracle's hooks.  Samples where they differ get a zero upstream gradient on all sides
(exact zeros in every spill, nothing added to the parameter gradients); they must stay below 1 % of the samples.

Observed on an MI355X (worst row error, HIP / plain fp32; 4 657 samples, 69 % valid; the whole file runs in ~4 s):
  decision flips: 1 sample (2e-4);
  IG: pix0 / nn0 / tw0 1.5e-4 / 1.2e-4, pix1 / nn1 / tw1 3.5e-3 / 2.1e-3, row_nn / row_tw / tex_xy 4.5e-5 / 4.7e-5;
  Ys: GeoVisFusion 5.6e-3 / 5.6e-3 (scale 1), mlp_geo 2.2e-4 / 1.6e-4, TexVisFusion 6.1e-4 / 6.1e-4, ibr_compress 1.7e-5 / 2.3e-5;
  Xs: 8.3e-5 / 7.2e-5 everywhere but GeoVisFusion scale 1's second layers (fconv_at1.2 2.7e-4 / 1.7e-4, fconv_ated1.2 5.4e-3 / 2.9e-3);
  parameter gradients: 5.0e-5 / 4.5e-5 of the tensor's max (all under TOL);
  HIP / plain fp32 <= 1.9 for every tensor whose error exceeds TOL.
With one GeoVisFusion gate's gradient 2 % off (a scratch build), all three variants of the per-sample test fail; of the existing tests,
test_hip_backward_at_the_real_patch_size and test_backward_chain_is_a_pure_function_of_the_sample pass."""
import pytest
import torch

from oracle import vanerf_oracle as orc
from tests.test_oracle_fp64 import IG_NAMES, RELU_LAYERS, param_keys, reference
from vanerf_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4
NEXT = {"geo_vis_fusion.fconv_at.0.weight": 1, "geo_vis_fusion.fconv_ated.0.weight": 3, "geo_vis_fusion.fconv_at1.0.weight": 5,
        "geo_vis_fusion.fconv_ated1.0.weight": 7, "tex_vis_fusion.fconv_at.0.weight": 17, "tex_vis_fusion.fconv.0.weight": 19}  # ReLU layer -> next layer


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import hip_backward as HB, renderer as R
    sd = synth.make_full_weights(0)
    frame = synth.make_frame(seed=5, tar_h=64, tar_w=64, half_mask=True)  # half the source view masked: a foreground-mask edge
    fd = synth.to_device(frame, "cuda")
    sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
    fdat = R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
    w0 = R.PackedWeights(sd, mode="fp32")
    return HB, R, sd, frame, fdat, w0


def _edge_points(frame):
    """Hand-placed points at the edges of the per-sample pass (source camera: focal 1500, principal point 128, 256 x 256, identity pose;
    depth range [0.71, 1.42]; columns < 119 masked out)."""
    def at(u, v, z):  # pixel (u, v) at depth z -> world point
        return [(u - 128.0) * z / 1500.0, (v - 128.0) * z / 1500.0, z]
    p = []
    for u in (254.5, 255.2, 255.9, 256.6, 250.0, 245.0, 240.0):  # the view's right border: [-1, 1] ends at 255, the eps band at 256.275,
        for v in (128.0, 60.0, 254.8):                           # the pixel-weight ramp covers the last 10 % of the view
            p.append(at(u, v, 1.0))
    for z in (0.7101, 0.7105, 0.712, 0.72, 0.7099, 0.70, 1.41, 1.4199):  # z = -1 (znear) and z = 1
        p.append(at(140.0, 130.0, z))
        p.append(at(200.0, 128.0, z))
    for u in (118.6, 118.9, 119.3, 119.9, 117.5, 121.0):  # the mask edge: fg_xy = u - 118 around the 0.1 threshold at u = 118.1
        for v in (100.0, 140.0):
            p.append(at(u, v, 1.0))
    return torch.tensor(p, dtype=torch.float32)


def _points(R, frame, fdat, n_rays=(8, 8), S=64):
    """Points on real rays of the target view at the training configuration (64 samples per ray through the box), points near the mesh of
    both hands, and the hand-placed edge points."""
    rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 28, 28, 1, n_rays[0], n_rays[1], S, device="cuda")
    on_rays = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"]).view(-1, 3).cpu()
    g = torch.Generator().manual_seed(4)
    v = frame["targets"]["vert_world"][0]
    near = v[torch.randint(0, v.shape[0], (512,), generator=g)] + 0.01 * torch.randn(512, 3, generator=g)
    return torch.cat([on_rays, near, _edge_points(frame)]).contiguous()


def _queries(R, fdat, pts):
    q_sdf, q_vis, knn = (t.view(-1) for t in R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts.cuda()))
    return q_sdf, q_vis, knn


def _row_err(got, want):
    """max over rows of |got - want| / (row max + 1e-3 tensor max), rows = samples."""
    got, want = got.double().cpu(), want.double().cpu()
    den = want.abs().amax(1) + 1e-3 * want.abs().max() + 1e-30
    return ((got - want).abs().amax(1) / den)


def _kernel_decisions(HB, ws, n, ref, noises):
    """Samples whose ReLU / `rad + noise > 0` decision differs between the kernel (read from its spills) and the fp64 oracle."""
    L = HB.layout()
    flip = torch.zeros(n, dtype=torch.bool)
    for name in RELU_LAYERS:
        lay = L["layers"][NEXT[name]]
        sl = lay["slots"]
        cols = (sl >= 0).nonzero().view(-1)
        x = ws.xs[lay["x_row"] + cols, :n].cpu().t()  # relu(Y) as the kernel computed it
        y = ref["layers"][name][1][:, sl[cols]]
        flip |= ((x > 0) != (y > 0)).any(1)
    rad = ws.raw[:n, 1].cpu()
    for nk, no in noises:  # (the kernel's draw, the oracle's)
        if nk is not None:
            flip |= ((rad + nk) > 0) != ((ref["raw"][:, 1] + no.double()) > 0)
    return flip


def _fp32_decisions(r32, ref, noises):
    """The same for the plain fp32 evaluation (the CPU oracle in fp32)."""
    flip = torch.zeros(ref["raw"].shape[0], dtype=torch.bool)
    for name in RELU_LAYERS:
        flip |= ((r32["layers"][name][1] > 0) != (ref["layers"][name][1] > 0)).any(1)
    for nk, no in noises:
        if nk is not None:
            flip |= ((r32["raw"][:, 1] + nk.float()) > 0) != ((ref["raw"][:, 1] + no.double()) > 0)
    return flip


def _check(what, got, want, got32, worst):
    """Row bound against fp64: TOL, or three times the worst row error of the plain fp32 evaluation of the same tensor where fp32 arithmetic
    itself cannot reach TOL (ill-conditioned rows: a gate's gradient is a sum of input x gradient products that cancel); and no more rows
    above TOL than twice as many as the fp32 evaluation has (+ 2)."""
    e, e32 = _row_err(got, want), _row_err(got32, want)
    bound = TOL + 3.0 * e32.max().item()
    worst[what] = (e.max().item(), e32.max().item())
    assert (e <= bound).all(), (what, int((e > bound).sum()), e.max().item(), int(e.argmax()), e32.max().item())
    assert int((e > TOL).sum()) <= 2 * int((e32 > TOL).sum()) + 2, (what, int((e > TOL).sum()), int((e32 > TOL).sum()))


def _run(HB, R, env, pts, d, noise=None, d2=None, noise2=None, ws=None, oracle_noise=None):
    """One block through the fused backward, the same samples through the fp64 oracle; kernel-vs-fp64 decision flips get d = 0 on both sides."""
    _, _, sd, frame, fdat, w0 = env
    n = pts.shape[0]
    q_sdf, q_vis, knn = _queries(R, fdat, pts)
    vert_vis = fdat.vert_vis.cpu()
    ref0 = reference(sd, frame, pts, q_sdf.cpu(), q_vis.cpu(), vert_vis)
    r32_0 = reference(sd, frame, pts, q_sdf.cpu(), q_vis.cpu(), vert_vis, dtype=torch.float32)
    ws = ws or HB.Workspace(n, "cuda")
    c = lambda t: None if t is None else t.cuda().contiguous()
    ws.dw.zero_()
    HB.run_block(ws, w0, fdat, pts.cuda(), q_sdf, q_vis, knn, c(d), c(noise), c(d2), c(noise2))
    torch.cuda.synchronize()
    assert torch.equal(ws.valid[:n].cpu().bool(), ref0["valid"])
    on = oracle_noise or {}
    noises = [(noise, on.get("noise", noise)), (noise2, on.get("noise2", noise2))]
    flip = _kernel_decisions(HB, ws, n, ref0, noises) | _fp32_decisions(r32_0, ref0, noises)
    d = d.clone(); d[flip] = 0.0
    if d2 is not None:
        d2 = d2.clone(); d2[flip] = 0.0
    ws.dw.zero_()
    ig, _ = HB.run_block(ws, w0, fdat, pts.cuda(), q_sdf, q_vis, knn, c(d), c(noise), c(d2), c(noise2))
    torch.cuda.synchronize()
    ref = reference(sd, frame, pts, q_sdf.cpu(), q_vis.cpu(), vert_vis, d=d, noise=on.get("noise", noise), d2=d2, noise2=on.get("noise2", noise2))
    r32 = reference(sd, frame, pts, q_sdf.cpu(), q_vis.cpu(), vert_vis, d=d, noise=noise, d2=d2, noise2=noise2, dtype=torch.float32)
    return ws, {k: v.cpu() for k, v in ig.items()}, ref, flip, knn.cpu().long(), q_vis.cpu(), r32


VARIANTS = {"d": (False, False), "d_noise": (True, False), "d_d2_noise": (True, True)}


def check_block_against_fp64(env, pts, variant, zeros_exact=False):
    """One block of `pts` (n, 3) of env's frame through the fused backward against fp64 autograd, sample by sample, with this file's bounds:
    IG (all nine tensors), Ys (every layer), Xs (every slot) and the block's parameter gradients (vanerf_weight_products); exact zeros where
    the reference's are.  env = (HB, R, sd, frame, fdat, w0) as the fixture above builds it (tests/test_posed_source.py builds one around a
    posed source camera; tests/test_weight_families.py around other weights).  zeros_exact: every parameter gradient that fp64 autograd gives
    as an exact zero must be an exact zero (their number is returned as worst["exact zeros"]).
    Returns (valid, knn, q_vis, flip, worst = {tensor: (HB error, plain fp32 error)})."""
    HB, R, sd, frame, fdat, w0 = env
    n = pts.shape[0]
    g = torch.Generator().manual_seed(7)
    d, d2 = torch.randn(n, 5, generator=g), torch.randn(n, 5, generator=g)
    noise, noise2 = 0.05 * torch.randn(n, generator=g), 0.05 * torch.randn(n, generator=g)
    use_noise, use_d2 = VARIANTS[variant]
    ws, ig, ref, flip, knn, q_vis, r32 = _run(HB, R, env, pts, d, noise if use_noise else None, d2 if use_d2 else None,
                                         noise2 if use_d2 else None)
    valid = ref["valid"]
    assert torch.equal(knn, orc.knn1(pts, frame["targets"]["vert_world"][0]))  # 1-NN index: bit-exact
    assert flip.float().mean() <= 0.01, f"{int(flip.sum())} of {n} samples took another ReLU branch in fp32"
    worst = {}
    # a. IG: the gradients of the gathered inputs
    for k in IG_NAMES:
        _check(k, ig[k], ref["d_gathered"][k], r32["d_gathered"][k], worst)
    for k in ("pix0", "nn0", "tw0", "pix1", "nn1", "tw1"):  # the reference's zeros are exact
        assert torch.equal(ig[k][~valid], torch.zeros_like(ig[k][~valid])), k
    # b. Ys: every layer's output gradient
    L = HB.layout()
    from vanerf_amd.hip_backward import LAYER_PARAMS
    for lay, (_, name) in zip(L["layers"], LAYER_PARAMS):
        got = ws.ys[lay["y_row"]:lay["y_row"] + lay["n_out"], :n].cpu().t()
        _check("Ys " + name, got, ref["d_y"][name][:, :lay["n_out"]], r32["d_y"][name][:, :lay["n_out"]], worst)
    head = L["layers"][14]
    assert torch.equal(ws.ys[head["y_row"]:head["y_row"] + 2, :n].cpu()[:, ~valid], torch.zeros(2, int((~valid).sum())))
    # c. Xs: every slot of every layer's operands
    for lay, (_, name) in zip(L["layers"], LAYER_PARAMS):
        sl = lay["slots"]
        xs = ws.xs[lay["x_row"]:lay["x_row"] + lay["n_slots"], :n].cpu().t()
        cols = (sl >= 0).nonzero().view(-1)
        _check("Xs " + name, xs[:, cols], ref["layers"][name][0][:, sl[cols]], r32["layers"][name][0][:, sl[cols]], worst)
        assert torch.equal(xs[:, sl == -2], torch.ones_like(xs[:, sl == -2])), name  # the bias operand
        assert torch.equal(xs[:, sl == -1], torch.zeros_like(xs[:, sl == -1])), name  # padding: the kernel feeds exact zeros
    # d. parameter gradients of the block (slot -> channel map, duplicated slots, weight-norm fold, biases)
    P = {k: v.cuda() for k, v in sd.items()}
    got = HB.parameter_gradients(ws, P)
    n_zero = 0
    for spec in LAYER_PARAMS:
        for key in param_keys(spec):
            want = ref["d_params"][key]
            e = ((got[key].double().cpu() - want).abs().max() / want.abs().max()).item()
            e32 = ((r32["d_params"][key].double() - want).abs().max() / want.abs().max()).item()
            worst["dP " + key] = (e, e32)
            assert e <= TOL + 3.0 * e32, (key, e, e32)
            if zeros_exact:
                zero = want == 0
                assert torch.equal(got[key].cpu()[zero], torch.zeros(int(zero.sum()))), (key, int((got[key].cpu()[zero] != 0).sum()), int(zero.sum()))
                n_zero += int(zero.sum())
    fc2 = got["tex_vis_fusion.fconv.2.weight"]
    assert torch.equal(fc2[3:], torch.zeros_like(fc2[3:]))
    print(f"[{variant}] n {n}, valid {valid.float().mean().item():.3f}, decision flips {int(flip.sum())} ({flip.float().mean().item():.2e})")
    for k, (e, e32) in worst.items():
        print(f"  {k:50s} HIP {e:.2e}  plain fp32 {e32:.2e}")
    if zeros_exact:
        worst["exact zeros"] = n_zero
        print(f"  exact zeros among the parameter gradients: {n_zero}")
    return valid, knn, q_vis, flip, worst


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_backward_per_sample_against_fp64(env, variant):
    """IG (all nine tensors), Ys (every layer), Xs (every slot) and the block's parameter gradients against fp64 autograd, sample by sample:
    real rays at the training configuration (valid and invalid samples), points around both hands, and hand-placed points at the border of
    the source view (eps band, pixel-weight ramp), at z = -1 and z = 1, at the foreground-mask edge; q_vis 0 and 1, nearest vertices on the
    other hand and with vert_vis = 0.  eval_func's derivative inside the backward: d only, d + noise, d + d2 + noise + noise2 (the coarse
    samples inside a fine batch).  Invalid samples: exact zeros in the geometry branch's IG and in the sdf / alpha rows of the head's Ys."""
    HB, R, sd, frame, fdat, w0 = env
    pts = _points(R, frame, fdat)
    valid, knn, q_vis, flip, _ = check_block_against_fp64(env, pts, variant)
    nn_vis = fdat.vert_vis.cpu()[knn]
    # the edges are there: both validities, both q_vis, the other hand, invisible nearest vertices
    assert 0.2 < valid.float().mean() < 0.9 and bool(q_vis.any()) and not bool(q_vis.all())
    assert bool((knn >= orc.NUM_V).any()) and bool((knn < orc.NUM_V).any()) and bool((nn_vis == 0).any()) and bool((nn_vis[valid] == 0).any())


def test_noise_at_the_relu_kink_and_invalid_samples(env):
    """eval_func's alpha = mask relu(rad + noise): with noise = -rad exactly the kernel passes no gradient to rad (its test is `> 0`, as is
    torch's relu backward at 0), and neither does the fp64 oracle given its own -rad; an invalid sample passes none to sdf_pred and rad
    whatever its noise, while its colour gradient goes through."""
    HB, R, sd, frame, fdat, w0 = env
    pts = _points(R, frame, fdat, n_rays=(4, 4))
    n = pts.shape[0]
    g = torch.Generator().manual_seed(9)
    d = torch.randn(n, 5, generator=g)
    noise = 0.05 * torch.randn(n, generator=g)
    q_sdf, q_vis, knn = _queries(R, fdat, pts)
    ws = HB.Workspace(n, "cuda")
    HB.run_block(ws, w0, fdat, pts.cuda(), q_sdf, q_vis, knn, d.cuda(), noise.cuda())
    rad_k = ws.raw[:n, 1].cpu().clone()
    ref0 = reference(sd, frame, pts, q_sdf.cpu(), q_vis.cpu(), fdat.vert_vis.cpu())
    kink = torch.arange(n) % 3 == 0
    noise_k = torch.where(kink, -rad_k, noise)
    noise_o = torch.where(kink, -ref0["raw"][:, 1], noise.double())
    ws, ig, ref, flip, _, _, r32 = _run(HB, R, env, pts, d, noise_k, ws=ws, oracle_noise={"noise": noise_o})
    valid = ref["valid"]
    head = HB.layout()["layers"][14]
    ys = ws.ys[head["y_row"]:head["y_row"] + 2, :n].cpu()
    at = kink & valid & ~flip
    assert int(at.sum()) > 50
    assert torch.equal(ys[1, at], torch.zeros(int(at.sum()))) and torch.equal(ref["d_y"]["mlp_geo.layers2.layers.2.linear"][at, 1], torch.zeros(int(at.sum()), dtype=torch.float64))
    assert (ys[0, at] != 0).all()  # (the sdf row still carries d)
    assert torch.equal(ys[:, ~valid], torch.zeros(2, int((~valid).sum())))
    tex = HB.layout()["layers"][19]
    assert (ws.ys[tex["y_row"]:tex["y_row"] + 3, :n].cpu()[:, ~valid & ~flip] != 0).any(0).all()
    worst = {}
    _check("head", ws.ys[head["y_row"]:head["y_row"] + 2, :n].cpu().t(), ref["d_y"]["mlp_geo.layers2.layers.2.linear"],
           r32["d_y"]["mlp_geo.layers2.layers.2.linear"], worst)
    for k in IG_NAMES:
        _check(k, ig[k], ref["d_gathered"][k], r32["d_gathered"][k], worst)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1000, 4097])
def test_tails_and_workspace_reuse(env, n):
    """Blocks whose n is not a multiple of 32, run in a fresh workspace of their own size and in a 65 536-sample workspace (the compact-spill
    path of run_block) after a full block has left its data there and after the workspace was filled with NaN: the same bits everywhere,
    Ys[:, n:npad] exactly zero (the backward writes every column < npad and the weight products read them), a finite dw -- and the same bits
    as those samples inside a full block of 4 128 (the chain is a pure function of the sample)."""
    HB, R, sd, frame, fdat, w0 = env
    pts = _points(R, frame, fdat)[:4128].cuda()
    q_sdf, q_vis, knn = _queries(R, fdat, pts)
    d = torch.randn(pts.shape[0], 5, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    noise = 0.05 * torch.randn(pts.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    npad = (n + 31) // 32 * 32
    args = lambda m: (pts[:m], q_sdf[:m], q_vis[:m], knn[:m], d[:m], noise[:m])

    def run(ws, m):
        npad = (m + 31) // 32 * 32
        ws.dw.zero_()
        ig, _ = HB.run_block(ws, w0, fdat, *args(m))
        ys = ws.ys.view(-1)[:ws.ys.shape[0] * npad].view(ws.ys.shape[0], npad) if ws.block != npad else ws.ys
        return ys[:, :npad].clone(), {k: v.clone() for k, v in ig.items()}, ws.dw.view(ws.slices, -1).sum(0).clone()

    full = HB.Workspace(4128, "cuda")
    ys_full, ig_full, _ = run(full, 4128)
    fresh = run(HB.Workspace(n, "cuda"), n)
    big = HB.Workspace(65536, "cuda")
    ws_pts = _points(R, frame, fdat, n_rays=(32, 32))[:65536].cuda()
    s2, v2, k2 = _queries(R, fdat, ws_pts)
    HB.run_block(big, w0, fdat, ws_pts, s2, v2, k2, torch.randn(ws_pts.shape[0], 5, device="cuda"))  # stale data of a full block
    stale = run(big, n)
    for t in (big.xs, big.aux, big.ys, big.ig, big.raw):
        t.fill_(float("nan"))
    nan = run(big, n)
    torch.cuda.synchronize()
    for other in (stale, nan):
        assert torch.equal(other[0], fresh[0])
        for k in fresh[1]:
            assert torch.equal(other[1][k], fresh[1][k]), k
        assert torch.equal(other[2], fresh[2])
    assert torch.equal(fresh[0][:, n:], torch.zeros_like(fresh[0][:, n:]))
    assert torch.isfinite(fresh[2]).all() and torch.isfinite(fresh[0]).all()
    assert torch.equal(fresh[0][:, :n], ys_full[:, :n])
    for k in fresh[1]:
        assert torch.equal(fresh[1][k], ig_full[k][:n]), k


def test_forward_spill_raw_outputs_equal_the_inference_kernel(env):
    """raw / valid of vanerf_query_forward_spill against the fp32 inference kernel (query_samples, raw outputs) on the same points: the same
    template, so the same bits -- valid flags, colour everywhere, sdf_pred / rad on valid samples."""
    HB, R, sd, frame, fdat, w0 = env
    pts = _points(R, frame, fdat).cuda()
    n = pts.shape[0]
    q_sdf, q_vis, knn = _queries(R, fdat, pts)
    ws = HB.Workspace(n, "cuda")
    HB.run_block(ws, w0, fdat, pts, q_sdf, q_vis, knn, torch.zeros(n, 5, device="cuda"))
    raw, valid = R.query_samples(w0, fdat, pts, q_sdf, q_vis, knn, want_valid=True, raw=True)
    torch.cuda.synchronize()
    v = valid.bool()
    assert torch.equal(ws.valid[:n], valid)
    assert torch.equal(ws.raw[:n, 2:], raw[:, 2:])
    assert torch.equal(ws.raw[:n][v], raw[v])


@pytest.mark.parametrize("C", [64, 8, 29])
@pytest.mark.parametrize("hw", [64, 128, 181, 256])
def test_scatter_add_taps(hw, C):
    """vanerf_scatter_add_taps (the backward of the bilinear pixel-tap gathers) against an fp64 index_add of the four weighted taps: channel
    counts of the three maps, map sizes where the LDS channel slice changes (64 x 64: 8 channels, 128 x 128: 2, 181 x 181: 1, just under the
    32 768-row limit; 256 x 256: the index_add_ fallback), a slice of the tap tables starting past 0 (the kernel addresses [4][ld] with
    ld = N > n), taps on the border (x0 == x1 or y0 == y1: two taps on one row), zero weights (coordinates on the pixel grid), heavy
    duplication, rows read in place from wider rows (29 of 32 floats), accumulation into a non-zero table."""
    from vanerf_amd import hip_backward as HB, renderer as R
    g = torch.Generator(device="cuda").manual_seed(hw * 100 + C)
    N, start, n = 90001, 7777, 70001
    xy = torch.rand(N, 2, device="cuda", generator=g) * 2.2 - 1.1  # beyond [-1, 1]: clamped onto the border
    xy[start:start + 5000] = xy[start:start + 20].repeat(250, 1)  # duplication
    grid = torch.randint(0, hw, (N, 2), device="cuda", generator=g).float() / (hw - 1) * 2 - 1
    xy[start + 5000:start + 10000] = grid[:5000]  # on the pixel grid: three of four weights exactly zero
    xy[start + 10000:start + 11000, 0] = 1.0  # last column: x1 == x0
    xy[start + 11000:start + 12000, 1] = -1.0  # first row, the weight of the second row zero
    xy[start + 12000:start + 13000] = torch.tensor([1.0, 1.0], device="cuda")  # corner: four taps on one row
    idx4, w4 = HB._taps(xy, hw, hw)
    assert idx4.shape == (4, N)
    wide = torch.randn(n, 32, device="cuda", generator=g)
    vals = wide[:, :C] if C <= 32 else torch.randn(n, C, device="cuda", generator=g)
    base = torch.randn(hw * hw, C, device="cuda", generator=g)
    sl = slice(start, start + n)
    want = base.double()
    for k in range(4):
        want = want.index_add(0, idx4[k, sl].long(), vals.double() * w4[k, sl].double()[:, None])
    got = R.scatter_add_taps(base.clone(), idx4, w4, sl, vals)
    torch.cuda.synchronize()
    err = (got.double() - want).abs().max().item()
    assert err <= 1e-5 * (1.0 + want.abs().max().item()), (hw, C, err)
    assert ((idx4[0, sl] == idx4[1, sl]).any() and (idx4[0, sl] == idx4[2, sl]).any() and (w4[:, sl] == 0).any())
