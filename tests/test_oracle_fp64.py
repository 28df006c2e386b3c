"""The CPU oracle's per-sample path in float64, and the hooks the per-sample tests of the fused backward read (tests/test_backward_per_sample.py).

`orc.query` keeps the dtype of its inputs: fp64 weights, frame and features give an fp64 reference of the per-sample networks, with the
same discrete inputs (knn1, q_sdf, q_vis) as in fp32.  Its `want["layers"]` / `want["gathered"]` hooks expose every layer's input and
pre-activation output and the gathered inputs whose gradients the kernel spills (IG); this file proves they mean what those tests assume."""
import pytest
import torch

from oracle import vanerf_oracle as orc
from tests.oracle_criterion import cast  # noqa: F401  (re-exported: tests/test_oracle_posed.py and the per-sample tests import it from here)
from vanerf_amd import synth
from vanerf_amd.hip_backward import LAYER_PARAMS

IG_WIDTHS = {"pix0": 64, "nn0": 64, "tw0": 64, "pix1": 8, "nn1": 8, "tw1": 8, "row_nn": 29, "row_tw": 29, "tex_xy": 8}
IG_NAMES = tuple(IG_WIDTHS)
# layers followed by a ReLU (the others: softplus, sigmoid gates or nothing)
RELU_LAYERS = ("geo_vis_fusion.fconv_at.0.weight", "geo_vis_fusion.fconv_ated.0.weight", "geo_vis_fusion.fconv_at1.0.weight",
               "geo_vis_fusion.fconv_ated1.0.weight", "tex_vis_fusion.fconv_at.0.weight", "tex_vis_fusion.fconv.0.weight")


def param_keys(spec):
    kind, name = spec
    return [name] if kind == "conv" else [name + ".weight", name + ".bias"] if kind == "lin" else [name + s for s in (".weight_v", ".weight_g", ".bias")]


def reference(sd, frame, pts, q_sdf, q_vis, vert_vis, d=None, noise=None, d2=None, noise2=None, dtype=torch.float64, shift=None):
    """The oracle's per-sample networks on CPU in `dtype`, n points (n, 3): raw (n, 5) [sdf_pred, rad, r, g, b], valid (n,) bool, the hooks
    (layers: name -> (X (n, kin), Y (n, n_out)); gathered: name -> (n, C)) and, given d (n, 5), the gradients of the loss
    sum(eval_func(raw, noise) d) [+ sum(eval_func(raw, noise2) d2)] with respect to the gathered inputs (d_gathered), every layer's output
    (d_y) and the per-sample networks' parameters (d_params).  q_sdf (n,), q_vis (n,) bool / uint8, vert_vis (NV,) {0, 1}."""
    n = pts.shape[0]
    sdx = {k: v.detach().to(dtype).requires_grad_(k in {p for s in LAYER_PARAMS for p in param_keys(s)}) if v.is_floating_point() else v
           for k, v in sd.items()}
    fr = cast(frame, dtype)
    view = torch.nn.functional.normalize(torch.ones(1, n, 3, dtype=dtype), dim=-1)  # (the IBR head is value-dead at one view)
    if shift is None:  # zero shifts: the gradient with respect to a gathered input (a feature map or a table that needs none, here)
        shift = {k: torch.zeros(1, n, c, dtype=dtype, requires_grad=d is not None) for k, c in IG_WIDTHS.items()}
    want = {"shift": shift}
    with torch.enable_grad():
        raw, valid = orc.query(sdx, pts.detach().to(dtype)[None], fr["cam_in"], fr["targets"], fr["feat_geo"], fr["feat_tex"],
                               vert_vis.reshape(1, -1, 1).float(), q_vis.reshape(1, n, 1).bool(), q_sdf.reshape(1, n).to(dtype),
                               fr["sp_data"], fr["img_in"], view, fr["src_foreground_mask"], want=want)
        out = {"raw": raw.detach()[0], "valid": valid[0, :, 0].bool(), "sdx": sdx,
               "layers": {k: (x.detach().reshape(n, -1), y.detach().reshape(n, -1)) for k, (x, y) in want["layers"].items()},
               "gathered": {k: v.detach().reshape(n, -1) for k, v in want["gathered"].items()}}
        if d is None:
            return out
        nml = frame["cam_in"]["nml_scale"]
        loss = (orc.eval_func(sdx, raw, valid, nml, noise=None if noise is None else noise.to(dtype).reshape(1, n, 1))[0] * d.to(dtype)).sum()
        if d2 is not None:
            loss = loss + (orc.eval_func(sdx, raw, valid, nml, noise=None if noise2 is None else noise2.to(dtype).reshape(1, n, 1))[0] * d2.to(dtype)).sum()
        gk = list(IG_NAMES)
        lk = [s[1] for s in LAYER_PARAMS]
        pk = [p for s in LAYER_PARAMS for p in param_keys(s)]
        grads = torch.autograd.grad(loss, [shift[k] for k in gk] + [want["layers"][k][1] for k in lk] + [sdx[k] for k in pk],
                                    allow_unused=True)
    z = lambda g, t: torch.zeros_like(t) if g is None else g
    out["d_gathered"] = {k: z(g, want["gathered"][k]).reshape(n, -1) for k, g in zip(gk, grads[:len(gk)])}
    out["d_y"] = {k: z(g, want["layers"][k][1]).reshape(n, -1) for k, g in zip(lk, grads[len(gk):len(gk) + len(lk)])}
    out["d_params"] = {k: z(g, sdx[k]) for k, g in zip(pk, grads[len(gk) + len(lk):])}
    return out


def frame_and_points(n=600, seed=3):
    """A small synthetic frame and n points around its mesh (some off the source view), with the oracle's mesh queries."""
    frame = synth.make_frame(seed=seed, tar_h=64, tar_w=64, half_mask=True)
    g = torch.Generator().manual_seed(seed)
    v = frame["targets"]["vert_world"][0]
    pts = v[torch.randint(0, v.shape[0], (n,), generator=g)] + 0.012 * torch.randn(n, 3, generator=g)
    pts[: n // 20] += torch.tensor([0.5, 0.0, 0.0])  # off the source view: invalid samples
    verts = frame["targets"]["vert_world"]
    xy01, z01 = orc.source_vert_xyz01(verts, frame["cam_in"])
    q_sdf, q_vis, vert_vis, _ = orc.cal_vis_sdf_batch(verts, frame["targets"]["face_world"].long(), pts[None], xy01, z01)
    return frame, pts, q_sdf[0], q_vis[0, :, 0], vert_vis[0, :, 0]


@pytest.fixture(scope="module")
def case():
    sd = synth.make_full_weights(0)
    frame, pts, q_sdf, q_vis, vert_vis = frame_and_points()
    g = torch.Generator().manual_seed(1)
    n = pts.shape[0]
    d, d2 = torch.randn(n, 5, generator=g), torch.randn(n, 5, generator=g)
    noise, noise2 = 0.05 * torch.randn(n, generator=g), 0.05 * torch.randn(n, generator=g)
    return sd, frame, pts, q_sdf, q_vis, vert_vis, d, d2, noise, noise2


def test_fp64_and_fp32_oracle_agree(case):
    """The same per-sample pass in fp64 and fp32: same validity, raw outputs and every hooked tensor within fp32 accuracy (observed: raw
    outputs within 2e-6, layer outputs within 2e-5 of the layer's largest value), and the hooks cover every layer of LAYER_PARAMS and
    every IG tensor with the kernel's widths."""
    sd, frame, pts, q_sdf, q_vis, vert_vis = case[:6]
    r64 = reference(sd, frame, pts, q_sdf, q_vis, vert_vis)
    r32 = reference(sd, frame, pts, q_sdf, q_vis, vert_vis, dtype=torch.float32)
    assert r64["raw"].dtype == torch.float64 and r32["raw"].dtype == torch.float32
    assert all(x.dtype == torch.float64 and y.dtype == torch.float64 for x, y in r64["layers"].values())
    assert torch.equal(r64["valid"], r32["valid"]) and 0.2 < r64["valid"].float().mean() < 0.9
    assert (r32["raw"].double() - r64["raw"]).abs().max() <= 1e-5
    assert sorted(r64["layers"]) == sorted(s[1] for s in LAYER_PARAMS)
    assert {k: v.shape[1] for k, v in r64["gathered"].items()} == IG_WIDTHS
    for k in r64["layers"]:
        for a, b in zip(r32["layers"][k], r64["layers"][k]):
            assert (a.double() - b).abs().max() <= 1e-4 * b.abs().max() + 1e-7, k
    for k in IG_NAMES:  # (bilinear taps of a map in [-1, 1]: fp32 coordinates x 63.5 pixels on the 128 x 128 map -> 2.3e-5 observed)
        assert (r32["gathered"][k].double() - r64["gathered"][k]).abs().max() <= 1e-4, k


def test_gradcheck_with_respect_to_the_gathered_inputs(case):
    """torch.autograd.gradcheck of the fp64 per-sample networks (through eval_func with noise, both sets of draws) with respect to all nine
    gathered inputs of a handful of samples, valid and invalid, added through the `shift` hook."""
    sd, frame, pts, q_sdf, q_vis, vert_vis, d, d2, noise, noise2 = case
    valid = reference(sd, frame, pts, q_sdf, q_vis, vert_vis)["valid"]
    sel = torch.cat([(~valid).nonzero()[:2, 0], valid.nonzero()[::90, 0][:4]])  # two invalid samples, four valid ones
    base = reference(sd, frame, pts[sel], q_sdf[sel], q_vis[sel], vert_vis)
    assert not base["valid"][:2].any() and base["valid"][2:].all() and len(sel) == 6
    sh = [torch.zeros(len(sel), v.shape[1], dtype=torch.float64, requires_grad=True) for v in base["gathered"].values()]
    names = list(base["gathered"])
    nml = frame["cam_in"]["nml_scale"]

    def g(*shifts):  # (reference() detaches its outputs: the same call, differentiable)
        sdx, fr = cast(sd, torch.float64), cast(frame, torch.float64)
        n = len(sel)
        view = torch.nn.functional.normalize(torch.ones(1, n, 3, dtype=torch.float64), dim=-1)
        raw, valid = orc.query(sdx, pts[sel].double()[None], fr["cam_in"], fr["targets"], fr["feat_geo"], fr["feat_tex"],
                               vert_vis.reshape(1, -1, 1).float(), q_vis[sel].reshape(1, n, 1).bool(), q_sdf[sel].reshape(1, n).double(),
                               fr["sp_data"], fr["img_in"], view, fr["src_foreground_mask"],
                               want={"shift": {k: s[None] for k, s in zip(names, shifts)}})
        return (orc.eval_func(sdx, raw, valid, nml, noise=noise[sel].double().reshape(1, n, 1)) * d[sel].double()
                + orc.eval_func(sdx, raw, valid, nml, noise=noise2[sel].double().reshape(1, n, 1)) * d2[sel].double())

    assert torch.autograd.gradcheck(g, tuple(sh), eps=1e-6, atol=1e-7, rtol=1e-5, fast_mode=True)


@pytest.mark.parametrize("variant", ["d", "d_noise", "d_d2_noise"])
def test_hooks_reproduce_the_parameter_gradients(case, variant):
    """For every layer, sum over the samples of dY (x) X from the hooks -- what the kernel's weight products compute from its Ys / Xs spills --
    reproduces the oracle's own autograd gradient of that layer's parameters (conv weight; Linear weight and bias; weight-norm v and g
    through the fold), and the gathered inputs' gradients are what the forward reads (invalid samples: no gradient into the geometry branch)."""
    sd, frame, pts, q_sdf, q_vis, vert_vis, d, d2, noise, noise2 = case
    kw = {"d": {"d": d}, "d_noise": {"d": d, "noise": noise}, "d_d2_noise": {"d": d, "noise": noise, "d2": d2, "noise2": noise2}}[variant]
    r = reference(sd, frame, pts, q_sdf, q_vis, vert_vis, **kw)
    for kind, name in LAYER_PARAMS:
        x, _ = r["layers"][name]
        dy = r["d_y"][name]
        dw = dy.t() @ x  # (n_out, kin)
        gp = r["d_params"]
        scale = lambda t: 1e-10 * (1.0 + t.abs().max().item())
        if kind == "conv":
            assert (dw - gp[name][:, :, 0]).abs().max() <= scale(gp[name]), name
            continue
        db = dy.sum(0)
        assert (db - gp[name + ".bias"]).abs().max() <= scale(gp[name + ".bias"]), name
        if kind == "lin":
            assert (dw - gp[name + ".weight"]).abs().max() <= scale(gp[name + ".weight"]), name
            continue
        v = r["sdx"][name + ".weight_v"].detach().requires_grad_(True)
        gg = r["sdx"][name + ".weight_g"].detach().requires_grad_(True)
        with torch.enable_grad():
            gv, g_g = torch.autograd.grad(v * (gg / v.norm(2, dim=1, keepdim=True)), [v, gg], dw)
        assert (gv - gp[name + ".weight_v"]).abs().max() <= scale(gp[name + ".weight_v"]), name
        assert (g_g - gp[name + ".weight_g"]).abs().max() <= scale(gp[name + ".weight_g"]), name
    inv = ~r["valid"]
    assert inv.any()
    for k in ("pix0", "nn0", "tw0", "pix1", "nn1", "tw1"):
        assert torch.equal(r["d_gathered"][k][inv], torch.zeros_like(r["d_gathered"][k][inv])), k
        assert r["d_gathered"][k][~inv].abs().max() > 0, k
    for k in ("mlp_geo.layers2.layers.2.linear",):  # eval_func: an invalid sample's sdf and alpha pass nothing back
        assert torch.equal(r["d_y"][k][inv], torch.zeros_like(r["d_y"][k][inv]))
    assert r["d_gathered"]["row_nn"][inv].abs().max() > 0  # (the colour does)
