"""Training step under autograd (first stage): HIP values, PyTorch-graph gradients.
The gradients are checked against the CPU oracle differentiated by torch.autograd at the same sample points."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vanerf_oracle as orc  # noqa: E402
from vanerf_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _net(noise):
    from vanerf_amd.config import default_config
    from vanerf_amd.model import VANeRF
    torch.manual_seed(0)
    cfg = default_config()
    cfg["models"]["VANeRF"].update(train_out_h=8, train_out_w=8)
    cfg["models"]["VANeRF"]["dr_kwargs"].update(sample_per_ray_c=8, sample_per_ray_f=8, rand_noise_std=noise, uniform=False, fine=True)
    net = VANeRF(cfg).cuda().train()
    net.load_state_dict(synth.make_full_weights(0), strict=False)
    net._keep_last_pass = True
    return net


def _step(net, frame):
    dr = {"img": frame["img_in"], "cam": frame["cam_in"], "cam_tar": frame["cam_tar"], "tar": torch.rand(1, 3, 64, 64, device="cuda"),
          "msk": torch.ones(1, 1, 64, 64, device="cuda")}
    return net(frame["img_in"], frame["cam_in"], frame["hand_type"], frame["targets"], None, None, n_views=1, sp_data=dict(frame["sp_data"]),
               dr_data=dr, src_foreground_mask=frame["src_foreground_mask"], bounds=frame["bounds"])["out"]["nerf"]


KEYS = ("tex_fg", "depth", "alpha", "tex_fg_fine", "depth_fine", "alpha_fine", "sdf")


@pytest.mark.parametrize("noise", [0.01, 0.0])
def test_training_step_values_and_gradients(noise):
    net = _net(noise)
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=64, tar_w=64), "cuda")
    # feature maps as leaves, so that their gradients can be compared (the encoders are ordinary torch modules behind them)
    fg = [f.clone().requires_grad_() for f in frame["feat_geo"]]
    ft = frame["feat_tex"].clone().requires_grad_()
    net.attach_geo_feat = lambda im, return_val=False: fg
    net.attach_tex_feat = lambda im, return_val=False: ft
    out = _step(net, frame)
    g = torch.Generator().manual_seed(1)
    rnd = {k: torch.randn(out[k].shape, generator=g) for k in KEYS}
    loss = sum((out[k] * rnd[k].cuda()).sum() for k in KEYS)
    assert all(out[k].requires_grad for k in KEYS)
    loss.backward()
    o, fd, cam_in = net._last_pass
    # ---- the same quantities from the CPU oracle under autograd, at the samples of the HIP pass ---------------------------------
    sd = {k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point) for k, v in net.state_dict().items()
          if not k.startswith(("geo_encoder.", "tex_encoder."))}
    cpu = synth.to_device(frame, "cpu")
    fgc = [f.detach().cpu().clone().requires_grad_() for f in fg]
    ftc = ft.detach().cpu().clone().requires_grad_()
    vert_vis = fd.vert_vis.cpu()[None, :, None]

    def oracle_pass(c, z):
        pts = c["pts"].cpu()
        qs, qv = c["q_sdf"].reshape(1, -1).cpu(), c["q_vis"].cpu().float().view(1, -1, 1)
        view = torch.nn.functional.normalize(torch.ones_like(pts), dim=-1)[None]
        rgba, valid = orc.query(sd, pts[None], cpu["cam_in"], cpu["targets"], fgc, ftc, vert_vis, qv, qs, cpu["sp_data"], cpu["img_in"], view,
                                cpu["src_foreground_mask"])
        nz = None if c["noise"] is None else c["noise"].cpu().view(1, -1, 1)
        rgba = orc.eval_func(sd, rgba, valid, cpu["cam_in"]["nml_scale"], nz).view(1, z.shape[0], -1, 5)
        return orc.rgba2out(sd, rgba, z.cpu()[None], c["q_sdf"].cpu()[None, ..., None])

    col, dep, acc, _, _ = oracle_pass(o["coarse"], o["z"])
    ref = {"tex_fg": col.view(1, 8, 8, 3).permute(0, 3, 1, 2), "depth": dep.view(1, 8, 8), "alpha": acc.view(1, 8, 8)}
    if noise > 0.0:
        # The HIP pass evaluates the networks once per point and applies eval_func twice to the coarse points (their draws in the coarse pass,
        # their draws inside the fine batch).  The oracle does what the reference does: every one of the Sc + Sf sorted samples of the fine
        # batch is evaluated again, with the draw it holds at its sorted position -- rebuilt here from the pass's origin map.
        c_, f_, cf_, src = o["coarse"], o["fine"], o["coarse_in_fine"], o["fine_src"].long()
        assert cf_ is not None and f_["pts"].shape[0] == c_["pts"].shape[0]
        Rr, Sc_ = o["z"].shape
        take = torch.where(src >= 0, src, Sc_ + (-src - 1))
        both = lambda a, b, w: torch.gather(torch.cat([a.reshape(Rr, Sc_, *w), b.reshape(Rr, -1, *w)], 1), 1,
                                            take.view(Rr, -1, *([1] * len(w))).expand(-1, -1, *w))
        merged = {"pts": both(c_["pts"], f_["pts"], (3,)).reshape(-1, 3), "q_sdf": both(c_["q_sdf"], f_["q_sdf"], ()),
                  "q_vis": both(c_["q_vis"], f_["q_vis"], ()).reshape(-1), "noise": both(cf_["noise"], f_["noise"], ()).reshape(-1)}
        colf, depf, accf, _, sdff = oracle_pass(merged, o["z_fine"])
        ref.update({"tex_fg_fine": colf.view(1, 8, 8, 3).permute(0, 3, 1, 2), "depth_fine": depf.view(1, 8, 8), "alpha_fine": accf.view(1, 8, 8),
                    "sdf": sdff.view(1, 8, 8)})
    keys = tuple(ref)
    for k in keys:  # values: HIP (what forward returned) against the oracle
        assert (out[k].detach().cpu() - ref[k].detach()).abs().max() <= 1e-4, k
    if noise == 0.0:
        return  # (with re-use the oracle comparison above covers the coarse outputs; the gradient check runs on the noise case)
    sum((ref[k] * rnd[k]).sum() for k in keys).backward()
    checked, worst = 0, {}
    named = dict(net.named_parameters())
    for k, v in sd.items():
        if v.grad is None or k.startswith("mlp_tex."):
            continue
        got = named[k].grad
        assert got is not None, k
        rel = ((got.cpu() - v.grad).norm() / (v.grad.norm() + 1e-12)).item()
        # the per-frame conv / LayerNorm stacks over 256x256 and 64x64 maps run on MIOpen here and on the CPU in the oracle: their
        # gradients are sums over 4e3..6e4 positions and agree to a few per cent; the per-sample networks agree to a few 1e-3
        # (1 536 samples here: one ReLU on the other side of its kink moves a gradient by ~1e-3)
        per_frame = k.startswith(("tex_vis_fusion.fconv3", "tex_vis_fusion.fconv4", "tex_vis_fusion.fconv_gt"))
        worst["frame" if per_frame else "sample"] = max(worst.get("frame" if per_frame else "sample", 0.0), rel)
        assert rel <= (5e-2 if per_frame else 1e-2), (k, rel)  # a wiring error gives O(1)
        checked += 1
    print("relative L2 error of the parameter gradients (worst):", worst)
    assert checked >= 30
    for a, b in zip(fg + [ft], fgc + [ftc]):
        assert (a.grad.cpu() - b.grad).norm() <= 5e-2 * b.grad.norm()  # feat_tex also feeds the per-frame stacks


def test_inference_is_unchanged_by_the_autograd_path():
    """eval / no_grad calls never touch torch_graph: forward() under no_grad gives plain tensors."""
    net = _net(0.0).eval()
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=64, tar_w=64), "cuda")
    f3 = frame
    net.attach_geo_feat = lambda im, return_val=False: f3["feat_geo"]
    net.attach_tex_feat = lambda im, return_val=False: f3["feat_tex"]
    with torch.no_grad():
        out = _step(net, frame)
    assert not out["tex_fg_fine"].requires_grad


def test_training_step_under_detect_anomaly():
    """The reference trains with Trainer(detect_anomaly=True): forward + backward through both encoders, the per-frame stacks and the
    per-sample networks must raise nothing, every parameter that receives a gradient receives a finite one, and an Adam step moves them."""
    net = _net(0.01)
    frame = synth.to_device(synth.make_frame(seed=5, tar_h=64, tar_w=64), "cuda")
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    with torch.autograd.detect_anomaly():
        out = _step(net, frame)
        loss = sum(out[k].square().mean() for k in KEYS)
        assert torch.isfinite(loss)
        loss.backward()
    with_grad = {k: p for k, p in net.named_parameters() if p.grad is not None}
    assert all(torch.isfinite(p.grad).all() for p in with_grad.values())
    for prefix in ("geo_encoder.", "tex_encoder.", "geo_vis_fusion.", "mlp_geo.", "tex_vis_fusion.", "ibr_compress_gfeat.", "sigmoid_beta"):
        assert any(k.startswith(prefix) and p.grad.abs().sum() > 0 for k, p in with_grad.items()), prefix
    opt.step()
    assert sum(int(not torch.equal(before[k], p.detach())) for k, p in with_grad.items()) >= 0.9 * len(with_grad)


def _grads_of_a_step(net, frame, seed=3):
    import numpy as np
    torch.manual_seed(seed)
    np.random.seed(seed)
    out = _step(net, frame)
    g = torch.Generator().manual_seed(1)
    sum((out[k] * torch.randn(out[k].shape, generator=g).cuda()).sum() for k in KEYS).backward()
    return {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}


def _compare_backends(a, b, rel, cos_min):
    """Every parameter: same set with a gradient; relative L2 and cosine per tensor.  mlp_tex (the IBR head, value-dead at one view) gets none."""
    assert set(a) == set(b)
    worst = (0.0, 1.0)
    gmax = max(v.norm().item() for v in a.values() if v is not None)  # noise floor of a sum over all samples: relative to the largest gradient
    for k in a:
        if k.startswith("mlp_tex."):
            assert (a[k] is None or float(a[k].abs().max()) == 0.0) and (b[k] is None or float(b[k].abs().max()) == 0.0), k
            continue
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is None:
            continue
        na, nb = a[k].norm().item(), b[k].norm().item()
        diff = (a[k] - b[k]).norm().item()
        assert diff <= rel * max(na, nb) + 1e-4 + 1e-5 * gmax, (k, diff, na, nb, gmax)
        if max(na, nb) < 1e-2 + 1e-3 * gmax:  # (a bias in front of a normalisation layer has a zero gradient up to rounding noise: no direction to compare)
            continue
        r, c = diff / max(na, nb), float((a[k] * b[k]).sum() / (na * nb))
        worst = (max(worst[0], r), min(worst[1], c))
        assert c >= cos_min, (k, r, c)
    return worst


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_hip_backward_matches_the_pytorch_graph(precision):
    """Row f-4: the fused HIP backward (csrc/query_backward.hip + hip_backward.py: forward spill, dX = W^T dY chain in registers, one matrix
    product per layer for dW, HIP scatters for the gathers) against the PyTorch graph of torch_graph.networks_at on the same training step --
    an independent second implementation differentiated by torch.autograd.  Both forward precisions (values from the bf16x3 or the fp32
    kernel; the gradient always runs in fp32)."""
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=64, tar_w=64), "cuda")
    res = []
    for hip in (True, False):
        net = _net(0.01)
        net.precision = precision
        net.kwargs["hip_backward"] = hip
        res.append(_grads_of_a_step(net, frame))
    worst = _compare_backends(res[0], res[1], 2e-3, 0.9999)
    print(f"HIP backward vs PyTorch graph [{precision}]: worst relative L2 {worst[0]:.2e}, worst cosine {worst[1]:.6f}")


def test_the_clamp_of_sigmoid_beta_in_the_step():
    """sdf_activation clamps sigmoid_beta at 2e-3.  The torch stage gets the clamp's derivative from torch.clamp itself, the HIP stage applies it
    on the host to the kernel's d / d clamp(sigmoid_beta) (pass_gradient._composite_gradients_hip): below the clamp both give exactly 0 and every
    other gradient agrees as in test_hip_backward_matches_the_pytorch_graph (the composites run at 1 / beta^2 = 2.5e5); above it the two
    gradients of sigmoid_beta agree within that test's bar."""
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=64, tar_w=64), "cuda")

    def both_backends(beta):
        res = []
        for hip in (True, False):
            net = _net(0.01)
            with torch.no_grad():
                net.sigmoid_beta.fill_(beta)
            net.kwargs["hip_backward"] = hip
            res.append(_grads_of_a_step(net, frame))
            assert float(net.sigmoid_beta) == float(torch.tensor(beta))  # the step left the parameter where it was: below the clamp
        return res

    below = both_backends(1e-3)
    for g, name in zip(below, ("hip", "torch")):
        assert g["sigmoid_beta"] is not None and torch.equal(g["sigmoid_beta"], torch.zeros_like(g["sigmoid_beta"])), (name, g["sigmoid_beta"])
    worst = _compare_backends(below[0], below[1], 2e-3, 0.9999)
    print(f"sigmoid_beta = 1e-3 (clamped): worst relative L2 {worst[0]:.2e}, worst cosine {worst[1]:.6f}")
    above = both_backends(0.01)
    a, b = above[0]["sigmoid_beta"], above[1]["sigmoid_beta"]
    print(f"sigmoid_beta = 0.01: d loss / d sigmoid_beta {a.item():.6e} (HIP stage) {b.item():.6e} (torch stage)")
    assert a.abs().item() > 0.0 and b.abs().item() > 0.0
    _compare_backends(above[0], above[1], 2e-3, 0.9999)  # sigmoid_beta among them: |a - b| <= 2e-3 max(|a|, |b|) + 1e-4 + 1e-5 gmax


def test_hip_backward_at_the_real_patch_size():
    """The same comparison at the training configuration of configs/vanerf.json: a 64x64 patch, 64 + 64 samples per ray (524 288 network
    evaluations, eight blocks of 65 536 samples through the HIP backward)."""
    from vanerf_amd.config import default_config
    from vanerf_amd.model import VANeRF
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=256, tar_w=256), "cuda")
    res = []
    for hip in (True, False):
        torch.manual_seed(0)
        cfg = default_config()
        cfg["models"]["VANeRF"]["dr_kwargs"].update(sample_per_ray_c=64, sample_per_ray_f=64, rand_noise_std=0.01, uniform=False, fine=True)
        net = VANeRF(cfg).cuda().train()
        net.load_state_dict(synth.make_full_weights(0), strict=False)
        net.kwargs["hip_backward"] = hip
        dr = {"img": frame["img_in"], "cam": frame["cam_in"], "cam_tar": frame["cam_tar"], "tar": torch.rand(1, 3, 256, 256, device="cuda"),
              "msk": torch.ones(1, 1, 256, 256, device="cuda")}
        import numpy as np
        torch.manual_seed(5)
        np.random.seed(5)
        torch.cuda.reset_peak_memory_stats()
        out = net(frame["img_in"], frame["cam_in"], frame["hand_type"], frame["targets"], None, None, n_views=1, sp_data=dict(frame["sp_data"]),
                  dr_data=dr, src_foreground_mask=frame["src_foreground_mask"], bounds=frame["bounds"])["out"]["nerf"]
        assert out["tex_fg_fine"].shape == (1, 3, 64, 64)
        g = torch.Generator().manual_seed(1)
        sum((out[k] * torch.randn(out[k].shape, generator=g).cuda()).sum() for k in KEYS).backward()
        res.append({k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()})
        print("hip" if hip else "torch", "backward: peak memory", round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "GiB")
        del net, out
    worst = _compare_backends(res[0], res[1], 5e-3, 0.9999)
    print(f"64x64 patch, 64 + 64 samples: worst relative L2 {worst[0]:.2e}, worst cosine {worst[1]:.6f}")


def test_fused_backward_with_torch_composites_beyond_256_samples_per_ray():
    """The mixed branch of the backward: vanerf_composite_backward takes at most 256 samples per ray, so at 136 + 128 samples (264 in the fine
    composite) the composites are differentiated by the torch graph while the per-sample networks stay on the fused HIP backward.  Against the
    PyTorch graph of the same step, with the bounds held at the real patch size (a larger sample count)."""
    from vanerf_amd import hip_backward as HB, renderer as R
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=64, tar_w=64), "cuda")
    calls = {"composite_backward": [], "run_block": [], "hip": None}  # per wrapped function: the hip_backward setting of the step that called it
    orig = {"composite_backward": R.composite_backward, "run_block": HB.run_block}
    res = []
    try:
        R.composite_backward = lambda *a, **k: (calls["composite_backward"].append(calls["hip"]), orig["composite_backward"](*a, **k))[1]
        HB.run_block = lambda *a, **k: (calls["run_block"].append(calls["hip"]), orig["run_block"](*a, **k))[1]
        for hip in (True, False):
            net = _net(0.01)
            net.kwargs["dr_kwargs"].update(sample_per_ray_c=136, sample_per_ray_f=128)
            net.kwargs["hip_backward"] = calls["hip"] = hip
            res.append(_grads_of_a_step(net, frame))
            assert net._last_pass[0]["z_fine"].shape == (64, 264)
    finally:
        R.composite_backward, HB.run_block = orig["composite_backward"], orig["run_block"]
    assert calls["composite_backward"] == [], "the composites of a 264-sample ray go through the torch graph"
    assert calls["run_block"] and all(calls["run_block"]), "the fused per-sample backend ran, and only in the hip_backward step"
    worst = _compare_backends(res[0], res[1], 5e-3, 0.9999)
    print(f"8x8 patch, 136 + 128 samples: worst relative L2 {worst[0]:.2e}, worst cosine {worst[1]:.6f}")


def test_chunked_backward_gives_the_same_gradients():
    """pass_gradient.PassGradient takes the gradient chunk of rays by chunk of rays when `grad_rays_per_chunk` is set, and the second stage of a
    chunk block of samples by block when `grad_samples_per_block` is (bounded memory): the sum over chunks / blocks is the gradient of the
    whole patch (rays and samples are independent; the shared per-frame vertex table is closed once)."""
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=64, tar_w=64), "cuda")
    grads = []
    # 64 rays: one chunk / chunks of 24 + 24 + 16 rays / blocks of 200 samples / both / blocks of 300 samples as replays of one HIP graph
    # ... and the fused HIP backward (the default): whole patch / chunks of rays / blocks of 256 samples / both
    for chunk, block, graph, hip in ((None, None, False, False), (24, None, False, False), (None, 200, False, False), (40, 96, False, False),
                                     (None, 300, True, False), (None, None, False, True), (24, None, False, True), (None, 256, False, True),
                                     (40, 96, False, True)):
        net = _net(0.01)
        net.kwargs["grad_rays_per_chunk"] = chunk
        net.kwargs["grad_samples_per_block"] = block
        net.kwargs["grad_graph_blocks"] = graph
        net.kwargs["hip_backward"] = hip
        if hip and block:
            net.kwargs["hip_backward_block"] = block
        torch.manual_seed(3)
        import numpy as np
        np.random.seed(3)
        out = _step(net, frame)
        g = torch.Generator().manual_seed(1)
        sum((out[k] * torch.randn(out[k].shape, generator=g).cuda()).sum() for k in KEYS).backward()
        grads.append({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert len(grads[0]) > 100
    for other in grads[1:]:
        assert set(grads[0]) == set(other)
        for k in grads[0]:
            # fp32 sums in another order (a wiring error gives O(1)); a bias in front of a normalisation layer has a zero gradient up to rounding noise
            assert (grads[0][k] - other[k]).norm() <= 3e-3 * grads[0][k].norm() + 1e-4, k


def test_geometry_branch_on_valid_samples_only_gives_the_same_gradients():
    """torch_graph.networks_at evaluates GeoVisFusion / positional encoding / geometry MLP only where the pixel weight is non-zero (samples
    inside the source view and foreground mask): the others pool to an exactly-zero latent and are masked by eval_func, so values and
    gradients must equal the graph evaluated on every sample (blocky random foreground mask: about half of the samples drop out)."""
    import numpy as np
    from vanerf_amd import torch_graph as G
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=64, tar_w=64), "cuda")
    blocks = (torch.rand(1, 1, 32, 32, generator=torch.Generator().manual_seed(5)) > 0.5).float()  # foreground in 8x8-pixel blocks
    frame["src_foreground_mask"] = torch.nn.functional.interpolate(blocks, scale_factor=8, mode="nearest").view(1, 1, 1, 256, 256).to(frame["src_foreground_mask"]).contiguous()
    grads, kept = [], []
    orig = G.geometry_mlp
    try:
        G.geometry_mlp = lambda P, pe, fused, weight, **k: (kept.append(pe.shape[0]), orig(P, pe, fused, weight, **k))[1]
        for compact in (False, True):
            G.COMPACT_VALID = compact
            net = _net(0.01)
            net.kwargs["hip_backward"] = False  # (this is about the PyTorch graph; the HIP backward meets the same mask at the end of the test)
            torch.manual_seed(3)
            np.random.seed(3)
            out = _step(net, frame)
            g = torch.Generator().manual_seed(1)
            sum((out[k] * torch.randn(out[k].shape, generator=g).cuda()).sum() for k in KEYS).backward()
            grads.append({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    finally:
        G.COMPACT_VALID, G.geometry_mlp = True, orig
    assert len(kept) == 2 and kept[1] < 0.8 * kept[0], kept  # samples the geometry branch saw: all of the patch's, then the valid ones only
    assert set(grads[0]) == set(grads[1]) and len(grads[0]) > 100
    for k in grads[0]:
        assert (grads[0][k] - grads[1][k]).norm() <= 3e-3 * grads[0][k].norm() + 1e-4, k
    # the fused HIP backward on the same half-masked frame: samples outside the mask have pixel weight 0 and eval_func masks them
    net = _net(0.01)
    hip = {k: v for k, v in _grads_of_a_step(net, frame).items() if v is not None}
    assert set(hip) == set(grads[0])
    for k in grads[0]:
        err = (grads[0][k] - hip[k]).norm().item()
        # (the per-frame conv / LayerNorm stacks amplify the fp32 summation order of the table's gradient: a few 1e-3, as against the oracle above)
        per_frame = k.startswith(("tex_vis_fusion.fconv3", "tex_vis_fusion.fconv4", "tex_vis_fusion.fconv_gt", "tex_encoder.", "geo_encoder."))
        assert err <= (1e-2 if per_frame else 3e-3) * grads[0][k].norm().item() + 1e-4, (k, err, grads[0][k].norm().item())


def test_graphed_encoders_give_the_same_step():
    """Config key `graph_encoders`: both image encoders as HIP graphs (forward and backward captured by torch.cuda.make_graphed_callables).
    The training step must return the same images and leave the same gradients on every parameter, encoders included."""
    import numpy as np
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=64, tar_w=64), "cuda")
    res = []
    for graphed in (False, True):
        net = _net(0.01)
        net.kwargs["graph_encoders"] = graphed
        vals = []
        for it in range(2):  # the second step replays the captured graphs
            torch.manual_seed(3 + it)
            np.random.seed(3 + it)
            net.zero_grad(set_to_none=True)
            out = _step(net, frame)
            g = torch.Generator().manual_seed(1)
            sum((out[k] * torch.randn(out[k].shape, generator=g).cuda()).sum() for k in KEYS).backward()
            vals.append(({k: out[k].detach().clone() for k in KEYS}, {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}))
        assert net._encoders_graphed == graphed
        net.eval()  # eval-mode calls take the encoders' eager path (the graphs hold the training-mode computation)
        with torch.no_grad():
            vals.append([f.clone() for f in net.attach_geo_feat(frame["img_in"], return_val=True)] + [net.attach_tex_feat(frame["img_in"], return_val=True).clone()])
        res.append(vals)
    for fa, fb in zip(res[0][2], res[1][2]):
        assert (fa - fb).abs().max() <= 2e-3 * fa.abs().max(), "eval-mode feature maps after graphed training steps"
    for it in range(2):
        (out_a, grad_a), (out_b, grad_b) = res[0][it], res[1][it]
        for k in KEYS:
            assert (out_a[k] - out_b[k]).abs().max() <= 2e-4, (it, k)  # (MIOpen may pick other convolution solvers under capture)
        assert set(grad_a) == set(grad_b) and any(k.startswith("geo_encoder.") for k in grad_a)
        for k in grad_a:
            assert (grad_a[k] - grad_b[k]).norm() <= 2e-2 * grad_a[k].norm() + 1e-4, (it, k)


def test_steps_repack_the_weights_on_the_device():
    """After the optimiser's step both weight handles (the forward's and the fp32 one of the fused backward) are re-packed in place on the device
    (vanerf_weights_update); the streams they then hold must be the bits a fresh host pack of the module's parameters gives, step after step,
    and the handles themselves stay the same objects (no allocation, no blocking copy in the step)."""
    from vanerf_amd import renderer as R
    net = _net(0.01)
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=64, tar_w=64), "cuda")
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    handles = None
    for it in range(3):
        out = _step(net, frame)
        held = (net._packed[1], net._packed_alt[1])
        sd = {k: v.detach().cpu() for k, v in net._hot_state().items()}
        assert torch.equal(R.stream_device(held[0], 0), R.stream_host(sd, 1)), it
        assert torch.equal(R.stream_device(held[1], 0), R.stream_host(sd, 0)), it
        assert torch.equal(R.stream_device(held[1], 2), R.stream_host(sd, 2)), it
        assert handles is None or (held[0] is handles[0] and held[1] is handles[1])
        handles = held
        opt.zero_grad(set_to_none=True)
        ((out["tex_fg_fine"] - out["tar_img"]).abs().mean() + out["alpha_fine"].mean()).backward()
        opt.step()
    assert abs(held[0].beta - max(float(net.sigmoid_beta.detach()), 2e-3)) < 1e-9


def test_backward_chain_is_a_pure_function_of_the_sample():
    """The fused backward processes 32-sample groups in a grid-stride loop; a sample's spilled dY and input gradients must not depend on which
    iteration of which wave took its group.  One block of 131 072 samples (four groups per wave) against the same samples in four blocks of
    32 768 (one group per wave), bit for bit -- a build of query_backward_kernel once restored wrong row offsets from spilled SGPRs in the second
    and later groups of a wave (one gate's gradient 2 % off) while every test at one group per wave passed."""
    from vanerf_amd import hip_backward as HB, renderer as R
    n, part = 131072, 32768
    sd = synth.make_full_weights(0)
    frame = synth.make_frame(seed=11, tar_h=512, tar_w=334, orbit_deg=15.0)
    fd = synth.to_device(frame, "cuda")
    sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
    fdat = R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
    w0 = R.PackedWeights(sd, mode="fp32")
    rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 0, 200, 1, 334, 64, 64, device="cuda")
    pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"]).view(-1, 3)[:n].contiguous()
    q_sdf, q_vis, knn = (t.view(-1) for t in R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts))
    d = torch.randn(n, 5, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    ws = HB.workspace(n, pts.device)
    ws.dw.zero_()
    ig, _ = HB.run_block(ws, w0, fdat, pts, q_sdf, q_vis, knn, d)
    ys_all, ig_all = ws.ys[:, :n].clone(), {k: v.clone() for k, v in ig.items()}
    assert int(ws.valid[:n].sum()) > n // 2 and torch.isfinite(ys_all).all()
    small = HB.Workspace(part, pts.device)
    for b0 in range(0, n, part):
        sl = slice(b0, b0 + part)
        ig, _ = HB.run_block(small, w0, fdat, pts[sl], q_sdf[sl], q_vis[sl], knn[sl], d[sl])
        assert torch.equal(small.ys[:, :part], ys_all[:, sl]), b0
        for k, v in ig.items():
            assert torch.equal(v, ig_all[k][sl]), (k, b0)


@pytest.mark.parametrize("npad", [65536, 2048, 96])
def test_weight_products_kernel_against_matrix_products(npad):
    """vanerf_weight_products (every layer's dW' += Ys Xs^T in one launch) against fp64 matrix products of the same spills, and against the sliced
    torch.baddbmm path it replaced: random spills, accumulation into a non-zero accumulator, a block too short for the slicing (one slice), and
    two launches in a row give the same bits (one wave per accumulator, fixed order)."""
    from vanerf_amd import hip_backward as HB
    ws = HB.Workspace(npad, "cuda")
    g = torch.Generator(device="cuda").manual_seed(npad)
    ws.xs.copy_(torch.randn(ws.xs.shape, device="cuda", generator=g))
    ws.ys.copy_(torch.randn(ws.ys.shape, device="cuda", generator=g))
    base = torch.randn(ws.dw.shape, device="cuda", generator=g)
    ws.dw.copy_(base)
    HB._weight_products_on(ws, ws.xs, ws.ys, npad)
    got = ws.dw.clone()
    ws.dw.copy_(base)
    HB._weight_products_on(ws, ws.xs, ws.ys, npad)
    assert torch.equal(ws.dw, got)
    ws.dw.copy_(base)
    HB._weight_products_on(ws, ws.xs, ws.ys, npad, use_torch=True)
    via_torch = ws.dw.clone()
    L = HB.layout()
    ws.dw.copy_(got)
    for li, lay in enumerate(L["layers"]):
        want = ws.ys[lay["y_row"]:lay["y_row"] + lay["n_out"]].double() @ ws.xs[lay["x_row"]:lay["x_row"] + lay["n_slots"]].double().t()
        ws.dw.copy_(base); b0 = ws.dw_l[li].double().sum(0)
        ws.dw.copy_(got); have = ws.dw_l[li].double().sum(0) - b0
        ws.dw.copy_(via_torch); ref = ws.dw_l[li].double().sum(0) - b0
        scale = want.abs().max().item()
        assert (have - want).abs().max().item() <= 2e-5 * scale + 1e-4, (li, (have - want).abs().max().item(), scale)
        assert (have - want).abs().max().item() <= 2.0 * (ref - want).abs().max().item() + 1e-4 * scale, li  # no worse than the library products


@pytest.mark.parametrize("S,Sn", [(16, 0), (64, 0), (128, 0), (200, 0), (64, 64), (40, 24), (8, 8)])
def test_composite_backward_against_autograd(S, Sn):
    """vanerf_composite_backward (one wave per ray; dL/dsigma from a suffix scan, no division by 1 - c) against torch.autograd through
    torch_graph.composite in fp64: single table and the merged [coarse | new] order with its origin map, opaque samples (c = 1 exactly in fp32:
    the case torch.cumprod's backward branches for), upstream gradients on every output or only on some, sigmoid_beta's share."""
    from vanerf_amd import renderer as R, torch_graph as G
    g = torch.Generator(device="cuda").manual_seed(100 * S + Sn)
    rays = 257
    sd = synth.make_full_weights(0)
    sd["sigmoid_beta"] = torch.tensor([0.05])
    w = R.PackedWeights(sd, mode="fp32")
    St = S + Sn
    z = torch.sort(torch.rand(rays, St, device="cuda", generator=g) * 0.3 + 0.4, dim=1)[0].contiguous()
    ra = torch.randn(rays, S, 5, device="cuda", generator=g) * 0.05
    ma = torch.randn(rays, S, device="cuda", generator=g) * 0.02
    ra[:, S // 2, 0] = -5.0   # an opaque sample in every ray: sigma dist ~ 1e3, c = 1 exactly
    ra[::7, :, 0] = 5.0       # rays that hit nothing: sigma ~ 0 everywhere, acc ~ 0
    rn = mn = src = None
    if Sn:
        rn = torch.randn(rays, Sn, 5, device="cuda", generator=g) * 0.05
        mn = torch.randn(rays, Sn, device="cuda", generator=g) * 0.02
        perm = torch.argsort(torch.rand(rays, St, device="cuda", generator=g), dim=1)  # merged position -> table entry
        src = torch.where(perm < S, perm, -(perm - S) - 1).to(torch.int32).contiguous()
    for with_all in (True, False):
        gc = torch.randn(rays, 3, device="cuda", generator=g)
        gd, ga, gs = (torch.randn(rays, device="cuda", generator=g) for _ in range(3))
        if not with_all:
            gd = gs = None
        d_a, d_n, d_beta = R.composite_backward(w, ra, z, ma, gc, gd, ga, gs, rgba_n=rn, sdf_n=mn, src=src)
        # the same through autograd, fp64
        beta = torch.tensor([0.05], dtype=torch.float64, device="cuda", requires_grad=True)
        xa = ra.double().requires_grad_(True)
        leaves = [xa, beta]
        if Sn:
            xn = rn.double().requires_grad_(True)
            leaves.append(xn)
            take = torch.where(src >= 0, src.long(), S + (-src.long() - 1))
            rgba = torch.gather(torch.cat([xa, xn], 1), 1, take[..., None].expand(-1, -1, 5))
            msdf = torch.gather(torch.cat([ma, mn], 1).double(), 1, take)
        else:
            rgba, msdf = xa, ma.double()
        col, dep, acc, sdf = G.composite({"sigmoid_beta": beta}, rgba, z.double(), msdf)
        loss = (col * gc.double()).sum() + (acc * ga.double()).sum()
        if with_all:
            loss = loss + (dep * gd.double()).sum() + (sdf * gs.double()).sum()
        grads = torch.autograd.grad(loss, leaves)
        def close(have, want, what):
            scale = want.abs().max().item() + 1e-12
            err = (have.double() - want).abs().max().item()
            assert err <= 2e-4 * scale + 1e-6, (what, S, Sn, with_all, err, scale)
        close(d_a, grads[0], "d_rgba")
        if Sn:
            close(d_n, grads[2], "d_rgba_n")
        assert abs(d_beta.double().sum().item() - grads[1].item()) <= 2e-3 * abs(grads[1].item()) + 1e-3, (d_beta.double().sum().item(), grads[1].item())
        assert torch.isfinite(d_a).all() and torch.isfinite(d_beta).all()


def test_bilinear_taps_kernel_against_the_torch_formula():
    """vanerf_bilinear_taps (row indices and weights of feat_sample's four taps, one launch) against the element-wise torch version it replaced:
    indices equal, weights within rounding, coordinates outside [-1, 1] clamped to the border, a one-pixel-wide map."""
    from vanerf_amd import hip_backward as HB
    g = torch.Generator(device="cuda").manual_seed(0)
    for H, W in ((64, 64), (128, 96), (1, 7), (5, 1)):
        xy = torch.rand(10007, 2, device="cuda", generator=g) * 2.6 - 1.3
        xy[:8] = torch.tensor([[-1.0, -1.0], [1.0, 1.0], [0.0, 0.0], [1.0, -1.0], [-1.3, 0.2], [0.999999, 0.5], [-0.999999, -0.5], [2.0, 2.0]], device="cuda")
        i_k, w_k = HB._taps(xy, H, W)
        i_t, w_t = HB._taps(xy, H, W, use_torch=True)
        assert torch.equal(i_k, i_t), (H, W)
        assert (w_k - w_t).abs().max().item() <= 1e-6, (H, W)
        assert (w_k.sum(0) - 1.0).abs().max().item() <= 1e-6
