"""A criterion that holds the CPU oracle to the reference's golden tensors on any host CPU (tests/test_oracle_golden.py,
tests/test_oracle_posed.py), and the fp64 evaluations it needs.  Loads the oracle alone, never the HIP library.

A golden tensor is the reference's fp32 result as the torch kernels of the machine that recorded it computed it; the oracle's fp32 result on
another CPU is a second legitimate fp32 evaluation of the same graph, and the two differ by the rounding of either.  Both are therefore
measured against o64, the same oracle function in fp64 on the golden's own inputs (every floating input, weight and feature map cast up;
discrete inputs and the fp32-rounded pi 2^l constants as they are):

  D = max |golden - o64|     does not depend on the host (fp64 rounding is far below every bar here)
  H = max |o32 - o64|        this host's fp32 error on the same graph
  bar = max(bar_today, 3 H + u),   u = one fp32 ulp of the golden's largest magnitude

and the assertion is D <= bar.  A mistake in the oracle moves o32 and o64 together: it grows D and leaves H where it was.  The factor 3 is
the project's convention for "what plain fp32 reaches against fp64" (tests/test_backward_per_sample.py); `bar_today`, the tolerance the
comparison had against the golden directly, is the floor, so that nothing that passed before can fail through the criterion."""
import numpy as np
import torch

from oracle import vanerf_oracle as orc

PASS_COARSE = ("tex_fg", "depth", "alpha")
PASS_FINE = ("tex_fg_fine", "depth_fine", "alpha_fine", "sdf")


def cast(obj, dtype):
    """Every floating tensor of a (nested) dict / list in `dtype`; integer and bool tensors and numbers unchanged."""
    if isinstance(obj, torch.Tensor):
        return obj.to(dtype) if obj.is_floating_point() else obj
    if isinstance(obj, dict):
        return {k: cast(v, dtype) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(cast(v, dtype) for v in obj)
    return obj


def ulp32(x):
    """One fp32 ulp at the magnitude of every element of x (tensor or number): float64 tensor of x's shape."""
    return torch.from_numpy(np.asarray(np.spacing(np.abs(np.asarray(x, dtype=np.float32))), dtype=np.float64))


def both(fn, *args):
    """(o32, o64): fn on the arguments as they are and on their fp64 cast."""
    return fn(*args), fn(*cast(args, torch.float64))


def hold(what, golden, o32, o64, bar_today, max_outlier_frac=None):
    """Asserts |golden - o64| <= max(bar_today, 3 H + u) for every element -- or, with `max_outlier_frac`, for all but that fraction of the
    elements, at least one allowed (conftest.assert_close_frac's cap, for outputs behind a decision that the last bit of a sample position
    flips).  Prints |o32 - golden|, D, H and D / H.  Returns (D, H, bar)."""
    assert golden.shape == o32.shape == o64.shape, (what, golden.shape, o32.shape, o64.shape)
    if golden.numel() == 0:
        return 0.0, 0.0, bar_today
    err = (golden.double() - o64.double()).abs()
    D = err.max().item()
    H = (o32.double() - o64.double()).abs().max().item()
    u = ulp32(golden.abs().max().item()).item()
    bar = max(bar_today, 3.0 * H + u)
    bad = int((~(err <= bar)).sum())  # (a NaN on either side is above every bar)
    allowed = 0 if max_outlier_frac is None else max(1, int(max_outlier_frac * err.numel()))
    print(f"criterion {what}: |o32 - golden| {(o32.double() - golden.double()).abs().max().item():.3e}  D {D:.3e}  H {H:.3e}  "
          f"D/H {D / H if H > 0 else float('nan'):.2f}  bar {bar:.3e}  above {bad}/{err.numel()} (allowed {allowed})")
    assert bad <= allowed, f"{what}: {bad}/{err.numel()} elements of |golden - fp64 oracle| above {bar:.3e} (D {D:.3e}, H {H:.3e}, allowed {allowed})"
    return D, H, bar


def remarch64(sd, frame, out, draws=None):
    """The image outputs of an fp32 pass `out` = orc.batch_render(sd, frame, ..., want={}, draws=draws), evaluated in fp64 at the samples that
    pass actually used.  batch_render has decisions inside (mesh queries, searchsorted, sort) and stays fp32; here its points, q_sdf, q_vis,
    vert_vis, depths and rays (and the recorded draws of a training pass) go through orc.query -> orc.eval_func -> orc.rgba2out with fp64
    weights, frame and feature maps.  Validity, the one decision query makes itself, must come out as in fp32.
    -> dict(tex_fg, depth, alpha, tex_fg_fine, depth_fine, alpha_fine, sdf), float64, shaped like out's."""
    sd64, fr = cast(sd, torch.float64), cast(frame, torch.float64)
    rays = out["cam_rays"].double()
    _, h, w = out["depth"].shape

    def march(c, zs, noise):
        S = zs.shape[-1]
        view = rays[:, :, None, :].expand(-1, -1, S, -1).reshape(1, -1, 3)
        rgba, valid = orc.query(sd64, c["pts"].double(), fr["cam_in"], fr["targets"], fr["feat_geo"], fr["feat_tex"], c["vert_vis"], c["q_vis"],
                                c["q_sdf"].view(1, -1).double(), fr["sp_data"], fr["img_in"], view, fr["src_foreground_mask"])
        assert rgba.dtype == torch.float64
        assert torch.equal(valid, c["inter"]["out_mask"].view_as(valid) > 0.0), "fp64 and fp32 disagree on a sample's validity"
        rgba = orc.eval_func(sd64, rgba, valid, fr["cam_in"]["nml_scale"], noise=None if noise is None else noise.double() * draws["std"])
        color, depth, alpha, _, sdf = orc.rgba2out(sd64, rgba.view(1, -1, S, 5), zs.double(), c["q_sdf"].double())
        return color.view(1, h, w, 3).permute(0, 3, 1, 2), depth.view(1, h, w), alpha.view(1, h, w), sdf.view(1, h, w)

    col, dep, acc, _ = march(out["coarse"], out["z"], None if draws is None else draws.get("noise_c"))
    colf, depf, accf, sdff = march(out["fine"], out["z_fine"], None if draws is None else draws.get("noise_f"))
    return {"tex_fg": col, "depth": dep, "alpha": acc, "tex_fg_fine": colf, "depth_fine": depf, "alpha_fine": accf, "sdf": sdff}


def hold_pass(tag, g, out, o64, bar_coarse=2e-6, bar_fine=2e-6, fine_outlier_frac=1e-3):
    """The seven image outputs of a pass under the criterion: the coarse ones with every element inside the bar, the fine ones -- behind the
    u = 1.0 tie of importance_sample (tests/test_oracle_golden.py) -- under the cap `fine_outlier_frac` (None: every element)."""
    for k in PASS_COARSE:
        hold(f"{tag}:{k}", g[k], out[k], o64[k], bar_coarse)
    for k in PASS_FINE:
        hold(f"{tag}:{k}", g[k], out[k], o64[k], bar_fine, fine_outlier_frac)
