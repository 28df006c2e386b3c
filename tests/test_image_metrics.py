"""Image scores on the GPU (vanerf_image_metrics, vanerf_amd/metrics.py): MSE, PSNR, scikit-image's SSIM on the crop to the bounding rectangle
of mask_at_box (Evaluator.compute_score, src/evaluator.py:84-114) and kornia's masked PSNR / Gaussian SSIM (compute_test_metric,
src/model.py:210-235).

Neither library is a dependency: parity against kornia 0.7.1 / scikit-image 0.16.2 is unpinned.  The yardstick is the fp64 numpy restatement
below (`ref_metrics`), written from the definitions of DESIGN.md section 0c: direct 49-tap sums, np.pad(mode="reflect"), the windows that lie
wholly inside the crop.  The CPU tests keep the yardstick honest (scipy's filters, an explicit loop over the windows, closed forms) and check
the ABI; the GPU tests hold the kernels to the yardstick.

Tolerances.  The kernels keep the window moments, S and every sum in fp64 and round each result to fp32 once, so the error against the fp64
restatement is that one rounding: at most half an ulp of the fp32 value (2^-25 = 3.0e-8 for an SSIM in [0.5, 1), 2^-20 = 9.5e-7 dB for a PSNR
in [16, 32), 2^-24 = 6.0e-8 relative for mse).  Measured on an MI355X, the largest difference per slot over the PARITY cases: mse 4.2e-8
relative, psnr 8.2e-7 dB, ssim_box 2.7e-8, psnr_masked 8.7e-7 dB, ssim_masked 2.5e-8.  The assertions allow ten times the measured figure
where that is below the cap (SSIMs 2.7e-7 against a cap of 1e-5, PSNRs 8.7e-6 dB against 1e-4 dB) and the cap itself for mse (1e-7
relative; ten times the measured figure would be 4.2e-7).  Slots 5-7 are exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from vanerf_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_SSIM, TOL_PSNR, TOL_MSE_REL = 2.7e-7, 8.7e-6, 1e-7
SLOT = {"mse": 0, "psnr": 1, "ssim_box": 2, "psnr_masked": 3, "ssim_masked": 4, "n_mask": 5, "box_w": 6, "box_h": 7}


# ------------------------------------------------------------------------------------------------------------------------------------
# fp64 restatement
# ------------------------------------------------------------------------------------------------------------------------------------
def gauss_window():
    """7 x 7 Gaussian, sigma 1.5: the normalised outer product of the 1-D kernel."""
    k = np.arange(7, dtype=np.float64) - 3.0
    g = np.exp(-(k * k) / (2.0 * 1.5 * 1.5))
    g /= g.sum()
    return np.outer(g, g), g


def window_moments(xp, yp, w2, oh, ow):
    """The five moments sum_w x, y, x^2, y^2, xy of the 7 x 7 window `w2` at every position where it fits into the (C, oh + 6, ow + 6) arrays
    xp, yp: 49 taps, added in row-major order."""
    m = [np.zeros(xp.shape[:-2] + (oh, ow)) for _ in range(5)]
    for dy in range(7):
        for dx in range(7):
            xs, ys = xp[..., dy:dy + oh, dx:dx + ow], yp[..., dy:dy + oh, dx:dx + ow]
            for acc, val in zip(m, (xs, ys, xs * xs, ys * ys, xs * ys)):
                acc += w2[dy, dx] * val
    return m


def gaussian_ssim_map(x, y, max_val=1.0):
    """kornia.metrics.ssim(window_size=7) restated: (C, H, W) fp64 -> the map S of the same shape."""
    H, W = x.shape[-2:]
    assert H >= 4 and W >= 4, "reflect padding by 3 needs 4 pixels"
    pad = [(0, 0)] * (x.ndim - 2) + [(3, 3), (3, 3)]
    mu1, mu2, e11, e22, e12 = window_moments(np.pad(x, pad, mode="reflect"), np.pad(y, pad, mode="reflect"), gauss_window()[0], H, W)
    C1, C2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    return ((2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2) + 1e-12)


def uniform_ssim_map(x, y):
    """skimage.structural_similarity on float images (data_range 2) restated: (C, h, w) fp64 -> S at the (h - 6) x (w - 6) windows inside."""
    h, w = x.shape[-2:]
    assert h >= 7 and w >= 7
    ux, uy, exx, eyy, exy = window_moments(x, y, np.full((7, 7), 1.0 / 49.0), h - 6, w - 6)
    C1, C2, cov = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2, 49.0 / 48.0
    vx, vy, vxy = cov * (exx - ux * ux), cov * (eyy - uy * uy), cov * (exy - ux * uy)
    return ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def uniform_ssim_loops(x, y):
    """The same by an explicit loop over the valid windows (small images only)."""
    C, h, w = x.shape
    C1, C2, cov = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2, 49.0 / 48.0
    out = np.zeros((C, h - 6, w - 6))
    for c in range(C):
        for i in range(h - 6):
            for j in range(w - 6):
                a, b = x[c, i:i + 7, j:j + 7], y[c, i:i + 7, j:j + 7]
                ux, uy = a.sum() / 49.0, b.sum() / 49.0
                vx, vy, vxy = cov * ((a * a).sum() / 49.0 - ux * ux), cov * ((b * b).sum() / 49.0 - uy * uy), cov * ((a * b).sum() / 49.0 - ux * uy)
                out[c, i, j] = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return out


def bounding_rect(m):
    """cv2.boundingRect of the nonzero pixels: (x, y, w, h); (0, 0, 0, 0) for an empty mask."""
    rows, cols = np.nonzero(m.any(1))[0], np.nonzero(m.any(0))[0]
    if rows.size == 0:
        return 0, 0, 0, 0
    return int(cols[0]), int(rows[0]), int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1)


def ref_metrics(pred, gt, mask=None, mask_at_box=None, max_val=1.0, clamp_pred=False):
    """One view: pred, gt (3, H, W) -> the eight slots in fp64."""
    x, y = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    if clamp_pred:
        x = np.clip(x, 0.0, 1.0)
    _, H, W = x.shape
    out = np.full(8, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[0] = np.mean((x - y) ** 2)
        out[1] = -10.0 * np.log10(out[0])
        bx, by, bw, bh = (0, 0, W, H) if mask_at_box is None else bounding_rect(np.asarray(mask_at_box) != 0)
        if bw >= 7 and bh >= 7:
            S = uniform_ssim_map(x[:, by:by + bh, bx:bx + bw], y[:, by:by + bh, bx:bx + bw])
            out[2] = np.mean([S[c].mean() for c in range(3)])  # per channel, then over the channels
        m = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
        if m.any():
            out[3] = 10.0 * np.log10(max_val ** 2 / np.mean((x - y)[:, m] ** 2))
            out[4] = gaussian_ssim_map(x, y, max_val)[:, m].mean()
        out[5], out[6], out[7] = m.sum(), bw, bh
    return out


def smooth_pair(seed, V, H, W, noise=0.04):
    """Seeded smooth random fields plus noise in about [0, 1]: gt and a pred that differs from it smoothly and by noise (SSIMs of 0.3-0.9)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W), indexing="ij")

    def field(n=4):
        f = np.zeros((V, 3, H, W))
        for _ in range(n):
            kx, ky, ph = rng.uniform(-9, 9, (V, 3, 1, 1)), rng.uniform(-9, 9, (V, 3, 1, 1)), rng.uniform(0, 6.28, (V, 3, 1, 1))
            f += rng.uniform(0.3, 1.0, (V, 3, 1, 1)) * np.sin(kx * xx + ky * yy + ph)
        return f / n

    gt = 0.5 + 0.4 * field()
    pred = gt + 0.12 * field() + noise * rng.standard_normal(gt.shape)
    return pred.astype(np.float32), gt.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement itself
# ------------------------------------------------------------------------------------------------------------------------------------
def test_restatement_agrees_with_scipy_filters():
    ndi = pytest.importorskip("scipy.ndimage")
    pred, gt = smooth_pair(11, 1, 23, 17)
    x, y = pred[0].astype(np.float64), gt[0].astype(np.float64)
    w2, g = gauss_window()
    pad = [(0, 0), (3, 3), (3, 3)]
    gm = window_moments(np.pad(x, pad, mode="reflect"), np.pad(y, pad, mode="reflect"), w2, 23, 17)
    um = window_moments(x, y, np.full((7, 7), 1.0 / 49.0), 17, 11)
    for mine_g, mine_u, val in zip(gm, um, (x, y, x * x, y * y, x * y)):
        for c in range(3):
            want_u = ndi.uniform_filter(val[c], size=7)[3:-3, 3:-3]
            want_g = ndi.correlate1d(ndi.correlate1d(val[c], g, axis=0, mode="mirror"), g, axis=1, mode="mirror")
            assert np.abs(mine_u[c] - want_u).max() <= 1e-12
            assert np.abs(mine_g[c] - want_g).max() <= 1e-12


def test_restatement_equals_an_explicit_loop_over_the_windows():
    pred, gt = smooth_pair(12, 1, 12, 10)
    x, y = pred[0].astype(np.float64), gt[0].astype(np.float64)
    assert np.abs(uniform_ssim_map(x, y) - uniform_ssim_loops(x, y)).max() <= 1e-13
    box = np.zeros((12, 10), np.uint8)
    box[2:11, 1:9] = 1
    assert abs(ref_metrics(x, y, mask_at_box=box)[2] - uniform_ssim_loops(x[:, 2:11, 1:9], y[:, 2:11, 1:9]).mean()) <= 1e-13
    assert bounding_rect(box) == (1, 2, 8, 9)
    ell = np.zeros((12, 10), np.uint8)
    ell[3:9, 2] = ell[8, 2:7] = 1  # an L: the rectangle is larger than its support
    assert bounding_rect(ell) == (2, 3, 5, 6) and bounding_rect(np.zeros((4, 4))) == (0, 0, 0, 0)


def test_identical_images_score_one():
    _, gt = smooth_pair(13, 1, 20, 15)
    r = ref_metrics(gt[0], gt[0])
    assert r[0] == 0.0 and r[1] == np.inf and r[3] == np.inf
    assert r[2] == 1.0
    # the Gaussian flavour divides by den + 1e-12: S = den / (den + 1e-12), below 1 by 1e-12 / den and exactly 1 in the fp32 table
    assert 0.0 <= 1.0 - r[4] <= 1e-12 / (0.01 ** 2 * 0.03 ** 2) and np.float32(r[4]) == np.float32(1.0)
    assert np.all(uniform_ssim_map(gt[0].astype(np.float64), gt[0].astype(np.float64)) == 1.0)


def test_constant_offset_on_a_constant_image_has_closed_forms():
    a, d, max_val = 0.375, 0.25, 1.0  # exact in binary: the windows' variances are exactly 0
    gt = np.full((3, 11, 9), a)
    pred = gt + d
    r = ref_metrics(pred, gt, max_val=max_val)
    assert abs(r[0] - d * d) <= 1e-15 and abs(r[1] + 20.0 * np.log10(d)) <= 1e-12 and abs(r[3] + 20.0 * np.log10(d)) <= 1e-12
    ux, uy = a + d, a
    C1, C2 = 0.02 ** 2, 0.06 ** 2  # evaluator flavour: the contrast term is C2 / C2
    assert abs(r[2] - (2.0 * ux * uy + C1) / (ux * ux + uy * uy + C1)) <= 1e-12
    C1, C2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    want = (2.0 * ux * uy + C1) * C2 / ((ux * ux + uy * uy + C1) * C2 + 1e-12)
    assert abs(r[4] - want) <= 1e-12
    assert (r[5], r[6], r[7]) == (99.0, 9.0, 11.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the ABI
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ffi():
    from vanerf_amd import build
    build.build()
    from vanerf_amd import _ffi
    return _ffi


def test_image_metrics_is_declared_and_exported(ffi):
    hdr = open(os.path.join(REPO, "include", "vanerf_hip.h")).read()
    assert re.search(r"\bint64_t\s+vanerf_image_metrics_scratch\s*\(", hdr) and re.search(r"\bint\s+vanerf_image_metrics\s*\(", hdr)
    for name in ("vanerf_image_metrics_scratch", "vanerf_image_metrics"):
        assert name in ffi.EXPORTS and hasattr(ffi.lib, name)
    assert ffi.lib.vanerf_abi_version() == 12
    from vanerf_amd import metrics
    assert metrics.SLOTS == tuple(sorted(SLOT, key=SLOT.get))


def test_scratch_size(ffi):
    f = ffi.lib.vanerf_image_metrics_scratch
    assert f(1, 7, 7) >= 32 + 32 and f(1, 512, 334) >= 32 + 16 * 11 * 32
    assert f(5, 512, 334) == 5 * f(1, 512, 334) and f(1, 33, 32) > f(1, 32, 32)
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 3, 8), (1, 8, 3), (1, 5000, 8), (1, 8, 5000)):
        assert f(*bad) == 0, bad


def test_image_metrics_rejects_bad_arguments_without_a_gpu(ffi):
    p = ctypes.c_void_p(256)  # never dereferenced: validation comes first
    need = ffi.lib.vanerf_image_metrics_scratch(2, 40, 21)
    args = dict(pred=p, gt=p, mask=None, box=None, V=2, H=40, W=21, max_val=1.0, clamp=0, scratch=p, scratch_bytes=need, out=p, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return ffi.lib.vanerf_image_metrics(*a.values()), ffi.lib.vanerf_last_error().decode()

    for k in ("pred", "gt", "scratch", "out"):
        rc, msg = call(**{k: None})
        assert rc == -22 and "null" in msg, k
    for kw, word in (({"V": 0}, "V=0"), ({"V": -2}, "V=-2"), ({"H": 3}, "H=3"), ({"W": 3}, "W=3"), ({"W": 5000}, "W=5000"),
                     ({"scratch_bytes": need - 1}, "scratch"), ({"scratch_bytes": 0}, "scratch"), ({"scratch": ctypes.c_void_p(264)}, "aligned"),
                     ({"pred": ctypes.c_void_p(258)}, "aligned"), ({"gt": ctypes.c_void_p(257)}, "aligned"),
                     ({"out": ctypes.c_void_p(262)}, "aligned"), ({"max_val": 0.0}, "max_val")):
        rc, msg = call(**kw)
        assert rc == -22 and word in msg, (kw, msg)


def test_python_interface_refuses_cpu_tensors_and_other_dtypes(ffi):
    from vanerf_amd import metrics
    a = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="GPU"):
        metrics.image_metrics(a, a)
    with pytest.raises(ValueError):
        metrics.compute_score(a, a, torch.ones(8, 8))
    with pytest.raises(ValueError):
        metrics.compute_test_metric(a, a)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernels against the restatement
# ------------------------------------------------------------------------------------------------------------------------------------
def _ellipse(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0).astype(np.uint8)


def _case(name):
    """-> pred, gt (V, 3, H, W) fp32, mask, mask_at_box (V, H, W) uint8 or None."""
    if name == "7x7":  # one valid uniform window; the reflect halo spans the whole image
        return smooth_pair(1, 1, 7, 7) + (None, None)
    if name == "4x9":  # the reflect minimum; the uniform crop is too small
        return smooth_pair(2, 1, 4, 9) + (None, None)
    if name == "3x40x21":
        pred, gt = smooth_pair(3, 3, 40, 21)
        box, mask = np.zeros((3, 40, 21), np.uint8), np.zeros((3, 40, 21), np.uint8)
        box[0, 25:40, 10:21] = 1  # touches the bottom and right borders, straddles the tile boundary at row 32
        box[1, 5:31, 3:7] = box[1, 27:31, 3:18] = 1  # an L: the rectangle (15 x 26) is larger than its support
        box[2, 29:36, 8:15] = 1  # exactly 7 x 7, across the tile boundary
        mask[0] = _ellipse(40, 21, 22, 9, 15, 7)
        mask[1, 30:40, :] = 1
        mask[2] = (np.random.RandomState(5).rand(40, 21) < 0.3)
        return pred, gt, mask, box
    if name == "2x70x45":
        pred, gt = smooth_pair(4, 2, 70, 45)
        box, mask = np.ones((2, 70, 45), np.uint8), np.ones((2, 70, 45), np.uint8)  # view 0: all ones
        box[1] = _ellipse(70, 45, 40, 30, 28, 14)  # clipped by the right border, over three tile rows and both tile columns
        mask[1] = _ellipse(70, 45, 30, 20, 25, 18)
        return pred, gt, mask, box
    if name == "512x334":
        pred, gt = smooth_pair(6, 1, 512, 334)
        m = _ellipse(512, 334, 250, 170, 200, 120)[None]
        return pred, gt, m, m.copy()
    raise KeyError(name)


PARITY = ["7x7", "4x9", "3x40x21", "2x70x45", "512x334"]
_REF = {}


def _reference(name, clamp_pred=False):
    """The restatement of a case, computed once and shared."""
    key = (name, clamp_pred)
    if key not in _REF:
        pred, gt, mask, box = _case(name)
        _REF[key] = np.stack([ref_metrics(pred[v], gt[v], None if mask is None else mask[v], None if box is None else box[v], clamp_pred=clamp_pred)
                              for v in range(pred.shape[0])])
    return _REF[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _assert_close(got, ref, what):
    """got (V, 8) fp32 from the device, ref (V, 8) fp64: NaNs in the same slots, the tolerances of the module docstring, slots 5-7 exact."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    err[np.isnan(ref)] = 0.0
    err[got == ref] = 0.0  # +inf == +inf
    rel_mse = err[:, 0] / ref[:, 0]
    print(f"{what}: mse rel {rel_mse.max():.2e} psnr {err[:, 1].max():.2e} ssim_box {err[:, 2].max():.2e} psnr_masked {err[:, 3].max():.2e} "
          f"ssim_masked {err[:, 4].max():.2e}")
    assert rel_mse.max() <= TOL_MSE_REL, what
    assert err[:, 1].max() <= TOL_PSNR and err[:, 3].max() <= TOL_PSNR, what
    assert err[:, 2].max() <= TOL_SSIM and err[:, 4].max() <= TOL_SSIM, what
    assert np.array_equal(got[:, 5:], ref[:, 5:]), what


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_kernel_matches_the_fp64_restatement(name):
    from vanerf_amd import metrics
    pred, gt, mask, box = _case(name)
    out = metrics.image_metrics(_dev(pred), _dev(gt), mask=_dev(mask), mask_at_box=_dev(box)).cpu().numpy()
    ref = _reference(name)
    _assert_close(out, ref, name)
    if name == "4x9":
        assert np.isnan(out[0, 2]) and np.isfinite(out[0, [0, 1, 3, 4]]).all()
    else:
        assert np.isfinite(out).all()
        assert ((ref[:, [2, 4]] > 0.2) & (ref[:, [2, 4]] < 0.95)).all(), ref[:, [2, 4]]  # neither saturated nor zero: the comparison says something
    if name == "3x40x21":
        assert [tuple(r) for r in out[:, 6:]] == [(11.0, 15.0), (15.0, 26.0), (7.0, 7.0)]


@pytest.mark.gpu
def test_bool_masks_and_a_mask_with_a_channel_axis():
    from vanerf_amd import metrics
    pred, gt, mask, box = _case("3x40x21")
    out = metrics.image_metrics(_dev(pred), _dev(gt), mask=_dev(mask).bool()[:, None], mask_at_box=_dev(box).float() * 3.0)
    _assert_close(out.cpu().numpy(), _reference("3x40x21"), "bool / float masks")


@pytest.mark.gpu
def test_degenerate_masks_give_nan_and_no_fault():
    from vanerf_amd import metrics
    pred, gt, mask, box = _case("3x40x21")
    mask, box = mask.copy(), box.copy()
    box[0] = 0  # empty mask_at_box
    mask[1] = 0  # empty mask
    box[2] = 0
    box[2, 3:30, 9:15] = 1  # six pixels wide
    out = metrics.image_metrics(_dev(pred), _dev(gt), mask=_dev(mask), mask_at_box=_dev(box)).cpu().numpy()
    ref = np.stack([ref_metrics(pred[v], gt[v], mask[v], box[v]) for v in range(3)])
    _assert_close(out, ref, "degenerate")
    assert np.isnan(out[0, 2]) and out[0, 6] == 0.0 and out[0, 7] == 0.0 and np.isfinite(out[0, [0, 1, 3, 4]]).all()
    assert np.isnan(out[1, 3]) and np.isnan(out[1, 4]) and out[1, 5] == 0.0 and np.isfinite(out[1, :3]).all()
    assert np.isnan(out[2, 2]) and (out[2, 6], out[2, 7]) == (6.0, 27.0)


@pytest.mark.gpu
def test_clamp_pred_scores_the_clamped_image():
    from vanerf_amd import metrics
    pred, gt, mask, box = _case("2x70x45")
    pred = (pred - 0.5) * 1.8 + 0.5  # well outside [0, 1] in places
    assert (pred < -0.05).any() and (pred > 1.05).any()
    ref = np.stack([ref_metrics(pred[v], gt[v], mask[v], box[v], clamp_pred=True) for v in range(2)])
    out = metrics.image_metrics(_dev(pred), _dev(gt), mask=_dev(mask), mask_at_box=_dev(box), clamp_pred=True)
    _assert_close(out.cpu().numpy(), ref, "clamp_pred")
    unclamped = metrics.image_metrics(_dev(pred), _dev(gt), mask=_dev(mask), mask_at_box=_dev(box))
    assert (unclamped[:, 0] > out[:, 0]).all()
    same = metrics.image_metrics(_dev(np.clip(pred, 0.0, 1.0)), _dev(gt), mask=_dev(mask), mask_at_box=_dev(box))
    assert torch.equal(_bits(same), _bits(out))


@pytest.mark.gpu
def test_max_val_scales_the_masked_pair():
    from vanerf_amd import metrics
    pred, gt, mask, box = _case("2x70x45")
    pred, gt = pred * 255.0, gt * 255.0
    ref = np.stack([ref_metrics(pred[v], gt[v], mask[v], box[v], max_val=255.0) for v in range(2)])
    out = metrics.image_metrics(_dev(pred), _dev(gt), mask=_dev(mask), mask_at_box=_dev(box), max_val=255.0)
    _assert_close(out.cpu().numpy(), ref, "max_val 255")


@pytest.fixture(scope="module")
def lib_ffi():
    """The binding as the GPU tests use it: the library travels with the tree, nothing is built here."""
    from vanerf_amd import _ffi
    return _ffi


def _raw_call(ffi, pred, gt, mask, box, scratch, out, stream=None):
    V, _, H, W = pred.shape
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = torch.cuda.current_stream() if stream is None else stream
    ffi.check(ffi.lib.vanerf_image_metrics(ptr(pred), ptr(gt), ptr(mask), ptr(box), V, H, W, 1.0, 0, ptr(scratch), scratch.numel() * scratch.element_size(),
                                           ptr(out), ctypes.c_void_p(st.cuda_stream)))


@pytest.mark.gpu
def test_calls_are_reproducible_and_ignore_what_the_scratch_block_held(lib_ffi):
    ffi = lib_ffi
    from vanerf_amd import metrics
    pred, gt, mask, box = (_dev(a) for a in _case("2x70x45"))
    a = metrics.image_metrics(pred, gt, mask=mask, mask_at_box=box)
    b = metrics.image_metrics(pred, gt, mask=mask, mask_at_box=box)
    assert torch.equal(_bits(a), _bits(b))
    n = ffi.lib.vanerf_image_metrics_scratch(2, 70, 45) // 8
    outs = []
    for fill in (0.0, float("nan")):
        scratch = torch.full((n,), fill, dtype=torch.float64, device="cuda")
        out = torch.full((2, 8), fill, device="cuda")
        _raw_call(ffi, pred, gt, mask, box, scratch, out)
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(a))
    with pytest.raises(ffi.VanerfError, match="scratch"):
        _raw_call(ffi, pred, gt, mask, box, scratch[: n // 2], out)


@pytest.mark.gpu
def test_a_view_scores_the_same_alone_and_in_a_batch():
    from vanerf_amd import metrics
    pred, gt, mask, box = (_dev(a) for a in _case("3x40x21"))
    batch = metrics.image_metrics(pred, gt, mask=mask, mask_at_box=box)
    for k in range(3):
        one = metrics.image_metrics(pred[k], gt[k], mask=mask[k], mask_at_box=box[k])
        assert one.shape == (1, 8) and torch.equal(_bits(one[0]), _bits(batch[k])), k
    out = torch.empty(3, 8, device="cuda")
    assert metrics.image_metrics(pred, gt, mask=mask, mask_at_box=box, out=out) is out and torch.equal(_bits(out), _bits(batch))


@pytest.mark.gpu
def test_two_streams_in_flight_with_their_own_scratch_blocks(lib_ffi):
    ffi = lib_ffi
    from vanerf_amd import metrics
    cases = [tuple(_dev(a) for a in _case(n)) for n in ("2x70x45", "3x40x21")]
    want = [metrics.image_metrics(p, g, mask=m, mask_at_box=b) for p, g, m, b in cases]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    blocks, outs = [], []
    for (p, g, m, b) in cases:
        V, _, H, W = p.shape
        blocks.append(torch.full((ffi.lib.vanerf_image_metrics_scratch(V, H, W) // 8,), float("nan"), dtype=torch.float64, device="cuda"))
        outs.append(torch.empty(V, 8, device="cuda"))
    torch.cuda.synchronize()
    for rep in range(3):  # both queues stay busy: neither stream waits for the other
        for (p, g, m, b), st, blk, o in zip(cases, streams, blocks, outs):
            _raw_call(ffi, p, g, m, b, blk, o, stream=st)
    torch.cuda.synchronize()
    for w, o in zip(want, outs):
        assert torch.equal(_bits(w), _bits(o))


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the reference's two signatures
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("batched", [False, True])
def test_compute_test_metric_and_compute_score(batched):
    from vanerf_amd import metrics
    pred, gt, mask, box = _case("3x40x21")
    ref = _reference("3x40x21")[0]
    p, g = _dev(pred[0]), _dev(gt[0])
    if batched:
        p, g = p[None], g[None]
    m = metrics.compute_test_metric(p, g, mask=_dev(mask[0]).bool())
    assert set(m) == {"psnr", "ssim"} and all(v.is_cuda and v.dim() == 0 for v in m.values())
    assert abs(m["psnr"].item() - ref[3]) <= TOL_PSNR and abs(m["ssim"].item() - ref[4]) <= TOL_SSIM
    unmasked = ref_metrics(pred[0], gt[0])
    m = metrics.compute_test_metric(p, g)
    assert abs(m["psnr"].item() - unmasked[3]) <= TOL_PSNR and abs(m["ssim"].item() - unmasked[4]) <= TOL_SSIM
    s = metrics.compute_score(p, g, _dev(box[0])[None] if batched else _dev(box[0]))
    assert set(s) == {"mse", "psnr", "ssim"} and "lpips" not in s and all(type(v) is float for v in s.values())
    assert abs(s["mse"] - ref[0]) <= TOL_MSE_REL * ref[0] and abs(s["psnr"] - ref[1]) <= TOL_PSNR and abs(s["ssim"] - ref[2]) <= TOL_SSIM


@pytest.mark.gpu
def test_interface_refuses_half_precision_and_mismatched_inputs():
    from vanerf_amd import metrics
    a = torch.rand(3, 8, 8, device="cuda")
    with pytest.raises(TypeError):
        metrics.image_metrics(a.half(), a.half())
    with pytest.raises(TypeError):
        metrics.compute_test_metric(a, a.half())
    with pytest.raises(ValueError):
        metrics.image_metrics(a, a.cpu())
    with pytest.raises(ValueError):
        metrics.image_metrics(a, a, mask=torch.ones(8, 8))  # a CPU mask
    with pytest.raises(ValueError):
        metrics.image_metrics(a, a, mask_at_box=torch.ones(4, 8, device="cuda"))
    with pytest.raises(ValueError):
        metrics.image_metrics(a, torch.rand(3, 8, 9, device="cuda"))
    from vanerf_amd._ffi import VanerfError
    with pytest.raises(VanerfError):
        metrics.image_metrics(a[:, :3], a[:, :3])  # H < 4: refused by the library


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the evaluation driver
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_evaluate_views_equals_per_view_renders_and_the_restatement():
    from vanerf_amd import metrics
    from vanerf_amd.config import default_config
    from vanerf_amd.model import VANeRF, get_360cameras
    from vanerf_amd.novel_views import camera_to_cam_tar
    torch.manual_seed(0)
    cfg = default_config()
    cfg["models"]["VANeRF"]["mfma_precision"] = "bf16x3"
    cfg["models"]["VANeRF"]["dr_kwargs"].update(sample_per_ray_c=16, sample_per_ray_f=16)
    net = VANeRF(cfg).cuda().eval()
    net.load_state_dict(synth.make_full_weights(0), strict=False)
    H = W = 16
    frame_cpu = synth.make_frame(seed=3, tar_h=H, tar_w=W)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    headpose = torch.eye(4)
    headpose[:3, 3] = frame_cpu["targets"]["vert_world"][0].mean(0)
    cams = get_360cameras(headpose[:3, :4].cuda(), 4.0 * W, 1.0, 1.0, W, H, 0.71, 1.42, n_frames=6)[:3]
    cam_tars = [camera_to_cam_tar(c) for c in cams]
    _, tar = smooth_pair(21, 3, H, W)
    box = np.zeros((3, H, W), np.uint8)
    box[0, 2:14, 3:13] = 1
    box[1] = 1
    box[2, 1:12, 4] = box[2, 11, 4:15] = 1
    mask = np.stack([_ellipse(H, W, 8, 8, 6, 5), np.ones((H, W), np.uint8), _ellipse(H, W, 6, 9, 5, 6)])
    tar_d, box_d, mask_d = _dev(tar), _dev(box), _dev(mask)

    scores, images = metrics.evaluate_views(net, trb, cam_tars, tar_d, box_d, masks=mask_d, views_per_pass=3)
    assert scores.shape == (3, 8) and scores.is_cuda and len(images) == 3 and all(i.shape == (3, H, W) for i in images)
    one_by_one, images1 = metrics.evaluate_views(net, trb, cam_tars, tar_d, box_d, masks=mask_d, views_per_pass=1)
    assert torch.equal(_bits(scores), _bits(one_by_one))
    default, _ = metrics.evaluate_views(net, trb, cam_tars, [t for t in tar_d], [b for b in box_d], masks=[m for m in mask_d])
    assert torch.equal(_bits(scores), _bits(default))
    assert all(torch.equal(a, b) for a, b in zip(images, images1))

    kw = dict(fine=True, uniform=True, sample_per_ray_c=16, sample_per_ray_f=16, src_foreground_mask=trb["src_foreground_mask"],
              bounds=trb["dr_data"]["bounds"])
    singles = []
    for cam_tar in cam_tars:
        with torch.no_grad():
            o = net.render_pifu_nerf(None, net, trb["im"], trb["cam"], trb["hand_type"], trb["targets"], cam_tar, level=1,
                                     sp_data=dict(trb["sp_data"]), mask_at_box=None, **kw)
        singles.append(o["tex_fg_fine"])
    assert all(torch.equal(a, b) for a, b in zip(images, singles))
    direct = metrics.image_metrics(torch.stack(singles), tar_d, mask=mask_d, mask_at_box=box_d, clamp_pred=True)
    assert torch.equal(_bits(scores), _bits(direct))
    rendered = torch.stack(singles).cpu().numpy()
    assert rendered.std() > 1e-3
    ref = np.stack([ref_metrics(rendered[v], tar[v], mask[v], box[v], clamp_pred=True) for v in range(3)])
    _assert_close(scores.cpu().numpy(), ref, "evaluate_views")
    with pytest.raises(ValueError):
        metrics.evaluate_views(net, trb, cam_tars, tar_d[:2], box_d)
    with pytest.raises(ValueError):
        metrics.evaluate_views(net, trb, cam_tars, tar_d, box_d, views_per_pass=0)
