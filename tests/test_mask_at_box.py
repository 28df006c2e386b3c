"""mask_at_box and the near / far range of target views on the GPU (vanerf_mask_at_box, vanerf_amd/mask_at_box.py): the dataset's
Dataset.get_mask_at_box -> get_rays / get_near_far (src/dataset.py:122-129, 609-658) and the bounds of load_human_bounds* restated.

The yardstick is the fp64 numpy restatement below (`restate`), written from the definition of DESIGN.md section 0d.  It takes the fp32 camera
table the kernel takes.  The CPU tests hold the yardstick to the reference's own outputs (tests/golden/mask_at_box.npz, written by
tools/gen_mask_at_box_golden.py) and check the ABI; the GPU tests hold the kernels to the yardstick.

Near-threshold pixels.  The mask is a comparison of hit points with the box faces; a pixel whose hit point has a coordinate (not the one on
the plane's own axis) within TAU = 1e-5 of b_min - 1e-6 or b_max + 1e-6 may come out either way and is left out of the mask comparison.  An
fp32 ulp of d moves a hit point by about 6e-8 t with t of the order of a metre, so TAU is some 100 times what a one-ulp difference in d can
move.  At most MAX_EXCLUDED = 0.5 % of a case's pixels may be left out (a condition of every comparison, not a measurement).

Tolerances.  The kernel forms the ray in fp64 and rounds it to fp32 once, as the restatement does; behind that everything is fp64 in the
operation order of the restatement and the library is built without contraction, so what is left is the one rounding of each result to fp32:
at most 2^-24 = 6.0e-8 relative.  Measured on an MI355X, the largest relative difference over the PARITY cases: per-ray near / far
5.9e-8 (MEASURED_RAY), near_min / far_max 3.9e-8 (MEASURED_SLOT).  The assertions allow ten times the measured figure (5.9e-7, 3.9e-7),
which is below the cap of 1e-6.  Against the reference the restatement's near_min / far_max are held to 1e-6 relative (the reference takes |d| in fp32:
9.6e-8 seen, times ten).  Slots 2-6 are exact."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from vanerf_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "mask_at_box.npz")
TAU, MAX_EXCLUDED = 1e-5, 0.005
TOL_REFERENCE = 1e-6                               # restatement against the reference's near.min() / far.max()
MEASURED_RAY, MEASURED_SLOT = 5.9e-8, 3.9e-8       # kernel against restatement, relative, largest over PARITY
TOL_RAY, TOL_SLOT = min(10 * MEASURED_RAY, 1e-6), min(10 * MEASURED_SLOT, 1e-6)
SLOT = {"near_min": 0, "far_max": 1, "n_mask": 2, "box_x": 3, "box_y": 4, "box_w": 5, "box_h": 6, "pad": 7}
PARITY = ["7x5", "40x21", "3x70x45", "334x512"]    # H x W; the cases of the fixture
NEW_EXPORTS = ("vanerf_mask_at_box_scratch", "vanerf_mask_at_box")


# ------------------------------------------------------------------------------------------------------------------------------------
# cameras
# ------------------------------------------------------------------------------------------------------------------------------------
def pinhole(f, cx, cy):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]], np.float32)


def look_at(eye, target, roll=0.0):
    """World -> camera (x_cam = R x + T) of a camera at `eye` whose +z axis points at `target`, rolled about it; fp32."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c, s = np.cos(roll), np.sin(roll)
    x, y = c * x + s * y, -s * x + c * y
    R = np.stack([x, y, z])
    return R.astype(np.float32), (-R @ eye).astype(np.float32)


def cam_tar(K, R, T, H, W, device="cpu"):
    """The cam_tar dict of render_pifu_nerf_views for fp32 K (3, 3), R (3, 3), T (3,)."""
    k4, rt = torch.eye(4), torch.eye(4)
    k4[:3, :3] = torch.from_numpy(np.asarray(K, np.float32))
    rt[:3, :3] = torch.from_numpy(np.asarray(R, np.float32))
    rt[:3, 3] = torch.from_numpy(np.asarray(T, np.float32))
    return {"K": k4[None].to(device), "RT": rt[None].to(device), "width": int(W), "height": int(H), "znear": 0.1, "zfar": 2.0}


def table_rows(K, R, T):
    """Rows of the fp32 camera table for (V, 3, 3), (V, 3, 3), (V, 3) fp32 cameras, made the way renderer.camera_table makes them (torch's
    fp32 inverse on the host), without importing the library."""
    rows = []
    for k, r, t in zip(K, R, T):
        k4 = torch.eye(4)
        k4[:3, :3] = torch.from_numpy(np.asarray(k, np.float32))
        inv_t = torch.inverse(k4[None][:, :3, :3]).transpose(1, 2)[0]  # (the expression of camera_table, on the same strided view)
        rt = np.concatenate([np.asarray(r, np.float32), np.asarray(t, np.float32)[:, None]], axis=1)
        rows.append(np.concatenate([inv_t.numpy().reshape(-1), rt.reshape(-1), np.zeros(3, np.float32)]))
    return np.stack(rows).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------
# fp64 restatement
# ------------------------------------------------------------------------------------------------------------------------------------
def bounding_rect(mask):
    """cv2.boundingRect of the nonzero pixels: x, y, w, h; 0, 0, 0, 0 for an empty mask."""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return (0, 0, 0, 0)
    return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))


def restate(row, bounds, H, W):
    """One view.  row: the 24 fp32 numbers of the camera table; bounds: (2, 3) fp32.  Returns a namespace: mask (H, W) bool, near, far (H, W)
    fp64 with NaN off the mask, near_min, far_max (NaN for an empty mask), n_mask, rect, and `unsure` (H, W) bool, the near-threshold pixels."""
    row = np.asarray(row, np.float32).astype(np.float64)
    Kt, M = row[:9].reshape(3, 3), row[9:21].reshape(3, 4)
    R, T = M[:, :3], M[:, 3]
    o64 = -((R[0] * T[0] + R[1] * T[1]) + R[2] * T[2])
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    pc = [((c * Kt[0, j] + r * Kt[1, j]) + Kt[2, j]) - T[j] for j in range(3)]
    d = []
    for j in range(3):
        dj = (((pc[0] * R[0, j] + pc[1] * R[1, j]) + pc[2] * R[2, j]) - o64[j]).astype(np.float32)
        dj[np.abs(dj) < np.float32(1e-5)] = np.float32(1e-5)
        d.append(dj.astype(np.float64))
    o = o64.astype(np.float32).astype(np.float64)
    b = np.asarray(bounds, np.float32).astype(np.float64).reshape(2, 3) + np.array([-0.01, 0.01])[:, None]
    lo, hi = b[0] - 1e-6, b[1] + 1e-6
    count = np.zeros((H, W), np.int64)
    unsure = np.zeros((H, W), bool)
    q = [np.zeros((H, W)), np.zeros((H, W))]  # squared distance of the first and the second hit from the origin
    for pl in range(6):
        ax = pl % 3
        t = (b.reshape(-1)[pl] - o[ax]) / d[ax]
        p = [t * d[j] + o[j] for j in range(3)]
        inside = np.ones((H, W), bool)
        for j in range(3):
            inside &= (p[j] >= lo[j]) & (p[j] <= hi[j])
            if j != ax:
                unsure |= (np.abs(p[j] - lo[j]) <= TAU) | (np.abs(p[j] - hi[j]) <= TAU)
        e = [p[j] - o[j] for j in range(3)]
        qq = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        q[0] = np.where(inside & (count == 0), qq, q[0])
        q[1] = np.where(inside & (count == 1), qq, q[1])
        count += inside
    mask = count == 2
    nd = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    d0, d1 = np.sqrt(q[0]) / nd, np.sqrt(q[1]) / nd
    near, far = np.where(mask, np.minimum(d0, d1), np.nan), np.where(mask, np.maximum(d0, d1), np.nan)
    empty = not mask.any()
    return types.SimpleNamespace(mask=mask, near=near, far=far, near_min=np.nan if empty else np.nanmin(near), far_max=np.nan if empty else np.nanmax(far),
                                 n_mask=int(mask.sum()), rect=bounding_rect(mask), unsure=unsure)


def masks_agree(got, ref, unsure, what):
    """Equal outside the near-threshold pixels, of which there may be at most MAX_EXCLUDED of the image."""
    frac = unsure.mean()
    assert frac <= MAX_EXCLUDED, (what, frac)
    bad = (np.asarray(got, bool) != np.asarray(ref, bool)) & ~unsure
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5])


_GOLDEN, _RESTATED = {}, {}


def golden(name):
    """-> K, R, T (V, 3, 3 / 3), bounds (2, 3), H, W, mask (V, H, W), near_min, far_max (V,) of a fixture case."""
    if not _GOLDEN:
        with np.load(GOLDEN) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    g = {k.split("/", 1)[1]: v for k, v in _GOLDEN.items() if k.startswith(name + "/")}
    if "H" in g:
        g["H"], g["W"] = int(g["H"]), int(g["W"])
    return types.SimpleNamespace(**g)


def restated(name):
    """The restatement of every view of a fixture case, computed once and shared."""
    if name not in _RESTATED:
        g = golden(name)
        _RESTATED[name] = [restate(row, g.bounds, g.H, g.W) for row in table_rows(g.K, g.R, g.T)]
    return _RESTATED[name]


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement against the reference's outputs
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PARITY)
def test_restatement_matches_the_reference(name):
    g = golden(name)
    assert g.K.dtype == g.R.dtype == g.T.dtype == g.bounds.dtype == np.float32
    assert g.mask.shape == (g.K.shape[0], g.H, g.W) and (g.H, g.W) == tuple(int(x) for x in name.split("x")[-2:])
    for v, ref in enumerate(restated(name)):
        what = f"{name}[{v}]"
        cover = g.mask[v].mean()
        masks_agree(ref.mask, g.mask[v], ref.unsure, what)
        rel_n, rel_f = abs(ref.near_min - g.near_min[v]) / g.near_min[v], abs(ref.far_max - g.far_max[v]) / g.far_max[v]
        print(f"{what}: cover {cover:.3f} excluded {ref.unsure.mean():.5f} near_min rel {rel_n:.2e} far_max rel {rel_f:.2e}")
        assert rel_n <= TOL_REFERENCE and rel_f <= TOL_REFERENCE, what
        if np.array_equal(ref.mask, g.mask[v] != 0):  # (always, unless a near-threshold pixel differs)
            assert ref.n_mask == int((g.mask[v] != 0).sum()) and ref.rect == bounding_rect(g.mask[v])
        assert 0.2 <= cover <= 0.8 or cover == 1.0, what  # (1.0: the camera inside the box)


def test_fixture_has_the_clamp_and_the_inside_cameras():
    g = golden("7x5")
    assert np.array_equal(g.R[0], np.eye(3, dtype=np.float32)) and g.K[0, 0, 2] == 2.0 and g.K[0, 1, 2] == 3.0
    row = table_rows(g.K, g.R, g.T)[0].astype(np.float64)
    Kt = row[:9].reshape(3, 3)
    pc = 2.0 * Kt[0] + 3.0 * Kt[1] + Kt[2]
    assert abs(pc[0]) < 1e-5 and abs(pc[1]) < 1e-5  # the central ray's d_x, d_y take the clamp
    ref = restated("7x5")[0]
    assert ref.mask[3, 2] and g.mask[0, 3, 2]
    g = golden("3x70x45")
    assert g.mask[1].all() and restated("3x70x45")[1].mask.all()  # view 1: the camera inside the box
    o = -g.R[1].T.astype(np.float64) @ g.T[1]
    assert np.all(o > g.bounds[0]) and np.all(o < g.bounds[1])


def test_rectangle_and_count_of_the_restatement():
    m = np.zeros((9, 7), bool)
    assert bounding_rect(m) == (0, 0, 0, 0)
    m[2, 5] = m[7, 1] = True
    assert bounding_rect(m) == (1, 2, 5, 6)


def test_frame_bounds_formula():
    from vanerf_amd.mask_at_box import frame_bounds
    g = golden("bounds_pred")
    got = frame_bounds(torch.from_numpy(g.verts))
    assert got.shape == (2, 3) and got.dtype == torch.float32 and np.array_equal(got.numpy(), g.bounds)
    assert np.array_equal(frame_bounds(torch.from_numpy(g.verts)[None], pad_z=0.0).numpy(), np.stack([g.verts.min(0), g.verts.max(0)]))
    with pytest.raises(ValueError):
        frame_bounds(torch.zeros(0, 3))
    with pytest.raises(ValueError):
        frame_bounds(torch.zeros(4, 2))


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the ABI
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ffi():
    from vanerf_amd import build
    build.build()
    from vanerf_amd import _ffi
    return _ffi


def test_mask_at_box_is_declared_and_exported(ffi):
    hdr = open(os.path.join(REPO, "include", "vanerf_hip.h")).read()
    assert re.search(r"\bint64_t\s+vanerf_mask_at_box_scratch\s*\(", hdr) and re.search(r"\bint\s+vanerf_mask_at_box\s*\(", hdr)
    for name in NEW_EXPORTS:
        assert name in ffi.EXPORTS and hasattr(ffi.lib, name)
    assert ffi.ABI_VERSION == 12 and ffi.lib.vanerf_abi_version() == 12 and "#define VANERF_ABI_VERSION 12" in hdr
    from vanerf_amd import mask_at_box as mab
    assert mab.SLOTS == tuple(sorted(SLOT, key=SLOT.get))


def test_scratch_size(ffi):
    f = ffi.lib.vanerf_mask_at_box_scratch
    for shape in ((1, 1, 1), (1, 7, 5), (3, 70, 45), (5, 334, 512), (65535, 4, 4), (1, 4096, 4096)):
        assert f(*shape) > 0 and f(*shape) % 16 == 0, shape
    assert f(5, 334, 512) == 5 * f(1, 334, 512) and f(1, 334, 512) > f(1, 70, 45) >= f(1, 7, 5)
    for bad in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, -3, 8), (1, 5000, 8), (1, 8, 5000)):
        assert f(*bad) == 0, bad


def test_mask_at_box_rejects_bad_arguments_without_a_gpu(ffi):
    p = ctypes.c_void_p(256)  # never dereferenced: validation comes first
    bounds = (ctypes.c_float * 6)(-0.1, -0.1, -0.1, 0.1, 0.1, 0.1)
    need = ffi.lib.vanerf_mask_at_box_scratch(2, 40, 21)
    args = dict(cams=p, V=2, H=40, W=21, bounds=bounds, mask=p, near=None, far=None, scratch=p, scratch_bytes=need, out=p, stream=None)

    def call(**kw):
        a = dict(args, **kw)
        return ffi.lib.vanerf_mask_at_box(*a.values()), ffi.lib.vanerf_last_error().decode()

    for k in ("cams", "bounds", "mask", "scratch", "out"):
        rc, msg = call(**{k: None})
        assert rc == -22 and "null" in msg, k
    for kw, word in (({"V": 0}, "V=0"), ({"V": -2}, "V=-2"), ({"V": 65536}, "V=65536"), ({"H": 0}, "H=0"), ({"W": 0}, "W=0"), ({"H": -1}, "H=-1"),
                     ({"W": 5000}, "W=5000"), ({"scratch_bytes": need - 1}, "scratch"), ({"scratch_bytes": 0}, "scratch"),
                     ({"scratch": ctypes.c_void_p(264)}, "aligned"), ({"near": ctypes.c_void_p(258)}, "aligned"),
                     ({"far": ctypes.c_void_p(257)}, "aligned"), ({"out": ctypes.c_void_p(262)}, "aligned")):
        rc, msg = call(**kw)
        assert rc == -22 and word in msg, (kw, msg)


def test_python_interface_refuses_cpu_tensors(ffi):
    from vanerf_amd import mask_at_box as mab
    g = golden("7x5")
    with pytest.raises(ValueError, match="GPU"):
        mab.mask_at_box([cam_tar(g.K[0], g.R[0], g.T[0], g.H, g.W)], torch.from_numpy(g.bounds))
    with pytest.raises(ValueError):
        mab.mask_at_box([], torch.from_numpy(g.bounds))


def test_camera_table_is_the_table_the_restatement_takes(ffi):
    from vanerf_amd import renderer
    g = golden("3x70x45")
    table = renderer.camera_table([cam_tar(g.K[v], g.R[v], g.T[v], g.H, g.W) for v in range(3)], "cpu").numpy()
    assert np.array_equal(table[:, :21], table_rows(g.K, g.R, g.T)[:, :21])


def test_evaluate_views_refuses_two_sources_of_the_mask(ffi):
    from vanerf_amd import metrics
    net = types.SimpleNamespace(kwargs={"dr_kwargs": {"fine": True}})
    cams = [cam_tar(pinhole(20.0, 4.0, 4.0), np.eye(3), np.zeros(3), 8, 8)]
    tar, box = torch.zeros(1, 3, 8, 8), torch.ones(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="mask_from_bounds"):
        metrics.evaluate_views(net, {"dr_data": {"bounds": torch.zeros(1, 2, 3)}}, cams, tar, box, mask_from_bounds=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the kernels against the restatement
# ------------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.uint8).cpu()


def _cams(name, device="cuda"):
    g = golden(name)
    return [cam_tar(g.K[v], g.R[v], g.T[v], g.H, g.W, device) for v in range(g.K.shape[0])]


_KERNEL = {}


def kernel(name):
    """mask, table, near, far of a fixture case from one call, computed once and shared (device tensors)."""
    if name not in _KERNEL:
        from vanerf_amd import mask_at_box as mab
        _KERNEL[name] = mab.mask_at_box(_cams(name), torch.from_numpy(golden(name).bounds), per_ray=True)
    return _KERNEL[name]


def _rel(got, ref):
    """Largest relative difference where ref is finite; NaNs must sit in the same places."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    return float((np.abs(got[ok] - ref[ok]) / np.abs(ref[ok])).max()) if ok.any() else 0.0


def _assert_view(mask, table, near, far, ref, what):
    """One view of the kernel (numpy arrays) against its restatement."""
    H, W = ref.mask.shape
    assert mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 1}
    masks_agree(mask, ref.mask, ref.unsure, what)
    # slots 2-6: exactly the count and rectangle of the kernel's own mask
    assert table[2] == int(mask.sum()) and tuple(int(x) for x in table[3:7]) == bounding_rect(mask) and table[7] == 0.0, (what, table)
    # NaN off the mask, numbers on it
    assert np.array_equal(np.isnan(near), mask == 0) and np.array_equal(np.isnan(far), mask == 0), what
    both = (mask != 0) & ref.mask
    rel_ray = max(_rel(near[both], ref.near[both]), _rel(far[both], ref.far[both]))
    if np.array_equal(mask != 0, ref.mask):
        rel_slot = max(_rel(table[:2], [ref.near_min, ref.far_max]), 0.0)
    else:  # a near-threshold pixel differs: the extrema of the kernel's own rays
        rel_slot = 0.0
        assert table[0] == np.nanmin(near) and table[1] == np.nanmax(far), what
    print(f"{what}: excluded {ref.unsure.mean():.5f} mask differs on {int(((mask != 0) != ref.mask).sum())} per-ray rel {rel_ray:.2e} "
          f"slots 0-1 rel {rel_slot:.2e}")
    assert rel_ray <= TOL_RAY and rel_slot <= TOL_SLOT, (what, rel_ray, rel_slot)
    if mask.any():  # the slots are the extrema of the per-ray values, to the bit
        assert table[0] == np.nanmin(near) and table[1] == np.nanmax(far), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_kernel_matches_the_fp64_restatement(name):
    mask, table, near, far = (t.cpu().numpy() for t in kernel(name))
    g = golden(name)
    assert mask.shape == near.shape == far.shape == (g.K.shape[0], g.H, g.W) and table.shape == (g.K.shape[0], 8)
    for v, ref in enumerate(restated(name)):
        _assert_view(mask[v], table[v], near[v], far[v], ref, f"{name}[{v}]")


@pytest.mark.gpu
def test_the_central_ray_takes_the_clamp_and_agrees():
    mask, _, near, far = (t.cpu().numpy() for t in kernel("7x5"))
    ref = restated("7x5")[0]
    assert ref.mask[3, 2] and not ref.unsure[3, 2] and mask[0, 3, 2] == 1
    assert abs(near[0, 3, 2] - ref.near[3, 2]) <= TOL_RAY * ref.near[3, 2] and abs(far[0, 3, 2] - ref.far[3, 2]) <= TOL_RAY * ref.far[3, 2]


@pytest.mark.gpu
def test_a_camera_inside_the_box_sees_it_everywhere():
    mask, table, near, _ = kernel("3x70x45")
    assert bool(mask[1].all()) and table[1, 2:7].tolist() == [70.0 * 45.0, 0.0, 0.0, 45.0, 70.0] and not bool(near[1].isnan().any())


def _with_a_view_turned_away():
    """The three 70 x 45 cameras with a fourth in second place that looks past the box at a right angle.  (A camera with its back to the box
    would still see it: the definition takes the whole line of a ray, t < 0 included, which is what lets a camera inside the box see it.)"""
    g = golden("3x70x45")
    centre = g.bounds.astype(np.float64).mean(0)
    eye = centre + np.array([0.1, -0.2, 0.9])
    R, T = look_at(eye, eye + np.cross(centre - eye, [0.0, 1.0, 0.0]))
    cams = _cams("3x70x45")
    away = cam_tar(g.K[0], R, T, g.H, g.W, "cuda")
    return g, [cams[0], away, cams[1], cams[2]], table_rows(g.K[:1], R[None], T[None])[0]


@pytest.mark.gpu
def test_a_view_turned_away_from_the_box_is_empty_and_leaves_the_others_alone():
    from vanerf_amd import mask_at_box as mab
    g, cams, row = _with_a_view_turned_away()
    ref = restate(row, g.bounds, g.H, g.W)
    assert ref.n_mask == 0 and ref.rect == (0, 0, 0, 0) and np.isnan(ref.near_min) and not ref.unsure.any()
    mask, table, near, far = mab.mask_at_box(cams, torch.from_numpy(g.bounds), per_ray=True)
    assert not bool(mask[1].any()) and bool(near[1].isnan().all()) and bool(far[1].isnan().all())
    t = table[1].cpu().numpy()
    assert np.isnan(t[0]) and np.isnan(t[1]) and t[2:].tolist() == [0.0] * 6
    want = kernel("3x70x45")
    for k, v in ((0, 0), (2, 1), (3, 2)):
        for got, ref_t in zip((mask, table, near, far), want):
            assert torch.equal(_bits(got[k]), _bits(ref_t[v])), (k, v)
    zn, zf = mab.near_far(table, 2)
    assert zn.is_cuda and zn.dim() == 0 and torch.equal(zn, want[1][1, 0]) and torch.equal(zf, want[1][1, 1])


def _raw_call(ffi, cams, bounds, V, H, W, scratch, per_ray=True, fill=0.0):
    """vanerf_mask_at_box with the caller's scratch block; outputs pre-filled with `fill`."""
    mask = torch.full((V, H, W), 7, dtype=torch.uint8, device="cuda")
    near, far = (torch.full((V, H, W), fill, device="cuda") for _ in range(2)) if per_ray else (None, None)
    out = torch.full((V, 8), fill, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    b6 = (ctypes.c_float * 6)(*[float(x) for x in np.asarray(bounds).reshape(-1)])
    ffi.check(ffi.lib.vanerf_mask_at_box(ptr(cams), V, H, W, b6, ptr(mask), ptr(near), ptr(far), ptr(scratch), scratch.numel() * scratch.element_size(),
                                         ptr(out), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return mask, out, near, far


@pytest.mark.gpu
def test_calls_are_reproducible_and_ignore_what_the_scratch_block_held():
    from vanerf_amd import _ffi as ffi, renderer
    g = golden("3x70x45")
    cams = renderer.camera_table(_cams("3x70x45"), torch.device("cuda"))
    n = ffi.lib.vanerf_mask_at_box_scratch(3, g.H, g.W)
    runs = []
    for byte, fill in ((0xFF, float("nan")), (0x00, 0.0)):
        scratch = torch.full((n,), byte, dtype=torch.uint8, device="cuda")
        runs.append(_raw_call(ffi, cams, g.bounds, 3, g.H, g.W, scratch, fill=fill))
    want = kernel("3x70x45")
    for a, b, w in zip(runs[0], runs[1], want):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(w))
    # near / far left out: nothing else changes
    mask, out, _, _ = _raw_call(ffi, cams, g.bounds, 3, g.H, g.W, torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda"), per_ray=False)
    assert torch.equal(mask, want[0]) and torch.equal(_bits(out), _bits(want[1]))
    with pytest.raises(ffi.VanerfError, match="scratch"):
        _raw_call(ffi, cams, g.bounds, 3, g.H, g.W, scratch[: n // 2])


@pytest.mark.gpu
def test_a_view_gives_the_same_bits_alone_and_in_a_batch():
    from vanerf_amd import mask_at_box as mab
    g = golden("3x70x45")
    cams, want = _cams("3x70x45"), kernel("3x70x45")
    for v in range(3):
        one = mab.mask_at_box([cams[v]], torch.from_numpy(g.bounds).cuda(), per_ray=True)
        for got, w in zip(one, want):
            assert got.shape[0] == 1 and torch.equal(_bits(got[0]), _bits(w[v])), v
    out = torch.empty(3, 8, device="cuda")
    two = mab.mask_at_box(cams, g.bounds, out=out)
    assert len(two) == 2 and two[1] is out and torch.equal(two[0], want[0]) and torch.equal(_bits(out), _bits(want[1]))


@pytest.mark.gpu
def test_image_metrics_reads_the_same_rectangle_and_count():
    from vanerf_amd import metrics
    for name in ("40x21", "3x70x45"):
        mask, table = kernel(name)[:2]
        V, H, W = mask.shape
        img = torch.rand(V, 3, H, W, device="cuda")
        s = metrics.image_metrics(img, img * 0.5, mask=mask, mask_at_box=mask)
        assert torch.equal(s[:, 6], table[:, 5]) and torch.equal(s[:, 7], table[:, 6]) and torch.equal(s[:, 5], table[:, 2]), name


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the evaluation driver
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_evaluate_views_makes_its_masks_from_the_bounds():
    from vanerf_amd import mask_at_box as mab, metrics
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
    tar = torch.rand(3, 3, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    bounds = trb["dr_data"]["bounds"]

    boxes, table = mab.mask_at_box(cam_tars, bounds)
    assert boxes.shape == (3, H, W) and boxes.dtype == torch.uint8 and table.shape == (3, 8)
    made, images = metrics.evaluate_views(net, trb, cam_tars, tar, None, mask_from_bounds=True)
    given, images_g = metrics.evaluate_views(net, trb, cam_tars, tar, boxes)
    assert torch.equal(_bits(made), _bits(given)) and all(torch.equal(a, b) for a, b in zip(images, images_g))
    grouped, _ = metrics.evaluate_views(net, trb, cam_tars, tar, None, views_per_pass=2, mask_from_bounds=True)
    assert torch.equal(_bits(made), _bits(grouped))
    # the default path is what it was: image_metrics on the rendered views with the masks it is given
    direct = metrics.image_metrics(torch.stack(images_g), tar, mask_at_box=boxes, clamp_pred=True)
    assert torch.equal(_bits(given), _bits(direct))
    assert torch.equal(made[:, 6], table[:, 5]) and torch.equal(made[:, 7], table[:, 6])
    with pytest.raises(ValueError, match="mask_from_bounds"):
        metrics.evaluate_views(net, trb, cam_tars, tar, boxes, mask_from_bounds=True)
