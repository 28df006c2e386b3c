"""The hand-over of all-invalid groups from the lean bf16x3 kernel to the short-only kernel (vanerf_amd/csrc/query_kernel.hip:
query_kernel<1, false, 2, HANDOVER> and query_short_kernel<2>; VANERF_SHORT_KERNEL).

A launch with a validity partition is two launches: the full kernel leaves at its first all-invalid round and records where in the second word
of the launch's queue word, the short-only kernel runs every group from there on.  The short-only kernel calls the stages of the full kernel's
short path with the same arguments in the same order, so every case here asserts EQUAL BITS against the single launch (VANERF_SHORT_KERNEL=0,
the parent's kernel) -- outputs, validity flags, and the short_groups counter bench.py prices FLOPs with -- never a tolerance."""
import contextlib
import os
from ctypes import byref

import pytest
import torch

from vanerf_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


@contextlib.contextmanager
def short_kernel(value):
    """VANERF_SHORT_KERNEL for the launches inside (the library reads it at every launch); None: unset."""
    keep = os.environ.pop("VANERF_SHORT_KERNEL", None)
    if value is not None:
        os.environ["VANERF_SHORT_KERNEL"] = value
    try:
        yield
    finally:
        os.environ.pop("VANERF_SHORT_KERNEL", None)
        if keep is not None:
            os.environ["VANERF_SHORT_KERNEL"] = keep


def _frame_data(R, sd, frame, mask=None):
    fd = synth.to_device(frame, "cuda")
    sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
    fg = fd["src_foreground_mask"] if mask is None else torch.full_like(fd["src_foreground_mask"], mask)
    return R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fg, fd["cam_in"], fd["targets"], fd["sp_data"])


@pytest.fixture(scope="module")
def case(R):
    """The half-masked frame of the lean and vertex-product tests with its mask as it is, zeroed and all ones; 8 192 + 37 points on rays of the
    target view (mixed population) and as many around the hand's vertices (inside the source view: valid wherever the mask is set); one lean
    bf16x3 handle.  Mesh queries once."""
    sd = synth.make_full_weights(0)
    frame = synth.make_frame(seed=5, tar_h=128, tar_w=128, orbit_deg=40.0, half_mask=True)
    fdats = {m: _frame_data(R, sd, frame, v) for m, v in (("half", None), ("zero", 0.0), ("one", 1.0))}
    fdat = fdats["half"]
    nmax = 8192 + 37
    rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 0, 0, 1, 128, 128, 16, device="cuda")
    ray_pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"])
    # every 31st sample: all depths and the whole image, so that both populations are well represented
    ray_pts = ray_pts[torch.arange(nmax, device="cuda") * 31 % ray_pts.shape[0]].contiguous()
    g = torch.Generator().manual_seed(2)
    v = fdat.verts3[torch.randint(0, fdat.verts3.shape[0], (2 * nmax,), generator=g).cuda()]
    near_pts = (v + 0.002 * torch.randn(2 * nmax, 3, generator=g).cuda()).contiguous()
    w = R.PackedWeights(sd, mode="bf16x3")
    assert R.lean_stream_enabled() and all(f.vertex_products(w) is not None for f in fdats.values())
    inputs = {}
    with short_kernel("0"):
        # "near": the points around the vertices that the source view holds (valid under the all-ones mask)
        ok = R.query_samples(w, fdats["one"], near_pts, *R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, near_pts), want_valid=True)[1].bool()
        assert int(ok.sum()) >= 8192
        near_pts = near_pts[ok][:8192].contiguous()
        # "mixed": 1 000 valid and 312 invalid ray points, shuffled -- the partition puts the boundary at slot 1 000, inside the fourth round of
        # 256 slots, and leaves 41 - 32 = 9 groups to the short-only kernel
        ok = R.query_samples(w, fdat, ray_pts, *R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, ray_pts), want_valid=True)[1].bool()
        assert int(ok.sum()) >= 1000 and int((~ok).sum()) >= 312
        mixed = torch.cat([ray_pts[ok][:1000], ray_pts[~ok][:312]])[torch.randperm(1312, generator=g).cuda()].contiguous()
    for name, pts in (("rays", ray_pts), ("near", near_pts), ("mixed", mixed)):
        inputs[name] = (pts,) + tuple(R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts))
    return {"R": R, "sd": sd, "frame": frame, "fdats": fdats, "w": w, "inputs": inputs}


def _expected_word(nv, n):
    """The hand-over word of a launch whose partition holds nv valid samples: the complement of the base of the first round (8 groups = 256
    slots) without a valid sample, 0 if there is no such round."""
    start = (nv + 255) // 256 * 8
    return (~start) & 0xffffffff if start < (n + 31) // 32 else 0


def _launch(c, mask, pts_name, n, switch, with_order=True, raw=False, noise=None):
    """One vanerf_query_samples with a queue word of the test's own -> outputs, flags, short_groups delta, the queue's second word."""
    from vanerf_amd._ffi import lib
    R, w, fdat = c["R"], c["w"], c["fdats"][mask]
    p, s, v, k = (t[:n].contiguous() for t in c["inputs"][pts_name])
    order = R.query_order(fdat, p) if with_order else None
    out = torch.empty(n, 5, dtype=torch.float32, device="cuda")
    valid = torch.empty(n, dtype=torch.uint8, device="cuda")
    queue = torch.full((2,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")  # the library zeroes it
    with short_kernel(switch):
        c0 = w.short_groups()
        R.check(lib.vanerf_query_samples(w.handle, byref(fdat.c), R._ptr(p), R._ptr(s), R._ptr(v), R._ptr(k), R._ptr(noise), R._ptr(order),
                                         int(raw), n, R._ptr(out), R._ptr(valid), R._ptr(queue), R._ptr(fdat.vertex_products(w)), R._stream()))
        short = w.short_groups() - c0
    return out, valid, short, int(queue[1].item()) & 0xffffffff


def _same(a, b, what):
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), f"{what}: outputs differ"
    assert torch.equal(a[1], b[1]), f"{what}: validity flags differ"
    assert a[2] == b[2], f"{what}: short_groups {a[2]} vs {b[2]}"


@pytest.mark.parametrize("n", [8192, 8192 + 37, 256 * 5 + 32])
def test_mixed_population_is_bit_identical(case, n):
    """Mixed populations; ragged last group; and n = 1 312 = 41 groups, where the boundary between valid and invalid falls inside a
    block-round and the short range is shorter than one block of the short-only kernel."""
    pts = "mixed" if n == 256 * 5 + 32 else "rays"
    off = _launch(case, "half", pts, n, "0")
    on = _launch(case, "half", pts, n, None)
    _same(on, off, f"n={n}")
    nv = int(off[1].sum())
    assert 0 < nv < n - 256 and off[3] == 0  # both populations; a single launch never writes the hand-over word
    ngroups = (n + 31) // 32
    # the full kernel left at the first round without a valid sample: the round behind the one that holds the last valid sample
    assert on[3] == _expected_word(nv, n) != 0
    if n == 256 * 5 + 32:
        assert nv == 1000 and ngroups - ((~on[3]) & 0xffffffff) == 9
    assert 0 < off[2] < ngroups


def test_all_invalid_runs_in_the_short_kernel_alone(case):
    """Mask zeroed: every block of the full kernel leaves at its first round, the hand-over word is ~0 and every group is a short group."""
    n = 8192 + 37
    off = _launch(case, "zero", "rays", n, "0")
    on = _launch(case, "zero", "rays", n, None)
    _same(on, off, "all invalid")
    assert not off[1].any() and on[3] == 0xffffffff and on[2] == (n + 31) // 32


def test_all_valid_leaves_the_word_zero(case):
    """Mask all ones, points inside the source view: no block meets an all-invalid round, the word stays 0 and the second launch is a no-op."""
    n = 8192
    off = _launch(case, "one", "near", n, "0")
    on = _launch(case, "one", "near", n, None)
    _same(on, off, "all valid")
    assert off[1].all() and on[3] == 0 and on[2] == 0


def test_raw_outputs_with_flags_and_noise(case):
    """raw = 1 ([sdf_pred, rad, r, g, b] + validity flags) and eval_func with per-sample noise, mixed population."""
    n = 8192 + 37
    _same(_launch(case, "half", "rays", n, None, raw=True), _launch(case, "half", "rays", n, "0", raw=True), "raw")
    noise = torch.randn(n, generator=torch.Generator().manual_seed(4)).cuda()
    _same(_launch(case, "half", "rays", n, None, noise=noise), _launch(case, "half", "rays", n, "0", noise=noise), "noise")


@pytest.mark.parametrize("n", [8192, 8192 + 37, 256 * 5 + 32])
def test_without_a_partition_nothing_changes(case, n):
    """order = None: one launch whatever the switch says -- the same bits, and the second word of the queue stays 0."""
    off = _launch(case, "half", "rays", n, "0", with_order=False)
    on = _launch(case, "half", "rays", n, None, with_order=False)
    _same(on, off, f"no order, n={n}")
    assert on[3] == 0 and off[3] == 0
    # the partition changes the order of work only (and with it how many groups are all-invalid: the counters are not comparable)
    part = _launch(case, "half", "rays", n, None)
    assert torch.equal(on[0].view(torch.int32), part[0].view(torch.int32)) and torch.equal(on[1], part[1])


PASS_KEYS = ("index", "hit", "z", "color", "depth", "alpha", "color_fine", "depth_fine", "alpha_fine", "sdf", "z_fine")


@pytest.mark.parametrize("entry", ["render_pass_c", "render_pass"])
def test_a_pass_that_partitions(case, entry):
    """64 x 64 rays at 64 + 64 samples: 262 144 samples per march, the smallest that partitions.  Every output of the pass, switch on and off."""
    R, w, fdat, frame = case["R"], case["w"], case["fdats"]["half"], case["frame"]
    assert 64 * 64 * 64 >= R.PARTITION_MIN_SAMPLES
    args = (w, fdat, frame["cam_tar"], frame["bounds"], 0, 0, 2, 64, 64, 64, 64)
    with short_kernel("0"):
        c0 = w.short_groups()
        off = getattr(R, entry)(*args)
        short_off = w.short_groups() - c0
    with short_kernel(None):
        c0 = w.short_groups()
        on = getattr(R, entry)(*args)
        short_on = w.short_groups() - c0
    for k in PASS_KEYS:
        assert torch.equal(on[k], off[k]), k
    assert short_on == short_off and 0 < short_on < 2 * 64 * 64 * 64 // 32
    assert on["hit"].any() and on["alpha_fine"].max() > 0
