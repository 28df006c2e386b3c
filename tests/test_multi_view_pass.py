"""Several target views of one source frame in a single pass (VanerfPassDesc.cams / n_views behind vanerf_ray_setup and vanerf_render_pass,
renderer.render_pass_views, VANeRF.render_pifu_nerf_views, render_novel_views(views_per_pass=...)).

Behind the ray setup nothing in a pass depends on the camera except the ray origin, and both ray kernels run one ray function, so a pass over
V views must give, view after view, the BITS of V single-view passes: every comparison on the GPU below is torch.equal, none has a tolerance.
The CPU tests cover the ABI surface (exports, scratch sizes, argument errors) and the frame grouping of the driver with a stub renderer."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vanerf_amd import synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("index", "hit", "z", "color", "depth", "alpha", "color_fine", "depth_fine", "alpha_fine", "sdf", "z_fine")


@pytest.fixture(scope="module")
def ffi():
    from vanerf_amd import _ffi
    return _ffi


# ------------------------------------------------------------------------------------------------
# CPU: ABI surface
# ------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported_and_declared(ffi):
    """ABI 12: the multi-view pass is the camera-table form of the one pass descriptor; the exports are exactly what the header declares."""
    header = open(os.path.join(REPO, "include", "vanerf_hip.h")).read()
    assert set(re.findall(r"\b(vanerf_[a-z0-9_]+)\s*\(", header)) == set(ffi.EXPORTS)
    for name in ("vanerf_ray_setup", "vanerf_sample_points", "vanerf_render_pass_scratch", "vanerf_render_pass"):
        assert name in ffi.EXPORTS and hasattr(ffi.lib, name)
        assert f"{name}(" in header
    assert not [n for n in ffi.EXPORTS if n.endswith("_views") or n.startswith("vanerf_ray_setup") and n != "vanerf_ray_setup"]  # one entry each: no per-form twins
    fields = [f for f, _ in ffi.VanerfPassDesc._fields_]
    assert "n_views" in fields and "cams" in fields and "const float* cams;" in header and "int n_views;" in header
    assert header.count("} VanerfPassDesc;") == 1 and "ViewsDesc" not in header  # one pass descriptor
    assert ffi.ABI_VERSION == 12 and ffi.lib.vanerf_abi_version() == 12 and "#define VANERF_ABI_VERSION 12" in header


def test_views_scratch_size(ffi):
    scratch = ffi.lib.vanerf_render_pass_scratch
    for R, Sc, Sf, fine, reuse in ((64 * 64, 16, 16, 1, 1), (40 * 20, 16, 16, 1, 0), (256 * 256, 64, 64, 1, 1), (64 * 64, 16, 16, 0, 1)):
        single = scratch(1, R, Sc, Sf, fine, reuse if fine else 0)
        sizes = [scratch(V, R, Sc, Sf, fine, reuse) for V in (1, 2, 3, 4, 8, 16)]
        assert single > 0 and sizes[0] >= single
        assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        assert sizes[3] <= 4 * sizes[0]  # a group needs no more than its views would need one by one
        for r in (0, 1, 2):  # a single view under every re-use mode (2: per-sample noise, more temporaries) fits what two views need
            assert 0 < scratch(1, R, Sc, Sf, fine, r) <= scratch(2, R, Sc, Sf, fine, r), (R, Sc, Sf, fine, r)
    for bad in ((0, 4096, 16, 16, 1, 1), (-1, 4096, 16, 16, 1, 1), (2, 0, 16, 16, 1, 1), (2, -5, 16, 16, 1, 1), (2, 4096, 0, 16, 1, 1), (2, 4096, 16, -1, 1, 1)):
        assert scratch(*bad) == 0, bad
    # 0 also for a shape the pass itself refuses (16 M rays x 128 samples do not fit the 32-bit sample index), so that 0 means "not a valid pass"
    assert scratch(16, 1024 * 1024, 64, 64, 1, 0) == 0
    assert scratch(16, 1024 * 1024, 64, 64, 1, 1) > 0  # with coarse re-use the largest march has 64 per ray


def _views_desc(ffi, p, **kw):
    """2 views of 16 x 16 rays at 16 + 16 samples from a camera table; p: a pointer that is never dereferenced."""
    d = ffi.VanerfPassDesc()
    d.n_views, d.x0, d.y0, d.step_x, d.step_y, d.y_block, d.nx, d.ny, d.width = 2, 0, 0, 1, 1, 1, 16, 16, 16
    d.cams, d.Sc, d.Sf, d.fine, d.reuse_coarse, d.t_lin_c, d.t_lin_f = p, 16, 16, 1, 1, p, p
    d.bounds = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_ray_setup_views_rejects_bad_arguments(ffi):
    lib = ffi.lib
    p = ctypes.c_void_p(8)  # never dereferenced: every call below fails its argument checks before anything touches a GPU

    def call(d="desc", index=p, cam_pos=p, z=p, **kw):
        d = _views_desc(ffi, p, **kw) if d == "desc" else d
        return lib.vanerf_ray_setup(ctypes.byref(d) if d is not None else None, index, p, cam_pos, p, p, p, z, None)

    assert call(None) == -22 and b"null" in lib.vanerf_last_error()  # no descriptor
    assert call(t_lin_c=None) == -22 and b"null" in lib.vanerf_last_error()  # the linspace table is required
    for out in ("index", "cam_pos", "z"):
        assert call(**{out: None}) == -22 and b"null" in lib.vanerf_last_error()
    assert call(cams=None) == -22 and b"n_views" in lib.vanerf_last_error() and b"cams" in lib.vanerf_last_error()  # two views need a table
    for V in (0, -3, 65536):
        assert call(n_views=V) == -22 and b"n_views" in lib.vanerf_last_error()
        assert call(n_views=V, cams=None) == -22 and b"n_views" in lib.vanerf_last_error()
    assert call(Sc=1) == -22 and b"S=1" in lib.vanerf_last_error()
    assert call(nx=0) == -22 and b"nx=0" in lib.vanerf_last_error()
    assert call(n_views=1, cams=None, Sc=1) == -22 and b"S=1" in lib.vanerf_last_error()  # the by-value form makes the same grid checks
    assert call(n_views=1, cams=None, nx=0) == -22 and b"nx=0" in lib.vanerf_last_error()
    assert call(n_views=1, cams=None, step_x=0) == -22 and b"bad grid" in lib.vanerf_last_error()
    assert call(n_views=8, nx=4096, ny=4096, Sc=64) == -22 and b"32-bit" in lib.vanerf_last_error()  # 8.6e9 samples
    # the table form is the evaluation form: the plain grid only
    assert call(pixels_xy=p) == -22 and b"pixels_xy" in lib.vanerf_last_error()
    assert call(row_blocks=p) == -22 and b"row_blocks" in lib.vanerf_last_error()
    assert call(y_block=2) == -22 and b"y_block" in lib.vanerf_last_error()
    # rows as a list of blocks (by-value camera): ny is a whole number of blocks
    assert call(n_views=1, cams=None, row_blocks=p, y_block=8, ny=20) == -22 and b"y_block" in lib.vanerf_last_error() and b"row_blocks" in lib.vanerf_last_error()
    assert call(n_views=1, cams=None, row_blocks=p, y_block=0) == -22 and b"bad grid" in lib.vanerf_last_error()
    assert lib.vanerf_sample_points(p, p, p, 10, 4, 8, p, None) == -22 and b"whole number of views" in lib.vanerf_last_error()
    assert lib.vanerf_sample_points(None, p, p, 8, 4, 8, p, None) == -22 and b"null" in lib.vanerf_last_error()
    assert lib.vanerf_sample_points(None, p, p, 8, 0, 8, p, None) == -22 and b"null" in lib.vanerf_last_error()
    assert lib.vanerf_sample_points(p, p, p, 8, -1, 8, p, None) == -22 and b"rays_per_view=-1" in lib.vanerf_last_error()


def test_render_pass_views_rejects_bad_arguments(ffi):
    lib = ffi.lib
    p = ctypes.c_void_p(8)
    frame, accel = ffi.VanerfFrame(), ffi.VanerfMeshAccel()
    desc = lambda **kw: _views_desc(ffi, p, **kw)
    out = ffi.VanerfPassOut()
    for k in ("index", "hit", "z", "color", "depth", "alpha"):
        setattr(out, k, p)

    def call(d, w=p, o=out, scratch=p, nbytes=0):
        return lib.vanerf_render_pass(w, ctypes.byref(frame), ctypes.byref(accel), p, 4, p, 4, ctypes.byref(d) if d is not None else None,
                                      ctypes.byref(o), scratch, nbytes, None, None)

    assert call(desc(), w=None) == -22 and b"null" in lib.vanerf_last_error()
    assert call(None) == -22 and b"null" in lib.vanerf_last_error()
    assert call(desc(), scratch=None) == -22 and b"null" in lib.vanerf_last_error()
    for V in (0, -1):
        assert call(desc(n_views=V)) == -22 and f"n_views={V}".encode() in lib.vanerf_last_error()
    assert call(desc(Sc=1)) == -22 and b"Sc=1" in lib.vanerf_last_error()
    assert call(desc(Sf=0)) == -22 and b"Sf=0" in lib.vanerf_last_error()
    assert call(desc(cams=None)) == -22 and b"n_views" in lib.vanerf_last_error() and b"cams" in lib.vanerf_last_error()  # n_views = 2 without a camera table
    assert call(desc(t_lin_c=None)) == -22 and b"linspace" in lib.vanerf_last_error()
    assert call(desc(t_lin_f=None)) == -22 and b"linspace" in lib.vanerf_last_error()  # no importance draws and no table to take their place
    assert call(desc(), o=ffi.VanerfPassOut()) == -22 and b"output pointer" in lib.vanerf_last_error()
    assert call(desc(n_views=8, nx=4096, ny=4096, Sc=64, Sf=64)) == -22 and b"32-bit" in lib.vanerf_last_error()
    assert call(desc(n_views=16, nx=1024, ny=1024, Sc=64, Sf=64, reuse_coarse=0)) == -22 and b"32-bit" in lib.vanerf_last_error()  # 16 M rays x 128
    assert call(desc(n_views=1, cams=None, nx=4096, ny=4096, Sc=64, Sf=64, reuse_coarse=0)) == -22 and b"32-bit" in lib.vanerf_last_error()  # every pass
    assert call(desc(), nbytes=1024) == -22 and b"scratch" in lib.vanerf_last_error()  # valid arguments, a block that is too small
    assert call(desc(n_views=1, cams=None), nbytes=1024) == -22 and b"scratch" in lib.vanerf_last_error()  # the same with the camera by value
    # the table form is the evaluation form: each field it does not take is refused by name
    assert call(desc(pixels_xy=p)) == -22 and b"pixels_xy" in lib.vanerf_last_error()
    assert call(desc(row_blocks=p)) == -22 and b"row_blocks" in lib.vanerf_last_error()
    assert call(desc(y_block=2)) == -22 and b"y_block" in lib.vanerf_last_error()
    assert call(desc(noise_c=p, noise_f=p)) == -22 and b"noise_c" in lib.vanerf_last_error()
    assert call(desc(noise_c=p)) == -22 and b"noise_c" in lib.vanerf_last_error()
    assert call(desc(n_views=1, cams=None, noise_c=p)) == -22 and b"noise_c without noise_f" in lib.vanerf_last_error()  # (by value: as before)


# ------------------------------------------------------------------------------------------------
# CPU: frame grouping of the driver (stub renderers)
# ------------------------------------------------------------------------------------------------
def _stub_cameras(n, h=32, w=32):
    cams = []
    for i in range(n):
        k = torch.eye(4)[None].clone()
        k[0, 3, 3] = i  # the tag of the camera, as tests/test_novel_views.py carries it
        cams.append({"w2cs": torch.eye(4), "intrinsics": k, "im_w": w, "im_h": h, "znear": 0.5, "zfar": 2.0})
    return cams


def _stub_frame(cam_tar):
    tag = float(cam_tar["K"][0, 3, 3])
    return {"tex_fg_fine": torch.full((3, cam_tar["height"], cam_tar["width"]), tag / 255.0)}


def _stub_render(net, tr_batch, cam_tar, level):
    return _stub_frame(cam_tar)


def _tr_batch():
    return {"im": torch.rand(1, 3, 64, 64), "dr_data": {"bounds": None}}


@pytest.mark.parametrize("group", [1, 3, 4])
def test_grouped_orbit_equals_the_per_frame_orbit_with_stub_renderers(group):
    from vanerf_amd.novel_views import render_novel_views
    cams = _stub_cameras(10)
    want, _ = render_novel_views(None, cams, _tr_batch(), only_renderings=True, render_fn=_stub_render)
    calls, seen = [], []

    def render_views(net, tr_batch, cam_tars, level):
        calls.append([int(c["K"][0, 3, 3]) for c in cam_tars])
        return [_stub_frame(c) for c in cam_tars]

    got, _ = render_novel_views(None, cams, _tr_batch(), only_renderings=True, render_views_fn=render_views, views_per_pass=group,
                                on_frame=lambda fi, img: seen.append((fi, int(img[0, 0, 0]))))
    assert np.array_equal(got, want) and got.shape == (10, 32, 32, 3)
    assert seen == [(i, i) for i in range(10)]  # once per frame, in frame order, each with its own image
    assert calls == [list(range(k, min(k + group, 10))) for k in range(0, 10, group)]  # consecutive groups, the last one short
    # the rank partition is the per-frame one: rank r of 2 renders frames r, r + 2, ... in groups of consecutive frames of ITS list
    for rank in range(2):
        calls.clear()
        own, _ = render_novel_views(None, cams, _tr_batch(), only_renderings=True, rank=rank, world=2, render_views_fn=render_views, views_per_pass=group)
        mine = list(range(rank, 10, 2))
        assert own[:, 0, 0, 0].tolist() == mine
        assert calls == [mine[k:k + group] for k in range(0, 5, group)]


def test_grouped_orbit_argument_errors_and_mixed_sizes():
    from vanerf_amd.novel_views import render_novel_views
    cams = _stub_cameras(4)
    views = lambda net, trb, cam_tars, level: [_stub_frame(c) for c in cam_tars]
    with pytest.raises(ValueError, match="shard"):
        render_novel_views(None, cams, _tr_batch(), shard="rays", views_per_pass=2, render_views_fn=views)
    with pytest.raises(ValueError):
        render_novel_views(None, cams, _tr_batch(), views_per_pass=0, render_views_fn=views)
    with pytest.raises(ValueError, match="render_views_fn"):
        render_novel_views(None, cams, _tr_batch(), views_per_pass=2, render_fn=_stub_render)  # a per-frame stub cannot render groups
    with pytest.raises(ValueError, match="returned"):
        render_novel_views(None, cams, _tr_batch(), views_per_pass=2, render_views_fn=lambda *a: [])
    # the default stays per frame: a plain render_fn call is untouched by the new arguments
    trb = _tr_batch()  # (the source image is pasted to the left of every frame)
    a = render_novel_views(None, cams, trb, render_fn=_stub_render)
    b = render_novel_views(None, cams, trb, render_fn=_stub_render, views_per_pass=1)
    assert np.array_equal(a, b)
    # a group never mixes image sizes
    calls = []
    mixed = _stub_cameras(2) + _stub_cameras(2, h=16, w=16)

    def record(net, trb, cam_tars, level):
        calls.append([c["height"] for c in cam_tars])
        return [_stub_frame(c) for c in cam_tars]

    with pytest.raises(RuntimeError):  # (the stack of two sizes cannot be formed: as without grouping)
        render_novel_views(None, mixed, _tr_batch(), views_per_pass=4, render_views_fn=record)
    assert calls == [[32, 32], [16, 16]]


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def sd():
    return synth.make_full_weights(0)


_SCENES = {}


def _scene(R, sd, W, H, n_frames=8):
    """synth frame (source camera as synth makes it), its per-frame tables, and the cam_tar dicts of a get_360cameras orbit around the hands."""
    key = (W, H, n_frames)
    if key not in _SCENES:
        from vanerf_amd.model import get_360cameras
        from vanerf_amd.novel_views import camera_to_cam_tar
        frame_cpu = synth.make_frame(seed=3, tar_h=H, tar_w=W)
        fd = synth.to_device(frame_cpu, "cuda")
        sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
        fdat = R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
        headpose = torch.eye(4)
        headpose[:3, 3] = frame_cpu["targets"]["vert_world"][0].mean(0)
        cams = get_360cameras(headpose[:3, :4].cuda(), 4.0 * max(W, H), 1.0, 1.0, W, H, 0.71, 1.42, n_frames=n_frames)
        _SCENES[key] = (fdat, [camera_to_cam_tar(c) for c in cams], fd["bounds"])
    return _SCENES[key]


def _weights(R, sd, precision, _cache={}):
    if precision not in _cache:
        _cache[precision] = R.PackedWeights(sd, mode=precision)
    return _cache[precision]


def _same_as_single_passes(R, w, fdat, cam_tars, bounds, grid, Sc, Sf, jitter=None, u=None, scratch=None, **kw):
    """render_pass_views over cam_tars against render_pass_c per camera: every returned tensor, every view, torch.equal."""
    x0, y0, step, nx, ny = grid
    V, Rn = len(cam_tars), nx * ny
    got = R.render_pass_views(w, fdat, cam_tars, bounds, x0, y0, step, nx, ny, Sc, Sf, jitter=jitter, u=u, scratch=scratch, **kw)
    singles = []
    for v, cam in enumerate(cam_tars):
        jv = None if jitter is None else jitter.view(V, Rn, Sc)[v].contiguous()
        uv = None if u is None else u.view(V, Rn, Sf)[v].contiguous()
        one = R.render_pass_c(w, fdat, cam, bounds, x0, y0, step, nx, ny, Sc, Sf, jitter=jv, u=uv, **kw)
        assert set(one) == set(got)
        for k in KEYS:
            if k in one:
                assert got[k].shape == (V,) + tuple(one[k].shape), k
                assert torch.equal(got[k][v], one[k]), (k, v, grid, Sc, Sf, kw)
        singles.append(one)
    torch.cuda.synchronize()
    return got, singles


@pytest.mark.gpu
def test_ray_setup_views_equals_ray_setup_per_view(R, sd):
    """One ray function behind both kernels: index, directions, origin, clip range, hit flags and coarse depths of every view carry the bits of
    the single-view kernel, with and without stratification draws, on a plain grid, a strided one and one whose 256-ray blocks end mid-row."""
    fdat, cams, bounds = _scene(R, sd, 64, 64)
    g = torch.Generator(device="cuda").manual_seed(1)
    for x0, y0, step, nx, ny, S in ((0, 0, 1, 64, 64, 16), (1, 1, 2, 31, 31, 12), (0, 0, 1, 40, 20, 16), (3, 5, 4, 13, 7, 64)):
        for V in (1, 3, 8):
            for jit in (False, True):
                jitter = torch.rand(V * nx * ny, S, device="cuda", generator=g) if jit else None
                got = R.ray_setup_views(cams[:V], bounds, x0, y0, step, nx, ny, S, jitter=jitter)
                for v in range(V):
                    jv = None if jitter is None else jitter.view(V, nx * ny, S)[v].contiguous()
                    one = R.ray_setup(cams[v], bounds, x0, y0, step, nx, ny, S, jitter=jv)
                    for k in ("index", "rays_d", "near", "far", "hit", "z"):
                        assert torch.equal(got[k][v], one[k]), (k, v, V, jit, nx, ny)
                    assert torch.equal(got["cam_pos"][v, :3], one["cam_pos"]), (v, V)
                assert got["hit"].any() and not got["hit"].all()
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_one_view_table_pass_equals_the_by_value_pass(R, sd, precision):
    """vanerf_render_pass itself (descriptors filled here, not by the renderer's wrappers), one target camera, twice: cams = NULL with the camera
    by value, and n_views = 1 with a one-row camera table.  20 x 13 = 260 rays (two 256-ray blocks, a tail of 4), 16 + 16 samples, fine, coarse
    re-use, jitter and u handed in.  The two forms differ in where the camera comes from, in the layout of cam_pos ([3] / [1][4]) and in
    rays_per_view (0 / 260): every field of VanerfPassOut must carry the same bits, and a direct vanerf_ray_setup must write the same origin."""
    ffi, lib = R._ffi, R._ffi.lib
    w = _weights(R, sd, precision)
    fdat, cams, bounds = _scene(R, sd, 64, 64)
    cam, nx, ny, Sc, Sf = cams[1], 20, 13, 16, 16
    Rn, dev = nx * ny, fdat.verts3.device
    g = torch.Generator(device="cuda").manual_seed(11)
    jitter, u = torch.rand(Rn, Sc, device="cuda", generator=g), torch.rand(Rn, Sf, device="cuda", generator=g)
    t_c, t_f = torch.linspace(0.0, 1.0, Sc).cuda(), torch.linspace(0.0, 1.0, Sf).cuda()
    table = R.camera_table([cam], dev)
    assert table.shape == (1, 24)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def desc(by_value):
        d = ffi.VanerfPassDesc()
        d.x0, d.y0, d.step_x, d.step_y, d.y_block, d.nx, d.ny, d.width, d.n_views = 2, 4, 3, 3, 1, nx, ny, int(cam["width"]), 1
        if by_value:
            inv_K_T, RT, (d.znear, d.zfar) = R._camera_floats(cam)
            d.invK_T, d.RT = (ctypes.c_float * 9)(*inv_K_T), (ctypes.c_float * 12)(*RT)
        else:
            d.cams = ptr(table)
        d.bounds = (ctypes.c_float * 6)(*R.host_copy(bounds).reshape(-1).tolist())
        d.Sc, d.Sf, d.fine, d.reuse_coarse = Sc, Sf, 1, 1
        d.t_lin_c, d.t_lin_f, d.jitter, d.u = ptr(t_c), ptr(t_f), ptr(jitter), ptr(u)
        return d

    nbytes = lib.vanerf_render_pass_scratch(1, Rn, Sc, Sf, 1, 1)
    assert nbytes > 0
    shapes = {"index": ((Rn,), torch.int64), "hit": ((Rn,), torch.uint8), "z": ((Rn, Sc), None), "color": ((Rn, 3), None), "depth": ((Rn,), None),
              "alpha": ((Rn,), None), "color_fine": ((Rn, 3), None), "depth_fine": ((Rn,), None), "alpha_fine": ((Rn,), None), "sdf": ((Rn,), None),
              "z_fine": ((Rn, Sc + Sf), None)}
    assert set(shapes) == {f for f, _ in ffi.VanerfPassOut._fields_}
    results, origins = [], []
    for by_value in (True, False):
        d = desc(by_value)
        out = {k: torch.full(shape, 77, dtype=dtype or torch.float32, device=dev) for k, (shape, dtype) in shapes.items()}
        o = ffi.VanerfPassOut()
        for k, t in out.items():
            setattr(o, k, ptr(t))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ffi.check(lib.vanerf_render_pass(w.handle, ctypes.byref(fdat.c), ctypes.byref(fdat.accel.c), ptr(fdat.verts3), fdat.verts3.shape[0], ptr(fdat.faces),
                                         fdat.faces.shape[0], ctypes.byref(d), ctypes.byref(o), ptr(scratch), nbytes, None, None))
        rays = {k: torch.empty(shape, dtype=dtype or torch.float32, device=dev)
                for k, (shape, dtype) in dict(index=shapes["index"], rays_d=((Rn, 3), None), near=((Rn,), None), far=((Rn,), None), hit=shapes["hit"], z=shapes["z"]).items()}
        cam_pos = torch.full((3,) if by_value else (1, 4), 77.0, device=dev)
        ffi.check(lib.vanerf_ray_setup(ctypes.byref(d), ptr(rays["index"]), ptr(rays["rays_d"]), ptr(cam_pos), ptr(rays["near"]), ptr(rays["far"]), ptr(rays["hit"]),
                                       ptr(rays["z"]), None))
        torch.cuda.synchronize()
        for k in ("index", "hit", "z"):  # the pass's rays are those of a direct ray setup
            assert torch.equal(rays[k], out[k]), (k, by_value)
        results.append(out)
        origins.append(cam_pos.reshape(-1)[:3].clone())
    for k in shapes:
        assert torch.equal(results[0][k], results[1][k]), k
        assert not torch.isnan(results[0][k].float()).any(), k
    assert torch.equal(origins[0], origins[1]) and not (origins[0] == 77.0).any()
    assert results[0]["hit"].any() and results[0]["color_fine"].std().item() > 1e-3  # the hands are in view


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_render_pass_views_equals_single_passes(R, sd, precision):
    """64x64 and 40x20 (ny not a multiple of 8: mesh-query tiles straddle two views and must fall back to the per-lane search without changing
    a bit) at 16 + 16 samples and V = 3; coarse only; no coarse re-use; stratification and importance draws handed in; a strided grid."""
    w = _weights(R, sd, precision)
    fdat, cams, bounds = _scene(R, sd, 64, 64)
    _same_as_single_passes(R, w, fdat, cams[:3], bounds, (0, 0, 1, 64, 64), 16, 16)
    fd2, cams2, b2 = _scene(R, sd, 40, 20)
    _same_as_single_passes(R, w, fd2, cams2[:3], b2, (0, 0, 1, 40, 20), 16, 16)
    got, _ = _same_as_single_passes(R, w, fdat, cams[1:4], bounds, (0, 0, 1, 64, 64), 16, 16, fine=False)
    assert "color_fine" not in got
    _same_as_single_passes(R, w, fdat, cams[2:5], bounds, (0, 0, 1, 64, 64), 16, 16, reuse_coarse=False)
    g = torch.Generator(device="cuda").manual_seed(7)
    n = 3 * 64 * 64
    _same_as_single_passes(R, w, fdat, cams[:3], bounds, (0, 0, 1, 64, 64), 16, 16, jitter=torch.rand(n, 16, device="cuda", generator=g),
                           u=torch.rand(n, 16, device="cuda", generator=g))
    _same_as_single_passes(R, w, fdat, cams[:3], bounds, (1, 1, 2, 31, 31), 16, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_batch_crosses_the_partition_threshold(R, sd, precision):
    """64x64 at 16 samples, V = 8: the group's march has 2^19 samples and is partitioned by validity, a single view's 2^16 are not.  The
    partition only reorders the work of the per-sample kernel: no bit may change."""
    w = _weights(R, sd, precision)
    fdat, cams, bounds = _scene(R, sd, 64, 64)
    assert 64 * 64 * 16 < R.PARTITION_MIN_SAMPLES <= 8 * 64 * 64 * 16
    _same_as_single_passes(R, w, fdat, cams[:8], bounds, (0, 0, 1, 64, 64), 16, 16)


@pytest.mark.gpu
def test_four_orbit_frames_of_256x256_at_64_plus_64(R, sd):
    """The orbit shape itself (bf16x3, the mode the orbit runs in): four 256x256 frames at 64 + 64 samples in one pass."""
    w = _weights(R, sd, "bf16x3")
    fdat, cams, bounds = _scene(R, sd, 256, 256)
    got, _ = _same_as_single_passes(R, w, fdat, [cams[0], cams[2], cams[3], cams[5]], bounds, (0, 0, 1, 256, 256), 64, 64)
    assert got["hit"].float().mean().item() > 0.05 and got["color_fine"].std().item() > 1e-3  # the hands are in view


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_views_with_their_own_clip_range_and_a_view_that_misses_the_box(R, sd, precision):
    """znear / zfar travel in the camera table, per view; a camera turned aside from the hands (no ray meets the bounding box) shares a group
    with cameras that see them."""
    w = _weights(R, sd, precision)
    fdat, cams, bounds = _scene(R, sd, 64, 64)
    away = dict(cams[1])
    # a quarter turn about the camera's y axis: same centre, the hands a metre off to the side.  (Half a turn would not do: the box test of
    # src/model.py:1496-1570 intersects the ray's LINE, so a box straight behind the camera still counts as crossed.)
    turn = torch.tensor([[0.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [-1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]], device="cuda")
    away["RT"] = (turn @ cams[1]["RT"][0])[None].contiguous()
    away["KRT"] = away["K"] @ away["RT"]
    group = [dict(cams[0], znear=0.5, zfar=1.1), away, dict(cams[2], znear=0.9, zfar=2.0), cams[3]]
    got, singles = _same_as_single_passes(R, w, fdat, group, bounds, (0, 0, 1, 64, 64), 16, 16)
    assert not got["hit"][1].any() and got["hit"][0].any() and got["hit"][2].any()
    assert not torch.equal(singles[0]["z"], R.render_pass_c(w, fdat, cams[0], bounds, 0, 0, 1, 64, 64, 16, 16)["z"])  # the clip range matters


@pytest.mark.gpu
def test_two_groups_in_flight_and_a_nan_filled_scratch_block(R, sd):
    """No device-side state: two groups on two streams with a scratch block each give the serial results; a block full of NaN bit patterns
    gives the same outputs as a fresh one (nothing is read before the pass has written it)."""
    w = _weights(R, sd, "bf16x3")
    fdat, cams, bounds = _scene(R, sd, 64, 64)
    ga, gb = cams[:4], cams[4:8]
    args = (bounds, 0, 0, 1, 64, 64, 16, 16)
    want_a, want_b = R.render_pass_views(w, fdat, ga, *args), R.render_pass_views(w, fdat, gb, *args)
    torch.cuda.synchronize()
    nbytes = R.render_pass_views_scratch(4, 64 * 64, 16, 16)
    assert nbytes > 0
    blocks = [torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(2)]  # 0xFFFFFFFF: a NaN in every float
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    for s, blk, grp in zip(streams, blocks, (ga, gb)):
        with torch.cuda.stream(s):
            outs.append(R.render_pass_views(w, fdat, grp, *args, scratch=blk))
    torch.cuda.synchronize()
    for got, want in zip(outs, (want_a, want_b)):
        for k in KEYS:
            assert torch.equal(got[k], want[k]), k
            assert not torch.isnan(got[k].float()).any(), k
    with pytest.raises(R._ffi.VanerfError, match="scratch"):
        R.render_pass_views(w, fdat, ga, *args, scratch=blocks[0][: nbytes // 2])


def _net(precision="bf16x3", Sc=16, Sf=16):
    from vanerf_amd.config import default_config
    from vanerf_amd.model import VANeRF
    torch.manual_seed(0)
    cfg = default_config()
    cfg["models"]["VANeRF"]["mfma_precision"] = precision
    cfg["models"]["VANeRF"]["dr_kwargs"].update(sample_per_ray_c=Sc, sample_per_ray_f=Sf)
    net = VANeRF(cfg).cuda().eval()
    net.load_state_dict(synth.make_full_weights(0), strict=False)
    return net


def _orbit(frame_cpu, W, H, n):
    from vanerf_amd.model import get_360cameras
    headpose = torch.eye(4)
    headpose[:3, 3] = frame_cpu["targets"]["vert_world"][0].mean(0)
    return get_360cameras(headpose[:3, :4].cuda(), 4.0 * W, 1.0, 1.0, W, H, 0.71, 1.42, n_frames=n)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_render_pifu_nerf_views_equals_render_pifu_nerf_per_view(precision):
    from vanerf_amd.novel_views import camera_to_cam_tar
    net = _net(precision)
    frame_cpu = synth.make_frame(seed=3, tar_h=48, tar_w=64)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    cam_tars = [camera_to_cam_tar(c) for c in _orbit(frame_cpu, 64, 48, 6)[:5]]
    kw = dict(fine=True, uniform=True, sample_per_ray_c=16, sample_per_ray_f=16, src_foreground_mask=trb["src_foreground_mask"],
              bounds=trb["dr_data"]["bounds"])
    outs = net.render_pifu_nerf_views(trb["im"], trb["cam"], trb["hand_type"], trb["targets"], cam_tars, sp_data=dict(trb["sp_data"]), **kw)
    assert len(outs) == 5
    for cam_tar, got in zip(cam_tars, outs):
        with torch.no_grad():
            want = net.render_pifu_nerf(None, net, trb["im"], trb["cam"], trb["hand_type"], trb["targets"], cam_tar, level=1, sp_data=dict(trb["sp_data"]),
                                        mask_at_box=None, **kw)
        for k in ("tex_fg", "depth", "alpha", "tex_fg_fine", "depth_fine", "alpha_fine", "sdf", "vert_xy", "vert_vis"):
            assert got[k].shape == want[k].shape, k
            assert torch.equal(got[k], want[k]), k
    assert not torch.equal(outs[0]["tex_fg_fine"], outs[2]["tex_fg_fine"]) and outs[0]["tex_fg_fine"].std() > 1e-3
    coarse = net.render_pifu_nerf_views(trb["im"], trb["cam"], trb["hand_type"], trb["targets"], cam_tars[:2], sp_data=dict(trb["sp_data"]),
                                        **dict(kw, fine=False))
    assert "tex_fg_fine" not in coarse[0] and torch.equal(coarse[1]["tex_fg"], outs[1]["tex_fg"])
    # what the multi-view pass does not take
    call = lambda cams, **over: net.render_pifu_nerf_views(trb["im"], trb["cam"], trb["hand_type"], trb["targets"], cams, sp_data=dict(trb["sp_data"]),
                                                           **dict(kw, **over))
    with pytest.raises(ValueError, match="rand_noise_std"):
        call(cam_tars, rand_noise_std=0.01)
    with pytest.raises(ValueError, match="uniform"):
        call(cam_tars, uniform=False)
    with pytest.raises(ValueError, match="width"):
        call([cam_tars[0], dict(cam_tars[1], width=32, height=32)])
    net.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            call(cam_tars)
    finally:
        net.eval()


@pytest.mark.gpu
def test_orbit_in_groups_of_four_equals_the_per_frame_orbit(tmp_path):
    """render_novel_views(views_per_pass=4) on a 12-frame orbit: the uint8 stack of views_per_pass=1; a group size that does not divide the
    orbit; render_video writes the same PNG bytes either way."""
    from vanerf_amd.novel_views import render_novel_views, render_video
    import vanerf_amd.novel_views as nv
    net = _net("bf16x3")
    frame_cpu = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    cams = _orbit(frame_cpu, 64, 64, 12)
    want, _ = render_novel_views(net, cams, trb, only_renderings=True)
    seen = []
    got, _ = render_novel_views(net, cams, trb, only_renderings=True, views_per_pass=4, on_frame=lambda fi, img: seen.append(fi))
    assert got.shape == (12, 64, 64, 3) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert seen == list(range(12)) and want.std() > 2 and not np.array_equal(want[0], want[5])
    got5, _ = render_novel_views(net, cams, trb, only_renderings=True, views_per_pass=5)
    assert np.array_equal(got5, want)
    with pytest.raises(ValueError, match="shard"):
        render_novel_views(net, cams, trb, only_renderings=True, views_per_pass=4, shard="rays")
    # render_video: 256x256 frames by its own camera constants
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=256, tar_w=256), "cuda")
    net8 = _net("bf16x3", 8, 8)
    trb = synth.to_tr_batch(frame)
    headpose = torch.inverse(frame["cam_tar"]["RT"][0])[:3, :4]
    batch = dict(trb, index={"segment": ["seq"]}, human=torch.tensor([3]), headpose=headpose[None])
    files = {}
    for vpp in (1, 4):
        written = render_video(net8, [batch], str(tmp_path / f"v{vpp}"), sc_factor=0.1, n_frames=6, views_per_pass=vpp)
        assert len(written) == 6
        files[vpp] = [open(tmp_path / f"v{vpp}" / "video" / "seq" / "3" / f"{fi:06d}.png", "rb").read() for fi in range(6)]
    assert files[1] == files[4] and len(set(files[1])) > 1
    for fn in (nv.render_novel_views, nv.render_video):  # the default stays one view per pass
        assert inspect.signature(fn).parameters["views_per_pass"].default == 1
