"""CPU-side checks of the registration feature (vanerf_amd/csrc/surface_lines.hip, surface.register_surface): the C ABI's new names, the
argument checks of the entry points and of the Python wrappers, and the fp64 restatement of bracket and refine that the GPU tests hold the
kernels to (tests/test_surface_register.py), on hand-made rows.  None of it needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_surface_register import COLS, FLT_MAX, STATE_FLOATS, ref_bracket, ref_refine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vanerf_line_state_floats", "vanerf_vertex_normals", "vanerf_line_points", "vanerf_line_bracket", "vanerf_line_refine")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def surface():
    from vanerf_amd import build
    build.build()  # no-op when up to date
    from vanerf_amd import surface
    return surface


def test_new_names_are_exported_and_declared(surface):
    from vanerf_amd import _ffi
    hdr = open(os.path.join(REPO, "include", "vanerf_hip.h")).read()
    declared = set(re.findall(r"\b(vanerf_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in _ffi.EXPORTS and name in declared and hasattr(_ffi.lib, name), name
    assert declared == set(_ffi.EXPORTS)
    assert _ffi.lib.vanerf_abi_version() == _ffi.ABI_VERSION == 12
    assert "surface_lines.hip" in __import__("vanerf_amd.build", fromlist=["SOURCES"]).SOURCES
    # the record layout: the header's offsets, the binding's and the restatement's agree
    offs = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VANERF_LS_([A-Z_]+) (\d+)", hdr)}
    assert offs == {k: (v.start if isinstance(v, slice) else v) for k, v in COLS.items()}
    assert offs == {k: (v.start if isinstance(v, slice) else v) for k, v in surface._LINE_FIELDS.items()}
    assert int(re.search(r"#define VANERF_LINE_STATE_FLOATS (\d+)", hdr).group(1)) == _ffi.lib.vanerf_line_state_floats() == STATE_FLOATS == surface.LINE_STATE_FLOATS
    assert int(re.search(r"#define VANERF_LINE_MAX_SAMPLES (\d+)", hdr).group(1)) == surface.MAX_LINE_SAMPLES == 256


def test_entry_points_refuse_bad_arguments_without_a_gpu(surface):
    from vanerf_amd import _ffi
    lib, p = _ffi.lib, ctypes.c_void_p(64)

    def refused(rc, word):
        assert rc == -22 and word in lib.vanerf_last_error(), (rc, lib.vanerf_last_error())

    # vanerf_vertex_normals(verts, nv, faces, nf, normals, stream)
    for args in ((None, 4, p, 2, p), (p, 4, None, 2, p), (p, 4, p, 2, None)):
        refused(lib.vanerf_vertex_normals(*args, None), b"null")
    refused(lib.vanerf_vertex_normals(p, 0, p, 2, p, None), b"nv=0")
    refused(lib.vanerf_vertex_normals(p, 4, p, -1, p, None), b"nf=-1")

    # vanerf_line_points(base, dir, n, K, t0, dt, t_dev, pts, stream)
    for args in ((None, p, 4, 3, 0.0, 1.0, None, p), (p, None, 4, 3, 0.0, 1.0, None, p), (p, p, 4, 3, 0.0, 1.0, None, None)):
        refused(lib.vanerf_line_points(*args, None), b"null")
    refused(lib.vanerf_line_points(p, p, -1, 3, 0.0, 1.0, None, p, None), b"n=-1")
    for K in (0, -3, 257):
        refused(lib.vanerf_line_points(p, p, 4, K, 0.0, 1.0, None, p, None), b"K=")
    refused(lib.vanerf_line_points(p, p, 4, 2, 0.0, 1.0, p, p, None), b"K must be 1")
    for t0, dt in ((NAN, 1.0), (INF, 1.0), (0.0, NAN), (0.0, INF), (0.0, 0.0), (0.0, -1.0)):
        refused(lib.vanerf_line_points(p, p, 4, 3, t0, dt, None, p, None), b"dt")
    refused(lib.vanerf_line_points(p, p, 1 << 30, 256, 0.0, 1.0, None, p, None), b"2^31")
    assert lib.vanerf_line_points(None, None, 0, 3, 0.0, 1.0, None, None, None) == 0  # n = 0 is a no-op

    # vanerf_line_bracket(f, rgb, n, K, t0, dt, iso, state, stream)
    for args in ((None, None, 4, 3, 0.0, 1.0, 0.0, p), (p, p, 4, 3, 0.0, 1.0, 0.0, None)):
        refused(lib.vanerf_line_bracket(*args, None), b"null")
    refused(lib.vanerf_line_bracket(p, None, -2, 3, 0.0, 1.0, 0.0, p, None), b"n=-2")
    for K in (1, 0, 257):
        refused(lib.vanerf_line_bracket(p, None, 4, K, 0.0, 1.0, 0.0, p, None), b"K=")
    for t0, dt in ((NAN, 1.0), (-INF, 1.0), (0.0, NAN), (0.0, INF), (0.0, 0.0), (0.0, -0.5)):
        refused(lib.vanerf_line_bracket(p, None, 4, 3, t0, dt, 0.0, p, None), b"dt")
    for iso in (NAN, INF, -INF):
        refused(lib.vanerf_line_bracket(p, None, 4, 3, 0.0, 1.0, iso, p, None), b"iso")
    refused(lib.vanerf_line_bracket(p, None, 4, 3, 0.0, 1.0, 0.0, ctypes.c_void_p(68), None), b"aligned")
    assert lib.vanerf_line_bracket(None, None, 0, 3, 0.0, 1.0, 0.0, None, None) == 0

    # vanerf_line_refine(f_new, rgb_new, n, iso, state, stream)
    for args in ((None, None, 4, 0.0, p), (p, None, 4, 0.0, None)):
        refused(lib.vanerf_line_refine(*args, None), b"null")
    refused(lib.vanerf_line_refine(p, None, -1, 0.0, p, None), b"n=-1")
    for iso in (NAN, INF):
        refused(lib.vanerf_line_refine(p, None, 4, iso, p, None), b"iso")
    refused(lib.vanerf_line_refine(p, None, 4, 0.0, ctypes.c_void_p(72), None), b"aligned")
    assert lib.vanerf_line_refine(None, None, 0, 0.0, None, None) == 0


def test_wrappers_check_their_arguments_without_a_device(surface):
    v, f = torch.zeros(5, 3), torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="device"):
        surface.vertex_normals(v, f)  # CPU tensors are refused, never silently computed
    with pytest.raises(ValueError):
        surface.vertex_normals(torch.zeros(5, 2), f)
    with pytest.raises(ValueError, match="device"):
        surface.line_points(v, v, 3, 0.0, 1.0)
    with pytest.raises(ValueError):
        surface.line_points(v, torch.zeros(4, 3), 3, 0.0, 1.0)
    with pytest.raises(ValueError):
        surface.line_points(v, v, t=torch.zeros(4))
    with pytest.raises(ValueError, match="device"):
        surface.line_bracket(torch.zeros(5, 9), -1.0, 0.25)
    with pytest.raises(ValueError):
        surface.line_bracket(torch.zeros(5), -1.0, 0.25)
    with pytest.raises(ValueError):
        surface.line_bracket(torch.zeros(5, 9), -1.0, 0.25, rgb=torch.zeros(5, 9))
    with pytest.raises(ValueError, match="device"):
        surface.line_refine(torch.zeros(5, 16), torch.zeros(5))
    with pytest.raises(ValueError):
        surface.line_refine(torch.zeros(5, 15), torch.zeros(5))
    with pytest.raises(ValueError):
        surface.line_refine(torch.zeros(5, 16), torch.zeros(4))
    with pytest.raises(ValueError):
        surface.line_state(torch.zeros(5, 15))
    views = surface.line_state(torch.arange(32.0).view(2, 16))
    assert views["t_next"].tolist() == [15.0, 31.0] and views["rgb_b"].tolist() == [[8.0, 9.0, 10.0], [24.0, 25.0, 26.0]] and views["found"].tolist() == [7.0, 23.0]
    for kw in (dict(samples=8), dict(samples=1), dict(samples=257), dict(band=0.0), dict(band=NAN), dict(refine=-1), dict(iso=INF)):
        with pytest.raises(ValueError):
            surface.register_surface(object(), {}, **kw)
    with pytest.raises(TypeError):
        surface.register_surface(object(), {})
    with pytest.raises(TypeError):
        surface.field_at_points(object(), {}, torch.zeros(4, 3))
    with pytest.raises(ValueError):
        surface.field_at_points(object(), {}, torch.zeros(4, 3), slab_points=0)
    from vanerf_amd.model import VANeRF
    assert callable(VANeRF.register_surface)


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement on hand-made rows: t0 = -1, dt = 0.5, five samples at t = -1, -0.5, 0, 0.5, 1
# ------------------------------------------------------------------------------------------------------------------------------------
T0, DT = -1.0, 0.5


def _row(*values):
    return np.float32([values])


def test_restatement_single_crossing():
    r = ref_bracket(_row(-3.0, -2.0, -1.0, 3.0, 4.0), T0, DT, 0.0, rgb=np.arange(15, dtype=np.float32).reshape(1, 5, 3))
    assert r["found"][0] and r["k"][0] == 2 and (r["ta"][0], r["tb"][0], r["ga"][0], r["gb"][0]) == (0.0, 0.5, -1.0, 3.0)
    assert r["t_est"][0] == 0.125 and r["t_next"][0] == 0.125  # w = 1/4
    assert r["rgb_a"][0].tolist() == [6.0, 7.0, 8.0] and r["rgb_b"][0].tolist() == [9.0, 10.0, 11.0] and r["rgb_est"][0].tolist() == [6.75, 7.75, 8.75]
    assert np.isinf(r["gap"][0])
    # a weight outside [1/8, 7/8] moves t_next, not t_est
    r = ref_bracket(_row(-3.0, -2.0, -0.25, 3.75, 4.0), T0, DT, 0.0)
    assert r["t_est"][0] == 0.03125 and r["t_next"][0] == 0.0625
    # another level
    r = ref_bracket(_row(-3.0, -2.0, -1.0, 3.0, 4.0), T0, DT, -1.5)
    assert r["k"][0] == 1 and r["t_est"][0] == -0.25


def test_restatement_two_crossings_equally_far_the_lower_k_wins():
    r = ref_bracket(_row(1.0, -1.0, -1.0, 1.0, 1.0), T0, DT, 0.0)  # cuts at t = -0.75 and t = +0.25 ... not a tie: the nearer one wins
    assert r["k"][0] == 2 and r["t_est"][0] == 0.25 and r["gap"][0] == 0.5
    r = ref_bracket(_row(1.0, 1.0, -1.0, 1.0, 1.0), T0, DT, 0.0)   # cuts at t = -0.25 and t = +0.25: a tie
    assert r["found"][0] and r["k"][0] == 1 and r["t_est"][0] == -0.25 and r["gap"][0] == 0.0
    assert (r["ta"][0], r["tb"][0], r["ga"][0], r["gb"][0]) == (-0.5, 0.0, 1.0, -1.0)


def test_restatement_a_value_equal_to_iso_is_outside():
    r = ref_bracket(_row(0.0, 0.0, 0.0, 0.0, 0.0), T0, DT, 0.0)
    assert not r["found"][0]
    r = ref_bracket(_row(2.0, 2.0, 0.0, -2.0, -2.0), T0, DT, 0.0)  # (0, -2) is the crossing, with w = 0: the cut is the sample itself
    assert r["found"][0] and r["k"][0] == 2 and r["t_est"][0] == 0.0 and r["t_next"][0] == 0.0625
    r = ref_bracket(_row(-2.0, -2.0, 0.25, 2.0, 2.0), T0, DT, 0.25)  # (-2, iso): w = 1
    assert r["k"][0] == 1 and r["t_est"][0] == 0.0 and r["t_next"][0] == -0.0625


def test_restatement_non_finite_entries_are_far_outside():
    r = ref_bracket(_row(NAN, INF, -INF, NAN, INF), T0, DT, 0.0)
    assert not r["found"][0]
    r = ref_bracket(_row(NAN, -1.0, -1.0, -1.0, -INF), T0, DT, 0.0)  # -inf is outside as well: two crossings, at t = -0.5 and t = 0.5 + 0
    assert r["found"][0] and r["k"][0] == 0 and (r["ga"][0], r["gb"][0]) == (FLT_MAX, -1.0) and r["t_est"][0] == -0.5 and r["gap"][0] == 0.0
    r = ref_bracket(_row(-1.0, -1.0, -1.0, INF, 3.0), T0, DT, 0.0)
    assert r["k"][0] == 2 and r["gb"][0] == FLT_MAX and abs(r["t_est"][0]) < 1e-30 and r["t_next"][0] == 0.0625
    assert np.isfinite([r[k][0] for k in ("ta", "tb", "ga", "gb", "t_est", "t_next")]).all()


def test_restatement_no_crossing():
    for row in (_row(1.0, 2.0, 3.0, 4.0, 5.0), _row(-1.0, -2.0, -3.0, -4.0, -5.0)):
        r = ref_bracket(row, T0, DT, 0.0, rgb=np.ones((1, 5, 3), np.float32))
        assert not r["found"][0] and r["k"][0] == -1 and np.isnan(r["t_est"][0]) and np.isnan(r["t_next"][0])
        assert all(r[k][0] == 0.0 for k in ("ta", "tb", "ga", "gb")) and not r["rgb_a"].any() and not r["rgb_b"].any() and not r["rgb_est"].any()
    r = ref_bracket(np.float32([[1.0, -1.0], [1.0, 2.0]]), T0, DT, 0.0)  # K = 2, two lines
    assert r["found"].tolist() == [True, False] and r["t_est"][0] == -0.75


def _state(ta, tb, ga, gb, found=1.0):
    s = np.zeros((1, STATE_FLOATS))
    s[0, :4] = ta, tb, ga, gb
    s[0, COLS["found"]] = found
    w = min(max((0.0 - ga) / (gb - ga), 0.0), 1.0) if found else 0.0
    s[0, COLS["t_est"]] = ta + w * (tb - ta) if found else NAN
    s[0, COLS["t_next"]] = ta + min(max(w, 0.125), 0.875) * (tb - ta) if found else NAN
    return s


def test_restatement_refine():
    s = _state(0.0, 0.5, -1.0, 3.0)  # t_next = 0.125
    a = ref_refine(s, np.float32([-0.5]), 0.0, rgb_new=np.float32([[1.0, 2.0, 3.0]]))  # inside, as a is: a moves
    assert a[0, :4].tolist() == [0.125, 0.5, -0.5, 3.0] and a[0, COLS["rgb_a"]].tolist() == [1.0, 2.0, 3.0] and not a[0, COLS["rgb_b"]].any()
    w = 0.5 / 3.5
    assert a[0, COLS["t_est"]] == 0.125 + w * 0.375 and a[0, COLS["t_next"]] == 0.125 + w * 0.375
    assert np.allclose(a[0, COLS["rgb_est"]], (1 - w) * np.float64([1.0, 2.0, 3.0]))
    b = ref_refine(s, np.float32([0.5]), 0.0)  # outside: b moves
    assert b[0, :4].tolist() == [0.0, 0.125, -1.0, 0.5] and b[0, COLS["t_next"]] == 0.125 * (2.0 / 3.0)
    c = ref_refine(s, np.float32([NAN]), 0.0)  # non-finite: far outside, b moves; t_next is held at 1/8 of the bracket
    assert c[0, :4].tolist() == [0.0, 0.125, -1.0, FLT_MAX] and c[0, COLS["t_next"]] == 0.125 * 0.125 and c[0, COLS["t_est"]] < 1e-30
    d = ref_refine(s, np.float32([0.0]), 0.0)  # equal to iso: outside
    assert d[0, :4].tolist() == [0.0, 0.125, -1.0, 0.0] and d[0, COLS["t_est"]] == 0.125 and d[0, COLS["t_next"]] == 0.125 * 0.875
    # an outside-to-inside bracket, and a line without a crossing (left alone)
    e = ref_refine(_state(-0.5, 0.0, 1.0, -1.0), np.float32([0.25]), 0.0)
    assert e[0, :4].tolist() == [-0.25, 0.0, 0.25, -1.0]
    miss = _state(0.0, 0.0, 0.0, 0.0, found=0.0)
    out = ref_refine(miss, np.float32([-1.0]), 0.0)
    assert np.array_equal(out, miss, equal_nan=True)
    for r in (a, b, c, d, e):  # every bracket still straddles iso and holds its estimate
        assert (r[0, 2] < 0.0) != (r[0, 3] < 0.0) and r[0, 0] <= r[0, COLS["t_est"]] <= r[0, 1]
