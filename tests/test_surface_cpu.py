"""CPU-side checks of the surface feature (vanerf_amd/surface.py, vanerf_amd/csrc/surface.hip): the PLY writer, the C ABI's new names and
the argument checks of the Python wrappers, none of which needs a device."""
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vanerf_grid_points", "vanerf_field_values", "vanerf_surface_scratch", "vanerf_surface_count", "vanerf_surface_emit")


@pytest.fixture(scope="module")
def surface():
    from vanerf_amd import build
    build.build()  # no-op when up to date
    from vanerf_amd import surface
    return surface


def read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    nv = int(next(l for l in header if l.startswith("element vertex")).split()[-1])
    nf = int(next(l for l in header if l.startswith("element face")).split()[-1])
    coloured = "property uchar red" in header
    vt = np.dtype([("xyz", "<f4", (3,))] + ([("rgb", "u1", (3,))] if coloured else []))
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    v = np.frombuffer(raw, vt, nv, end)
    f = np.frombuffer(raw, ft, nf, end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nf * ft.itemsize == len(raw)
    return header, v, f


@pytest.mark.parametrize("coloured", [False, True])
def test_save_ply_round_trip(surface, tmp_path, coloured):
    rng = np.random.default_rng(0)
    verts = rng.standard_normal((37, 3)).astype(np.float32)
    faces = rng.integers(0, 37, (51, 3)).astype(np.int32)
    colors = rng.random((37, 3)).astype(np.float32) if coloured else None
    if coloured:
        colors[0] = [-0.5, 1.5, np.nan]  # clamped; NaN -> 0
    path = str(tmp_path / "mesh.ply")
    assert surface.save_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), None if colors is None else torch.from_numpy(colors)) == path
    header, v, f = read_ply(path)
    assert header[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 37"]
    assert header[3:6] == ["property float x", "property float y", "property float z"]
    assert header[-3:] == ["element face 51", "property list uchar int vertex_indices", "end_header"]
    assert len(header) == (12 if coloured else 9)
    assert np.array_equal(v["xyz"], verts) and (f["n"] == 3).all() and np.array_equal(f["v"], faces)
    if coloured:
        want = np.rint(np.clip(np.nan_to_num(colors.astype(np.float64)), 0, 1) * 255).astype(np.uint8)
        assert np.array_equal(v["rgb"], want) and tuple(v["rgb"][0]) == (0, 255, 0)
    # an empty mesh is a valid file; bad shapes and indices are refused
    surface.save_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    header, v, f = read_ply(path)
    assert len(v) == 0 and len(f) == 0
    with pytest.raises(ValueError):
        surface.save_ply(path, verts[:, :2], faces)
    with pytest.raises(ValueError):
        surface.save_ply(path, verts, faces + 37)
    with pytest.raises(ValueError):
        surface.save_ply(path, verts, faces, np.zeros((36, 3)))


def test_new_names_are_exported_and_declared(surface):
    from vanerf_amd import _ffi
    hdr = open(os.path.join(REPO, "include", "vanerf_hip.h")).read()
    declared = set(re.findall(r"\b(vanerf_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in _ffi.EXPORTS and name in declared and hasattr(_ffi.lib, name), name
    assert "surface.hip" in __import__("vanerf_amd.build", fromlist=["SOURCES"]).SOURCES
    # the host-side checks of the C entry points answer before anything touches a GPU
    lib = _ffi.lib
    assert lib.vanerf_surface_scratch(9, 8, 7) > 4 * 9 * 8 * 7 and lib.vanerf_surface_scratch(1, 8, 7) == 0
    assert lib.vanerf_surface_scratch(700, 700, 700) == 0 and lib.vanerf_surface_scratch(600, 600, 600) > 0  # 7 n^3 against 2^31
    assert lib.vanerf_surface_count(None, 4, 4, 4, 0.0, None, 0, None, None) == -22 and b"null" in lib.vanerf_last_error()
    assert lib.vanerf_field_values(None, None, 5, None, None, None) == -22 and b"null" in lib.vanerf_last_error()
    assert lib.vanerf_field_values(None, None, 0, None, None, None) == 0
    assert lib.vanerf_grid_points(surface._f3((0, 0, 0)), surface._f3((1, 1, 1)), 4, 4, 4, 3, 2, None, None) == -22 and b"layers" in lib.vanerf_last_error()
    assert lib.vanerf_grid_points(surface._f3((0, 0, 0)), surface._f3((1, -1, 1)), 4, 4, 4, 0, 1, None, None) == -22 and b"spacing" in lib.vanerf_last_error()


def test_wrappers_check_their_arguments_without_a_device(surface):
    b = [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]]
    assert surface.grid_spec(b, dims=(3, 5, 7)) == ((0.0, 0.0, 0.0), (0.5, 0.5, 0.5), (3, 5, 7))
    assert surface.grid_spec(b, voxel_size=0.5) == ((0.0, 0.0, 0.0), (0.5, 0.5, 0.5), (3, 5, 7))
    assert surface.grid_spec(torch.tensor([b]), voxel_size=4.0)[2] == (2, 2, 2)
    for kw in ({}, dict(dims=(3, 3, 3), voxel_size=0.1), dict(dims=(1, 3, 3)), dict(dims=(3, 3)), dict(voxel_size=0.0), dict(voxel_size=float("nan")),
               dict(dims=(1000, 1000, 1000))):
        with pytest.raises(ValueError):
            surface.grid_spec(b, **kw)
    with pytest.raises(ValueError):
        surface.grid_spec([[0, 0, 0], [1, 0, 1]], dims=(3, 3, 3))  # an empty axis
    with pytest.raises(ValueError):
        surface.grid_spec([0, 1, 2], dims=(3, 3, 3))
    f = torch.zeros(4, 4, 4)
    with pytest.raises(ValueError, match="device"):
        surface.march(f, (0, 0, 0), (1, 1, 1))  # CPU tensors are refused, never silently computed
    with pytest.raises(ValueError):
        surface.march(torch.zeros(1, 4, 4), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        surface.march(torch.zeros(4, 4), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        surface.march(f, (0, 0, 0), (1, 1, 1), iso=float("inf"))
    with pytest.raises(ValueError):
        surface.grid_points((0, 0, 0), (1, 1, 1), (4, 4, 4), z0=3, nz_out=2)
    with pytest.raises(TypeError):
        surface.field_on_grid(object(), {}, dims=(4, 4, 4))
    with pytest.raises(TypeError):
        surface.extract_surface(object(), {})
    with pytest.raises(ValueError):
        surface.field_on_grid(object(), {}, dims=(4, 4, 4), voxel_size=0.1)
    with pytest.raises(ValueError):
        surface.field_on_grid(object(), {}, dims=(4, 4, 4), slab_points=0)
    from vanerf_amd.model import VANeRF
    assert callable(VANeRF.extract_surface)
