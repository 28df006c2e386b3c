"""The mesh query's item order: vanerf_mesh_tile_order (every 8 x 8 pixel tile's sample indices sorted by depth) and
vanerf_mesh_query_accel_ordered (a wave takes a 64-slot slab of that table instead of depth k of the tile).

The order is scheduling only: every point's answer is exact, so every comparison of query outputs below is torch.equal on bits, and the
table itself is compared with a stable CPU sort, entry by entry.  Nothing here has a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import mesh_geometry_ref as G  # noqa: E402
from vanerf_amd import synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


# ---------------------------------------------------------------------------------------------------------------------
# depth sets (CPU, seeded)
# ---------------------------------------------------------------------------------------------------------------------
def _clip_ranges_10x(nx, ny, S, g, near=(0.5, 1.0), width=0.05):
    """Per-ray clip ranges whose widths differ 10x between neighbours (checkerboard: `width` and 10 `width`), each with a near plane of its own."""
    x, y = torch.arange(nx)[None, :].expand(ny, nx), torch.arange(ny)[:, None].expand(ny, nx)
    w = torch.where((x + y) % 2 == 0, width, 10.0 * width).reshape(-1, 1).float()
    n0 = near[0] + (near[1] - near[0]) * torch.rand(nx * ny, 1, generator=g)
    return (n0 + w * torch.linspace(0.0, 1.0, S)[None]).contiguous()


def _depths(kind, nx, ny, S):
    g = torch.Generator().manual_seed(1000 * nx + 10 * ny + S)
    n = nx * ny
    if kind == "linspace":
        return torch.linspace(0.71, 1.42, S)[None].expand(n, S).contiguous()
    if kind == "clip10x":
        return _clip_ranges_10x(nx, ny, S, g)
    if kind == "ties":  # equal depths across rays (ray 1 repeats ray 0, the last ray repeats the first) and within a ray; a +0 / -0 pair
        z = torch.rand(n, S, generator=g)
        z[n // 2:] = z[:n - n // 2].clone()
        if n > 1:
            z[1] = z[0]
        if S > 1:
            z[:, S - 1] = z[:, 0]
            z[0, 0], z[n - 1, 1] = 0.0, -0.0
        return z.contiguous()
    if kind == "negative":
        return torch.randn(n, S, generator=g).contiguous()
    raise KeyError(kind)


def _tile_rays(nx, ny):
    """Per tile (row-major over the tile grid): the ray indices of its 8 x 8 pixels inside the grid, in pixel order."""
    tiles = []
    for ty in range((ny + 7) // 8):
        for tx in range((nx + 7) // 8):
            tiles.append([y * nx + x for y in range(8 * ty, min(8 * ty + 8, ny)) for x in range(8 * tx, min(8 * tx + 8, nx))])
    return tiles


def _expected_table(z, nx, ny):
    S = z.shape[1]
    out = torch.full((len(_tile_rays(nx, ny)), 64 * S), -1, dtype=torch.int32)
    for t, rays in enumerate(_tile_rays(nx, ny)):
        r = torch.tensor(rays)
        idx = (r[:, None] * S + torch.arange(S)[None]).reshape(-1)
        perm = torch.sort(z[r].reshape(-1), stable=True)[1]
        out[t, :idx.numel()] = idx[perm].int()
    return out


def _assert_names_every_sample_once(table, nx, ny, S):
    """-1 only behind a tile's samples, as many as its border rays have slots; every sample index once, inside its own tile."""
    for t, rays in enumerate(_tile_rays(nx, ny)):
        row, k = table[t], len(rays) * S
        assert bool((row[k:] == -1).all()) and bool((row[:k] >= 0).all()), f"tile {t}: -1 slots are not exactly the {64 * S - k} at its end"
        want = (torch.tensor(rays)[:, None] * S + torch.arange(S)[None]).reshape(-1).int()
        assert torch.equal(torch.sort(row[:k])[0], want), f"tile {t}: not a permutation of its own samples"


GRIDS = [(8, 8, 1), (8, 8, 64), (13, 5, 3), (1, 1, 2), (16, 24, 65), (9, 17, 128)]


@pytest.mark.parametrize("kind", ["linspace", "clip10x", "ties", "negative"])
@pytest.mark.parametrize("nx,ny,S", GRIDS)
def test_the_table_is_the_stable_sort_of_every_tile(R, nx, ny, S, kind):
    z = _depths(kind, nx, ny, S)
    got = R.mesh_tile_order(z.cuda(), nx, ny).cpu().reshape(-1, 64 * S)
    _assert_names_every_sample_once(got, nx, ny, S)
    assert torch.equal(got, _expected_table(z, nx, ny)), f"{int((got != _expected_table(z, nx, ny)).sum())} slots differ from the stable sort"
    assert torch.equal(got, R.mesh_tile_order(z.cuda(), nx, ny).cpu().reshape(-1, 64 * S))  # the same table on every run


@pytest.mark.parametrize("nx,ny,S", GRIDS)
def test_non_finite_depths_still_give_a_permutation(R, nx, ny, S):
    """NaN and +-inf depths (a ray that is all NaN, single samples, descending rays): any permutation of the tile is valid, but it is one."""
    z = _depths("clip10x", nx, ny, S)
    g = torch.Generator().manual_seed(7)
    bad = torch.tensor([float("nan"), float("inf"), float("-inf"), -float("nan")])
    m = torch.rand(z.shape, generator=g) < 0.05
    z[m] = bad[torch.randint(0, 4, (int(m.sum()),), generator=g)]
    z[0, 0] = float("nan")
    z[-1] = float("nan")
    got = R.mesh_tile_order(z.cuda(), nx, ny).cpu().reshape(-1, 64 * S)
    _assert_names_every_sample_once(got, nx, ny, S)


def test_more_than_128_samples_per_ray_are_refused(R):
    from vanerf_amd._ffi import VanerfError
    with pytest.raises(VanerfError, match="129 samples per ray"):
        R.mesh_tile_order(torch.zeros(64, 129, device="cuda"), 8, 8)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the query: bits do not depend on the order
# ---------------------------------------------------------------------------------------------------------------------
def _v4(verts):
    return torch.cat([verts, torch.zeros(verts.shape[0], 1, device=verts.device)], 1).contiguous()


def _assert_same(a, b, what):
    for x, y, k in zip(a, b, ("sdf", "vis", "face", "knn")):
        x, y = (x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) if x.dtype == torch.float32 else (x, y)
        assert torch.equal(x, y), f"{what}: {k} differs on {int((x != y).sum())} of {x.numel()} points"


_MESHES = {}


def _mesh(name):
    if name not in _MESHES:
        if name == "two_fingered_hands":
            verts, faces, _, _ = G.placed_mesh(name, 0)
        else:  # the synthetic frame's own mesh
            t = synth.make_frame(seed=3)["targets"]
            verts, faces = t["vert_world"][0].float().contiguous(), t["face_world"][0].long()
        _MESHES[name] = (verts.cuda(), faces.to(torch.int32).cuda().contiguous(), G.vertex_flags(verts.shape[0], 1).cuda())
    return _MESHES[name]


def _ray_points(R, verts, nx, ny, S, kind, zoom=1.2):
    """Samples of real rays at the depths of `kind`: z (R, S) on the device and the points made from them.  zoom: as G.ray_camera (1.2: the
    view takes in the mesh; more: a window in the middle of it, pixels that much closer together)."""
    cam, bounds = G.ray_camera(verts.cpu(), nx, ny, zoom=zoom)
    rays = R.ray_setup(cam, bounds, 0, 0, 1, nx, ny, S, device="cuda")
    if kind == "linspace":
        z = rays["z"]
    else:  # the mesh sits about 1.1 m from this camera: ranges of 0.06 m and 0.6 m that start 0.5 .. 1.0 m out
        z = _clip_ranges_10x(nx, ny, S, torch.Generator().manual_seed(nx + S), width=0.06).cuda()
    return z.contiguous(), R.sample_points(rays["rays_d"], rays["cam_pos"], z.contiguous())


@pytest.mark.parametrize("kind", ["linspace", "clip10x"])
@pytest.mark.parametrize("nx,ny,S", [(16, 16, 24), (13, 5, 7)])
@pytest.mark.parametrize("name", ["two_fingered_hands", "frame"])
def test_ordered_query_equals_the_plain_and_the_exhaustive_kernels(R, name, nx, ny, S, kind):
    """(a) linspace depths, (b) clip ranges 10x apart between neighbours, each with (c) the sorted table and a seeded random permutation of
    the whole table (the -1 slots land anywhere) and (d) NaN points.  Against vanerf_mesh_query_accel and the exhaustive kernels, all four
    outputs, bit for bit.  Launches of this size run the one-depth kernel; the two-depth one is the next test.

    The camera looks at a window of a twelfth of the mesh (zoom 12: a tile is some 5 mm wide, as in a real view; at zoom 1.2 a tile of a
    16 x 16 view spans 10 cm and no group gets a tile search at all).  (b) by index spans decimetres per group (neighbouring rays' k-th
    samples lie up to 0.5 m apart), beyond the 25 mm at which the tile search gives up.  Checked with the phase counters of a
    -DVANERF_MESH_PHASES build (tools/perf_mesh.py --phases prints them), 16 x 16 x 24, closest-face search, of 96 groups, the same on both
    meshes: (a) by index and by the table 95 .. 96 tile searches, of which 1 ends on a full cluster list (two_fingered_hands) and 14 .. 39
    on a full candidate table; (b) by index 96 groups too wide, all by the per-lane search; (b) by the table 67 tile searches, 28 groups
    too wide, 1 full cluster list, 3 .. 9 full candidate tables; the random table: 96 too wide.  (13 x 5 x 7: 14 groups; by the table 6
    tile searches and 8 too wide.)"""
    verts, faces, vv = _mesh(name)
    accel = R.MeshAccel(verts, faces)
    z, pts = _ray_points(R, verts, nx, ny, S, kind, zoom=12.0)
    grid = (nx, ny, S)
    table = R.mesh_tile_order(z, nx, ny)
    flat = table.reshape(-1)
    shuffled = flat[torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(5)).cuda()].contiguous()
    nan_pts = pts.clone()
    nan_pts[torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(6))[:pts.shape[0] // 50].cuda()] = float("nan")
    nan_pts[3, 1] = float("inf")
    for tag, p in (("", pts), (" with NaN points", nan_pts)):
        want = (*R.mesh_query(verts, faces, vv, p, want_face=True), R.knn1(_v4(verts), p))
        _assert_same(R.mesh_query_accel(accel, verts, faces, vv, p, want_face=True, grid=grid), want, f"by index{tag}")
        _assert_same(R.mesh_query_accel(accel, verts, faces, vv, p, want_face=True, grid=grid, item_order=table), want, f"sorted table{tag}")
        _assert_same(R.mesh_query_accel(accel, verts, faces, vv, p, want_face=True, grid=grid, item_order=shuffled), want, f"random table{tag}")
    assert (want[0] < 0).any() and (want[0] > 0).any()  # (2 % .. 50 % of the points of these windows are inside)


@pytest.mark.parametrize("kind", ["linspace", "clip10x"])
def test_ordered_query_with_two_depths_per_item(R, kind):
    """288 x 288 rays x 33 depths = 2.74 M samples: 21 384 two-depth items, above the four items per wave (16 384 on 256 CUs) from which the
    library takes two slabs per item; 33 is odd, so the last item of a tile has one slab.  The whole batch against vanerf_mesh_query_accel, with
    the sorted and with a randomly permuted table; every 8th ray against the exhaustive kernels."""
    nx, ny, S = 288, 288, 33
    verts, faces, vv = _mesh("two_fingered_hands")
    accel = R.MeshAccel(verts, faces)
    z, pts = _ray_points(R, verts, nx, ny, S, kind)
    table = R.mesh_tile_order(z, nx, ny)
    plain = R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True, grid=(nx, ny, S))
    _assert_same(R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True, grid=(nx, ny, S), item_order=table), plain, "sorted table")
    # whole 64-slot slabs change places (a permutation within the slabs as well would make every slab as wide as the view: minutes)
    slabs = table.reshape(-1, 64)
    mixed = slabs[torch.randperm(slabs.shape[0], generator=torch.Generator().manual_seed(8)).cuda()].flip(1).contiguous()
    _assert_same(R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True, grid=(nx, ny, S), item_order=mixed), plain, "slabs permuted")
    sel = (torch.arange(0, nx * ny, 8, device="cuda")[:, None] * S + torch.arange(S, device="cuda")[None]).reshape(-1)
    sub = pts[sel].contiguous()
    _assert_same(tuple(t[sel] for t in plain), (*R.mesh_query(verts, faces, vv, sub, want_face=True), R.knn1(_v4(verts), sub)), "every 8th ray")


def test_order_without_a_grid_is_refused(R):
    from vanerf_amd._ffi import VanerfError
    verts, faces, vv = _mesh("two_fingered_hands")
    pts = torch.zeros(64, 3, device="cuda")
    with pytest.raises((VanerfError, ValueError)):
        R.mesh_query_accel(R.MeshAccel(verts, faces), verts, faces, vv, pts, item_order=torch.zeros(64, dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# the pass: VANERF_MESH_TILE_ORDER is read by the library, so each setting runs in a child process of its own
# ---------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from vanerf_amd import renderer as R, synth
from vanerf_amd.model import get_360cameras
from vanerf_amd.novel_views import camera_to_cam_tar

sd = synth.make_full_weights(0)
w = R.PackedWeights(sd, mode="bf16x3")
sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
out = {}
for (W, Sc) in ((16, 16), (64, 64)):
    frame_cpu = synth.make_frame(seed=3, tar_h=W, tar_w=W)
    fd = synth.to_device(frame_cpu, "cuda")
    fdat = R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
    headpose = torch.eye(4)
    headpose[:3, 3] = frame_cpu["targets"]["vert_world"][0].mean(0)
    cams = [camera_to_cam_tar(c) for c in get_360cameras(headpose[:3, :4].cuda(), 4.0 * W, 1.0, 1.0, W, W, 0.71, 1.42, n_frames=8)]
    for views in (1, 2):
        for reuse in (True, False):
            cam = cams[1] if views == 1 else [cams[1], cams[4]]
            d, keep = R._pass_desc(cam, fd["bounds"], 0, 0, 1, W, W, Sc, fdat.verts3.device, Sc, True, reuse)
            nbytes = R.render_pass_views_scratch(views, W * W, Sc, Sc, True, reuse)
            scratch = torch.full((nbytes // 4 + 1,), float("nan"), device="cuda").view(torch.uint8)  # a NaN-filled scratch block
            res = R._run_pass(w, fdat, d, scratch)
            for k, v in res.items():
                out[f"c_{W}_{views}_{int(reuse)}_{k}"] = v.cpu().numpy()
    # the Python sequence of the same pass (what bench.py times)
    res = R.render_pass(w, fdat, cams[1], fd["bounds"], 0, 0, 1, W, W, Sc, Sc)
    for k in ("color", "depth", "alpha", "color_fine", "depth_fine", "alpha_fine", "sdf", "z_fine"):
        out[f"py_{W}_{k}"] = res[k].cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[2], **out)
"""


@pytest.fixture(scope="module")
def pass_outputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_order_pass")
    got = {}
    for tag, value in (("default", None), ("off", "0")):
        env = {k: v for k, v in os.environ.items() if k != "VANERF_MESH_TILE_ORDER"}
        if value is not None:
            env["VANERF_MESH_TILE_ORDER"] = value
        path = os.path.join(d, tag + ".npz")
        res = subprocess.run([sys.executable, "-c", _CHILD, REPO, path], env=env, capture_output=True, text=True)
        assert res.returncode == 0, f"VANERF_MESH_TILE_ORDER={value}: exit {res.returncode}\n{res.stderr[-3000:]}"
        with np.load(path) as z:
            got[tag] = {k: z[k] for k in z.files}
    return got


def test_the_pass_does_not_depend_on_the_tile_order(pass_outputs):
    """vanerf_render_pass at 16 x 16 rays, 16 + 16 samples and at 64 x 64, 64 + 64 (524 288 samples per march: above PARTITION_MIN_SAMPLES): a
    single view and a two-view camera table (the tiles of the stacked grid are those of either view: 16 and 64 rows are whole tiles), with and
    without coarse re-use, in a NaN-filled scratch block; and renderer.render_pass.  VANERF_MESH_TILE_ORDER unset against 0: every output,
    bit for bit."""
    a, b = pass_outputs["default"], pass_outputs["off"]
    assert set(a) == set(b) and len(a) >= 2 * (4 * 11 + 8)
    for k in sorted(a):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{k} differs between VANERF_MESH_TILE_ORDER unset and 0"
    assert a["c_64_2_1_hit"].any()  # rays that hit the bounding box: the marches had something to do
