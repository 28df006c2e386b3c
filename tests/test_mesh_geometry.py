"""The mesh queries -- signed distance, closest face, visibility flag, 1-NN vertex -- held to an fp64 reference written from their mathematical
definition (tests/mesh_geometry_ref.py), on closed meshes that are not star-shaped: hands with five thin lobes and deep gaps, two of them
interpenetrating, a torus, a sphere with a cavity; at four placements (offset, scale) of the coordinate range the library is used in.

The chain: fp64 definition  <-bars->  oracle/mesh_oracle.c (CPU tests, no GPU)  <-bits->  vanerf_mesh_query / vanerf_knn1 (exhaustive)
<-bits->  vanerf_mesh_query_accel (per-lane search, tile searches with the ray-grid hint, one and two depths per item); the accelerated
kernel is also held to the fp64 reference directly (torch float64 on the device).

Bars, the same for the oracle and every HIP path; U = 2^-23 max |coordinate| over the mesh and the points of a case (1.3e-7 at the frames'
placement): the rounding step of a coordinate difference at that magnitude.
  distance   | |sdf| - sqrt(d64^2 + 1e-6) | <= 4 U
  sign       (sdf < 0) == parity of the rounded winding number wherever d64 > 100 U; at most 5 % of a case undecided
  face       d64(p, reported face) - d64 <= 4 U; a point exactly on a vertex reports the lowest-index face that holds the vertex
  visibility the flag equals (sum_k w_k vert_vis >= 0.1) in fp64 wherever |sum - 0.1| > 1e-4; at most 1 % of a case undecided
  1-NN       d64(p, v[idx]) - min <= 4 U; a point exactly on a vertex reports that vertex

What this file found: the +x parity ray of the inside test decided an exact tie of an edge function by vertex index alone.  That is sound on
an edge and unsound at a vertex: a point that shares y and z with a vertex (the ray meets the vertex' projection, every edge function of the
fan ties) got 0, 1 or 2 crossings from the fan whatever its geometry.  Of 4 000 such points per mesh, decided ones only, the C oracle (and
the kernels, bit-equal to it) had the wrong sign on 28 (fingered hand), 32-33 (two hands, by placement), 10 (fine hand), 83 (torus) and 0 (shells);
three points of the torus' axis line are among them.  A tie is now decided as if the point were displaced by (eps^2, eps) in (y,z), the same
for every edge (oracle/mesh_oracle.c:edge_side, csrc/mesh_device.h:edges_agree): 0 wrong on all of them.
A point at distance exactly 0 keeps the index rule: its sign means nothing under either, and the earlier tests and fixtures, whose only exact
ties are points placed on vertices, recorded that one -- every result computed before this file existed is unchanged, bit for bit.

Observed, C oracle on the CPU (this file's quarter-size point sets, ~2 600 points per case) -- worst |distance error|, face excess, 1-NN
excess in U, undecided signs / flags in % of the case; no sign or flag mismatch anywhere:
  fingered_hand       0.70  0.20  0.00   2.61 / 0.000      torus               0.37  0.21  0.12   3.58 / 0.000
  two_fingered_hands  0.60  0.41  0.00   2.57 / 0.000      nested_shells       0.41  0.17  0.00   3.03 / 0.000
  fingered_hand_fine  0.70  0.29  0.00   2.72 / 0.000      two hands p1 p2 p3  0.54 0.78 0.47 (distance)  4.15 2.34 2.94 / 0.075 0 0
Observed on the MI355X (vanerf_mesh_query_accel against torch float64 on the device; the exhaustive kernels and the oracle agree with it
bit for bit) -- the worst over a case's point set (~10 000 points) and its two ray grids; undecided shares are the point set's (on the ray
grids: signs <= 0.11 %, flags <= 0.015 %); no sign or flag mismatch anywhere:
  fingered_hand       0.91  0.60  0.00   2.78 / 0.010      torus               0.81  0.43  0.13   3.59 / 0.000
  two_fingered_hands  0.91  0.74  0.00   2.74 / 0.000      nested_shells       0.48  0.15  0.00   3.36 / 0.020
  fingered_hand_fine  0.85  0.67  0.00   2.82 / 0.010      two hands p1 p2 p3  0.64 0.93 0.85 (distance)  0.53 0.93 0.55 (face)
                                                                               4.18 2.69 3.09 / 0.000 0.000 0.010
  (two_fingered_hands includes the border bands at 1 .. 256 cells, 0.71, and the two-depth case, 0.91 / 0.74.)  The HIP paths need no more
  than the oracle: they compute its bits.
On these meshes the tile searches overflow often (a library built with -DVANERF_MESH_PHASES): of the 1 024 waves of the 64 x 64 x 16 grid
about two_fingered_hands, 229 overflow the cluster list (TL_LIST) and fall back to the per-lane search, 440 evaluate their candidates in
batches (TL_CAND); of the 20 736 items of the two-depth case 187 and 5 450.  The torus and the shells are metres wide: all their tiles are too
wide for the tile search and take the per-lane search, as do the x2 placement's at 40 x 24.
"""
import ctypes
import functools

import pytest
import torch

from oracle import vanerf_oracle as orc
from tests import mesh_geometry_ref as G

EXPECTED_COUNTS = {"fingered_hand": (779, 1554), "two_fingered_hands": (1558, 3108), "fingered_hand_fine": (2402, 4800), "torus": (960, 1920),
                   "nested_shells": (244, 480)}
RAY_GRIDS = ((64, 64, 16), (40, 24, 15))  # (an odd number of depths: the last depth group of a tile is half empty)
FP64_POINTS = 20000  # at most this many points of a case go through the fp64 reference


def oracle_query(verts, faces, vert_vis, pts):
    """oracle/mesh_oracle.c:mesh_query through the library itself, with given vertex flags -> sdf (N,), vis (N,) uint8, face (N,) int32."""
    V, F, vv, P = verts.float().contiguous(), faces.to(torch.int32).contiguous(), vert_vis.float().contiguous(), pts.float().contiguous()
    n = P.shape[0]
    sdf, vis, face = torch.empty(n), torch.empty(n, dtype=torch.uint8), torch.empty(n, dtype=torch.int32)
    orc._mesh_lib().mesh_query(orc._fp(V), ctypes.c_int(V.shape[0]), orc._fp(F), ctypes.c_int(F.shape[0]), orc._fp(vv), orc._fp(P),
                               ctypes.c_int64(n), orc._fp(sdf), orc._fp(vis), orc._fp(face))
    return sdf, vis, face


@functools.lru_cache(maxsize=None)
def _mesh(name, placement):
    verts, faces, _, _ = G.placed_mesh(name, placement)
    return verts, faces, G.vertex_flags(verts.shape[0], placement)


@functools.lru_cache(maxsize=None)
def _case(name, placement, quarter):
    """A case on the CPU, computed once and shared: the placed mesh, its flags, the point set and the C oracle's answers."""
    verts, faces, vv = _mesh(name, placement)
    k = 4 if quarter else 1
    pts = G.point_set(name, placement, 6400 // k, 200 // k, 1200 // k, 2000 // k, 160 // k)
    sdf, vis, face = oracle_query(verts, faces, vv, pts)
    return dict(verts=verts, faces=faces, vv=vv, pts=pts, sdf=sdf, vis=vis, face=face, knn=orc.knn1(pts, verts))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the meshes, and the C oracle against the fp64 definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.MESHES))
def test_meshes_are_closed_and_consistently_oriented(name):
    """Every undirected edge belongs to exactly two faces, once in each direction; the enclosed (signed) volume is positive: outward winding."""
    v, f = G.MESHES[name]()
    assert (v.shape[0], f.shape[0]) == EXPECTED_COUNTS[name] and v.dtype.name == "float32" and f.dtype.name == "int64"
    f = torch.from_numpy(f)
    nv = v.shape[0]
    assert f.min() == 0 and f.max() == nv - 1 and torch.unique(f).numel() == nv
    a, b = torch.cat([f[:, 0], f[:, 1], f[:, 2]]), torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    assert (a != b).all()
    directed = a * nv + b
    assert torch.unique(directed).numel() == directed.numel()  # no directed edge twice: two faces never run along an edge the same way
    assert torch.equal(directed.sort()[0], (b * nv + a).sort()[0])  # ... and every directed edge has its reverse: exactly two faces per edge
    t = torch.from_numpy(v).double()[f]
    assert (t[:, 0] * torch.cross(t[:, 1], t[:, 2], dim=-1)).sum() / 6.0 > 0
    assert torch.unique(torch.from_numpy(v), dim=0).shape[0] == nv  # no two vertices coincide (the on-vertex rules assume it)


@pytest.mark.parametrize("name,placement", G.CASES, ids=G.CASE_IDS)
def test_oracle_within_the_bars_of_the_fp64_definition(name, placement):
    c = _case(name, placement, True)
    ref = G.reference(c["verts"], c["faces"], c["pts"], c["vv"], c["face"], c["knn"])
    fig = G.check_bars(ref, G.unit_step(c["verts"], c["pts"]), c["sdf"], c["vis"], c["face"], c["knn"], f"oracle {name}-p{placement}", faces=c["faces"])
    assert 0.1 < fig["inside"] < 0.6  # both signs occur


def test_oracle_on_every_vertex():
    """A point exactly on a vertex: that vertex is its 1-NN and its face is the lowest-index face that holds the vertex -- all 1 558 vertices of
    two_fingered_hands, at every placement."""
    for placement in range(len(G.PLACEMENTS)):
        verts, faces, vv = _mesh("two_fingered_hands", placement)
        sdf, _, face = oracle_query(verts, faces, vv, verts)
        assert torch.equal(face.long(), G.lowest_incident_face(faces, verts.shape[0])), placement
        assert torch.equal(orc.knn1(verts, verts), torch.arange(verts.shape[0])), placement
        assert torch.equal(sdf.abs(), torch.full_like(sdf, 1e-6).sqrt()), placement  # the distance is exactly 0


def test_oracle_on_points_aligned_with_vertices():
    """Points that share y and z with a vertex and lie beside it along x: the +x ray of the inside test meets the vertex' projection, every
    edge function of the fan about it ties.  The sign is the fp64 parity at every decided point (see the module's docstring)."""
    for name in ("fingered_hand", "torus"):
        verts, faces, vv = _mesh(name, 0)
        g = torch.Generator().manual_seed(5)
        pts = verts[torch.randint(0, verts.shape[0], (1500,), generator=g)].clone()
        pts[:, 0] += 0.3 * float(verts[:, 0].max() - verts[:, 0].min()) * torch.randn(1500, generator=g)
        sdf, _, _ = oracle_query(verts, faces, vv, pts)
        ref = G.reference(verts, faces, pts)
        decided = ref["d"] > 100.0 * G.unit_step(verts, pts)
        wrong = int((((sdf < 0) != ref["inside"]) & decided).sum())
        print(f"{name}: {wrong} wrong signs of {int(decided.sum())} decided points aligned with a vertex, inside {100 * float(ref['inside'].double().mean()):.1f} %")
        assert wrong == 0 and decided.double().mean() > 0.95 and 0.1 < ref["inside"].double().mean() < 0.9


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


def _bits(t):
    return t.contiguous().view(torch.int32)


def _v4(verts):
    return torch.cat([verts, torch.zeros(verts.shape[0], 1, device=verts.device)], 1).contiguous()


@functools.lru_cache(maxsize=None)
def _device_mesh(name, placement):
    verts, faces, vv = _mesh(name, placement)
    return verts.cuda(), faces.to(torch.int32).cuda().contiguous(), vv.cuda()


def _assert_same(a, b, what):
    for x, y, k in zip(a, b, ("sdf", "vis", "face", "knn")):
        x, y = (_bits(x), _bits(y)) if x.dtype == torch.float32 else (x, y)
        assert torch.equal(x, y), f"{what}: {k} differs on {int((x != y).sum())} of {x.numel()} points"


def _fp64_bars(verts, faces, vv, pts, got, what, every=1):
    """The bars for `got` = (sdf, vis, face, knn) of `pts` on the device, on every `every`-th point (at most FP64_POINTS)."""
    sel = torch.arange(0, pts.shape[0], every, device=pts.device)
    assert sel.numel() <= FP64_POINTS
    p = pts[sel].contiguous()
    s, v, f, k = (t[sel] for t in got)
    ref = G.reference(verts, faces.long(), p, vv, f, k)
    return G.check_bars(ref, G.unit_step(verts, p), s, v, f, k, what, faces=faces.long())


@pytest.mark.gpu
@pytest.mark.parametrize("name,placement", G.CASES, ids=G.CASE_IDS)
def test_exhaustive_kernels_equal_the_oracle_bit_for_bit(R, name, placement):
    c = _case(name, placement, False)
    verts, faces, vv = _device_mesh(name, placement)
    pts = c["pts"].cuda()
    sdf, vis, face = R.mesh_query(verts, faces, vv, pts, want_face=True)
    knn = R.knn1(_v4(verts), pts)
    _assert_same((sdf.cpu(), vis.cpu(), face.cpu(), knn.cpu().long()), (c["sdf"], c["vis"], c["face"], c["knn"]), f"{name}-p{placement}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,placement", G.CASES, ids=G.CASE_IDS)
def test_accelerated_kernel_on_the_point_sets(R, name, placement):
    """The per-lane search (no hint) and the tile searches (the point set declared as a grid: the hint is about speed only) equal the
    exhaustive kernels bit for bit and keep the bars of the fp64 definition."""
    c = _case(name, placement, False)
    verts, faces, vv = _device_mesh(name, placement)
    pts = c["pts"].cuda()
    want = (*R.mesh_query(verts, faces, vv, pts, want_face=True), R.knn1(_v4(verts), pts))
    accel = R.MeshAccel(verts, faces)
    got = R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True)
    _assert_same(got, want, f"{name}-p{placement} no hint")
    n = pts.shape[0]
    S = next(s for s in (16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1) if n % s == 0)
    _assert_same(R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True, grid=(n // S, 1, S)), want, f"{name}-p{placement} hint")
    _fp64_bars(verts, faces, vv, pts, got, f"accel {name}-p{placement}")


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,S", RAY_GRIDS)
@pytest.mark.parametrize("name,placement", G.CASES, ids=G.CASE_IDS)
def test_accelerated_kernel_on_ray_grids(R, name, placement, nx, ny, S):
    """The samples of real rays (R.ray_setup: a target camera about 1 m from the mesh, bounds = the mesh's box with the frames' padding), with the
    ray-grid hint and without: bit-equal to the exhaustive kernels, within the bars of the fp64 definition."""
    verts, faces, vv = _device_mesh(name, placement)
    cam, bounds = G.ray_camera(verts.cpu(), nx, ny)
    rays = R.ray_setup(cam, bounds, 0, 0, 1, nx, ny, S, device="cuda")
    pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"])
    want = (*R.mesh_query(verts, faces, vv, pts, want_face=True), R.knn1(_v4(verts), pts))
    accel = R.MeshAccel(verts, faces)
    got = R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True, grid=(nx, ny, S))
    _assert_same(got, want, f"{name}-p{placement} hint")
    _assert_same(R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True), want, f"{name}-p{placement} no hint")
    every = -(-pts.shape[0] // FP64_POINTS)
    every += 1 - every % 2  # (odd: the subset visits every depth)
    fig = _fp64_bars(verts, faces, vv, pts, got, f"rays {nx}x{ny}x{S} {name}-p{placement}", every=every)
    hit = rays["hit"].float().mean().item()
    print(f"    inside {100 * (got[0] < 0).float().mean().item():.1f} % of the samples, {100 * hit:.0f} % of the rays hit the box")
    assert (got[0] < 0).float().mean() >= 0.02 and hit >= 0.05 and fig["inside"] < 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("cells", [1, 8, 64, 256])
def test_points_about_the_border_of_the_cell_grid(R, cells):
    """The inside test's `beside` shortcut (a point more than a cell outside the (y,z) extent counts no crossing) and its border cells: points
    whose y or z lies within 3 cells of the border of the extent, for a coarse .. fine cell grid, and points about the surface so that both
    signs occur."""
    name, placement = "two_fingered_hands", 0
    verts, faces, vv = _device_mesh(name, placement)
    g = torch.Generator().manual_seed(cells)
    pts = torch.cat([G.yz_band(verts.cpu(), 6144, cells, g), _case(name, placement, False)["pts"][:2048]], 0)
    pts = pts[torch.randperm(pts.shape[0], generator=g)].contiguous().cuda()
    accel = R.MeshAccel(verts, faces, grid=cells, cell_capacity=1024 * faces.shape[0])
    assert accel.table("grid", torch.float32, (5,))[4:5].view(torch.int32).item() == cells  # (the capacity sufficed: the grid was not folded into one cell)
    want = (*R.mesh_query(verts, faces, vv, pts, want_face=True), R.knn1(_v4(verts), pts))
    got = R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True)
    _assert_same(got, want, f"G={cells} no hint")
    _assert_same(R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True, grid=(32, 16, 16)), want, f"G={cells} hint")
    fig = _fp64_bars(verts, faces, vv, pts, got, f"border band G={cells}")
    assert 0.02 < fig["inside"] < 0.9


@pytest.mark.gpu
def test_batches_of_1_63_and_65_points(R):
    """Less than a wave, and one point more than a wave: every kernel against the oracle's answers for the same points."""
    name, placement = "two_fingered_hands", 0
    c = _case(name, placement, False)
    verts, faces, vv = _device_mesh(name, placement)
    accel = R.MeshAccel(verts, faces)
    for n in (1, 63, 65):
        pts = c["pts"][100:100 + n].contiguous().cuda()
        want = tuple(c[k][100:100 + n] for k in ("sdf", "vis", "face", "knn"))
        cpu = lambda r: (r[0].cpu(), r[1].cpu(), r[2].cpu(), r[3].cpu().long())
        _assert_same(cpu((*R.mesh_query(verts, faces, vv, pts, want_face=True), R.knn1(_v4(verts), pts))), want, f"exhaustive, {n} points")
        _assert_same(cpu(R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True)), want, f"accelerated, {n} points")
        _assert_same(cpu(R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True, grid=(n, 1, 1))), want, f"accelerated with a hint, {n} points")


@pytest.mark.gpu
def test_every_vertex_and_points_aligned_with_vertices(R):
    """On the device: a point exactly on a vertex answers that vertex and its lowest-index face (all vertices of two_fingered_hands at every
    placement), and points that share y and z with a vertex get the fp64 parity (the tie rule of the inside test, see the module's docstring)."""
    for placement in range(len(G.PLACEMENTS)):
        verts, faces, vv = _device_mesh("two_fingered_hands", placement)
        first = G.lowest_incident_face(faces.cpu().long(), verts.shape[0]).cuda()
        accel = R.MeshAccel(verts, faces)
        for tag, (sdf, vis, face, knn) in (("exhaustive", (*R.mesh_query(verts, faces, vv, verts, want_face=True), R.knn1(_v4(verts), verts))),
                                           ("accelerated", R.mesh_query_accel(accel, verts, faces, vv, verts, want_face=True))):
            assert torch.equal(face.long(), first) and torch.equal(knn.long(), torch.arange(verts.shape[0], device="cuda")), (tag, placement)
    for name in ("fingered_hand", "torus"):
        verts, faces, vv = _device_mesh(name, 0)
        g = torch.Generator().manual_seed(5)
        pts = verts.cpu()[torch.randint(0, verts.shape[0], (8192,), generator=g)].clone()
        pts[:, 0] += 0.3 * float(verts[:, 0].max() - verts[:, 0].min()) * torch.randn(8192, generator=g)
        pts = pts.cuda()
        want = (*R.mesh_query(verts, faces, vv, pts, want_face=True), R.knn1(_v4(verts), pts))
        got = R.mesh_query_accel(R.MeshAccel(verts, faces), verts, faces, vv, pts, want_face=True, grid=(32, 16, 16))
        _assert_same(got, want, f"{name} aligned")
        _fp64_bars(verts, faces, vv, pts, got, f"aligned with vertices, {name}")


@pytest.mark.gpu
def test_two_depths_per_item_on_a_hand_shaped_mesh(R):
    """288 x 288 rays x 32 depths = 2.65 M samples about two_fingered_hands at the frames' placement: large enough for the kernel variant that takes
    two depths of a pixel tile per item.  Every 8th ray against the exhaustive kernels (bit for bit) and, on every 17th of those samples
    (19 517 points, every depth), against the fp64 definition; the whole batch with the hint against the per-lane search."""
    name, placement, (nx, ny, S) = "two_fingered_hands", 0, (288, 288, 32)
    verts, faces, vv = _device_mesh(name, placement)
    cam, bounds = G.ray_camera(verts.cpu(), nx, ny)
    rays = R.ray_setup(cam, bounds, 0, 0, 1, nx, ny, S, device="cuda")
    pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"])
    accel = R.MeshAccel(verts, faces)
    got = R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True, grid=(nx, ny, S))
    sel = (torch.arange(0, nx * ny, 8, device="cuda")[:, None] * S + torch.arange(S, device="cuda")[None]).reshape(-1)
    sub = pts[sel].contiguous()
    want = (*R.mesh_query(verts, faces, vv, sub, want_face=True), R.knn1(_v4(verts), sub))
    got_sub = tuple(t[sel] for t in got)
    _assert_same(got_sub, want, "every 8th ray")
    _fp64_bars(verts, faces, vv, sub, got_sub, f"two depths per item, {name}-p{placement}", every=17)
    _assert_same(got, R.mesh_query_accel(accel, verts, faces, vv, pts, want_face=True), "hint against no hint")
    assert (got[0] < 0).float().mean() >= 0.02 and rays["hit"].float().mean() >= 0.05
