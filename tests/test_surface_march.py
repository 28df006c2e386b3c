"""Marching tetrahedra on the GPU (vanerf_surface_count / vanerf_surface_emit, vanerf_amd/csrc/surface.hip) against an fp64 numpy
restatement written here with the same conventions (include/vanerf_hip.h).  Needs a real MI355X: `pytest -m gpu`.

The fields are analytic, computed here in fp32 and uploaded.  The restatement is unindexed: it lists the triangles of every tetrahedron by
the grid edges their corners lie on, and orients each by the gradient of the tetrahedron's own linear interpolant.  A HIP mesh is compared
with it by matching every HIP vertex to the crossed grid edge it lies on (positions within 1e-6 x the grid extent, one to one), after which
the two triangle sets are compared as sets of oriented edge triples.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
# two corners inside: the quadrilateral is cut along the diagonal between the cut points of these two edges (local corners of the
# tetrahedron v0 ... v3; keyed by the pair that holds v0)
DIAGONAL = {frozenset((0, 1)): ((0, 2), (1, 3)), frozenset((0, 2)): ((0, 3), (1, 2)), frozenset((0, 3)): ((0, 1), (2, 3))}


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import surface
    return surface


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def grid_xyz(origin, spacing, dims):
    """(nz, ny, nx, 3) fp64 positions from the fp32 origin and spacing: index x spacing is exact in fp64 and so is the sum at these magnitudes,
    so rounding it to fp32 once is the kernels' fmaf."""
    nx, ny, nz = dims
    o, s = np.asarray(origin, np.float32).astype(np.float64), np.asarray(spacing, np.float32).astype(np.float64)
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([o[0] + xx * s[0], o[1] + yy * s[1], o[2] + zz * s[2]], -1)


def local_triangles(m):
    """The triangles of a tetrahedron whose corners k with bit k of m set are inside, as triples of local edges (a, b), a < b; unoriented."""
    ins = [k for k in range(4) if m >> k & 1]
    out = [k for k in range(4) if not m >> k & 1]
    edge = lambda a, b: (min(a, b), max(a, b))  # noqa: E731
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        pair = frozenset(ins) if 0 in ins else frozenset(out)
        d0, d1 = DIAGONAL[pair]
        rest = [edge(a, b) for a in ins for b in out if edge(a, b) not in (d0, d1)]
        assert len(rest) == 2
        return [(d0, d1, rest[0]), (d0, d1, rest[1])]
    a, others = (ins[0], out) if len(ins) == 1 else (out[0], ins)
    return [tuple(edge(a, b) for b in others)]


def march_ref(f, origin, spacing, iso):
    """f (nz, ny, nx) fp32 -> (edges (E, 2) int64: the crossed grid edges as linear indices lo < hi, sorted; pos (E, 3) fp64: their vertices;
    tris (T, 3) int64 into edges, oriented with the normal towards growing f)."""
    f = np.asarray(f, np.float32)
    nz, ny, nx = f.shape
    g = np.where(np.isfinite(f), f.astype(np.float64), FLT_MAX).reshape(-1)
    inside = g < float(iso)
    xyz = grid_xyz(origin, spacing, (nx, ny, nz)).reshape(-1, 3)
    zz, yy, xx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    base = np.stack([xx, yy, zz], -1).reshape(-1, 3)
    ends, grads = [], []
    for perm in itertools.permutations(range(3)):
        offs = [np.zeros(3, np.int64)]
        for ax in perm:
            o = offs[-1].copy()
            o[ax] += 1
            offs.append(o)
        P = base[:, None, :] + np.stack(offs)[None]
        lin = (P[..., 2] * ny + P[..., 1]) * nx + P[..., 0]                 # (cells, 4): v0 ... v3, ascending
        mask = (inside[lin] * (1 << np.arange(4))).sum(1)
        for m in range(1, 15):
            sel = lin[mask == m]
            if not len(sel):
                continue
            # gradient of the linear interpolant: rows (v_k - v_0) . grad = g_k - g_0
            A = xyz[sel[:, 1:]] - xyz[sel[:, :1]]
            grad = np.linalg.solve(A, (g[sel[:, 1:]] - g[sel[:, :1]])[..., None])[..., 0]
            for tri in local_triangles(m):
                ends.append(np.stack([np.stack([sel[:, a], sel[:, b]], -1) for a, b in tri], 1))  # (n, 3, 2)
                grads.append(grad)
    if not ends:
        return np.zeros((0, 2), np.int64), np.zeros((0, 3)), np.zeros((0, 3), np.int64)
    ends, grads = np.concatenate(ends), np.concatenate(grads)
    key = ends[..., 0] * (nx * ny * nz) + ends[..., 1]
    ukey, inv = np.unique(key.reshape(-1), return_inverse=True)
    edges = np.stack([ukey // (nx * ny * nz), ukey % (nx * ny * nz)], -1)
    ga, gb = g[edges[:, 0]], g[edges[:, 1]]
    t = (float(iso) - ga) / (gb - ga)
    pos = xyz[edges[:, 0]] + t[:, None] * (xyz[edges[:, 1]] - xyz[edges[:, 0]])
    tris = inv.reshape(-1, 3)
    p = pos[tris]
    flip = (np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) * grads).sum(1) < 0
    tris[flip] = tris[flip][:, [0, 2, 1]]
    return edges, pos, tris


def canonical(tris):
    """Rows rotated so that the smallest entry leads (orientation kept), then sorted."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    k = tris.argmin(1)
    rot = np.stack([tris[np.arange(len(tris)), (k + j) % 3] for j in range(3)], -1)
    return rot[np.lexsort(rot.T[::-1])]


def match_vertices(verts, pos, tol):
    """HIP vertex -> index of the restatement's vertex: nearest, within tol, one to one."""
    assert verts.shape == pos.shape, (verts.shape, pos.shape)
    idx = np.empty(len(verts), np.int64)
    for s in range(0, len(verts), 1024):
        d = np.abs(verts[s:s + 1024, None, :].astype(np.float64) - pos[None]).max(-1)
        idx[s:s + 1024] = d.argmin(1)
        assert d.min(1).max() <= tol, (d.min(1).max(), tol)
    assert len(np.unique(idx)) == len(pos)
    return idx


def edge_use(faces):
    """directed edge (i, j) -> count, as a dict keyed by i * V + j with V past the largest index"""
    f = np.asarray(faces, np.int64)
    V = int(f.max()) + 1 if f.size else 1
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    keys, cnt = np.unique(d[:, 0] * V + d[:, 1], return_counts=True)
    return V, keys, cnt


def assert_manifold(faces, closed):
    """No directed edge twice; closed: every directed edge has its reverse.  Open: an edge is then used once, or twice in opposite directions."""
    V, keys, cnt = edge_use(faces)
    assert (cnt == 1).all(), "a directed edge is used by two triangles"
    rev = (keys % V) * V + keys // V
    has_rev = np.isin(rev, keys)
    if closed:
        assert has_rev.all(), f"{int((~has_rev).sum())} boundary edges on a closed surface"
    return int(has_rev.sum()) // 2 + int((~has_rev).sum())  # undirected edges


def signed_volume(pos, tris):
    p = np.asarray(pos, np.float64)[np.asarray(tris, np.int64)]
    return float((p[:, 0] * np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# fields and the HIP side
# ---------------------------------------------------------------------------------------------------------------------------------
def sphere(dims, origin, spacing, centre, radius):
    p = grid_xyz(origin, spacing, dims)
    return (np.linalg.norm(p - np.asarray(centre), axis=-1) - radius).astype(np.float32)


def torus(dims, origin, spacing, centre, R, r):
    p = grid_xyz(origin, spacing, dims) - np.asarray(centre)
    return (np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R) ** 2 + p[..., 2] ** 2) - r).astype(np.float32)


def hip_march(S, f, origin, spacing, iso=0.0, rgb=None):
    fd = torch.from_numpy(np.ascontiguousarray(f, np.float32)).cuda()
    rd = None if rgb is None else torch.from_numpy(np.ascontiguousarray(rgb, np.float32)).cuda()
    v, t, c = S.march(fd, origin, spacing, iso, rd)
    torch.cuda.synchronize()
    return v.cpu().numpy(), t.cpu().numpy(), None if c is None else c.cpu().numpy()


def extent(spacing, dims):
    return float(max(s * (n - 1) for s, n in zip(spacing, dims)))


def compare_with_restatement(S, f, origin, spacing, iso=0.0, separated=True):
    """Counts, vertex positions and the oriented triangle set of the HIP mesh against the restatement -> (verts, faces, edges, pos, tris)."""
    nz, ny, nx = f.shape
    edges, pos, tris = march_ref(f, origin, spacing, iso)
    verts, faces, _ = hip_march(S, f, origin, spacing, iso)
    assert (len(verts), len(faces)) == (len(pos), len(tris)), ((len(verts), len(faces)), (len(pos), len(tris)))
    assert np.isfinite(verts).all()
    if len(faces):
        assert faces.min() >= 0 and faces.max() < len(verts)
    if separated and len(verts):
        tol = 1e-6 * extent(spacing, (nx, ny, nz))
        idx = match_vertices(verts, pos, tol)
        assert np.array_equal(canonical(idx[faces]), canonical(tris))
        # each vertex lies on its grid edge: between the ends on every axis, in fp32, and on the line where the ends share a coordinate
        xyz = grid_xyz(origin, spacing, (nx, ny, nz)).astype(np.float32).reshape(-1, 3)
        a, b = xyz[edges[idx, 0]], xyz[edges[idx, 1]]
        assert (verts >= np.minimum(a, b)).all() and (verts <= np.maximum(a, b)).all()
    return verts, faces, edges, pos, tris


SPHERE_GRID = dict(dims=(9, 8, 7), origin=(-0.31, 0.12, 0.55), spacing=(0.11, 0.13, 0.17))


def test_sphere_off_centre_on_unequal_axes(S):
    g = SPHERE_GRID
    f = sphere(g["dims"], g["origin"], g["spacing"], centre=(0.17, 0.53, 1.09), radius=0.33)
    assert f[0].min() > 0 and f[-1].min() > 0 and f[:, 0].min() > 0 and f[:, -1].min() > 0 and f[:, :, 0].min() > 0 and f[:, :, -1].min() > 0
    verts, faces, edges, pos, tris = compare_with_restatement(S, f, g["origin"], g["spacing"])
    assert len(verts) > 100
    E = assert_manifold(faces, closed=True)
    assert len(verts) - E + len(faces) == 2
    vol, vol_ref = signed_volume(verts, faces), signed_volume(pos, tris)
    assert vol > 0 and abs(vol - vol_ref) <= 1e-5 * vol_ref
    assert 0.5 * 4 / 3 * np.pi * 0.33 ** 3 < vol_ref < 4 / 3 * np.pi * 0.33 ** 3  # (the restatement itself: the distance is convex, so its cuts lie inside)


def test_torus(S):
    dims, origin, spacing = (17, 17, 9), (-0.8, -0.8, -0.3), (0.1, 0.1, 0.075)
    f = torus(dims, origin, spacing, centre=(0.013, -0.021, 0.007), R=0.47, r=0.19)
    verts, faces, _, pos, tris = compare_with_restatement(S, f, origin, spacing)
    E = assert_manifold(faces, closed=True)
    assert len(verts) - E + len(faces) == 0
    vol, vol_ref = signed_volume(verts, faces), signed_volume(pos, tris)
    assert vol > 0 and abs(vol - vol_ref) <= 1e-5 * vol_ref


@pytest.mark.parametrize("dims", [(33, 33, 33), (65, 3, 3)])
def test_more_than_one_brick(S, dims):
    """33^3: five bricks per axis, 125 blocks in the scans; 65 x 3 x 3: nine bricks along x, partial in y and z."""
    spacing = (0.031, 0.029, 0.033) if dims[1] > 3 else (0.02, 0.3, 0.3)
    origin = (-0.5, -0.45, -0.52) if dims[1] > 3 else (-0.64, -0.31, -0.28)
    if dims[1] > 3:
        f = sphere(dims, origin, spacing, centre=(0.004, 0.011, -0.003), radius=0.41)
    else:  # a cylinder of ripples along x: the surface crosses every brick
        p = grid_xyz(origin, spacing, dims)
        f = (np.sin(9.0 * p[..., 0]) * 0.2 + 0.37 * p[..., 1] - 0.23 * p[..., 2] + 0.011).astype(np.float32)
    verts, faces, *_ = compare_with_restatement(S, f, origin, spacing)
    assert len(faces) > 50
    assert_manifold(faces, closed=dims[1] > 3)


def test_single_cell_all_sign_cases(S):
    """2 x 2 x 2, the smallest legal grid: all 256 sign patterns of the cell's corners, so each of the six tetrahedra meets each of its 16
    cases.  The restatement orients every triangle by the gradient of its tetrahedron's linear interpolant."""
    origin, spacing = (0.1, -0.2, 0.3), (0.7, 1.1, 1.3)
    seen = set()
    for pattern in range(256):
        mag = 0.3 + 0.07 * np.arange(8)
        f = np.where(pattern >> np.arange(8) & 1, -mag, mag).astype(np.float32).reshape(2, 2, 2)  # corner c = dx | dy << 1 | dz << 2
        verts, faces, edges, pos, tris = compare_with_restatement(S, f, origin, spacing)
        assert len(faces) == sum(len(local_triangles(m)) for m in tet_masks(pattern))
        seen.update((t, m) for t, m in enumerate(tet_masks(pattern)))
    assert len(seen) == 96


def tet_masks(pattern):
    out = []
    for perm in itertools.permutations(range(3)):
        c1 = 1 << perm[0]
        c2 = c1 | 1 << perm[1]
        out.append((pattern & 1) | (pattern >> c1 & 1) << 1 | (pattern >> c2 & 1) << 2 | (pattern >> 7 & 1) << 3)
    return out


def test_values_equal_to_iso_count_as_outside(S):
    dims, origin, spacing = (9, 7, 6), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    p = grid_xyz(origin, spacing, dims)
    f = (p[..., 0] + p[..., 1] + p[..., 2] - 9.0).astype(np.float32)  # exact zeros on a whole plane of grid points
    assert (f == 0).sum() > 20
    verts, faces, edges, pos, tris = compare_with_restatement(S, f, origin, spacing, separated=False)  # (vertices coincide at those points)
    assert len(faces) > 0 and np.isfinite(verts).all() and faces.min() >= 0 and faces.max() < len(verts)
    assert not (f.reshape(-1)[edges] < 0).all(1).any() and (f.reshape(-1)[edges] < 0).any(1).all()
    iso = 2.0  # and with another level
    verts, faces, *_ = compare_with_restatement(S, f, origin, spacing, iso=iso, separated=False)
    assert len(faces) > 0 and np.isfinite(verts).all()


def test_non_finite_values_read_as_outside(S):
    g = SPHERE_GRID
    f = sphere(g["dims"], g["origin"], g["spacing"], centre=(0.17, 0.53, 1.09), radius=0.33)
    f[:, :, 4] = np.nan
    f[:, 3, :3] = np.inf
    f[2, :, 5:] = -np.inf
    assert (f < 0).sum() > 10
    # (the vertices of edges that end at a non-finite value sit on the finite end, several in one place: counts only, no matching)
    verts, faces, *_ = compare_with_restatement(S, f, g["origin"], g["spacing"], separated=False)
    assert np.isfinite(verts).all() and len(faces) > 20
    assert_manifold(faces, closed=True)  # the non-finite points are outside like any other, so the surface still closes
    _, faces_big, _ = hip_march(S, np.where(np.isfinite(f), f, np.float32(1e30)), g["origin"], g["spacing"])
    assert np.array_equal(faces, faces_big)  # the same mesh as with a large finite value in their place


def test_surface_cut_by_the_grid_boundary_is_open(S):
    g = SPHERE_GRID
    f = sphere(g["dims"], g["origin"], g["spacing"], centre=(0.02, 0.5, 1.0), radius=0.45)  # reaches past x = 0 .. and z
    assert f[:, :, 0].min() < 0
    verts, faces, *_ = compare_with_restatement(S, f, g["origin"], g["spacing"])
    V, keys, cnt = edge_use(faces)
    assert (cnt == 1).all()  # never two triangles on one side of an edge: an edge is used once, or twice in opposite directions
    rev = (keys % V) * V + keys // V
    assert (~np.isin(rev, keys)).sum() > 0  # and there is a boundary


def _raw(S):
    from vanerf_amd import _ffi
    return _ffi.lib


def _count(lib, fd, dims, iso, scratch, counts, stream=None):
    nx, ny, nz = dims
    return lib.vanerf_surface_count(ctypes.c_void_p(fd.data_ptr()), nx, ny, nz, iso, ctypes.c_void_p(scratch.data_ptr()), scratch.numel() * 8,
                                    ctypes.c_void_p(counts.data_ptr()), stream)


def _emit(lib, S, fd, rgb, origin, spacing, dims, iso, scratch, n, verts, colors, tris, caps, stream=None):
    nx, ny, nz = dims
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    return lib.vanerf_surface_emit(p(fd), p(rgb), S._f3(origin), S._f3(spacing), nx, ny, nz, iso, p(scratch), scratch.numel() * 8, n[0], n[1],
                                   p(verts), p(colors), p(tris), caps[0], caps[1], stream)


def test_empty_grids_capacities_and_limits(S):
    lib = _raw(S)
    g = SPHERE_GRID
    dims, origin, spacing = g["dims"], g["origin"], g["spacing"]
    nx, ny, nz = dims
    for value in (-1.0, 1.0):  # all inside, all outside
        verts, faces, _ = hip_march(S, np.full((nz, ny, nx), value, np.float32), origin, spacing)
        assert verts.shape == (0, 3) and faces.shape == (0, 3)
    assert lib.vanerf_surface_emit(None, None, S._f3(origin), S._f3(spacing), nx, ny, nz, 0.0, None, 0, 0, 0, None, None, None, 0, 0, None) == 0

    f = sphere(dims, origin, spacing, centre=(0.17, 0.53, 1.09), radius=0.33)
    fd = torch.from_numpy(f).cuda()
    scratch = torch.empty(lib.vanerf_surface_scratch(nx, ny, nz) // 8 + 2, dtype=torch.float64, device="cuda")
    counts = torch.empty(2, dtype=torch.int64, device="cuda")
    assert _count(lib, fd, dims, 0.0, scratch, counts) == 0
    nv, nt = counts.tolist()
    assert nv > 100 and nt > 100
    SENT_F, SENT_I = -12345.0, -777
    verts = torch.full((nv, 3), SENT_F, device="cuda")
    tris = torch.full((nt, 3), SENT_I, dtype=torch.int32, device="cuda")
    # too small a capacity for the counts passed back: an error, and nothing is written
    for caps in ((nv - 1, nt), (nv, nt - 1)):
        assert _emit(lib, S, fd, None, origin, spacing, dims, 0.0, scratch, (nv, nt), verts, None, tris, caps) == -22
        assert b"capacity" in lib.vanerf_last_error()
    torch.cuda.synchronize()
    assert (verts == SENT_F).all() and (tris == SENT_I).all()
    # a caller that passes smaller counts than the device holds: the kernels stop at the capacities
    hv, ht = nv // 2, nt // 3
    assert _emit(lib, S, fd, None, origin, spacing, dims, 0.0, scratch, (hv, ht), verts, None, tris, (hv, ht)) == 0
    torch.cuda.synchronize()
    assert (verts[hv:] == SENT_F).all() and (tris[ht:] == SENT_I).all()
    assert (verts[:hv] != SENT_F).any(1).all() and (tris[:ht] != SENT_I).all()
    full_v, full_t, _ = hip_march(S, f, origin, spacing)
    assert np.array_equal(verts[:hv].cpu().numpy(), full_v[:hv]) and np.array_equal(tris[:ht].cpu().numpy(), full_t[:ht])

    # limits are errors with a message
    p = ctypes.c_void_p(scratch.data_ptr())
    for bad in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 0, 0), (1024, 1024, 1024), (40000, 40000, 2)):
        assert lib.vanerf_surface_scratch(*bad) == 0
        assert lib.vanerf_surface_count(p, *bad, 0.0, p, 1 << 40, p, None) == -22
        msg = lib.vanerf_last_error()
        assert (b"at least 2" in msg) if min(bad) < 2 else (b"2^31" in msg), msg
        assert lib.vanerf_surface_emit(p, None, S._f3(origin), S._f3(spacing), *bad, 0.0, p, 1 << 40, 1, 1, p, None, p, 1, 1, None) == -22
        assert lib.vanerf_grid_points(S._f3(origin), S._f3(spacing), *bad, 0, 1, p, None) == -22
    assert _count(lib, fd, dims, float("nan"), scratch, counts) == -22 and b"iso" in lib.vanerf_last_error()
    assert lib.vanerf_surface_count(p, nx, ny, nz, 0.0, p, 64, p, None) == -22 and b"scratch" in lib.vanerf_last_error()
    assert _emit(lib, S, fd, None, origin, (0.1, 0.0, 0.1), dims, 0.0, scratch, (nv, nt), verts, None, tris, (nv, nt)) == -22
    assert b"spacing" in lib.vanerf_last_error()
    with pytest.raises(ValueError):
        S.march(fd.cpu(), origin, spacing)
    with pytest.raises(ValueError):
        S.march(fd[:1], origin, spacing)


def test_bit_reproducible_whatever_scratch_and_stream(S):
    lib = _raw(S)
    dims, origin, spacing = (33, 20, 11), (-0.5, -0.3, -0.2), (0.031, 0.033, 0.041)
    nx, ny, nz = dims
    f = sphere(dims, origin, spacing, centre=(0.004, 0.011, -0.003), radius=0.19)
    p = grid_xyz(origin, spacing, dims)
    rgb = np.stack([p[..., 0] + 0.5, 0.3 * p[..., 1], p[..., 2] * p[..., 0]], -1).astype(np.float32)
    fd, rd = torch.from_numpy(f).cuda(), torch.from_numpy(rgb).cuda()
    nwords = lib.vanerf_surface_scratch(nx, ny, nz) // 8 + 2
    side = torch.cuda.Stream()
    results = []
    for fill, stream in ((float("nan"), None), (float("nan"), None), (1e300, side), (0.0, None)):
        scratch = torch.full((nwords,), fill, dtype=torch.float64, device="cuda")
        counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        st = ctypes.c_void_p(stream.cuda_stream) if stream is not None else ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert _count(lib, fd, dims, 0.0, scratch, counts, st) == 0
        if stream is not None:
            stream.synchronize()
        nv, nt = counts.tolist()
        verts = torch.full((nv, 3), float("nan"), device="cuda")
        cols = torch.full((nv, 3), float("nan"), device="cuda")
        tris = torch.full((nt, 3), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert _emit(lib, S, fd, rd, origin, spacing, dims, 0.0, scratch, (nv, nt), verts, cols, tris, (nv, nt), st) == 0
        torch.cuda.synchronize()
        results.append((verts.cpu(), cols.cpu(), tris.cpu()))
    assert results[0][0].shape[0] > 500
    for r in results[1:]:
        for a, b in zip(results[0], r):
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.isfinite(results[0][0]).all() and torch.isfinite(results[0][1]).all()


def test_colours_follow_a_linear_colour_field(S):
    g = SPHERE_GRID
    dims, origin, spacing = g["dims"], g["origin"], g["spacing"]
    f = sphere(dims, origin, spacing, centre=(0.17, 0.53, 1.09), radius=0.33)
    A = np.array([[0.9, -0.3, 0.2], [0.1, 0.7, -0.4], [-0.5, 0.25, 0.6]])
    b = np.array([0.3, 0.5, 0.1])
    rgb = (grid_xyz(origin, spacing, dims) @ A.T + b).astype(np.float32)
    verts, faces, colors = hip_march(S, f, origin, spacing, rgb=rgb)
    assert colors.shape == verts.shape and len(verts) > 100
    assert np.abs(colors - (verts.astype(np.float64) @ A.T + b)).max() <= 1e-5
    verts2, faces2, none = hip_march(S, f, origin, spacing)
    assert none is None and np.array_equal(verts, verts2) and np.array_equal(faces, faces2)
