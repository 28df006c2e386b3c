"""An fp64 statement of ray generation, the bounding-box clip and the coarse depths, and the inputs of tests/test_ray_geometry*.py.

Plain torch in float64, written from the formulas (src/model.py:1191-1238, 1496-1570); nothing here calls the package or the oracle.  The
fp32 inputs (camera matrices, bounds, origins, directions, jitter) are taken as exact.

  rays            pixel -> direction, origin, znear / zfar along the ray (a linear solve with K, not its inverse)
  box_clip        the reference's rule restated literally: +-0.01 offset, |d| < 1e-5 -> +1e-5, six plane points, inside test with
                  eps 1e-6, a hit iff exactly two
  slab            the textbook slab test of the LINE o + t d (the reference's rule has no t >= 0 either): shares nothing with box_clip
  decision_margin how far a ray is from every decision that fp32 rounding could take the other way
  depths          uniform / stratified rows of S depths
  pixel_rows      the pixel grid of a launch; pixel_index = x + y * width in int64

decision_margin is the smallest of
  * |coordinate - (face +- eps)| over the inside comparisons on the two axes ACROSS a plane's normal.  The comparison along the normal is left
    out of this term: there the plane point sits, in exact arithmetic, at eps = 1e-6 from the bound for every ray, so an absolute 1e-4 would call
    every ray undecided.  It is decided as long as the fp32 rounding of t*d + o, at most 2^-24 (3 |plane - o| + |plane|), stays below eps;
    a ray for which it does not gets margin 0.
  * ||d_a| - 1e-5| / 1e-5, relative: an absolute 1e-4 would call every direction with a component below 1.1e-4 undecided, the tiny
    components that the tests are about among them.  The relative form leaves out fewer rays, never more.
  * |z1 - zn| and |z2 - zf| where a hit's range is clipped against the camera's (only with zn, zf given).
A ray with a margin below UNDECIDED = 1e-4 is "undecided in fp32"; a direction with a NaN or an infinite component misses whatever the
rounding (margin inf)."""
import math

import torch

F64 = torch.float64
UNDECIDED = 1e-4
OFFSET, TINY, EPS = 0.01, 1e-5, 1e-6
U32 = 2.0 ** -24  # unit round-off of fp32


def _f64(x):
    return torch.as_tensor(x).to(F64)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------------------
def rays(K, RT, znear, zfar, px):
    """K (3,3), RT (3,4) world -> camera, px (R,2) integer pixels -> d (R,3) unit, o (3,), zn, zf (R,)."""
    K, RT = _f64(K)[:3, :3], _f64(RT)[:3, :4]
    gh = torch.cat([_f64(px), torch.ones(px.shape[0], 1, dtype=F64)], 1)
    c = torch.linalg.solve(K, gh.T).T  # K c = (x, y, 1)
    n = c.norm(dim=1)
    Rm, t = RT[:, :3], RT[:, 3]
    d = c @ Rm  # R^T c
    return d / d.norm(dim=1, keepdim=True).clamp_min(1e-12), -(Rm.T @ t), float(znear) * n, float(zfar) * n


def _offset_box(bounds):
    b = _f64(bounds).reshape(2, 3)
    return b[0] - OFFSET, b[1] + OFFSET


def _plane_points(bounds, o, d):
    """The six plane points of the reference's rule: p (R,6,3), planes in the order min_x, min_y, min_z, max_x, max_y, max_z."""
    lo, hi = _offset_box(bounds)
    o, d = _f64(o).reshape(1, 3), _f64(d).clone()
    d[d.abs() < TINY] = TINY
    planes = torch.cat([lo, hi])  # (6,)
    axis = torch.arange(6) % 3
    t = (planes[None] - o[:, axis]) / d[:, axis]  # (R,6)
    return lo, hi, o, d, planes, axis, t[..., None] * d[:, None] + o[:, None]


def box_clip(bounds, o, d):
    """bounds (2,3), o (3,), d (R,3) -> hit (R,) bool, near, far (R,) (1.0 where there is no hit)."""
    lo, hi, o, d, _, _, p = _plane_points(bounds, o, d)
    inside = ((p >= lo - EPS) & (p <= hi + EPS)).all(-1)  # (R,6)
    hit = inside.sum(1) == 2
    dist = (p - o[:, None]).norm(dim=2) / d.norm(dim=1, keepdim=True)
    big = torch.where(inside, dist, torch.full_like(dist, math.inf))
    small = torch.where(inside, dist, torch.full_like(dist, -math.inf))
    one = torch.ones(d.shape[0], dtype=F64)
    return hit, torch.where(hit, big.min(1)[0], one), torch.where(hit, small.max(1)[0], one)


def slab(bounds, o, d):
    """The line o + t d against the offset box, slab by slab, with the direction as given (no 1e-5 rule) -> hit, t_in, t_out (R,)."""
    lo, hi = _offset_box(bounds)
    o, d = _f64(o).reshape(1, 3).expand(d.shape[0], 3), _f64(d)
    par = d == 0
    safe = torch.where(par, torch.ones_like(d), d)
    t1, t2 = (lo - o) / safe, (hi - o) / safe
    within = (o >= lo) & (o <= hi)
    t_in = torch.where(par, torch.where(within, -math.inf, math.inf), torch.minimum(t1, t2)).max(1)[0]
    t_out = torch.where(par, torch.where(within, math.inf, -math.inf), torch.maximum(t1, t2)).min(1)[0]
    return t_in <= t_out, t_in, t_out


def decision_margin(bounds, o, d, zn=None, zf=None):
    """(R,) the smallest distance of a ray from a decision (module docstring)."""
    d_in = _f64(d)
    lo, hi, o, d, planes, axis, p = _plane_points(bounds, o, d_in)
    m = ((d_in.abs() - TINY).abs() / TINY).min(1)[0]
    across = torch.arange(3)[None] != axis[:, None]  # (6,3): the comparisons of a plane's point on the two other axes
    gap = torch.minimum((p - (lo - EPS)).abs(), (p - (hi + EPS)).abs())  # (R,6,3)
    m = torch.minimum(m, torch.where(across[None], gap, torch.full_like(gap, math.inf)).flatten(1).min(1)[0])
    rounding = U32 * (3.0 * (planes[None] - o[:, axis]).abs() + planes.abs()[None])  # (R,6): of the point's coordinate along the normal
    m = torch.where((rounding >= EPS).any(1), torch.zeros_like(m), m)
    if zn is not None:
        hit, z1, z2 = box_clip(bounds, o[0], d_in)
        far_off = torch.full_like(m, math.inf)
        m = torch.minimum(m, torch.where(hit, torch.minimum((z1 - _f64(zn)).abs(), (z2 - _f64(zf)).abs()), far_off))
    return torch.where(torch.isfinite(d_in).all(1), m, torch.full_like(m, math.inf))


def depths(near, far, S, jitter=None):
    """near, far (R,) -> z (R,S): near + (far - near) t with t = i / (S - 1), or drawn in the stratum about it (jitter (R,S) in [0, 1))."""
    t = torch.arange(S, dtype=F64) / max(S - 1, 1)
    if jitter is not None:
        mid = 0.5 * (t[1:] + t[:-1])
        lower, upper = torch.cat([t[:1], mid]), torch.cat([mid, t[-1:]])
        t = lower[None] + _f64(jitter) * (upper - lower)[None]
    else:
        t = t[None]
    near, far = _f64(near)[:, None], _f64(far)[:, None]
    return near + (far - near) * t


def clip_to_camera(hit, z1, z2, zn, zf):
    """src/model.py:1217-1220: the box's range where it is inside the camera's, else the camera's."""
    return torch.where(hit & (z1 > zn), z1, zn), torch.where(hit & (z2 < zf), z2, zf)


def pixel_rows(x0, y0, step, y_step, y_block, row_blocks, nx, ny):
    """(nx*ny, 2) int64 pixels, row-major: x = x0 + ix*step; rows come in blocks of y_block rows `step` apart, block b starting at
    row_blocks[b] if given, else at y0 + b*y_step."""
    iy = torch.arange(ny, dtype=torch.int64)
    y_step = step if y_step is None else y_step
    first = torch.as_tensor(row_blocks, dtype=torch.int64)[iy // y_block] if row_blocks is not None else y0 + (iy // y_block) * y_step
    y = first + (iy % y_block) * step
    x = x0 + torch.arange(nx, dtype=torch.int64) * step
    return torch.stack([x[None].expand(ny, nx), y[:, None].expand(ny, nx)], -1).reshape(-1, 2)


def pixel_index(px, width):
    return px[:, 0].to(torch.int64) + px[:, 1].to(torch.int64) * int(width)


# ------------------------------------------------------------------------------------------------------------------------------------------
# inputs of the box clip: family(name, bounds, R) -> origin (3,) fp32, directions (R,3) fp32
# ------------------------------------------------------------------------------------------------------------------------------------------
BBOX_R = (1, 255, 257, 4099)  # one ray, one short of a block, one past it, many blocks with a partial last one
TINY_VALUES = (0.0, -0.0, 1e-6, -1e-6, 0.99e-5, -0.99e-5, 1.01e-5, -1.01e-5)
# exactly at an edge or corner and 1e-7 .. 1e-3 beside it: two steps that fp32 decides for every one that it may not, in turn, so that a
# short set holds both kinds
_SMALL = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4)
_LARGE = tuple(s * v * 1e-4 for v in (10.0, 9.5, 9.0, 8.5, 8.0, 7.5, 7.0, 6.5, 6.0) for s in (1.0, -1.0))
BESIDE = tuple(v for k, small in enumerate(_SMALL) for v in (_LARGE[2 * k], _LARGE[2 * k + 1], small))
# name -> the most undecided rays it may hold: the deliberately degenerate families are sets of their own
FAMILIES = {"outside": 0.05, "inside": 0.05, "on_face": 0.05, "on_offset_face": 0.05, "miss": 0.05, "not_unit": 0.05, "not_finite": 0.05,
            "tiny_one": 0.5, "tiny_two": 0.5, "edges_corners": 0.5}


def _box32(bounds):
    """The offset box as the fp32 rule computes it."""
    b = torch.as_tensor(bounds, dtype=torch.float32).reshape(2, 3)
    return (b[0] - torch.tensor(0.01)).to(F64), (b[1] + torch.tensor(0.01)).to(F64)


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def _sphere(n, g):
    return _unit(torch.randn(n, 3, generator=g, dtype=F64))


def _in_box(n, lo, hi, g, shrink=0.9):
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo) * shrink
    return c + (2.0 * torch.rand(n, 3, generator=g, dtype=F64) - 1.0) * h


def _edge_corner_targets(lo, hi, g):
    """(20,3) points on the 12 edges (off their middles) and the 8 corners of the box, and two unit vectors (20,2,3) to step beside them along."""
    pts, nrm = [], []
    ends = (lo, hi)
    eye = torch.eye(3, dtype=F64)
    for a in range(3):  # the edges along axis a
        b, c = (a + 1) % 3, (a + 2) % 3
        for sb in (0, 1):
            for sc in (0, 1):
                p = torch.zeros(3, dtype=F64)
                p[a] = lo[a] + (hi[a] - lo[a]) * (0.2 + 0.6 * torch.rand((), generator=g, dtype=F64))
                p[b], p[c] = ends[sb][b], ends[sc][c]
                pts.append(p)
                nrm.append(torch.stack([eye[b], eye[c]]))
    for sx in (0, 1):
        for sy in (0, 1):
            for sz in (0, 1):
                pts.append(torch.stack([ends[sx][0], ends[sy][1], ends[sz][2]]))
                out = torch.tensor([2.0 * sx - 1.0, 2.0 * sy - 1.0, 2.0 * sz - 1.0], dtype=F64)  # beside a corner: along two of its diagonals
                nrm.append(torch.stack([out, out * torch.tensor([1.0, 1.0, -1.0], dtype=F64)]) / math.sqrt(3.0))
    return torch.stack(pts), torch.stack(nrm)


def family(name, bounds, R, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + sorted(FAMILIES).index(name))
    lo, hi = _box32(bounds)
    centre, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    outside = centre + torch.tensor([0.55, -0.35, -0.9], dtype=F64)
    o = outside
    aimed = lambda n, src: _unit(_in_box(n, lo, hi, g) - src)
    if name == "outside":  # half aimed at the box, half anywhere (lines through the box behind the origin count as hits)
        d = torch.cat([aimed(R - R // 2, o), _sphere(R // 2, g)])
    elif name == "inside":
        o = _in_box(1, lo, hi, g, 0.8)[0]
        d = _sphere(R, g)
    elif name in ("on_face", "on_offset_face"):  # exactly on a face plane of the bounds / of the offset box, the other two coordinates inside
        o = _in_box(1, lo, hi, g, 0.8)[0]
        b32 = torch.as_tensor(bounds, dtype=torch.float32).reshape(2, 3).to(F64)
        o[0] = b32[0, 0] if name == "on_face" else lo[0]
        d = _sphere(R, g)
    elif name in ("tiny_one", "tiny_two"):  # seen from below the box along z, so that a ray with tiny x / y still goes through it
        o = centre + torch.tensor([0.3 * half[0], -0.2 * half[1], -0.8], dtype=F64)
        d = aimed(R, o)
        k = torch.arange(R)
        tiny = torch.tensor(TINY_VALUES, dtype=F64)
        if name == "tiny_one":
            d[k, k % 2] = tiny[(k // 2) % len(tiny)]
        else:
            d[:, 0] = tiny[k % len(tiny)]
            d[:, 1] = tiny[(k // len(tiny)) % len(tiny)]
    elif name == "edges_corners":
        tgt, nrm = _edge_corner_targets(lo, hi, g)
        k = torch.arange(R)
        which, side, beside = k % 20, (k // 20) % 2, torch.tensor(BESIDE, dtype=F64)[(k // 40) % len(BESIDE)]
        d = _unit(tgt[which] + beside[:, None] * nrm[which, side] - o)
    elif name == "miss":  # aimed at a shell about the box, two to three half-diagonals out, across the line of sight
        u = _sphere(R, g)
        to_box = _unit(centre - o)
        u = _unit(u - (u @ to_box)[:, None] * to_box)
        d = _unit(centre + u * half.norm() * (2.0 + torch.rand(R, 1, generator=g, dtype=F64)) - o)
    elif name == "not_unit":  # lengths from 0.01 to 100, as a training caller may pass them
        d = torch.cat([aimed(R - R // 3, o), _sphere(R // 3, g)]) * 10.0 ** (4.0 * torch.rand(R, 1, generator=g, dtype=F64) - 2.0)
    elif name == "not_finite":
        d = aimed(R, o)
        k = torch.arange(R)
        bad = torch.tensor([math.nan, math.inf, -math.inf], dtype=F64)
        d[k, k % 3] = bad[(k // 3) % 3]
        two = (k // 9) % 2 == 1
        d[two, (k[two] + 1) % 3] = bad[(k[two] // 18) % 3]
    else:
        raise KeyError(name)
    return o.to(torch.float32), d.to(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------------------
# cameras and grids of the ray set-up
# ------------------------------------------------------------------------------------------------------------------------------------------
WIDTH, HEIGHT = 800, 600  # of every camera below (the views of one launch share them)


def _rotation(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=F64)
    Rx = torch.tensor([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], dtype=F64)
    Rz = torch.tensor([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]], dtype=F64)
    return Rz @ Rx @ Ry


def _camera(fx, fy, skew, cx, cy, Rm, eye, znear, zfar):
    K = torch.eye(4, dtype=F64)
    K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2] = fx, skew, cx, fy, cy
    E = torch.eye(4, dtype=F64)
    E[:3, :3], E[:3, 3] = Rm, -(Rm @ eye)
    K, E = K.float(), E.float()
    return {"K": K[None], "RT": E[None], "KRT": (K @ E)[None], "width": WIDTH, "height": HEIGHT, "nml_scale": 100.0, "znear": znear, "zfar": zfar}


def _pixel_direction(fx, fy, skew, cx, cy, Rm, x, y):
    """World direction of pixel (x, y) for a camera with this K and rotation."""
    c = torch.tensor([((x - cx) - skew * (y - cy) / fy) / fx, (y - cy) / fy, 1.0], dtype=F64)
    return _unit(Rm.T @ c)


CAMERAS = ("inside", "away", "axis", "long_lens", "corner")  # (a) .. (e)
AXIS_PIXEL = (7, 5)  # camera "axis": the pixel whose ray is (0, 0, 1) exactly


def camera(name, bounds):
    """The cameras (a)-(e): K with unequal focal lengths, an off-centre principal point and skew, RT from a rotation with roll ("axis" has
    neither skew nor rotation, that is its point).  Every grid of GRIDS starts near pixel (0, 0), so the cameras are placed by that corner."""
    lo, hi = _box32(bounds)
    centre = 0.5 * (lo + hi)
    if name == "inside":  # (a)
        k = (310.0, 295.0, 1.5, 21.5, 13.25)
        Rm = _rotation(0.4, -0.3, 0.7)
        eye = centre + 0.3 * (hi - lo) * torch.tensor([0.5, -0.6, 0.4], dtype=F64)
        return _camera(*k, Rm, eye, 0.02, 1.42)
    if name == "away":  # (b) the box lies along the camera's x axis, far outside a narrow field of view: no LINE of a pixel meets it
        k = (900.0, 880.0, 2.0, 30.5, 20.25)
        Rm = _rotation(-0.5, 0.2, 1.1)
        eye = centre - 1.2 * Rm.T[:, 0]
        return _camera(*k, Rm, eye, 0.71, 1.42)
    if name == "axis":  # (c) powers of two: K's inverse, and with it the ray of AXIS_PIXEL, is exact
        k = (64.0, 128.0, 0.0, float(AXIS_PIXEL[0]), float(AXIS_PIXEL[1]))
        eye = centre - torch.tensor([0.0, 0.0, 1.0], dtype=F64)
        return _camera(*k, torch.eye(3, dtype=F64), eye, 0.71, 1.42)
    if name == "long_lens":  # (d) focal 1500, the principal point thousands of pixels outside the image
        k = (1500.0, 1480.0, 2.0, 5000.0, -3000.0)
        Rm = _rotation(0.9, 0.5, -0.6)
        eye = centre - 1.2 * _pixel_direction(*k, Rm, 12.0, 9.0)
        return _camera(*k, Rm, eye, 0.1, 1.0)
    if name == "corner":  # (e) the box about pixel (0, 0) and some 12 pixels wide: a block of 256 rays holds hits and misses
        k = (60.0, 55.0, 0.8, 40.5, 33.25)
        Rm = _rotation(-0.7, 0.35, 0.4)
        eye = centre - 1.2 * _pixel_direction(*k, Rm, 2.0, 3.0)
        return _camera(*k, Rm, eye, 0.71, 1.42)
    raise KeyError(name)


# name -> x0, y0, step, y_step, y_block, row_blocks, nx, ny, S, jitter: rays per launch 1, 255, 257 and 3*256+1; steps 1 and 3 with offsets;
# blocks of 8 rows (regular and listed in no order); S = 2, 3 and 64 with and without jitter (S = 1 is refused by the entry)
GRIDS = {
    "one_ray": (5, 7, 1, None, 1, None, 1, 1, 2, True),
    "r255_step3": (1, 2, 3, None, 1, None, 15, 17, 3, True),
    "r257_row": (0, 3, 1, None, 1, None, 257, 1, 64, False),
    "r769": (2, 0, 3, None, 1, None, 769, 1, 2, False),
    "r769_s3": (0, 1, 1, None, 1, None, 769, 1, 3, True),
    "y_blocks": (3, 1, 3, 40, 8, None, 11, 24, 3, False),
    "row_list": (0, 0, 1, None, 8, (50, 10, 30), 11, 24, 64, True),
    "s64_jitter": (0, 0, 3, None, 1, None, 5, 4, 64, True),
}
VIEW_GRIDS = ("one_ray", "r255_step3", "r257_row", "r769", "r769_s3", "s64_jitter")  # the camera-table form takes the plain grid only


def jitter_rows(R, S, seed):
    """(R,S) fp32 draws in [0, 1): the first row exactly 0, the second (if any) the largest float below 1, the third alternating the two."""
    j = torch.rand(R, S, generator=torch.Generator().manual_seed(seed))
    top = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    j[0] = 0.0
    if R > 1:
        j[1] = top
    if R > 2:
        j[2, 0::2], j[2, 1::2] = top, 0.0
    return j.clamp_(0.0, top)


def pixel_list(R, seed):
    """(R,2) int32 pixels of a training patch in no order, a quarter of them listed twice."""
    g = torch.Generator().manual_seed(seed)
    px = torch.stack([torch.randint(0, 40, (R,), generator=g), torch.randint(0, 30, (R,), generator=g)], 1)
    px[R // 2: R // 2 + R // 4] = px[: R // 4]
    return px[torch.randperm(R, generator=g)].to(torch.int32).contiguous()
