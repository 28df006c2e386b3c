"""Ray generation, the box clip, the coarse depths and the sample positions (ray_setup_kernel, ray_setup_views_kernel, ray_bbox_kernel,
sample_points_kernel of csrc/render_kernels.hip) against the fp64 statement of tests/ray_geometry_ref.py and against the fp32 CPU oracle, on
edge cameras, rays and grids.  tests/test_ray_geometry_cpu.py holds the same inputs and the fp64 statement itself to the oracle without a GPU.

Bars: the project's own (test_hip_parity.py::test_ray_setup): 1e-6 on rays_d and cam_pos, 2e-6 * max(1, |want|) on near / far / z.  None had
to be widened: on these inputs the fp32 CPU oracle stays within 1.5e-6 (box clip, the family on_offset_face; every other family within
2.6e-7), 1.4e-7 (rays_d), 9.2e-8 (cam_pos), 3.2e-7 (near / far of the cameras) and 1.3e-7 (z) of the fp64 statement (the CPU file prints them).
Two things about how the fp64 values are used:
  * near / far of ray_setup are held to the fp64 clip of the rays_d and cam_pos that the kernel wrote (which are held to fp64 themselves): the
    distance to a plane that a ray grazes magnifies the last bit of its direction by 1 / |d_a| (4.6e-6 for the fp32 oracle on a ray of camera
    "corner" with d_y = 0.007), which says nothing about the clip.  z is likewise held to the depths of the near / far that the kernel wrote.
  * near <= z holds exactly (rounding is monotone and t >= 0); z <= far holds up to the one rounding of near + (far - near) * 1, which the
    reference's own fp32 formula exceeds on 26 of 200 140 samples of these launches: 2^-24 (|far - near| + |far|).
A ray is left out of an fp64 comparison only where ray_geometry_ref.decision_margin calls it undecided in fp32; no ray is left out of a
comparison with the oracle.  S = 1 is refused by the entry (test_multi_view_pass.py holds it to that), so S = 1 asserts the refusal.

Every launch of the set-up writes into buffers that go on past its rays (256 more, filled with a pattern that must survive), and reads its
jitter from one, so a block that handles rays it does not have is seen and stays inside memory that the test owns.

Mutation record: scratch builds of render_kernels.hip with one line changed, run against this file and against the suite as it was.
  1. `d[a] < 1e-5f` for `fabsf(d[a]) < 1e-5f` (every negative component becomes +1e-5)
  2. `cnt >= 2` for `cnt == 2`
  3. `if (r > R) return;` for `if (r >= R) return;` in ray_bbox_kernel
  4. `nr = blockDim.x` in the z loop of ray_setup_block
Each went red here; none of the scratch code is kept.
  1. red: test_ray_bbox (7 of the 10 families), test_ray_bbox_writes_only_its_rays[255, 257, 4099], test_ray_setup[inside, axis, long_lens],
     test_ray_setup_views (all six grids).  The suite as it was also went red (170 tests, from test_multi_view_pass to the posed marches): a
     negative component is no edge case.
  2. red: test_ray_bbox[edges_corners] (from 255 rays on) and test_ray_bbox[on_face] (ray 1245 of 4099), both in the comparison with the oracle
     that leaves no ray out; every fp64 comparison stayed green, as three and more plane points happen only on rays that fp32 may decide either
     way.  Of the suite as it was, test_hip_parity.py::test_ray_setup went red (hit against the oracle on its 171 k rays), nothing else.
  3. red: test_ray_bbox_writes_only_its_rays at all four R.  The suite as it was hands the entry buffers of exactly R rays and looks at nothing
     behind them, so it cannot see the stray ray; it was not run on this build, which writes past those buffers.
  4. red: test_ray_setup (all five cameras) and test_ray_setup_views (every grid that was run), "z: written past the launch's rays".  Run on
     the launches of _launch only; the suite as it was owns no memory behind z and was not run on this build for the same reason."""
import ctypes

import pytest
import torch

from oracle import vanerf_oracle as orc
from tests import ray_geometry_ref as ref
from vanerf_amd import synth

pytestmark = pytest.mark.gpu

BAR_D, BAR_Z = 1e-6, 2e-6
PAD = 256  # rays past the end of every buffer of a set-up launch
MARK_F, MARK_I, MARK_B = -7.25, -77, 0xAB


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def bounds():
    return synth.make_frame(seed=3, tar_h=64, tar_w=64)["bounds"]  # (1,2,3), on the host


def _scaled(got, want):
    return (got.double() - want).abs() / want.abs().clamp_min(1.0)


def _oracle_clip(bounds, o, d):
    near, far, hit = orc.ray_bbox_intersection(bounds, o.reshape(1, 1, 3), d[None])
    return hit[0, :, 0], near[0, :, 0], far[0, :, 0]


# ------------------------------------------------------------------------------------------------------------------------------------------
# vanerf_ray_bbox
# ------------------------------------------------------------------------------------------------------------------------------------------
def _check_clip(bounds, o, d, hit_g, near_g, far_g, what):
    """The clip of fp32 rays (o, d) as the kernel returned it: against the oracle on every ray, against fp64 on every decided one."""
    hit_g = hit_g.bool()
    hit32, near32, far32 = _oracle_clip(bounds, o, d)
    assert torch.equal(hit_g, hit32), f"{what}: hit differs from the oracle on rays {torch.nonzero(hit_g != hit32)[:8, 0].tolist()}"
    assert (near_g[~hit_g] == 1.0).all() and (far_g[~hit_g] == 1.0).all(), what
    if hit32.any():
        assert _scaled(near_g, near32.double())[hit32].max() <= BAR_Z and _scaled(far_g, far32.double())[hit32].max() <= BAR_Z, what
    hit, near, far = ref.box_clip(bounds[0], o, d)
    decided = ref.decision_margin(bounds[0], o, d) >= ref.UNDECIDED
    assert torch.equal(hit_g[decided], hit[decided]), f"{what}: hit differs from fp64 on decided rays"
    both = decided & hit
    if both.any():
        worst = max(_scaled(near_g, near)[both].max().item(), _scaled(far_g, far)[both].max().item())
        print(f"{what}: near / far off fp64 by {worst:.2e}")
        assert worst <= BAR_Z, what


@pytest.mark.parametrize("name", sorted(ref.FAMILIES))
def test_ray_bbox(R, bounds, name):
    for n in ref.BBOX_R:
        o, d = ref.family(name, bounds[0], n)
        near, far, hit = R.ray_bbox(bounds[0], o, d.cuda())
        assert near.shape == far.shape == hit.shape == (n,) and hit.dtype == torch.uint8 and bool((hit <= 1).all())
        _check_clip(bounds, o, d, hit.cpu(), near.cpu(), far.cpu(), f"{name} R={n}")


@pytest.mark.parametrize("n", ref.BBOX_R)
def test_ray_bbox_writes_only_its_rays(R, bounds, n):
    """The entry itself with buffers that go on past R: the directions behind the last ray all hit the box (so a thread that took one would
    write a hit and its distances), the outputs behind it hold a pattern."""
    from vanerf_amd._ffi import lib
    o, d = ref.family("tiny_one", bounds[0], n + 64)  # every ray of this family hits
    d_dev = d.cuda()
    near, far = (torch.full((n + 64,), MARK_F, device="cuda") for _ in range(2))
    hit = torch.full((n + 64,), MARK_B, dtype=torch.uint8, device="cuda")
    rc = lib.vanerf_ray_bbox(R._farr(bounds.reshape(-1).tolist(), 6), R._farr(o.tolist(), 3), R._ptr(d_dev), n, R._ptr(near), R._ptr(far), R._ptr(hit),
                             R._stream())
    assert rc == 0
    near, far, hit = near.cpu(), far.cpu(), hit.cpu()
    assert (near[n:] == MARK_F).all() and (far[n:] == MARK_F).all() and (hit[n:] == MARK_B).all()
    assert (hit[:n] == 1).all()
    _check_clip(bounds, o, d[:n], hit[:n], near[:n], far[:n], f"R={n} of {n + 64}")


# ------------------------------------------------------------------------------------------------------------------------------------------
# vanerf_ray_setup
# ------------------------------------------------------------------------------------------------------------------------------------------
def _launch(R, cams, bounds, grid, S, jitter=None, pixels=None):
    """vanerf_ray_setup into buffers with PAD more rays than the launch has; cams: a camera, or a list of them (the camera-table form).
    grid: x0, y0, step, y_step, y_block, row_blocks, nx, ny.  Returns the outputs on the host, cut to the launch's rays."""
    from vanerf_amd._ffi import lib
    x0, y0, step, y_step, y_block, row_blocks, nx, ny = grid
    views = isinstance(cams, list)
    V, n = (len(cams) if views else 1), nx * ny
    total = V * n
    rows = None if row_blocks is None else torch.tensor(row_blocks, dtype=torch.int32).cuda()
    listed = None if pixels is None else pixels.cuda()  # (held here until the launch has run, as the other inputs are)
    jit = None
    if jitter is not None:
        assert jitter.shape == (total, S)
        jit = torch.cat([jitter, torch.full((PAD, S), 0.5)]).cuda()
    d, keep = R._pass_desc(cams, bounds.cuda(), x0, y0, step, nx, ny, S, "cuda", jitter=None if jit is None else jit[:total], y_step=y_step,
                           pixels=listed, y_block=y_block, row_blocks=rows)
    full = lambda tail, fill, dtype=torch.float32: torch.full((total + PAD, *tail), fill, dtype=dtype, device="cuda")
    out = dict(index=full((), MARK_I, torch.int64), rays_d=full((3,), MARK_F), cam_pos=torch.zeros(V, 4, device="cuda"), near=full((), MARK_F),
               far=full((), MARK_F), hit=full((), MARK_B, torch.uint8), z=full((S,), MARK_F))
    rc = lib.vanerf_ray_setup(ctypes.byref(d), *(R._ptr(t) for t in out.values()), R._stream())
    assert rc == 0, lib.vanerf_last_error()
    out = {k: v.cpu() for k, v in out.items()}
    for k, mark in (("index", MARK_I), ("rays_d", MARK_F), ("near", MARK_F), ("far", MARK_F), ("hit", MARK_B), ("z", MARK_F)):
        assert (out[k][total:] == mark).all(), f"{k}: written past the launch's {total} rays"
        out[k] = out[k][:total]
    assert (out["cam_pos"][:, 3] == 0).all()
    out["cam_pos"] = out["cam_pos"][:, :3]
    return out


def _check_view(bounds, cam, px, S, jitter, got, v, what):
    """View v of a launch (rays v*R .. v*R + R - 1 of its outputs) against the fp64 statement."""
    n = px.shape[0]
    sl = slice(v * n, (v + 1) * n)
    index, d_g, o_g, near_g, far_g, hit_g, z_g = (got["index"][sl], got["rays_d"][sl], got["cam_pos"][v], got["near"][sl], got["far"][sl],
                                                  got["hit"][sl].bool(), got["z"][sl])
    assert torch.equal(index, ref.pixel_index(px, cam["width"])), f"{what}: index"
    d, o, zn, zf = ref.rays(cam["K"][0], cam["RT"][0], cam["znear"], cam["zfar"], px)
    assert (d_g.double() - d).abs().max() <= BAR_D and (o_g.double() - o).abs().max() <= BAR_D, f"{what}: rays_d / cam_pos"
    assert bool((got["hit"][sl] <= 1).all())
    # the clip of the rays that the kernel wrote: the oracle on every one of them, bit for bit
    hit32 = _oracle_clip(bounds, o_g, d_g)[0]
    assert torch.equal(hit_g, hit32), f"{what}: hit differs from the oracle on rays {torch.nonzero(hit_g != hit32)[:8, 0].tolist()}"
    # fp64: the decisions from the fp64 rays, the distances from the fp32 rays (module docstring)
    hit, z1, z2 = ref.box_clip(bounds[0], o, d)
    decided = ref.decision_margin(bounds[0], o, d, zn, zf) >= ref.UNDECIDED
    assert (~decided).float().mean() <= 0.05
    assert torch.equal(hit_g[decided], hit[decided]), f"{what}: hit differs from fp64 on decided rays"
    hit_s, z1_s, z2_s = ref.box_clip(bounds[0], o_g, d_g)
    near, far = ref.clip_to_camera(hit_s, z1_s, z2_s, zn, zf)
    if decided.any():
        worst = max(_scaled(near_g, near)[decided].max().item(), _scaled(far_g, far)[decided].max().item())
        assert worst <= BAR_Z, f"{what}: near / far off fp64 by {worst:.2e}"
    # depths
    z = ref.depths(near_g, far_g, S, jitter)
    worst = _scaled(z_g, z).max().item()
    assert worst <= BAR_Z, f"{what}: z off fp64 by {worst:.2e}"
    ordered = near_g < far_g
    rounding = ref.U32 * ((far_g - near_g).abs() + far_g.abs()).double() * 1.0001
    assert (z_g >= near_g[:, None])[ordered].all() and (z_g.double() <= far_g.double()[:, None] + rounding[:, None])[ordered].all(), f"{what}: z outside near .. far"
    assert (z_g[:, 1:] >= z_g[:, :-1])[ordered].all(), f"{what}: z decreases along a ray"
    return hit_g


def _grids():
    for name, (x0, y0, step, y_step, y_block, row_blocks, nx, ny, S, jittered) in ref.GRIDS.items():
        yield name, (x0, y0, step, y_step, y_block, row_blocks, nx, ny), S, jittered


@pytest.mark.parametrize("name", ref.CAMERAS)
def test_ray_setup(R, bounds, name):
    cam = ref.camera(name, bounds[0])
    hits = rays = 0
    for k, (gname, grid, S, jittered) in enumerate(_grids()):
        n = grid[6] * grid[7]
        px = ref.pixel_rows(*grid)
        jitter = ref.jitter_rows(n, S, 10 + k) if jittered else None
        got = _launch(R, cam, bounds, grid, S, jitter)
        hit = _check_view(bounds, cam, px, S, jitter, got, 0, f"{name} {gname}")
        hits, rays = hits + int(hit.sum()), rays + n
        if name == "axis" and gname == "r255_step3":  # the ray of the principal point: two components are exactly zero and take the 1e-5 rule
            k_axis = px.tolist().index(list(ref.AXIS_PIXEL))
            assert torch.equal(got["rays_d"][k_axis], torch.tensor([0.0, 0.0, 1.0])) and bool(hit[k_axis])
        if name == "corner" and n >= 255:
            assert 0 < int(hit[:256].sum()) < min(n, 256)  # hits and misses in one block
    # a training patch: listed pixels in no order, some of them twice
    for n, S, seed in ((300, 2, 3), (257, 3, 4)):
        pixels = ref.pixel_list(n, seed)
        assert len({tuple(p) for p in pixels.tolist()}) < n
        jitter = ref.jitter_rows(n, S, seed)
        got = _launch(R, cam, bounds, (0, 0, 1, None, 1, None, n, 1), S, jitter, pixels=pixels)
        hit = _check_view(bounds, cam, pixels.long(), S, jitter, got, 0, f"{name} pixel list of {n}")
        hits, rays = hits + int(hit.sum()), rays + n
    if name == "inside":
        assert hits == rays
    if name == "away":
        assert hits == 0  # near / far were the camera's own range on every ray, and z well formed (_check_view)


@pytest.mark.parametrize("gname", ref.VIEW_GRIDS)
def test_ray_setup_views(R, bounds, gname):
    """The cameras (a)-(e) in one launch: every view against its own fp64 values."""
    cams = [ref.camera(name, bounds[0]) for name in ref.CAMERAS]
    x0, y0, step, y_step, y_block, row_blocks, nx, ny, S, jittered = ref.GRIDS[gname]
    grid, n, V = (x0, y0, step, y_step, y_block, row_blocks, nx, ny), nx * ny, len(cams)
    px = ref.pixel_rows(*grid)
    jitter = ref.jitter_rows(V * n, S, 21) if jittered else None
    got = _launch(R, cams, bounds, grid, S, jitter)
    for v, name in enumerate(ref.CAMERAS):
        _check_view(bounds, cams[v], px, S, None if jitter is None else jitter[v * n:(v + 1) * n], got, v, f"view {name} of {gname}")
    if gname != "r255_step3":
        return
    # the public calls give the same bits (they own their buffers: nothing past the end to look at)
    pub = R.ray_setup_views(cams, bounds.cuda(), x0, y0, step, nx, ny, S, jitter=jitter.cuda())
    one = R.ray_setup(cams[3], bounds.cuda(), x0, y0, step, nx, ny, S, jitter=jitter[3 * n:4 * n].cuda())
    for k in ("index", "rays_d", "near", "far", "hit", "z"):
        assert torch.equal(pub[k].cpu().reshape(got[k].shape), got[k]), k
        assert torch.equal(one[k].cpu(), got[k][3 * n:4 * n]), k
    assert torch.equal(pub["cam_pos"].cpu()[:, :3], got["cam_pos"]) and torch.equal(one["cam_pos"].cpu(), got["cam_pos"][3])


def test_one_sample_per_ray_is_refused(R, bounds):
    from vanerf_amd._ffi import VanerfError
    cam = ref.camera("corner", bounds[0])
    with pytest.raises(VanerfError, match=r"-22.*S=1"):
        R.ray_setup(cam, bounds.cuda(), 0, 0, 1, 4, 4, 1, jitter=torch.zeros(16, 1, device="cuda"))
    with pytest.raises(VanerfError, match=r"-22.*S=1"):
        R.ray_setup_views([cam, cam], bounds.cuda(), 0, 0, 1, 4, 4, 1)


def test_pixel_index_past_2_to_31(R, bounds):
    """A camera 65536 pixels wide, pixels of row 40000: x + y * width does not fit 32 bits.  Only the index is looked at, so no image is needed."""
    cam = dict(ref.camera("corner", bounds[0]), width=65536, height=65536)
    pixels = torch.tensor([[5, 40000], [65535, 40000], [0, 32768], [65535, 65535], [7, 3]], dtype=torch.int32)
    got = R.ray_setup(cam, bounds.cuda(), 0, 0, 1, pixels.shape[0], 1, 2, pixels=pixels.cuda())
    want = ref.pixel_index(pixels, 65536)
    assert want.max() == 65535 + 65535 * 65536 and (want[:4] >= 2 ** 31).all()
    assert torch.equal(got["index"].cpu(), want)
    # the regular grid computes its rows itself
    got = R.ray_setup(cam, bounds.cuda(), 65530, 39990, 5, 2, 3, 2)
    assert torch.equal(got["index"].cpu(), ref.pixel_index(ref.pixel_rows(65530, 39990, 5, None, 1, None, 2, 3), 65536))


# ------------------------------------------------------------------------------------------------------------------------------------------
# vanerf_sample_points
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ["r255_step3", "r769_s3"])  # R*S = 5 * 765 and 5 * 2307 samples: no whole number of blocks of 256
def test_sample_points(R, bounds, gname):
    cams = [ref.camera(name, bounds[0]) for name in ref.CAMERAS]
    x0, y0, step, y_step, y_block, row_blocks, nx, ny, S, _ = ref.GRIDS[gname]
    n, V = nx * ny, len(cams)
    assert (V * n * S) % 256 != 0 and (n * S) % 256 != 0
    rays = R.ray_setup_views(cams, bounds.cuda(), x0, y0, step, nx, ny, S, jitter=ref.jitter_rows(V * n, S, 33).cuda())
    d, o, z = rays["rays_d"].cpu(), rays["cam_pos"].cpu(), rays["z"].cpu()
    want32 = (o[:, None, None, :3] + d[:, :, None] * z[..., None]).reshape(V, n * S, 3)  # torch fp32: a mul, then an add
    dz = d.double()[:, :, None] * z.double()[..., None]
    want64 = (o.double()[:, None, None, :3] + dz).reshape(V, n * S, 3)
    bound = (ref.U32 * (dz.abs().reshape(V, n * S, 3) + want64.abs()) * 1.0001 + 1e-30)  # the two roundings of fl(fl(d z) + o)
    # every view's own origin, in one call
    got = R.sample_points(rays["rays_d"].view(-1, 3), rays["cam_pos"], rays["z"].view(-1, S), rays_per_view=n).cpu().view(V, n * S, 3)
    assert torch.equal(got, want32)
    assert ((got.double() - want64).abs() <= bound).all()
    assert len({tuple(row) for row in o[:, :3].tolist()}) == V  # five different origins: a wrong view's would show
    # one origin for every ray
    for v in (0, V - 1):
        got = R.sample_points(rays["rays_d"][v], rays["cam_pos"][v], rays["z"][v]).cpu()
        assert torch.equal(got, want32[v])
        assert ((got.double() - want64[v]).abs() <= bound[v]).all()
