"""Keeps tests/ray_geometry_ref.py and the inputs of tests/test_ray_geometry.py honest without a GPU: the fp64 statement of the box clip
against the fp32 CPU oracle on every input family, the slab test as a second opinion, the caps on how many rays a family may leave
undecided, and the cameras and grids against the oracle's ray generation.

Bars: the project's own (tests/test_hip_parity.py::test_ray_setup): 1e-6 on rays_d and cam_pos, 2e-6 * max(1, |want|) on near / far / z.
Every test prints what the fp32 oracle reaches against the fp64 statement before it asserts (pytest -s shows it)."""
import pytest
import torch

from oracle import vanerf_oracle as orc
from tests import ray_geometry_ref as ref
from vanerf_amd import synth

BAR_D, BAR_Z = 1e-6, 2e-6


@pytest.fixture(scope="module")
def bounds():
    return synth.make_frame(seed=3, tar_h=64, tar_w=64)["bounds"]  # (1,2,3)


def _oracle_clip(bounds, o, d):
    near, far, hit = orc.ray_bbox_intersection(bounds, o[None, None], d[None])
    return hit[0, :, 0], near[0, :, 0], far[0, :, 0]


def _scaled(got, want):
    return ((got.double() - want).abs() / want.abs().clamp_min(1.0))


@pytest.mark.parametrize("R", ref.BBOX_R)
@pytest.mark.parametrize("name", sorted(ref.FAMILIES))
def test_box_clip_against_the_oracle(bounds, name, R):
    o, d = ref.family(name, bounds[0], R)
    assert d.shape == (R, 3) and d.dtype == torch.float32
    hit32, near32, far32 = _oracle_clip(bounds, o, d)
    hit, near, far = ref.box_clip(bounds[0], o, d)
    decided = ref.decision_margin(bounds[0], o, d) >= ref.UNDECIDED
    assert torch.equal(hit32[decided], hit[decided])
    both = decided & hit
    worst = max(_scaled(near32, near)[both].max().item(), _scaled(far32, far)[both].max().item()) if both.any() else 0.0
    print(f"{name} R={R}: hits {int(hit.sum())}, undecided {int((~decided).sum())}, fp32 oracle near/far off by {worst:.2e} (bar {BAR_Z:.0e})")
    assert worst <= BAR_Z
    assert (near32[~hit32] == 1.0).all() and (far32[~hit32] == 1.0).all() and (near[~hit] == 1.0).all() and (far[~hit] == 1.0).all()
    if name == "miss":
        assert not hit.any()
    if name == "not_finite":
        assert not hit.any() and not hit32.any() and not torch.isfinite(d).all(1).any()


@pytest.mark.parametrize("name", sorted(ref.FAMILIES))
def test_undecided_rays_are_capped(bounds, name):
    """An input set that hides its own cases fails here: at most 5 % of a set's rays, 50 % of a deliberately degenerate set's, may be left out
    of the fp64 comparison (a single ray is not a fraction: the sets of 255 rays and more)."""
    for R in ref.BBOX_R[1:]:
        o, d = ref.family(name, bounds[0], R)
        undecided = (ref.decision_margin(bounds[0], o, d) < ref.UNDECIDED).float().mean().item()
        print(f"{name} R={R}: {100 * undecided:.1f} % undecided (cap {100 * ref.FAMILIES[name]:.0f} %)")
        assert undecided <= ref.FAMILIES[name]
    if ref.FAMILIES[name] > 0.05:  # a degenerate set is degenerate: it does hold rays that fp32 may decide either way, or tiny components
        o, d = ref.family(name, bounds[0], ref.BBOX_R[-1])
        assert (ref.decision_margin(bounds[0], o, d) < ref.UNDECIDED).any() or (d.abs() < 1.1e-5).any()


@pytest.mark.parametrize("name", sorted(ref.FAMILIES))
def test_slab_second_opinion(bounds, name):
    o, d = ref.family(name, bounds[0], ref.BBOX_R[-1])
    hit, near, far = ref.box_clip(bounds[0], o, d)
    decided = ref.decision_margin(bounds[0], o, d) >= ref.UNDECIDED
    s_hit, t_in, t_out = ref.slab(bounds[0], o, d)
    lo, hi = ref._offset_box(bounds[0])
    within = name in ("inside", "on_face", "on_offset_face")
    assert within == bool(((o.double() > lo - 1e-6) & (o.double() < hi + 1e-6)).all())
    if not within:
        assert torch.equal(s_hit[decided], hit[decided])
        return
    if name == "on_offset_face":  # the origin is on the box's own face: a line along it is the slab test's own edge case
        decided &= d[:, 0].abs() > 1e-3
    # An origin inside the box: every line leaves it once ahead and once behind, so the rule finds exactly two points and reports |p - o| of
    # both, the one behind the origin included: near is the smaller of the two distances whichever side it lies on.
    assert hit[decided].all() and s_hit[decided].all() and (t_in[decided] <= 0).all() and (t_out[decided] >= 0).all()
    length = d.double().norm(dim=1)  # t counts in units of |d|; the 1e-5 rule moves no direction of these sets by more than 2e-5
    behind, ahead = -t_in * length, t_out * length
    assert (near - torch.minimum(behind, ahead)).abs()[decided].max() <= 1e-4 and (far - torch.maximum(behind, ahead)).abs()[decided].max() <= 1e-4
    closer_behind = decided & (behind < ahead - 1e-3)
    assert closer_behind.sum() > 100  # near = the distance to the plane BEHIND the origin on all of these
    assert (near - behind).abs()[closer_behind].max() <= 1e-4


def test_axis_camera_has_an_exact_axis_ray(bounds):
    cam = ref.camera("axis", bounds[0])
    px = torch.tensor([list(ref.AXIS_PIXEL)])
    d32 = orc.generate_rays(px[None], cam, bounds, cam["znear"], cam["zfar"])[0]
    assert torch.equal(d32[0, 0], torch.tensor([0.0, 0.0, 1.0]))  # two exactly-zero components: both take the 1e-5 rule
    assert torch.equal(ref.rays(cam["K"][0], cam["RT"][0], cam["znear"], cam["zfar"], px)[0][0], torch.tensor([0.0, 0.0, 1.0], dtype=ref.F64))
    assert list(ref.AXIS_PIXEL) in ref.pixel_rows(*ref.GRIDS["r255_step3"][:8]).tolist()  # a launch of the GPU test holds this ray


@pytest.mark.parametrize("grid", sorted(ref.GRIDS))
@pytest.mark.parametrize("name", ref.CAMERAS)
def test_cameras_and_grids_against_the_oracle(bounds, name, grid):
    cam = ref.camera(name, bounds[0])
    x0, y0, step, y_step, y_block, row_blocks, nx, ny, S, jittered = ref.GRIDS[grid]
    px = ref.pixel_rows(x0, y0, step, y_step or step, y_block, row_blocks, nx, ny)
    R = nx * ny
    assert px.shape == (R, 2) and (px >= 0).all()
    d32, o32, near32, far32, hit32 = orc.generate_rays(px[None], cam, bounds, cam["znear"], cam["zfar"])
    d32, o32, near32, far32, hit32 = d32[0], o32[0, 0], near32[0, :, 0], far32[0, :, 0], hit32[0, :, 0]
    d, o, zn, zf = ref.rays(cam["K"][0], cam["RT"][0], cam["znear"], cam["zfar"], px)
    assert (d32.double() - d).abs().max() <= BAR_D and (o32.double() - o).abs().max() <= BAR_D
    hit, z1, z2 = ref.box_clip(bounds[0], o, d)
    decided = ref.decision_margin(bounds[0], o, d, zn, zf) >= ref.UNDECIDED
    assert (~decided).float().mean() <= 0.05
    assert torch.equal(hit32[decided], hit[decided])
    # near / far of the fp32 rays: the clip of a grazing ray magnifies the direction's last bit by 1 / |d_a|, so the clip is held to the fp64
    # clip of the SAME fp32 rays (the rays themselves are held to fp64 above)
    hit_s, z1_s, z2_s = ref.box_clip(bounds[0], o32, d32)
    near, far = ref.clip_to_camera(hit_s, z1_s, z2_s, zn, zf)
    worst = max(_scaled(near32, near)[decided].max().item(), _scaled(far32, far)[decided].max().item()) if decided.any() else 0.0
    jitter = ref.jitter_rows(R, S, 5) if jittered else None
    t32 = orc.stratified(S, jitter[None])[0] if jittered else torch.linspace(0.0, 1.0, S)[None]
    z32 = near32[:, None] + (far32 - near32)[:, None] * t32
    worst_z = _scaled(z32, ref.depths(near32, far32, S, jitter)).max().item()
    print(f"{name} {grid}: hits {int(hit.sum())}/{R}, undecided {int((~decided).sum())}, fp32 oracle near/far off by {worst:.2e}, z by {worst_z:.2e} (bar {BAR_Z:.0e})")
    assert worst <= BAR_Z and worst_z <= BAR_Z
    if name == "inside":
        lo, hi = ref._offset_box(bounds[0])
        assert ((o > lo) & (o < hi)).all() and hit[decided].all()
    if name == "away":
        assert not hit.any() and not hit32.any()  # near / far are the camera's own range (held to zn, zf above)
    if name == "corner" and R >= 255:
        assert 0 < int(hit[:256].sum()) < min(R, 256)  # the first block holds both


def test_the_cameras_reach_what_they_are_for(bounds):
    lens = ref.camera("long_lens", bounds[0])["K"][0]
    assert lens[0, 0] == 1500.0 and lens[0, 2] > 4 * ref.WIDTH and lens[1, 2] < -4 * ref.HEIGHT
    for name in ref.CAMERAS:
        K = ref.camera(name, bounds[0])["K"][0]
        assert K[0, 0] != K[1, 1] and K[0, 2] != ref.WIDTH / 2 and K[1, 2] != ref.HEIGHT / 2 and (name == "axis" or K[0, 1] != 0)
    sizes = sorted({g[6] * g[7] for g in ref.GRIDS.values()})
    assert {1, 255, 257, 3 * 256 + 1} <= set(sizes) and {g[2] for g in ref.GRIDS.values()} == {1, 3}
    assert {g[8] for g in ref.GRIDS.values()} == {2, 3, 64} and {(g[8], g[9]) for g in ref.GRIDS.values()} >= {(2, True), (3, True), (64, True), (64, False)}


def test_depths_and_pixel_rows():
    near, far = torch.tensor([0.5, 2.0, 1.0]), torch.tensor([1.5, 1.0, 1.0])
    for S in (1, 2, 3, 64):
        want = near[:, None] + (far - near)[:, None] * torch.linspace(0.0, 1.0, S)[None]
        assert (ref.depths(near, far, S) - want.double()).abs().max() <= 2e-7
        jitter = ref.jitter_rows(3, S, 9)
        assert (jitter[0] == 0).all() and (jitter[1] < 1).all() and (jitter[1] == jitter.max()).all() and jitter.max() == 1.0 - 2.0 ** -24
        want = near[:, None] + (far - near)[:, None] * orc.stratified(S, jitter[None])[0]
        got = ref.depths(near, far, S, jitter)
        assert (got - want.double()).abs().max() <= 3e-7
        assert (got[0, 1:] >= got[0, :-1]).all() and got[0, 0] == 0.5 and (got[1, 1:] <= got[1, :-1]).all() and (got[2] == 1.0).all()
    grids, index = orc.pixel_grid(40, 24, 3, torch.tensor([[[3, 1]]]))  # the oracle's evaluation grid: step 4 from (3, 1)
    px = ref.pixel_rows(3, 1, 4, 4, 1, None, 10, 6)
    assert torch.equal(px, grids[0]) and torch.equal(ref.pixel_index(px, 40), index[0])
    # blocks of 2 rows 3 apart, the blocks 10 apart or listed
    assert ref.pixel_rows(0, 5, 3, 10, 2, None, 1, 6)[:, 1].tolist() == [5, 8, 15, 18, 25, 28]
    assert ref.pixel_rows(0, 5, 3, 10, 2, (40, 7, 20), 2, 6)[:, 1].tolist() == [40, 40, 43, 43, 7, 7, 10, 10, 20, 20, 23, 23]
    assert ref.pixel_index(torch.tensor([[65535, 40000]]), 65536).item() == 65535 + 40000 * 65536 > 2 ** 31
