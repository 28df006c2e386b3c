"""The learned field on a grid and the surface extracted from it (vanerf_amd/surface.py) on the synthetic two-hand frame: grid points bit for
bit, the field against the CPU oracle's per-sample query, slab independence, and extract_surface end to end.  Needs a real MI355X.

Grid: 24 x 20 x 16 points over the frame's bounds, frame seed 3, weights seed 0, both precisions of the per-sample kernel."""
import numpy as np
import pytest
import torch

from oracle import vanerf_oracle as orc
from tests.test_surface_march import assert_manifold, edge_use, grid_xyz
from vanerf_amd import synth

pytestmark = pytest.mark.gpu

DIMS = (24, 20, 16)
TOL = 1e-4           # tests/test_hip_parity.py's per-sample bar
N_SUBSET, SUBSET_SEED = 512, 11
MAX_EXCUSED = 5      # 1 % of the 512 points
# Checked on the CPU when this test was written: the oracle against itself at these 512 points moved by +-1e-6 per coordinate (seed 12).
# valid flag: 0 points flip; 1-NN vertex: 0; closest face: 24 -- and 15 to 38 for every other frame seed (5, 7, 9, 11) and subset seed tried.
# Those are ties, not instabilities: about one point in twenty of a box around the hands has its closest point on an edge or a vertex of
# the mesh, where the faces around it are equally near and the last bit picks one; the distance, and f, are the same for each.  So no
# choice of seed brings the perturbed oracle under the cap by that count, and the count says little about this test, which hands both
# sides the SAME points bit for bit (test_grid_points_equal_the_numpy_expression): the mesh query is then bit-exact with the oracle,
# ties included (tests/test_hip_parity.py::test_mesh_query_bit_exact), and the flips expected here are none.  The cap is asserted as set.
# (The same perturbation moves f itself by up to 6e-4: the synthetic network's slope, not a discrete decision.)


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def scene(R):
    """One frame, its device data, the grid and the oracle's field at the subset: computed once, shared, left unchanged."""
    from vanerf_amd import surface
    sd = synth.make_full_weights(0)
    frame = synth.make_frame(seed=3, tar_h=64, tar_w=64)
    fd = synth.to_device(frame, "cuda")
    sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
    fdat = R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
    origin, spacing, dims = surface.grid_spec(frame["bounds"], dims=DIMS)
    pts_np = grid_xyz(origin, spacing, dims).astype(np.float32).reshape(-1, 3)
    sub = np.sort(np.random.default_rng(SUBSET_SEED).choice(len(pts_np), N_SUBSET, replace=False))
    return dict(sd=sd, frame=frame, fdat=fdat, origin=origin, spacing=spacing, dims=dims, pts_np=pts_np, sub=sub, oracle=oracle_field(sd, frame, pts_np[sub]))


def oracle_field(sd, frame, pts_np):
    """alpha + mesh_sdf with the CPU oracle's mesh and query functions (the calls of tests/test_hip_parity.py's per-sample parity), and the
    discrete decisions behind it."""
    pts = torch.from_numpy(np.ascontiguousarray(pts_np))
    verts = frame["targets"]["vert_world"]
    xy01, z01 = orc.source_vert_xyz01(verts, frame["cam_in"])
    q_sdf, q_vis, vert_vis, cface = orc.cal_vis_sdf_batch(verts, frame["targets"]["face_world"].long(), pts[None], xy01, z01)
    view = torch.nn.functional.normalize(torch.ones_like(pts), dim=-1)[None]
    rgba, valid = orc.query(sd, pts[None], frame["cam_in"], frame["targets"], frame["feat_geo"], frame["feat_tex"], vert_vis, q_vis, q_sdf,
                            frame["sp_data"], frame["img_in"], view, frame["src_foreground_mask"])
    ref = orc.eval_func(sd, rgba, valid, frame["cam_in"]["nml_scale"])[0]
    return dict(f=(ref[:, 0] + q_sdf.reshape(-1)).numpy(), valid=valid.reshape(-1).bool().numpy(), face=cface[0].long().numpy(),  # (the closest face as its vertex triple)
                knn=orc.knn1(pts, verts[0]).long().numpy(), rgb=ref[:, 2:5].numpy())


def test_grid_points_equal_the_numpy_expression(scene):
    from vanerf_amd import surface
    got = surface.grid_points(scene["origin"], scene["spacing"], scene["dims"]).cpu().numpy()
    assert got.shape == scene["pts_np"].shape and np.array_equal(got.view(np.int32), scene["pts_np"].view(np.int32))
    nx, ny, nz = scene["dims"]
    slab = surface.grid_points(scene["origin"], scene["spacing"], scene["dims"], z0=5, nz_out=3).cpu().numpy()
    assert np.array_equal(slab, scene["pts_np"][5 * nx * ny:8 * nx * ny])
    lo, hi = scene["frame"]["bounds"][0, 0].numpy(), scene["frame"]["bounds"][0, 1].numpy()
    assert np.array_equal(got[0], lo) and np.abs(got[-1] - hi).max() <= 1e-6  # the grid spans the frame's bounds


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_field_against_the_oracle(R, scene, precision):
    from vanerf_amd import surface
    w = R.PackedWeights(scene["sd"], mode=precision)
    fdat, sub, want = scene["fdat"], scene["sub"], scene["oracle"]
    f, rgb = surface.field_on_grid(w, fdat, scene["frame"]["bounds"], dims=DIMS, want_rgb=True)
    nx, ny, nz = DIMS
    assert f.shape == (nz, ny, nx) and rgb.shape == (nz, ny, nx, 3) and torch.isfinite(f).all()
    got = f.reshape(-1)[torch.from_numpy(sub).cuda()].cpu().numpy()
    # the HIP path's own discrete decisions at the subset
    pts = torch.from_numpy(scene["pts_np"][sub]).cuda()
    sdf, vis, face, knn = R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts, want_face=True)
    _, valid = R.query_samples(w, fdat, pts, sdf, vis, knn, want_valid=True)
    face3 = scene["frame"]["targets"]["face_world"][0].long().numpy()[face.cpu().numpy()]
    flipped = ((valid.cpu().numpy() != 0) != want["valid"]) | (face3 != want["face"]).any(1) | (knn.cpu().numpy() != want["knn"])
    err = np.abs(got - want["f"])
    print(f"{precision}: max |f - oracle| = {err.max():.3e}, away from flipped decisions {err[~flipped].max():.3e}; flipped {int(flipped.sum())} of {len(sub)}; "
          f"inside {(want['f'] < 0).mean():.3f}, valid {want['valid'].mean():.3f}")
    assert flipped.sum() <= MAX_EXCUSED
    assert err[~flipped].max() <= TOL
    assert 0.02 < (want["f"] < 0).mean() < 0.9 and want["valid"].mean() > 0.5  # the subset sees both sides of the surface
    got_rgb = rgb.reshape(-1, 3)[torch.from_numpy(sub).cuda()].cpu().numpy()
    assert np.abs(got_rgb - want["rgb"])[~flipped].max() <= TOL


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_slab_size_changes_no_bit(R, scene, precision):
    from vanerf_amd import surface
    w = R.PackedWeights(scene["sd"], mode=precision)
    nx, ny, nz = DIMS
    args = (w, scene["fdat"], scene["frame"]["bounds"])
    whole, whole_rgb = surface.field_on_grid(*args, dims=DIMS, want_rgb=True, slab_points=nx * ny * nz)
    for layers in (8, 6, 5, 1):  # two slabs; three, the last one short; four, the last a single layer; a slab per layer
        f, rgb = surface.field_on_grid(*args, dims=DIMS, want_rgb=True, slab_points=layers * nx * ny + 7)
        assert torch.equal(f.view(torch.int32), whole.view(torch.int32)) and torch.equal(rgb.view(torch.int32), whole_rgb.view(torch.int32)), layers
    alone = surface.field_on_grid(*args, dims=DIMS)
    assert torch.equal(alone.view(torch.int32), whole.view(torch.int32))


def _net(precision, zero=False):
    from vanerf_amd.config import default_config
    from vanerf_amd.model import VANeRF
    torch.manual_seed(0)
    cfg = default_config()
    cfg["models"]["VANeRF"]["mfma_precision"] = precision
    net = VANeRF(cfg).cuda().eval()
    sd = synth.make_full_weights(0)
    if zero:  # every effective weight of the per-sample networks is zero (weight-normed layers: g = 0, their direction v stays): rad = 0
        from vanerf_amd.synth import PACKED_PREFIXES
        sd = {k: (torch.zeros_like(v) if k.startswith(PACKED_PREFIXES) and k != "sigmoid_beta" and not k.endswith("weight_v") else v) for k, v in sd.items()}
    net.load_state_dict(sd, strict=False)
    return net


def _straddled_edges(f, iso):
    """The grid edges (seven per point, towards +x, +y, +xy, +z, ...) whose ends straddle iso in f (nz, ny, nx) fp32: (E, 2) linear indices."""
    nz, ny, nx = f.shape
    g = np.where(np.isfinite(f), f, np.finfo(np.float32).max)
    inside = g < np.float32(iso)
    lin = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    out = []
    for d in range(1, 8):
        dx, dy, dz = d & 1, d >> 1 & 1, d >> 2
        a = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        b = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        m = inside[a] != inside[b]
        out.append(np.stack([lin[a][m], lin[b][m]], -1))
    return np.concatenate(out)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_extract_surface_end_to_end(R, scene, precision):
    from vanerf_amd import surface
    net = _net(precision)
    trb = synth.to_tr_batch(synth.to_device(scene["frame"], "cuda"))
    voxel = 0.008
    mesh = surface.extract_surface(net, trb, voxel_size=voxel)
    verts, faces, colors = mesh["verts"], mesh["faces"], mesh["colors"]
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and colors.shape == verts.shape and verts.is_cuda
    assert len(verts) > 500 and len(faces) > 1000
    assert int(faces.min()) >= 0 and int(faces.max()) < len(verts)
    assert torch.isfinite(verts).all() and torch.isfinite(colors).all()
    assert mesh["mano_verts"].shape == (1558, 3) and torch.equal(mesh["mano_verts"], trb["targets"]["vert_world"][0])
    assert torch.equal(mesh["mano_faces"].long(), trb["targets"]["face_world"][0].long())

    # every vertex lies on a grid edge whose ends straddle iso in the HIP field: exactly
    origin, spacing, dims = surface.grid_spec(trb["dr_data"]["bounds"], voxel_size=voxel)
    f = surface.field_on_grid(net, trb, voxel_size=voxel)
    assert tuple(f.shape) == dims[::-1]
    edges = _straddled_edges(f.cpu().numpy(), 0.0)
    assert len(edges) == len(verts)
    xyz = grid_xyz(origin, spacing, dims).astype(np.float32).reshape(-1, 3)
    a, b = xyz[edges[:, 0]], xyz[edges[:, 1]]
    fa, fb = f.reshape(-1).cpu().numpy()[edges[:, 0]], f.reshape(-1).cpu().numpy()[edges[:, 1]]
    t = ((np.float32(0.0) - fa) / (fb - fa)).astype(np.float64)
    want = a + t[:, None] * (b.astype(np.float64) - a)  # where the cut of each straddled edge is
    v = verts.cpu().numpy()
    for s0 in range(0, len(v), 256):
        d = np.abs(v[s0:s0 + 256, None, :].astype(np.float64) - want[None]).max(-1)
        e = d.argmin(1)  # the vertex's edge: the nearest cut, 1e-6 away at most ...
        assert d.min(1).max() <= 1e-6
        # ... and the vertex is ON it, in fp32: between the ends on every axis, which pins the coordinates the ends share
        assert (v[s0:s0 + 256] >= np.minimum(a, b)[e]).all() and (v[s0:s0 + 256] <= np.maximum(a, b)[e]).all()

    # manifold away from the bounds: no edge with two triangles on one side; boundary edges only at the faces of the grid's box
    fc = faces.cpu().numpy()
    assert_manifold(fc, closed=False)
    V, keys, cnt = edge_use(fc)
    rev = (keys % V) * V + keys // V
    open_edges = keys[~np.isin(rev, keys)]
    ends = np.stack([v[open_edges // V], v[open_edges % V]], 1)  # (n, 2, 3)
    lo, hi = xyz[0], xyz[-1]
    on_box = ((ends == lo) | (ends == hi)).any(-1).all(-1)
    assert on_box.all(), f"{int((~on_box).sum())} open edges inside the grid"

    # VANeRF.extract_surface returns the same tensors
    again = net.extract_surface(trb, voxel_size=voxel)
    for k in ("verts", "faces", "colors", "mano_verts", "mano_faces"):
        assert torch.equal(again[k], mesh[k]), k
    no_col = net.extract_surface(trb, voxel_size=voxel, colors=False)
    assert no_col["colors"] is None and torch.equal(no_col["verts"], verts) and torch.equal(no_col["faces"], faces)
    by_res = net.extract_surface(trb, resolution=24)
    assert len(by_res["verts"]) > 100


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_zero_weights_give_the_mano_surface(R, scene, precision):
    """rad = 0, so f = mesh_sdf: the level set at 0 is the input mesh, up to the grid: every vertex within one cell diagonal of it."""
    from vanerf_amd import surface
    net = _net(precision, zero=True)
    trb = synth.to_tr_batch(synth.to_device(scene["frame"], "cuda"))
    voxel = 0.008
    mesh = surface.extract_surface(net, trb, voxel_size=voxel, colors=False)
    assert len(mesh["verts"]) > 500
    fdat = scene["fdat"]
    sdf, _ = R.mesh_query(fdat.verts3, fdat.faces, fdat.vert_vis, mesh["verts"].contiguous())
    print(f"{precision}: max |mesh_sdf| at the extracted vertices = {float(sdf.abs().max()):.3e} (cell diagonal {voxel * 3 ** 0.5:.3e})")
    assert float(sdf.abs().max()) <= voxel * 3 ** 0.5
    f = surface.field_on_grid(net, trb, voxel_size=voxel)
    pts = surface.grid_points(*surface.grid_spec(trb["dr_data"]["bounds"], voxel_size=voxel))
    ref, _ = R.mesh_query(fdat.verts3, fdat.faces, fdat.vert_vis, pts)
    assert torch.equal(f.reshape(-1), ref)  # f = 0 + mesh_sdf, to the bit
