"""MANO skinning (vanerf_amd/mano.py, vanerf_amd/csrc/mano_skin.hip) on a real MI355X: vertices and joints against the
fp64 restatement on every case of tests/test_mano_skin_cpu.py, the rules that hold bit for bit (the seal, two hands, a pose alone and in a
batch, determinism, a NaN stays in its pose), and the end-to-end path from a pose track to posed_sequence's frames.

The restatement, the cases and their draws are those of tests/test_mano_skin_cpu.py, which checks the restatement on cases worked out by hand
and shows that every case has E32 <= 1e-6 and that a structural mistake moves the vertices by 1e-3 or more.

Bar: vertices and joints within 4 E32 of the fp64 restatement, per case and per output, E32 = max |fp32 - fp64| of the restatement on the same
inputs, computed here on the CPU (sections 0g / 0i); the worst error of every case is printed before it is asserted."""
import numpy as np
import pytest
import torch

from tests import test_baked_volume as B
from tests import test_mano_skin_cpu as C
from vanerf_amd import synth

pytestmark = pytest.mark.gpu

R = B.R  # the module fixture: the renderer, or a failure without a GPU
bits = B.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_MODELS = {}


def device_case(case):
    """A case's ManoModel (packed once per case) and its parameters on the device."""
    from vanerf_amd import mano
    nv, nj, nb, P, tree_name = case[:5]
    model, ring, pose, betas, trans = C.draw(nv, nj, nb, P, tree_name)
    if case[:5] not in _MODELS:
        _MODELS[case[:5]] = mano.ManoModel.from_arrays(**model, seal_ring=ring)
    return _MODELS[case[:5]], dev(pose), dev(betas), dev(trans)


def check(got, want, e32, what):
    err = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max())
    print(f"{what}: err {err:.3e} (E32 {e32:.3e}, bar {4 * e32:.3e})")
    assert err <= 4 * e32, (what, err, e32)


MAIN = (778, 16, 10, 130, "mano", False)


def small_case():
    return next(c for c in C.cases() if c[0] == 63)


# ------------------------------------------------------------------------------------------------
# 1. values
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.cases(), ids=lambda c: "nv{}-nj{}-nb{}-P{}-{}-{}".format(*c[:5], "flat" if c[5] else "mean"))
def test_vertices_and_joints_against_fp64(R, case):
    from vanerf_amd import mano
    mm, pose, betas, trans = device_case(case)
    v64, j64, ev, ej = C.reference(*case)
    verts, joints = mano.skin_hand(mm, pose, betas, trans, flat_hand_mean=case[5])
    assert verts.shape == (case[3], case[0] + 1, 3) and joints.shape == (case[3], case[1], 3) and verts.dtype == joints.dtype == torch.float32 and verts.is_cuda
    check(verts, v64, ev, f"{case} vertices")
    check(joints, j64, ej, f"{case} joints")
    unsealed, j2 = mano.skin_hand(mm, pose, betas, trans, flat_hand_mean=case[5], seal=False)
    assert unsealed.shape == (case[3], case[0], 3) and torch.equal(bits(unsealed), bits(verts[:, :-1])) and torch.equal(bits(j2), bits(joints))


def test_zero_pose_gives_the_shaped_template(R):
    from vanerf_amd import mano
    mm, _, betas, trans = device_case(MAIN)
    model, _, _, b, t = C.draw(*MAIN[:5])
    zero = np.zeros((MAIN[3], 48), dtype=np.float32)
    v64, j64 = C.restate(model, zero, b, t, np.float64, True)
    v32, j32 = C.restate(model, zero, b, t, np.float32, True)
    v_shaped = model["v_template"].astype(np.float64)[None] + np.einsum("vkb,pb->pvk", model["shapedirs"].astype(np.float64), b.astype(np.float64))
    J = np.einsum("jv,pvk->pjk", model["J_regressor"].astype(np.float64), v_shaped)
    verts, joints = mano.skin_hand(mm, dev(zero), betas, trans, flat_hand_mean=True, seal=False)
    check(verts, v_shaped + t[:, None].astype(np.float64), float(np.abs(v32 - v64).max()), "zero pose: vertices against v_shaped + trans")
    check(joints, J + t[:, None].astype(np.float64), float(np.abs(j32 - j64).max()), "zero pose: joints against J + trans")


# ------------------------------------------------------------------------------------------------
# 2. rules that hold bit for bit
# ------------------------------------------------------------------------------------------------
def test_the_sealed_vertex_is_the_fp32_ring_mean_of_the_output(R):
    from vanerf_amd import mano
    model, _, pose, betas, trans = C.draw(*MAIN[:5])
    args = (dev(pose), dev(betas), dev(trans))
    right = mano.ManoModel.from_arrays(**model, seal_ring=mano.MANO_SEAL_RING)
    left = mano.ManoModel.from_arrays(**model, seal_ring=mano.MANO_SEAL_RING[::-1])
    sealed = {}
    for name, mm in (("ring", right), ("reversed ring", left)):
        verts, _ = mano.skin_hand(mm, *args)
        host = verts.cpu().numpy()
        want = C.ring_mean(host[:, :778], mm.seal_ring, np.float32)
        assert want.dtype == np.float32 and np.array_equal(host[:, 778].view(np.int32), want.view(np.int32)), name
        sealed[name] = host
    assert np.array_equal(sealed["ring"][:, :778].view(np.int32), sealed["reversed ring"][:, :778].view(np.int32))
    d = np.abs(sealed["ring"][:, 778] - sealed["reversed ring"][:, 778]).max()
    assert d <= 1e-6  # the same point, summed in the other order
    mm, p, b, t = device_case(small_case())  # a drawn ring on a small model
    verts, _ = mano.skin_hand(mm, p, b, t)
    host = verts.cpu().numpy()
    assert np.array_equal(host[:, 63].view(np.int32), C.ring_mean(host[:, :63], mm.seal_ring, np.float32).view(np.int32))


def test_two_hands_are_two_calls_into_the_halves(R):
    from vanerf_amd import mano
    right = mano.ManoModel.from_arrays(**synth.mano_like_model(1), seal_ring=mano.MANO_SEAL_RING)
    left = mano.ManoModel.from_arrays(**synth.mano_like_model(2), seal_ring=mano.MANO_SEAL_RING[::-1])
    rng = np.random.default_rng(9)
    P = 5
    pose, betas, trans = dev((rng.standard_normal((P, 2, 48)) * 0.5).astype(np.float32)), dev(rng.standard_normal((P, 2, 10)).astype(np.float32)), \
        dev(rng.uniform(-1, 1, (P, 2, 3)).astype(np.float32))
    verts, joints = mano.skin_two_hands(right, left, pose, betas, trans)
    assert verts.shape == (P, 1558, 3) and joints.shape == (P, 32, 3) and verts.is_contiguous() and joints.is_contiguous()
    for h, mm in enumerate((right, left)):
        v, j = mano.skin_hand(mm, pose[:, h].contiguous(), betas[:, h].contiguous(), trans[:, h].contiguous())
        assert torch.equal(bits(verts[:, 779 * h:779 * (h + 1)]), bits(v)) and torch.equal(bits(joints[:, 16 * h:16 * (h + 1)]), bits(j)), h
    assert not torch.equal(verts[:, :779], verts[:, 779:])
    filled = torch.full((P, 1558, 3), float("nan"), device="cuda"), torch.full((P, 32, 3), float("nan"), device="cuda")
    into = mano.skin_two_hands(right, left, pose, betas, trans, out=filled)
    assert into[0] is filled[0] and torch.equal(bits(filled[0]), bits(verts)) and torch.equal(bits(filled[1]), bits(joints))
    open_v, _ = mano.skin_two_hands(right, left, pose, betas, trans, seal=False)
    assert open_v.shape == (P, 1556, 3) and torch.equal(bits(open_v[:, 778:]), bits(verts[:, 779:1557]))
    empty_v, empty_j = mano.skin_two_hands(right, left, pose[:0], betas[:0], trans[:0])
    assert empty_v.shape == (0, 1558, 3) and empty_j.shape == (0, 32, 3)


def test_a_pose_has_the_bits_it_has_alone(R):
    from vanerf_amd import mano
    mm, pose, betas, trans = device_case(MAIN)
    verts, joints = mano.skin_hand(mm, pose, betas, trans)
    for p in (0, 1, 2, 3, 64, 127, 129):
        v, j = mano.skin_hand(mm, pose[p:p + 1], betas[p:p + 1], trans[p:p + 1])
        assert torch.equal(bits(v[0]), bits(verts[p])) and torch.equal(bits(j[0]), bits(joints[p])), p
    v, j = mano.skin_hand(mm, pose[3:10], betas[3:10], trans[3:10])  # another place in the batch, another place in a lane's group of poses
    assert torch.equal(bits(v), bits(verts[3:10])) and torch.equal(bits(j), bits(joints[3:10]))


def test_the_same_bits_every_call(R):
    from vanerf_amd import mano
    mm, pose, betas, trans = device_case(MAIN)
    first = mano.skin_hand(mm, pose, betas, trans)
    again = mano.skin_hand(mm, pose, betas, trans)
    filled = torch.full((130, 779, 3), float("nan"), device="cuda"), torch.full((130, 16, 3), float("nan"), device="cuda")
    into = mano.skin_hand(mm, pose, betas, trans, out=filled)
    assert all(a is b for a, b in zip(into, filled))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = mano.skin_hand(mm, pose, betas, trans)
    side.synchronize()
    for a, b, c, d in zip(first, again, into, on_side):
        assert torch.isfinite(a).all() and torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c)) and torch.equal(bits(a), bits(d))


@pytest.mark.parametrize("where", ["pose", "betas", "trans"])
def test_a_nan_stays_in_its_pose(R, where):
    from vanerf_amd import mano
    mm, pose, betas, trans = device_case(MAIN)
    pose, betas, trans = pose[:9].clone(), betas[:9].clone(), trans[:9].clone()
    clean = mano.skin_hand(mm, pose, betas, trans)
    {"pose": pose, "betas": betas, "trans": trans}[where][5, 1] = float("nan")  # (pose: a component of the root's rotation)
    v, j = mano.skin_hand(mm, pose, betas, trans)
    others = [p for p in range(9) if p != 5]
    assert torch.equal(bits(v[others]), bits(clean[0][others])) and torch.equal(bits(j[others]), bits(clean[1][others]))
    first = 1 if where == "pose" else 0  # (the root JOINT is J_0 + trans whatever the pose)
    assert not torch.isfinite(v[5]).all(-1).any() and not torch.isfinite(j[5, first:]).all(-1).any()  # every vertex and joint of the pose


def test_the_python_layer_checks_shapes_and_devices(R):
    from vanerf_amd import mano
    mm, pose, betas, trans = device_case(small_case())
    with pytest.raises(ValueError, match="pose: expected"):
        mano.skin_hand(mm, pose[:, :-1], betas, trans)
    with pytest.raises(ValueError, match="betas: expected"):
        mano.skin_hand(mm, pose, betas[:-1], trans)
    with pytest.raises(ValueError, match="trans: expected"):
        mano.skin_hand(mm, pose, betas, trans.double())
    with pytest.raises(ValueError, match="contiguous rows"):
        mano.skin_hand(mm, pose.t().contiguous().t(), betas, trans)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mano.skin_hand(mm, pose.cpu(), betas, trans)
    with pytest.raises(ValueError, match=r"out\[0\]"):
        mano.skin_hand(mm, pose, betas, trans, out=(torch.empty(pose.shape[0], 63, 3, device="cuda"), torch.empty(pose.shape[0], 16, 3, device="cuda")))
    open_model = mano.ManoModel.from_arrays(**C.draw(63, 16, 10, pose.shape[0], "mano")[0])
    with pytest.raises(ValueError, match="no seal_ring"):
        mano.skin_hand(open_model, pose, betas, trans)
    assert mm.to("cuda") is mm and mm.to(mm.device) is mm


def test_a_model_from_a_file_is_the_model_from_its_arrays(R, tmp_path):
    from vanerf_amd import mano
    mm, pose, betas, trans = device_case(MAIN)
    model, ring = C.draw(*MAIN[:5])[:2]
    C.save_as_the_model_file_has_it(tmp_path / "hand.npz", model, ring)  # posedirs (nv, 3, 135), kintree_table, the ring in the file
    loaded = mano.ManoModel.from_npz(tmp_path / "hand.npz")
    assert (loaded.nv, loaded.nj, loaded.nb, loaded.seal_ring) == (778, 16, 10, ring)
    for a, b in zip(mano.skin_hand(loaded, pose, betas, trans), mano.skin_hand(mm, pose, betas, trans)):
        assert torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------
# 3. end to end: a pose track to posed_sequence's frames
# ------------------------------------------------------------------------------------------------
def test_end_to_end_on_the_synthetic_frame(R, monkeypatch):
    from vanerf_amd import baked, mano, posed
    from vanerf_amd.mask_at_box import frame_bounds
    from vanerf_amd.novel_views import camera_to_cam_tar
    net = B._net("fp32")
    frame_cpu = synth.make_frame(seed=3, tar_h=16, tar_w=16)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    S = 32
    cams = [camera_to_cam_tar(c) for c in B._orbit(frame_cpu, 8)[:3]]
    frame_verts = frame_cpu["targets"]["vert_world"][0].numpy()
    assert frame_verts.shape == (1558, 3)
    hands = [mano.ManoModel.from_arrays(**dict(synth.mano_like_model(20 + h, nv=779), v_template=frame_verts[779 * h:779 * (h + 1)])) for h in range(2)]
    rng = np.random.default_rng(11)
    P = 3
    pose, betas, trans = dev((rng.standard_normal((P, 2, 48)) * 0.03).astype(np.float32)), dev((rng.standard_normal((P, 2, 10)) * 0.3).astype(np.float32)), \
        dev(rng.uniform(-0.005, 0.005, (P, 2, 3)).astype(np.float32))
    kw = dict(flat_hand_mean=True, seal=False)
    verts, _ = mano.skin_two_hands(*hands, pose, betas, trans, **kw)
    moved = (verts - dev(frame_verts)[None]).norm(dim=-1).max(dim=1).values
    print("the three poses move the frame's vertices by up to", [f"{1e3 * float(m):.1f} mm" for m in moved])
    assert verts.shape == (P, 1558, 3) and 1e-3 < float(moved.min()) and float(moved.max()) < 0.03

    bakes = []
    real = baked.bake_volume
    monkeypatch.setattr(baked, "bake_volume", lambda *a, **k: bakes.append(real(*a, **k)) or bakes[-1])
    frames = list(posed.mano_sequence(net, trb, *hands, pose, betas, trans, cams[0], resolution=32, samples=S, **kw))
    assert len(frames) == P and len(bakes) == 1
    vol = bakes[0]  # the sequence's own bake serves the comparisons below
    want = list(posed.posed_sequence(net, trb, [verts[p] for p in range(P)], cams[0], samples=S, volume=vol))
    assert len(bakes) == 1
    keys = {"tex_fg", "depth", "alpha", "tex_fg_fine", "vert_xy"}
    for a, b in zip(frames, want):
        assert set(a) == set(b) == keys and all(torch.equal(bits(a[k]), bits(b[k])) for k in keys)
    assert float(frames[0]["alpha"].max()) > 0.5 and not torch.equal(frames[0]["alpha"], frames[1]["alpha"])  # the views see the hands, and they move
    by_method = net.mano_sequence(trb, *hands, pose, betas, trans, cams, volume=vol, samples=S, **kw)  # one camera per pose
    per_pose = list(posed.posed_sequence(net, trb, [verts[p] for p in range(P)], cams, samples=S, volume=vol))
    assert isinstance(by_method, list) and len(by_method) == P and len(bakes) == 1
    for a, b in zip(by_method, per_pose):
        assert set(a) == keys and all(torch.equal(bits(a[k]), bits(b[k])) for k in keys)
    # the bounds render_posed_volume marches are the dataset's rule on the skinned vertices
    faces = posed._frame_faces(trb, vol.voxels.device)
    o = posed.render_posed_volume(vol, faces, verts[1], [cams[0]], samples=S)
    given = posed.render_posed_volume(vol, faces, verts[1], [cams[0]], samples=S, bounds=frame_bounds(verts[1]))
    rays = R.ray_setup_views([cams[0]], frame_bounds(verts[1]), 0, 0, 1, 16, 16, S)
    assert torch.equal(o["hit"], rays["hit"]) and torch.equal(o["index"], rays["index"])
    assert all(torch.equal(bits(o[k]), bits(given[k])) for k in ("color", "depth", "alpha", "sdf"))
    assert torch.equal(bits(frames[1]["alpha"].view(-1)), bits(o["alpha"][0]))
