"""What tests/test_mano_skin.py rests on, checked without a GPU: the numpy restatement of MANO skinning (the definition
in the comment of vanerf_mano_skin, include/vanerf_hip.h) on cases worked out by hand, the cases and draws of the GPU tests against their
conditions, the argument checks of the C entries before any device call, and the Python layer's refusals.

`restate(model, pose, betas, trans, dtype)` is the yardstick in fp64 and gives E32 = max |fp32 - fp64| of itself in fp32 (sections 0g / 0i).

One hand-worked case is held differently from how it was first stated.  "A quarter turn about z carries (1, 0, 0) to (0, 1, 0)" cannot hold to
1e-12: the definition's angle is |r + 1e-8|, so the turn is short of a quarter by 6e-9 (the 2e-8 that Rodrigues differs from scipy by has the
same origin).  The test therefore holds the case to 1e-12 against the definition's own closed form -- the angle and axis with the constant
in them, worked out by hand below -- and to 2e-8 against (0, 1, 0)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from vanerf_amd import synth

# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def rodrigues(r, dtype=np.float64):
    """r (..., 3) axis-angle -> R (..., 3, 3): angle = |r + 1e-8| (the constant on every component, in the norm only), d = r / angle,
    K = skew(d), R = I + sin(angle) K + (1 - cos(angle)) K K, all in dtype."""
    r = np.asarray(r, dtype=dtype)
    e = r + dtype(1e-8)
    angle = np.sqrt((e * e).sum(-1, keepdims=True))
    d = r / angle
    K = np.zeros(r.shape[:-1] + (3, 3), dtype=dtype)
    K[..., 0, 1], K[..., 0, 2] = -d[..., 2], d[..., 1]
    K[..., 1, 0], K[..., 1, 2] = d[..., 2], -d[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -d[..., 1], d[..., 0]
    s, c = np.sin(angle)[..., None], np.cos(angle)[..., None]
    return np.eye(3, dtype=dtype) + s * K + (dtype(1) - c) * (K @ K)


def ring_mean(verts, ring, dtype):
    """The seal's arithmetic: the sum of verts[:, ring[u]] in the ring's order, from the left, times 1 / n, in dtype."""
    v = np.asarray(verts, dtype=dtype)
    s = v[:, ring[0]].copy()
    for u in ring[1:]:
        s = s + v[:, u]
    return s * (dtype(1) / dtype(len(ring)))


def restate(model, pose, betas, trans, dtype=np.float64, flat_hand_mean=False, ring=None, parts=False):
    """model: a dict of arrays under smplx's names (synth.mano_like_model); pose (P, nj*3), betas (P, nb), trans (P, 3) -> verts (P, nv, 3)
    (with the sealed vertex appended when a ring is given) and joints (P, nj, 3), every step in dtype.  parts=True: a dict of the steps."""
    c = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    vt, sd, pd, Jr, W, hm = (c(model[k]) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "hands_mean"))
    parents = [int(p) for p in model["parents"]]
    pose, betas, trans = c(pose), c(betas), c(trans)
    P, nj, nv = pose.shape[0], Jr.shape[0], vt.shape[0]
    full = pose.copy()
    if not flat_hand_mean:
        full[:, 3:] = full[:, 3:] + hm
    v_shaped = vt[None] + np.einsum("vkb,pb->pvk", sd, betas)
    J = np.einsum("jv,pvk->pjk", Jr, v_shaped)
    R = rodrigues(full.reshape(P, nj, 3), dtype)
    feat = (R[:, 1:] - np.eye(3, dtype=dtype)).reshape(P, (nj - 1) * 9)
    v_posed = v_shaped + (feat @ pd).reshape(P, nv, 3)
    G = np.zeros((P, nj, 4, 4), dtype=dtype)
    for j in range(nj):
        L = np.zeros((P, 4, 4), dtype=dtype)
        L[:, :3, :3], L[:, 3, 3] = R[:, j], 1
        L[:, :3, 3] = J[:, j] if j == 0 else J[:, j] - J[:, parents[j]]
        G[:, j] = L if j == 0 else G[:, parents[j]] @ L
    joints = G[:, :, :3, 3] + trans[:, None]
    A = G[:, :, :3, :].copy()
    A[..., 3] = A[..., 3] - np.einsum("pjrc,pjc->pjr", G[:, :, :3, :3], J)
    T = np.einsum("vj,pjrc->pvrc", W, A)
    verts = np.einsum("pvrc,pvc->pvr", T[..., :3], v_posed) + T[..., 3] + trans[:, None]
    assert verts.dtype == dtype and joints.dtype == dtype
    if ring is not None:
        verts = np.concatenate([verts, ring_mean(verts, ring, dtype)[:, None]], 1)
    if parts:
        return dict(full=full, v_shaped=v_shaped, J=J, R=R, v_posed=v_posed, G=G, verts=verts, joints=joints)
    return verts, joints


# ------------------------------------------------------------------------------------------------
# the cases of the GPU tests (tests/test_mano_skin.py) and their draws
# ------------------------------------------------------------------------------------------------
def tree(name, nj):
    if name == "mano":
        return None  # synth's default: fingers of three joints, MANO's tree at nj = 16
    return [-1] + [j - 1 if name == "chain" else 0 for j in range(1, nj)]


def cases():
    """(nv, nj, nb, P, tree, flat_hand_mean): nv on both sides of a wave and of a block of 256 and MANO's own; nj and nb at 1, at MANO's and at
    the entry's limits; P at 1, 2, 3, 130 and around the vertex kernel's poses per lane; MANO's tree, a single chain (the deepest recursion)
    and a star.  Every case has at least 48 output values of either kind, so that its E32 is the maximum of a sample and not one rounding."""
    from vanerf_amd import build
    build.build()  # in-tree hipcc build; a no-op when up to date
    from vanerf_amd import _ffi
    L = int(_ffi.lib.vanerf_mano_poses_per_lane())
    out = [(778, 16, 10, 130, "mano", False), (778, 16, 10, 1, "mano", True), (257, 16, 10, 2, "chain", False), (65, 16, 1, 3, "star", True),
           (63, 16, 10, L, "mano", True), (64, 16, 10, L + 1, "chain", True), (1, 1, 1, 130, "chain", False), (257, 2, 1, 8 * L + 1, "star", False),
           (65, 32, 16, 2, "chain", False)]
    if L > 1:
        out.append((64, 2, 10, 8 * L - 1, "chain", False))
        out.append((257, 16, 10, L - 1, "star", False))
    return out


@functools.lru_cache(maxsize=None)
def draw(nv, nj, nb, P, tree_name, seed=0):
    """A case's model, ring and parameters: translations up to 1 m, root rotations of sigma 1.5 rad, finger rotations of sigma 0.5 rad, betas of
    sigma 1; the ring is min(16, nv) distinct vertices in a drawn order."""
    model = synth.mano_like_model(100 + seed, nv, nj, nb, parents=tree(tree_name, nj))
    rng = np.random.default_rng([seed, nv, nj, nb, P])
    pose = rng.standard_normal((P, nj, 3)) * 0.5
    pose[:, 0] *= 3.0
    pose = pose.reshape(P, nj * 3).astype(np.float32)
    betas = rng.standard_normal((P, nb)).astype(np.float32)
    trans = rng.uniform(-1.0, 1.0, (P, 3)).astype(np.float32)
    ring = tuple(int(i) for i in rng.permutation(nv)[:16])
    return model, ring, pose, betas, trans


@functools.lru_cache(maxsize=None)
def reference(nv, nj, nb, P, tree_name, flat, seed=0):
    """-> (verts64, joints64, E32 of the vertices, E32 of the joints): computed once per case and shared."""
    model, ring, pose, betas, trans = draw(nv, nj, nb, P, tree_name, seed)
    v64, j64 = restate(model, pose, betas, trans, np.float64, flat, ring)
    v32, j32 = restate(model, pose, betas, trans, np.float32, flat, ring)
    assert v32.dtype == np.float32 and j32.dtype == np.float32
    return v64, j64, float(np.abs(v32 - v64).max()), float(np.abs(j32 - j64).max())


def tiny_model(nj=2):
    """Three vertices on the x axis at 0, 1, 2; joint 0 at the origin and joint 1 at (1, 0, 0); vertex 2 moves with the last joint."""
    m = {"v_template": np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=np.float64), "shapedirs": np.zeros((3, 3, 1)),
         "posedirs": np.zeros(((nj - 1) * 9, 9)), "J_regressor": np.eye(3)[:nj], "weights": np.zeros((3, nj)),
         "parents": np.array([-1, 0][:nj]), "hands_mean": np.zeros((nj - 1) * 3)}
    m["weights"][0, 0] = m["weights"][1, 0] = m["weights"][2, nj - 1] = 1.0
    return m


# ------------------------------------------------------------------------------------------------
# the restatement on its own
# ------------------------------------------------------------------------------------------------
def test_zero_rotation_is_exactly_the_identity():
    for dtype in (np.float64, np.float32):
        assert np.array_equal(rodrigues(np.zeros((2, 3)), dtype), np.broadcast_to(np.eye(3, dtype=dtype), (2, 3, 3)))


def test_rodrigues_against_scipy():
    from scipy.spatial.transform import Rotation
    r = np.random.default_rng(0).standard_normal((100, 3)) * 1.5
    err = np.abs(rodrigues(r) - Rotation.from_rotvec(r).as_matrix()).max()
    print(f"Rodrigues against scipy on 100 vectors: {err:.3e} (the +1e-8 of the definition)")
    assert err <= 1e-7


def test_a_quarter_turn_about_z():
    m = tiny_model(1)
    m["v_template"] = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 0, 0]])
    m["J_regressor"] = np.array([[0.5, 0.5, 0.0]])  # the joint at the origin
    q = np.pi / 2
    verts, joints = restate(m, np.array([[0, 0, q]]), np.zeros((1, 1)), np.zeros((1, 3)))
    # by hand, with the definition's constant: angle a = sqrt(2e-16 + (q + 1e-8)^2), axis (0, 0, q / a), so that
    # R (1, 0, 0) = (1 - (1 - cos a) dz^2, sin a dz, 0)
    a = np.sqrt(2e-16 + (q + 1e-8) ** 2)
    dz = q / a
    want = np.array([1 - (1 - np.cos(a)) * dz * dz, np.sin(a) * dz, 0.0])
    assert np.abs(verts[0, 0] - want).max() <= 1e-12 and np.abs(verts[0, 1] + want).max() <= 1e-12 and np.abs(joints).max() <= 1e-12
    assert np.abs(verts[0, 0] - [0, 1, 0]).max() <= 2e-8


def test_a_child_turns_about_its_own_joint():
    m = tiny_model(2)
    pose = np.array([[0, 0, 0.3, 0.2, -0.4, np.pi / 2]])
    trans = np.array([[0.5, -0.25, 2.0]])
    verts, joints = restate(m, pose, np.zeros((1, 1)), trans)
    R0, R1 = rodrigues(pose[0, :3]), rodrigues(pose[0, 3:])
    J1 = np.array([1.0, 0, 0])
    assert np.abs(verts[0, 2] - (R0 @ (J1 + R1 @ (np.array([2.0, 0, 0]) - J1)) + trans[0])).max() <= 1e-12
    assert np.abs(verts[0, 1] - (R0 @ J1 + trans[0])).max() <= 1e-12 and np.abs(verts[0, 0] - trans[0]).max() <= 1e-12
    assert np.abs(joints[0, 0] - trans[0]).max() <= 1e-12 and np.abs(joints[0, 1] - (R0 @ J1 + trans[0])).max() <= 1e-12
    # the child's rotation alone leaves its own joint and the parent's vertices where they were
    still, _ = restate(m, np.array([[0, 0, 0, 0, 0, 0.0]]), np.zeros((1, 1)), trans)
    turned, _ = restate(m, np.array([[0, 0, 0, 0.2, -0.4, 1.0]]), np.zeros((1, 1)), trans)
    assert np.abs(turned[0, :2] - still[0, :2]).max() <= 1e-12 and np.abs(turned[0, 2] - still[0, 2]).max() > 0.1


def dyadic_model():
    """mano_like_model with weights and regressor rows that sum to 1 EXACTLY (halves and quarters), so that a zero pose is exact."""
    m = dict(synth.mano_like_model(5, nv=40, nj=16, nb=10))
    for key in ("weights", "J_regressor"):
        w = np.zeros_like(m[key], dtype=np.float64)
        for i, row in enumerate(m[key]):
            ids = np.flatnonzero(row)[:3]
            w[i, ids] = [0.5, 0.25, 0.25][:len(ids)] if len(ids) == 3 else 1.0 / len(ids)
        m[key] = w
    return m


def test_zero_pose_is_the_shaped_template():
    m = dyadic_model()
    rng = np.random.default_rng(1)
    betas, trans = rng.standard_normal((3, 10)), rng.uniform(-1, 1, (3, 3))
    verts, joints = restate(m, np.zeros((3, 48)), betas, trans, flat_hand_mean=True)
    v_shaped = m["v_template"].astype(np.float64)[None] + np.einsum("vkb,pb->pvk", m["shapedirs"].astype(np.float64), betas)
    assert np.abs(verts - (v_shaped + trans[:, None])).max() <= 1e-12
    assert np.abs(joints - (np.einsum("jv,pvk->pjk", m["J_regressor"], v_shaped) + trans[:, None])).max() <= 1e-12


def test_hands_mean_is_a_pose_offset():
    m = synth.mano_like_model(6, nv=50)
    assert np.abs(m["hands_mean"]).min() > 0
    rng = np.random.default_rng(2)
    pose, betas, trans = rng.standard_normal((2, 48)) * 0.4, rng.standard_normal((2, 10)), rng.uniform(-1, 1, (2, 3))
    explicit = pose.copy()
    explicit[:, 3:] += m["hands_mean"].astype(np.float64)
    a = restate(m, pose, betas, trans, flat_hand_mean=False)
    b = restate(m, explicit, betas, trans, flat_hand_mean=True)
    assert np.abs(a[0] - b[0]).max() <= 1e-12 and np.abs(a[1] - b[1]).max() <= 1e-12
    mean_only = restate(m, np.zeros((1, 48)), betas[:1], trans[:1])[0]
    flat = restate(m, np.zeros((1, 48)), betas[:1], trans[:1], flat_hand_mean=True)[0]
    assert np.abs(mean_only - flat).max() > 1e-3  # and the mean does move the hand


def test_one_posedirs_entry_moves_one_coordinate():
    m = dict(synth.mano_like_model(7, nv=30))
    j, r, c, v, k = 5, 2, 1, 17, 2
    pd = np.zeros_like(m["posedirs"])
    pd[(j - 1) * 9 + 3 * r + c, 3 * v + k] = 0.25
    m["posedirs"] = pd
    pose = np.random.default_rng(3).standard_normal((1, 48)) * 0.5
    o = restate(m, pose, np.zeros((1, 10)), np.zeros((1, 3)), parts=True)
    moved = o["v_posed"] - o["v_shaped"]
    want = np.zeros_like(moved)
    want[0, v, k] = 0.25 * (o["R"][0, j] - np.eye(3))[r, c]
    assert np.abs(moved - want).max() <= 1e-12 and abs(want[0, v, k]) > 1e-3
    assert np.abs(o["R"][0, j] - rodrigues(o["full"][0, 3 * j:3 * j + 3])).max() == 0


def test_the_sealed_vertex_is_the_ring_mean():
    m = synth.mano_like_model(8)
    from vanerf_amd.mano import MANO_PARENTS, MANO_SEAL_RING
    assert tuple(m["parents"]) == MANO_PARENTS and len(set(MANO_SEAL_RING)) == 16 and max(MANO_SEAL_RING) < 778
    rng = np.random.default_rng(4)
    pose, betas, trans = rng.standard_normal((2, 48)) * 0.5, rng.standard_normal((2, 10)), rng.uniform(-1, 1, (2, 3))
    plain, _ = restate(m, pose, betas, trans)
    right, _ = restate(m, pose, betas, trans, ring=MANO_SEAL_RING)
    left, _ = restate(m, pose, betas, trans, ring=MANO_SEAL_RING[::-1])
    assert right.shape == (2, 779, 3) and np.array_equal(right[:, :778], plain)
    assert np.abs(right[:, 778] - plain[:, list(MANO_SEAL_RING)].mean(1)).max() <= 1e-12
    assert np.abs(left[:, 778] - right[:, 778]).max() <= 1e-12


# ------------------------------------------------------------------------------------------------
# the GPU tests' inputs
# ------------------------------------------------------------------------------------------------
def test_the_gpu_cases_meet_their_conditions():
    seen = {"nv": set(), "nj": set(), "nb": set(), "P": set(), "tree": set(), "flat": set()}
    for case in cases():
        v64, j64, ev, ej = reference(*case)
        print(f"{case}: E32 verts {ev:.3e}, joints {ej:.3e}")
        assert np.isfinite(v64).all() and np.isfinite(j64).all() and 0 < ev <= 1e-6 and 0 < ej <= 1e-6, case
        assert v64.size - 3 * case[3] >= 48 and j64.size >= 48
        for k, x in zip(seen, case):
            seen[k].add(x)
    from vanerf_amd import _ffi
    L = int(_ffi.lib.vanerf_mano_poses_per_lane())
    assert seen["nv"] >= {1, 63, 64, 65, 257, 778} and seen["nj"] >= {1, 2, 16} and seen["nb"] >= {1, 10}
    assert seen["P"] >= {1, 2, 3, 130, L, L + 1} | ({L - 1} if L > 1 else set())
    assert seen["tree"] == {"mano", "chain", "star"} and seen["flat"] == {False, True}


def test_structural_mistakes_show_up_far_above_the_bar():
    """What the bar of the GPU tests can tell apart: on the MANO-sized case a transposed R, a posedirs read in the other order, a missing
    hands_mean and a parent off by one each move the vertices by 1e-3 or more."""
    case = (778, 16, 10, 130, "mano", False)
    model, ring, pose, betas, trans = draw(*case[:5])
    v64, _, ev, _ = reference(*case)
    wrong = {"no mean": restate(model, pose, betas, trans, flat_hand_mean=True, ring=ring)[0]}
    swapped = dict(model, posedirs=np.ascontiguousarray(model["posedirs"].reshape(15, 3, 3, 778, 3).transpose(0, 2, 1, 3, 4)).reshape(135, 2334))
    wrong["posedirs rows transposed"] = restate(swapped, pose, betas, trans, ring=ring)[0]
    swapped = dict(model, posedirs=np.ascontiguousarray(model["posedirs"].reshape(135, 778, 3).transpose(0, 2, 1)).reshape(135, 2334))
    wrong["posedirs columns [k][v]"] = restate(swapped, pose, betas, trans, ring=ring)[0]
    wrong["transposed R"] = restate(model, -pose - 2 * np.concatenate([np.zeros(3), model["hands_mean"]]), betas, trans, ring=ring)[0]
    par = model["parents"].copy()
    par[2:] = np.maximum(par[2:] - 1, 0)
    wrong["parent off by one"] = restate(dict(model, parents=par), pose, betas, trans, ring=ring)[0]
    for what, v in wrong.items():
        d = float(np.abs(v - v64).max())
        print(f"{what}: {d:.3e} against a bar of {4 * ev:.3e}")
        assert d >= 1e-3, what


def test_the_synthetic_model_is_seeded_and_of_manos_kind():
    a, b, c = synth.mano_like_model(3), synth.mano_like_model(3), synth.mano_like_model(4)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["shapedirs"], c["shapedirs"])
    assert a["v_template"].shape == (778, 3) and a["shapedirs"].shape == (778, 3, 10) and a["posedirs"].shape == (135, 2334)
    assert a["J_regressor"].shape == (16, 778) and a["weights"].shape == (778, 16) and a["hands_mean"].shape == (45,) and a["parents"].shape == (16,)
    assert all(a[k].dtype == np.float32 for k in a if k != "parents")
    assert (a["J_regressor"] >= 0).all() and (np.count_nonzero(a["J_regressor"], axis=1) <= 8).all() and np.abs(a["J_regressor"].sum(1) - 1).max() <= 1e-6
    assert (a["weights"] >= 0).all() and (np.count_nonzero(a["weights"], axis=1) <= 4).all() and np.abs(a["weights"].sum(1) - 1).max() <= 1e-6
    assert np.abs(a["hands_mean"]).min() > 0 and 1e-4 < a["shapedirs"].std() < 1e-2 and 1e-4 < a["posedirs"].std() < 1e-2
    ext = np.ptp(a["v_template"], axis=0)
    assert 0.05 < ext.max() < 0.3  # hand-sized, in metres
    small = synth.mano_like_model(0, nv=5, nj=3, nb=2, parents=[-1, 0, 0])
    assert small["posedirs"].shape == (18, 15) and tuple(small["parents"]) == (-1, 0, 0) and small["weights"].shape == (5, 3)


# ------------------------------------------------------------------------------------------------
# the C entries and the Python layer, without a device
# ------------------------------------------------------------------------------------------------
def pack_args(**change):
    p = ctypes.c_void_p(64)
    par = (ctypes.c_int * 32)(-1, *range(31))
    good = dict(v_template=p, shapedirs=p, posedirs=p, J_regressor=p, weights=p, parents=par, hands_mean=p, nv=778, nj=16, nb=10, packed=p,
                packed_bytes=1 << 40, stream=None)
    return dict(good, **change)


def skin_args(**change):
    p = ctypes.c_void_p(64)
    ring = (ctypes.c_int * 64)(*range(64))
    good = dict(packed=p, nv=778, nj=16, nb=10, pose=p, pose_stride=48, betas=p, betas_stride=10, trans=p, trans_stride=3, P=4, flat=0, ring=ring,
                n_ring=16, workspace=p, workspace_bytes=1 << 40, verts=p, verts_stride=779 * 3, joints=p, joints_stride=48, stream=None)
    return dict(good, **change)


def entry_refusals(lib):
    tried = []

    def refused(entry, args, msg):
        rc = getattr(lib, entry)(*args.values())
        assert rc == -22 and msg in lib.vanerf_last_error().decode(), (entry, msg, rc, lib.vanerf_last_error())
        tried.append(msg)

    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "parents", "hands_mean", "packed"):
        refused("vanerf_mano_pack", pack_args(**{k: None}), "null argument")
    for entry, args in (("vanerf_mano_pack", pack_args), ("vanerf_mano_skin", skin_args)):
        refused(entry, args(nv=0), "nv=0")
        refused(entry, args(nv=-5), "nv=-5")
        refused(entry, args(nj=0), "nj=0")
        refused(entry, args(nj=33), "nj=33")
        refused(entry, args(nb=0), "nb=0")
        refused(entry, args(nb=17), "nb=17")
    bad = (ctypes.c_int * 32)(-1, *range(31))
    bad[5] = 5
    refused("vanerf_mano_pack", pack_args(parents=bad), "parents[5]=5")
    bad[5] = 9
    refused("vanerf_mano_pack", pack_args(parents=bad), "parents[5]=9")
    bad[5], bad[0] = 4, 0
    refused("vanerf_mano_pack", pack_args(parents=bad), "parents[0]=0")
    bad[0], bad[1] = -1, -1
    refused("vanerf_mano_pack", pack_args(parents=bad), "parents[1]=-1")
    need = lib.vanerf_mano_packed_bytes(778, 16, 10)
    refused("vanerf_mano_pack", pack_args(packed_bytes=need - 1), "packed_bytes")
    refused("vanerf_mano_pack", pack_args(packed=ctypes.c_void_p(72)), "16-byte aligned")
    for k in ("packed", "pose", "betas", "trans", "workspace", "verts", "joints"):
        refused("vanerf_mano_skin", skin_args(**{k: None}), "null argument")
    refused("vanerf_mano_skin", skin_args(ring=None), "null argument")
    refused("vanerf_mano_skin", skin_args(P=-1), "P=-1")
    refused("vanerf_mano_skin", skin_args(n_ring=65), "n_ring=65")
    refused("vanerf_mano_skin", skin_args(n_ring=-1), "n_ring=-1")
    ring = (ctypes.c_int * 64)(*range(64))
    ring[3] = 778
    refused("vanerf_mano_skin", skin_args(ring=ring), "ring[3]=778")
    ring[3] = -1
    refused("vanerf_mano_skin", skin_args(ring=ring), "ring[3]=-1")
    refused("vanerf_mano_skin", skin_args(pose_stride=47), "pose_stride=47")
    refused("vanerf_mano_skin", skin_args(betas_stride=9), "betas_stride=9")
    refused("vanerf_mano_skin", skin_args(trans_stride=2), "trans_stride=2")
    refused("vanerf_mano_skin", skin_args(verts_stride=779 * 3 - 1), "verts_stride")
    refused("vanerf_mano_skin", skin_args(n_ring=0, verts_stride=778 * 3 - 1), "verts_stride")  # (and 778 * 3 is enough without the seal: below)
    refused("vanerf_mano_skin", skin_args(joints_stride=47), "joints_stride=47")
    refused("vanerf_mano_skin", skin_args(workspace_bytes=lib.vanerf_mano_workspace_bytes(16, 4) - 1), "workspace_bytes")
    refused("vanerf_mano_skin", skin_args(packed=ctypes.c_void_p(72)), "16-byte aligned")
    return len(tried)


def test_the_entries_check_their_arguments_before_any_device_call():
    from vanerf_amd import _ffi
    lib = _ffi.lib
    assert _ffi.ABI_VERSION == 12
    assert {"vanerf_mano_pack", "vanerf_mano_skin", "vanerf_mano_packed_bytes", "vanerf_mano_workspace_bytes", "vanerf_mano_poses_per_lane"} <= set(_ffi.EXPORTS)
    assert entry_refusals(lib) > 40
    # P = 0 is valid and a no-op, whatever the pointers
    assert lib.vanerf_mano_skin(*skin_args(P=0).values()) == 0
    assert lib.vanerf_mano_skin(*skin_args(P=0, packed=None, pose=None, betas=None, trans=None, workspace=None, verts=None, joints=None, ring=None, n_ring=0,
                                           workspace_bytes=0).values()) == 0
    # the host-only size queries
    assert 1 <= lib.vanerf_mano_poses_per_lane() <= 16
    n = lib.vanerf_mano_packed_bytes(778, 16, 10)
    assert n % 16 == 0 and n >= 4 * 778 * (3 + 30 + 405 + 16) + 8 * 16 * 3 * 12  # the four fp32 tables and the fp64 joint tables
    assert lib.vanerf_mano_workspace_bytes(16, 0) == 0 and lib.vanerf_mano_workspace_bytes(16, 3) == 3 * 4 * (16 * 12 + 15 * 9)
    assert lib.vanerf_mano_workspace_bytes(1, 2) == 2 * 4 * 12
    assert lib.vanerf_mano_packed_bytes(0, 16, 10) == -22 and b"nv=0" in lib.vanerf_last_error()
    assert lib.vanerf_mano_packed_bytes(778, 33, 10) == -22 and lib.vanerf_mano_workspace_bytes(33, 1) == -22 and lib.vanerf_mano_workspace_bytes(16, -1) == -22


def test_the_python_layer_refuses_cpu_tensors():
    from vanerf_amd import mano, posed
    m = synth.mano_like_model(0, nv=20)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mano.ManoModel.from_arrays(**m, device="cpu")
    pose, betas, trans = torch.zeros(2, 48), torch.zeros(2, 10), torch.zeros(2, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mano.skin_hand(None, pose, betas, trans)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mano.skin_two_hands(None, None, torch.zeros(2, 2, 48), torch.zeros(2, 2, 10), torch.zeros(2, 2, 3))
    with pytest.raises(ValueError, match="no CPU fallback"):
        posed.mano_sequence(None, None, None, None, torch.zeros(2, 2, 48), torch.zeros(2, 2, 10), torch.zeros(2, 2, 3), [])
    # what is wrong with a model's arrays is said before any device is touched
    with pytest.raises(ValueError, match="parents"):
        mano.ManoModel.from_arrays(**dict(m, parents=[-1, 0, 2] + [0] * 13), device="cpu")
    with pytest.raises(ValueError, match="posedirs"):
        mano.ManoModel.from_arrays(**dict(m, posedirs=m["posedirs"][:-1]), device="cpu")
    with pytest.raises(ValueError, match="weights"):
        mano.ManoModel.from_arrays(**dict(m, weights=m["weights"][:, :-1]), device="cpu")
    with pytest.raises(ValueError, match=r"1 <= nj <= 32"):
        mano.ManoModel.from_arrays(**synth.mano_like_model(0, nv=5, nj=33), device="cpu")
    with pytest.raises(ValueError, match="seal_ring"):
        mano.ManoModel.from_arrays(**m, seal_ring=[0, 20], device="cpu")


def save_as_the_model_file_has_it(path, m, ring=None):
    """A model under the names and layouts of the file smplx reads: posedirs (nv, 3, (nj-1)*9), weights, kintree_table with 2^32 - 1 for the root."""
    nv = m["v_template"].shape[0]
    kin = np.stack([np.where(m["parents"] < 0, 2 ** 32 - 1, m["parents"]).astype(np.int64), np.arange(len(m["parents"]))])
    extra = {} if ring is None else {"seal_ring": np.asarray(ring)}
    np.savez(path, v_template=m["v_template"], shapedirs=m["shapedirs"], posedirs=np.ascontiguousarray(m["posedirs"].T).reshape(nv, 3, -1),
             J_regressor=m["J_regressor"], weights=m["weights"], kintree_table=kin, hands_mean=m["hands_mean"], **extra)


def test_from_npz_reads_both_spellings(tmp_path):
    from vanerf_amd import mano
    m = synth.mano_like_model(0, nv=20)
    save_as_the_model_file_has_it(tmp_path / "file.npz", m)
    np.savez(tmp_path / "smplx.npz", **{("lbs_weights" if k == "weights" else k): v for k, v in m.items()})
    for name in ("file.npz", "smplx.npz"):  # both parse and pass every check of the arrays; what refuses them is the device alone
        with pytest.raises(ValueError, match="no CPU fallback"):
            mano.ManoModel.from_npz(tmp_path / name, device="cpu")
    np.savez(tmp_path / "short.npz", **dict(m, posedirs=m["posedirs"][:, :-3]))
    with pytest.raises(ValueError, match="posedirs"):
        mano.ManoModel.from_npz(tmp_path / "short.npz", device="cpu")
