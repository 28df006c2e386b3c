"""MANO skinning on the GPU (vanerf_amd/csrc/mano_skin.hip): pose, shape and translation parameters of a batch of P
poses -> the frame's vertices and joints, in one call, on the device, with no host read.  The definition is the comment of vanerf_mano_skin in
include/vanerf_hip.h (what smplx computes with lbs and pose2rot=True); the output plugs straight into posed.render_posed_views and
posed.posed_sequence (posed.mano_sequence does it).

The licensed MANO file is not part of this project: a model comes in as arrays (ManoModel.from_arrays, or from_npz for arrays saved under
smplx's attribute names).  The known sign error of the LEFT hand's shapedirs in the files smplx reads (shapedirs[:, 0, :] has the right hand's
sign) is the caller's data preparation; nothing is flipped here.  synth.mano_like_model draws a seeded model of MANO's shapes.
"""
import ctypes
from ctypes import c_void_p

import numpy as np
import torch

from ._ffi import check, lib
from .surface import _stream

# MANO's kinematic tree (wrist, then index, middle, little, ring and thumb, three joints each) and the boundary loop of its open wrist in the
# order the dataset seals it (reversed for the left hand, whose mesh is the mirror image).
MANO_PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)
MANO_SEAL_RING = (108, 79, 78, 121, 214, 215, 279, 239, 234, 92, 38, 122, 118, 117, 119, 120)
MAX_JOINTS, MAX_BETAS, MAX_RING = 32, 16, 64


def _ring_arg(ring, nv):
    if ring is None:
        return None, 0
    ring = [int(i) for i in ring]
    if not 1 <= len(ring) <= MAX_RING or any(not 0 <= i < nv for i in ring):
        raise ValueError(f"seal_ring: expected 1 .. {MAX_RING} vertex ids in [0, {nv})")
    return (ctypes.c_int * len(ring))(*ring), len(ring)


class ManoModel:
    """A MANO-shaped model on a device: its sizes (nv, nj, nb), its packed tables (vanerf_mano_pack, once) and the wrist ring of its seal.
    The arrays it was made from stay on the host (`arrays`), so that .to(device) packs them again there."""

    def __init__(self, arrays, seal_ring, device):
        self.arrays, self.seal_ring = arrays, None if seal_ring is None else tuple(int(i) for i in seal_ring)
        self.nv, self.nj, self.nb = arrays["v_template"].shape[0], arrays["J_regressor"].shape[0], arrays["shapedirs"].shape[2]
        _ring_arg(self.seal_ring, self.nv)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"ManoModel: expected a GPU device, got {self.device} (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        nbytes = lib.vanerf_mano_packed_bytes(self.nv, self.nj, self.nb)
        if nbytes < 0:
            check(int(nbytes))
        with torch.cuda.device(self.device):
            dev = {k: torch.from_numpy(v).to(self.device) for k, v in arrays.items() if k != "parents"}
            self.packed = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            par = (ctypes.c_int * self.nj)(*[int(p) for p in arrays["parents"]])
            ptr = lambda k: c_void_p(dev[k].data_ptr()) if dev[k].numel() else None  # noqa: E731
            check(lib.vanerf_mano_pack(ptr("v_template"), ptr("shapedirs"), ptr("posedirs"), ptr("J_regressor"), ptr("weights"), par, ptr("hands_mean"),
                                       self.nv, self.nj, self.nb, c_void_p(self.packed.data_ptr()), nbytes, _stream()))
        # (`dev` is released here: the allocator hands its memory out again in stream order, behind the pack)

    @classmethod
    def from_arrays(cls, v_template, shapedirs, posedirs, J_regressor, weights, parents, hands_mean=None, seal_ring=None, device="cuda"):
        """v_template (nv, 3), shapedirs (nv, 3, nb), posedirs ((nj-1)*9, nv*3) as smplx keeps it -- or (nv, 3, (nj-1)*9) as the model file has
        it --, J_regressor (nj, nv), weights (nv, nj), parents (nj) with parents[0] = -1 (any negative or the file's 2^32 - 1 is read as -1)
        and parents[j] < j, hands_mean ((nj-1)*3) or None for zeros.  seal_ring: the vertex ids whose mean seals the wrist, or None."""
        f = lambda a: np.ascontiguousarray(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=np.float32)  # noqa: E731
        a = {"v_template": f(v_template), "shapedirs": f(shapedirs), "J_regressor": f(J_regressor), "weights": f(weights)}
        if a["v_template"].ndim != 2 or a["v_template"].shape[1] != 3 or a["v_template"].shape[0] < 1:
            raise ValueError("v_template: expected (nv, 3)")
        nv = a["v_template"].shape[0]
        if a["J_regressor"].ndim != 2 or a["J_regressor"].shape[1] != nv or not 1 <= a["J_regressor"].shape[0] <= MAX_JOINTS:
            raise ValueError(f"J_regressor: expected (nj, {nv}) with 1 <= nj <= {MAX_JOINTS}")
        nj = a["J_regressor"].shape[0]
        if a["shapedirs"].ndim != 3 or a["shapedirs"].shape[:2] != (nv, 3) or not 1 <= a["shapedirs"].shape[2] <= MAX_BETAS:
            raise ValueError(f"shapedirs: expected ({nv}, 3, nb) with 1 <= nb <= {MAX_BETAS}")
        if a["weights"].shape != (nv, nj):
            raise ValueError(f"weights: expected ({nv}, {nj})")
        pd = f(posedirs) if posedirs is not None else np.zeros(((nj - 1) * 9, nv * 3), dtype=np.float32)
        if pd.ndim == 3 and pd.shape == (nv, 3, (nj - 1) * 9):
            pd = np.ascontiguousarray(pd.reshape(nv * 3, (nj - 1) * 9).T)
        if pd.shape != ((nj - 1) * 9, nv * 3):
            raise ValueError(f"posedirs: expected ({(nj - 1) * 9}, {nv * 3}) or ({nv}, 3, {(nj - 1) * 9})")
        a["posedirs"] = pd
        hm = f(hands_mean).reshape(-1) if hands_mean is not None else np.zeros((nj - 1) * 3, dtype=np.float32)
        if hm.shape != ((nj - 1) * 3,):
            raise ValueError(f"hands_mean: expected ({(nj - 1) * 3},)")
        a["hands_mean"] = hm
        par = np.asarray(parents.detach().cpu() if torch.is_tensor(parents) else parents).astype(np.int64).reshape(-1)
        if par.shape != (nj,):
            raise ValueError(f"parents: expected ({nj},)")
        par = np.where((par < 0) | (par >= 2 ** 31), -1, par).astype(np.int32)
        if par[0] != -1 or any(not 0 <= par[j] < j for j in range(1, nj)):
            raise ValueError("parents: expected parents[0] = -1 and 0 <= parents[j] < j")
        a["parents"] = par
        return cls(a, seal_ring, device)

    @classmethod
    def from_npz(cls, path, seal_ring=None, device="cuda"):
        """Arrays saved under smplx's attribute names: v_template, shapedirs, posedirs, J_regressor, lbs_weights (or weights), parents (or
        kintree_table, whose first row it is) and hands_mean (absent: zeros).  A seal_ring stored in the file is used unless one is given."""
        with np.load(path) as z:
            weights = z["lbs_weights"] if "lbs_weights" in z else z["weights"]
            parents = z["parents"] if "parents" in z else z["kintree_table"][0]
            ring = seal_ring if seal_ring is not None else (z["seal_ring"] if "seal_ring" in z else None)
            return cls.from_arrays(z["v_template"], z["shapedirs"], z["posedirs"], z["J_regressor"], weights, parents,
                                   z["hands_mean"] if "hands_mean" in z else None, ring, device)

    def to(self, device):
        device = torch.device(device)
        same = device == self.device or (device.type == "cuda" and device.index is None and self.device.index == torch.cuda.current_device())
        return self if same else ManoModel(self.arrays, self.seal_ring, device)


def _rows(t, cols, P, dev, what):
    """A (P, cols) fp32 tensor on dev whose rows are contiguous -> (pointer, row stride in floats); a view of a wider tensor (one hand of
    (P, 2, cols)) is taken as it is."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{what}: expected a fp32 device tensor ({P if P is not None else 'P'}, {cols}) (no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != cols or (P is not None and t.shape[0] != P) or t.device != dev:
        raise ValueError(f"{what}: expected a fp32 tensor ({P if P is not None else 'P'}, {cols}) on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if (cols > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < cols):
        raise ValueError(f"{what}: expected contiguous rows (strides {t.stride()})")
    return c_void_p(t.data_ptr()), (t.stride(0) if t.shape[0] > 1 else cols)


def _out_rows(t, n, P, dev, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (P, n, 3) and t.device == dev):
        raise ValueError(f"{what}: expected a fp32 device tensor ({P}, {n}, 3) on {dev} (no CPU fallback)")
    if P > 0 and n > 0 and (t.stride(2) != 1 or (n > 1 and t.stride(1) != 3) or (P > 1 and t.stride(0) < 3 * n)):
        raise ValueError(f"{what}: expected contiguous rows (strides {t.stride()})")
    return c_void_p(t.data_ptr()), (t.stride(0) if P > 1 else 3 * n)


def skin_hand(model, pose, betas, trans, flat_hand_mean=False, seal=True, out=None):
    """vanerf_mano_skin: pose (P, nj*3) axis-angle per joint with the root first, betas (P, nb), trans (P, 3), fp32 on the model's device (rows
    contiguous; the row stride is free, so one hand of a (P, 2, .) tensor is passed as a view) -> verts (P, nv + 1, 3) with the wrist sealed by
    the mean of model.seal_ring as its last vertex (seal=False: (P, nv, 3)) and joints (P, nj, 3).  flat_hand_mean=False adds the model's
    hands_mean to the finger poses, as the reference's layers do.  out=(verts, joints): written in place (views of a larger tensor are
    fine); every element is written.  P = 0 is valid."""
    for t, what in ((pose, "pose"), (betas, "betas"), (trans, "trans")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: expected a fp32 device tensor (no CPU fallback)")
    if not isinstance(model, ManoModel):
        raise ValueError("model: expected a ManoModel")
    dev = model.device
    pp, ps = _rows(pose, model.nj * 3, None, dev, "pose")
    P = pose.shape[0]
    bp, bs = _rows(betas, model.nb, P, dev, "betas")
    tp, ts = _rows(trans, 3, P, dev, "trans")
    if seal and model.seal_ring is None:
        raise ValueError("seal=True: the model carries no seal_ring")
    ring, n_ring = _ring_arg(model.seal_ring if seal else None, model.nv)
    nvo = model.nv + (1 if seal else 0)
    with torch.cuda.device(dev):
        if out is None:
            verts, joints = torch.empty(P, nvo, 3, dtype=torch.float32, device=dev), torch.empty(P, model.nj, 3, dtype=torch.float32, device=dev)
        else:
            verts, joints = out
        vp, vs = _out_rows(verts, nvo, P, dev, "out[0] (verts)")
        jp, js = _out_rows(joints, model.nj, P, dev, "out[1] (joints)")
        nbytes = lib.vanerf_mano_workspace_bytes(model.nj, P)
        if nbytes < 0:
            check(int(nbytes))
        ws = torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=dev)
        check(lib.vanerf_mano_skin(c_void_p(model.packed.data_ptr()), model.nv, model.nj, model.nb, pp, ps, bp, bs, tp, ts, P, int(bool(flat_hand_mean)),
                                   ring, n_ring, c_void_p(ws.data_ptr()), nbytes, vp, vs, jp, js, _stream()))
    return verts, joints


def skin_two_hands(right, left, pose, betas, trans, flat_hand_mean=False, seal=True, out=None):
    """The frame's mesh: pose (P, 2, nj*3), betas (P, 2, nb), trans (P, 2, 3) with the RIGHT hand at index 0 -> verts (P, nvr + nvl, 3), right
    then left (each nv + 1 vertices when sealed: (P, 1558, 3) for MANO), and joints (P, 2 nj, 3).  Two skin_hand calls that read the halves of
    the inputs and write the halves of the outputs in place: no copy, and the same bits as those calls."""
    for t, what in ((pose, "pose"), (betas, "betas"), (trans, "trans")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: expected a fp32 device tensor (P, 2, .) (no CPU fallback)")
    if not (isinstance(right, ManoModel) and isinstance(left, ManoModel)):
        raise ValueError("right, left: expected two ManoModels")
    if right.device != left.device or right.nj != left.nj or right.nb != left.nb:
        raise ValueError("right, left: expected models of the same nj and nb on one device")
    for t, c, what in ((pose, right.nj * 3, "pose"), (betas, right.nb, "betas"), (trans, 3, "trans")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: expected a fp32 device tensor (P, 2, {c}) (no CPU fallback)")
        if t.dim() != 3 or t.shape[1:] != (2, c) or t.shape[0] != pose.shape[0]:
            raise ValueError(f"{what}: expected a tensor (P, 2, {c}), got {tuple(t.shape)}")
    P, dev = pose.shape[0], right.device
    nvr, nvl = right.nv + (1 if seal else 0), left.nv + (1 if seal else 0)
    if out is None:
        with torch.cuda.device(dev):
            out = torch.empty(P, nvr + nvl, 3, dtype=torch.float32, device=dev), torch.empty(P, 2 * right.nj, 3, dtype=torch.float32, device=dev)
    verts, joints = out
    _out_rows(verts, nvr + nvl, P, dev, "out[0] (verts)")
    _out_rows(joints, 2 * right.nj, P, dev, "out[1] (joints)")
    skin_hand(right, pose[:, 0], betas[:, 0], trans[:, 0], flat_hand_mean, seal, out=(verts[:, :nvr], joints[:, :right.nj]))
    skin_hand(left, pose[:, 1], betas[:, 1], trans[:, 1], flat_hand_mean, seal, out=(verts[:, nvr:], joints[:, right.nj:]))
    return verts, joints


__all__ = ["MANO_PARENTS", "MANO_SEAL_RING", "ManoModel", "skin_hand", "skin_two_hands"]
