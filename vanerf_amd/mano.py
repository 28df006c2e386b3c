"""MANO skinning on the GPU (vanerf_amd/csrc/mano_skin.hip): pose, shape and translation parameters of a batch of P
poses -> the frame's vertices and joints, in one call, on the device, with no host read.  The definition is the comment of vanerf_mano_skin in
include/vanerf_hip.h (what smplx computes with lbs and pose2rot=True); the output plugs straight into posed.render_posed_views and
posed.posed_sequence (posed.mano_sequence does it).

The opposite direction (vanerf_amd/csrc/mano_skin_backward.hip): skin_hand and skin_two_hands are differentiable with
respect to pose, betas and trans (vanerf_mano_skin_backward, first order), and fit_hand / fit_two_hands recover the parameters of a mesh in the
model's topology by Adam on the device.

The same fit by Levenberg-Marquardt (vanerf_amd/csrc/mano_skin_normal.hip): skin_normal_equations returns J^T W J, J^T W r
and the loss of the fit's data term (vanerf_mano_skin_normal), lm_solve is a Cholesky solve with one wave per pose (vanerf_mano_lm_solve), and
fit_hand_lm / fit_two_hands_lm take fit_hand's arguments and need some ten iterations.

The licensed MANO file is not part of this project: a model comes in as arrays (ManoModel.from_arrays, or from_npz for arrays saved under
smplx's attribute names).  The known sign error of the LEFT hand's shapedirs in the files smplx reads (shapedirs[:, 0, :] has the right hand's
sign) is the caller's data preparation; nothing is flipped here.  synth.mano_like_model draws a seeded model of MANO's shapes.
"""
import ctypes
from ctypes import c_void_p

import numpy as np
import torch
from torch.autograd.function import once_differentiable

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


def _rows_apart(t, n, P):
    """Whether a (P, n, 3) tensor is anything but rows of n packed triples (the stride between the rows is free)."""
    return P > 0 and n > 0 and (t.stride(2) != 1 or (n > 1 and t.stride(1) != 3) or (P > 1 and t.stride(0) < 3 * n))


def _out_rows(t, n, P, dev, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (P, n, 3) and t.device == dev):
        raise ValueError(f"{what}: expected a fp32 device tensor ({P}, {n}, 3) on {dev} (no CPU fallback)")
    if _rows_apart(t, n, P):
        raise ValueError(f"{what}: expected contiguous rows (strides {t.stride()})")
    return c_void_p(t.data_ptr()), (t.stride(0) if P > 1 else 3 * n)


def _on_device(pose, betas, trans, shape=""):
    for t, what in ((pose, "pose"), (betas, "betas"), (trans, "trans")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: expected a fp32 device tensor {shape}(no CPU fallback)")


def _model_seal(model, seal):
    """The model and seal check -> (nv + seal, the ring as the library takes it, its length)."""
    if not isinstance(model, ManoModel):
        raise ValueError("model: expected a ManoModel")
    if seal and model.seal_ring is None:
        raise ValueError("seal=True: the model carries no seal_ring")
    return (model.nv + (1 if seal else 0), *_ring_arg(model.seal_ring if seal else None, model.nv))


def _two_models(right, left, seal):
    """The two-model check -> the vertex counts (nvr, nvl) of their outputs."""
    if not (isinstance(right, ManoModel) and isinstance(left, ManoModel)):
        raise ValueError("right, left: expected two ManoModels")
    if right.device != left.device or right.nj != left.nj or right.nb != left.nb:
        raise ValueError("right, left: expected models of the same nj and nb on one device")
    return right.nv + (1 if seal else 0), left.nv + (1 if seal else 0)


def _workspace(query, *sizes, dev):
    """What `query(*sizes)` of the library asks for (a negative answer is its refusal), allocated on dev -> (pointer, bytes, the tensor to keep
    alive).  Never empty, so that the pointer is one."""
    nbytes = query(*sizes)
    if nbytes < 0:
        check(int(nbytes))
    ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
    return c_void_p(ws.data_ptr()), nbytes, ws


def _skin(model, pose, betas, trans, flat_hand_mean=False, seal=True, out=None):
    """skin_hand without autograd: the checks and the one call into the library."""
    _on_device(pose, betas, trans)
    nvo, ring, n_ring = _model_seal(model, seal)
    dev = model.device
    pp, ps = _rows(pose, model.nj * 3, None, dev, "pose")
    P = pose.shape[0]
    bp, bs = _rows(betas, model.nb, P, dev, "betas")
    tp, ts = _rows(trans, 3, P, dev, "trans")
    with torch.cuda.device(dev):
        if out is None:
            verts, joints = torch.empty(P, nvo, 3, dtype=torch.float32, device=dev), torch.empty(P, model.nj, 3, dtype=torch.float32, device=dev)
        else:
            verts, joints = out
        vp, vs = _out_rows(verts, nvo, P, dev, "out[0] (verts)")
        jp, js = _out_rows(joints, model.nj, P, dev, "out[1] (joints)")
        wp, nbytes, _ws = _workspace(lib.vanerf_mano_workspace_bytes, model.nj, P, dev=dev)
        check(lib.vanerf_mano_skin(c_void_p(model.packed.data_ptr()), model.nv, model.nj, model.nb, pp, ps, bp, bs, tp, ts, P, int(bool(flat_hand_mean)),
                                   ring, n_ring, wp, nbytes, vp, vs, jp, js, _stream()))
    return verts, joints


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def _grad_rows(t, n, P, dev, what):
    """An upstream gradient (P, n, 3), or None -> (the tensor to keep alive, pointer or None, row stride).  Whatever layout autograd hands over
    (an expanded scalar, a transposed view) is made contiguous; a half of a contiguous (P, n + m, 3) tensor is taken as it is."""
    if t is None:
        return None, None, 3 * n
    if t.dtype != torch.float32 or tuple(t.shape) != (P, n, 3) or t.device != dev:
        raise ValueError(f"{what}: expected a fp32 tensor ({P}, {n}, 3) on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if _rows_apart(t, n, P):
        t = t.contiguous()
    return t, c_void_p(t.data_ptr()), (t.stride(0) if P > 1 else 3 * n)


def _skin_backward(model, pose, betas, flat_hand_mean, seal, grad_verts, grad_joints, want=(True, True, True), out=None):
    """vanerf_mano_skin_backward: the gradients of the vertices (P, nv + seal, 3) and joints (P, nj, 3) -- either may be None, which is zeros
    -> (grad_pose, grad_betas, grad_trans), None where `want` says not wanted.  out=(gp, gb, gt): written in place (one hand's half of a
    (P, 2, .) tensor is a view); entries that are not wanted are ignored."""
    dev, P = model.device, pose.shape[0]
    pp, ps = _rows(pose, model.nj * 3, None, dev, "pose")
    bp, bs = _rows(betas, model.nb, P, dev, "betas")
    nvo, ring, n_ring = _model_seal(model, seal)
    with torch.cuda.device(dev):
        gv, gvp, gvs = _grad_rows(grad_verts, nvo, P, dev, "grad_verts")
        gj, gjp, gjs = _grad_rows(grad_joints, model.nj, P, dev, "grad_joints")
        if gv is None and gj is None:
            raise ValueError("grad_verts, grad_joints: both are None (nothing to differentiate)")
        grads, ptrs = [], []
        for i, (cols, what) in enumerate(((model.nj * 3, "grad_pose"), (model.nb, "grad_betas"), (3, "grad_trans"))):
            if not want[i]:
                grads.append(None)
                ptrs += [None, cols]
                continue
            g = out[i] if out is not None and out[i] is not None else torch.empty(P, cols, dtype=torch.float32, device=dev)
            grads.append(g)
            ptrs += list(_rows(g, cols, P, dev, what))
        wp, nbytes, _ws = _workspace(lib.vanerf_mano_skin_backward_workspace_bytes, model.nv, model.nj, model.nb, P, dev=dev)
        check(lib.vanerf_mano_skin_backward(c_void_p(model.packed.data_ptr()), model.nv, model.nj, model.nb, pp, ps, bp, bs, P, int(bool(flat_hand_mean)),
                                            ring, n_ring, gvp, gvs, gjp, gjs, wp, nbytes, *ptrs, _stream()))
    return tuple(grads)


class _SkinHand(torch.autograd.Function):
    """skin_hand under autograd: the forward is _skin (the same call, the same bits); the backward recomputes what it needs from pose and betas."""

    @staticmethod
    def forward(ctx, model, flat_hand_mean, seal, pose, betas, trans):
        ctx.model, ctx.flat, ctx.seal = model, flat_hand_mean, seal
        ctx.save_for_backward(pose, betas)
        ctx.set_materialize_grads(False)
        return _skin(model, pose, betas, trans, flat_hand_mean, seal)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_verts, grad_joints):
        want = tuple(ctx.needs_input_grad[3:6])
        if (grad_verts is None and grad_joints is None) or not any(want):
            return (None,) * 6
        pose, betas = ctx.saved_tensors
        return (None, None, None) + _skin_backward(ctx.model, pose, betas, ctx.flat, ctx.seal, grad_verts, grad_joints, want)


class _SkinTwoHands(torch.autograd.Function):
    """skin_two_hands under autograd: two backward calls that read the halves of the gradients and write the halves of (P, 2, .) tensors."""

    @staticmethod
    def forward(ctx, right, left, flat_hand_mean, seal, pose, betas, trans):
        ctx.hands, ctx.flat, ctx.seal = (right, left), flat_hand_mean, seal
        ctx.save_for_backward(pose, betas)
        ctx.set_materialize_grads(False)
        return _skin_two(right, left, pose, betas, trans, flat_hand_mean, seal)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_verts, grad_joints):
        want = tuple(ctx.needs_input_grad[4:7])
        if (grad_verts is None and grad_joints is None) or not any(want):
            return (None,) * 7
        pose, betas = ctx.saved_tensors
        right, left = ctx.hands
        P, dev, nj = pose.shape[0], right.device, right.nj
        nvr, nvl = right.nv + (1 if ctx.seal else 0), left.nv + (1 if ctx.seal else 0)
        with torch.cuda.device(dev):
            gv = None if grad_verts is None else _grad_rows(grad_verts, nvr + nvl, P, dev, "grad_verts")[0]
            gj = None if grad_joints is None else _grad_rows(grad_joints, 2 * nj, P, dev, "grad_joints")[0]
            grads = [torch.empty(P, 2, c, dtype=torch.float32, device=dev) if w else None for c, w in zip((nj * 3, right.nb, 3), want)]
        for h, (mm, v0, v1) in enumerate(((right, 0, nvr), (left, nvr, nvr + nvl))):
            _skin_backward(mm, pose[:, h], betas[:, h], ctx.flat, ctx.seal, None if gv is None else gv[:, v0:v1],
                           None if gj is None else gj[:, nj * h:nj * (h + 1)], want, out=[None if g is None else g[:, h] for g in grads])
        return (None, None, None, None) + tuple(grads)


def skin_hand(model, pose, betas, trans, flat_hand_mean=False, seal=True, out=None):
    """vanerf_mano_skin: pose (P, nj*3) axis-angle per joint with the root first, betas (P, nb), trans (P, 3), fp32 on the model's device (rows
    contiguous; the row stride is free, so one hand of a (P, 2, .) tensor is passed as a view) -> verts (P, nv + 1, 3) with the wrist sealed by
    the mean of model.seal_ring as its last vertex (seal=False: (P, nv, 3)) and joints (P, nj, 3).  flat_hand_mean=False adds the model's
    hands_mean to the finger poses, as the reference's layers do.  out=(verts, joints): written in place (views of a larger tensor are
    fine); every element is written.  P = 0 is valid.
    Differentiable: with grad mode on and pose, betas or trans requiring grad, the result carries vanerf_mano_skin_backward as its backward
    (first order only; inputs that do not require grad are not differentiated); the forward's bits are the same either way.  out= cannot be
    combined with that and raises."""
    if _wants_grad(pose, betas, trans):
        if out is not None:
            raise ValueError("out=: cannot be combined with an input that requires grad (autograd needs outputs of its own)")
        return _SkinHand.apply(model, bool(flat_hand_mean), bool(seal), pose, betas, trans)
    return _skin(model, pose, betas, trans, flat_hand_mean, seal, out)


def _skin_two(right, left, pose, betas, trans, flat_hand_mean=False, seal=True, out=None):
    """skin_two_hands without autograd."""
    _on_device(pose, betas, trans, "(P, 2, .) ")
    nvr, nvl = _two_models(right, left, seal)
    for t, c, what in ((pose, right.nj * 3, "pose"), (betas, right.nb, "betas"), (trans, 3, "trans")):
        if t.dim() != 3 or t.shape[1:] != (2, c) or t.shape[0] != pose.shape[0]:
            raise ValueError(f"{what}: expected a tensor (P, 2, {c}), got {tuple(t.shape)}")
    P, dev = pose.shape[0], right.device
    if out is None:
        with torch.cuda.device(dev):
            out = torch.empty(P, nvr + nvl, 3, dtype=torch.float32, device=dev), torch.empty(P, 2 * right.nj, 3, dtype=torch.float32, device=dev)
    verts, joints = out
    _out_rows(verts, nvr + nvl, P, dev, "out[0] (verts)")
    _out_rows(joints, 2 * right.nj, P, dev, "out[1] (joints)")
    _skin(right, pose[:, 0], betas[:, 0], trans[:, 0], flat_hand_mean, seal, out=(verts[:, :nvr], joints[:, :right.nj]))
    _skin(left, pose[:, 1], betas[:, 1], trans[:, 1], flat_hand_mean, seal, out=(verts[:, nvr:], joints[:, right.nj:]))
    return verts, joints


def skin_two_hands(right, left, pose, betas, trans, flat_hand_mean=False, seal=True, out=None):
    """The frame's mesh: pose (P, 2, nj*3), betas (P, 2, nb), trans (P, 2, 3) with the RIGHT hand at index 0 -> verts (P, nvr + nvl, 3), right
    then left (each nv + 1 vertices when sealed: (P, 1558, 3) for MANO), and joints (P, 2 nj, 3).  Two skin_hand calls that read the halves of
    the inputs and write the halves of the outputs in place: no copy, and the same bits as those calls.  Differentiable as skin_hand is: two
    backward calls on the halves of the gradient tensors, no copy; out= with an input that requires grad raises."""
    if _wants_grad(pose, betas, trans):
        if out is not None:
            raise ValueError("out=: cannot be combined with an input that requires grad (autograd needs outputs of its own)")
        return _SkinTwoHands.apply(right, left, bool(flat_hand_mean), bool(seal), pose, betas, trans)
    return _skin_two(right, left, pose, betas, trans, flat_hand_mean, seal, out)


# ------------------------------------------------------------------------------------------------
# fitting pose, shape and translation to a mesh in the model's topology
# ------------------------------------------------------------------------------------------------
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
FIT_LR_RATIOS = (1.0, 2.0, 0.2)  # pose, betas, trans: multiples of lr


def _cross_rows(M):
    """(..., 3, 3) -> the cofactor matrix (rows m1 x m2, m2 x m0, m0 x m1) and the determinant, without a solver library."""
    m0, m1, m2 = M[..., 0, :], M[..., 1, :], M[..., 2, :]
    cof = torch.stack([torch.linalg.cross(m1, m2), torch.linalg.cross(m2, m0), torch.linalg.cross(m0, m1)], -2)
    return cof, (m0 * cof[..., 0, :]).sum(-1)


def _polar_rotation(M, iterations=30):
    """The orthogonal polar factor of M (..., 3, 3) by a fixed count of Newton steps Q <- (Q + Q^-T) / 2 from M scaled to unit size: the
    rotation nearest to M when det M > 0."""
    Q = M * (3.0 ** 0.5 / M.flatten(-2).norm(dim=-1).clamp_min(1e-30))[..., None, None]
    for _ in range(iterations):
        cof, det = _cross_rows(Q)
        Q = 0.5 * (Q + cof / det[..., None, None])
    return Q


def _kabsch(src, tgt, use_svd=True):
    """src (n, 3), tgt (P, n, 3) -> the rotations (P, 3, 3) with R (src - mean) ~ tgt - mean in the least-squares sense.  One batched 3 x 3
    SVD; where the device has no SVD, the polar iteration."""
    a, b = src - src.mean(0), tgt - tgt.mean(1, keepdim=True)
    H = torch.einsum("ni,pnj->pij", a, b)  # sum of a b^T: R = V diag(1, 1, det) U^T of H = U S V^T
    if use_svd:
        try:
            U, _, Vh = torch.linalg.svd(H)
        except RuntimeError:
            U = None
        if U is not None:
            V = Vh.transpose(-1, -2)
            d = _cross_rows(V @ U.transpose(-1, -2))[1]
            flip = torch.ones_like(H[:, 0])
            flip[:, 2] = torch.where(d < 0, -1.0, 1.0).to(H.dtype)
            return (V * flip[:, None, :]) @ U.transpose(-1, -2)
    return _polar_rotation(H.transpose(-1, -2))


def _axis_angle(R):
    """Rotations (P, 3, 3) -> axis-angle (P, 3); the identity gives zeros (a half turn, whose axis this formula cannot see, does too)."""
    w = torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
    s2 = w.norm(dim=-1, keepdim=True)
    angle = torch.atan2(s2, (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0)[:, None])
    return w * (angle / s2.clamp_min(1e-20))


def _rigid_start(rest, root, target, use_svd=True):
    """The zero-pose mesh `rest` (n, 3) with its root joint `root` (3) and the targets (P, n, 3) -> the root's axis-angle (P, 3) and the
    translation (P, 3) that carry the one onto the other rigidly: the root turns the mesh about its own joint."""
    R = _kabsch(rest, target, use_svd)
    moved = torch.einsum("pij,j->pi", R, rest.mean(0) - root) + root
    return _axis_angle(R), target.mean(1) - moved


def _fit(forward, backward, params, target_verts, target_joints, vert_weight, full_offset, steps, lr, prior):
    """Adam (torch.optim.Adam's arithmetic) on pose, betas, trans -- updated in place -- for a fixed count of steps, on whatever device the tensors are
    on, with nothing read back.  forward(pose, betas, trans) -> verts, joints; backward(pose, betas, grad_verts, grad_joints) -> the three
    gradients.  The loss, per pose: mean_v w_v |v - v*|^2 + mean_j |j - j*|^2 (either term absent if its target is)
    + prior[0] |pose[3:] + full_offset|^2 + prior[1] |betas|^2."""
    pose, betas, trans = params
    moments = [(torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    b1, b2 = ADAM_BETAS
    for step in range(1, int(steps) + 1):
        verts, joints = forward(pose, betas, trans)
        gv = gj = None
        if target_verts is not None:
            gv = (verts - target_verts) * (2.0 / verts.shape[1])
            if vert_weight is not None:
                gv = gv * vert_weight
        if target_joints is not None:
            gj = (joints - target_joints) * (2.0 / joints.shape[1])
        grads = backward(pose, betas, gv, gj)
        if prior[0]:
            grads[0][:, 3:] += (2.0 * prior[0]) * (pose[:, 3:] + full_offset)
        if prior[1]:
            grads[1].add_(betas, alpha=2.0 * prior[1])
        c1, c2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        for p, g, (m, v), ratio in zip(params, grads, moments, FIT_LR_RATIOS):
            m.mul_(b1).add_(g, alpha=1.0 - b1)
            v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
            p.addcdiv_(m, (v.sqrt() / c2 ** 0.5).add_(ADAM_EPS), value=-(lr * ratio) / c1)


def _targets(model, nvo, P, target_verts, target_joints, vert_weight, rows):
    """The checks of the targets and of where the weights are that the fits and skin_normal_equations share -> the targets detached and
    contiguous, or None.  `rows` is how the first refusal writes the count of poses; the shape of the weights is the caller's to check."""
    if target_verts is None and target_joints is None:
        raise ValueError("target_verts, target_joints: expected at least one target")
    got = []
    for t, n, what in ((target_verts, nvo, "target_verts"), (target_joints, model.nj, "target_joints")):
        if t is not None:
            if not torch.is_tensor(t) or not t.is_cuda:
                raise ValueError(f"{what}: expected a fp32 device tensor ({rows}, {n}, 3) (no CPU fallback)")
            if t.dtype != torch.float32 or tuple(t.shape) != (P, n, 3) or t.device != model.device:
                raise ValueError(f"{what}: expected a fp32 tensor ({P}, {n}, 3) on {model.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
            t = t.detach().contiguous()
        got.append(t)
    if vert_weight is not None and (not torch.is_tensor(vert_weight) or not vert_weight.is_cuda):
        raise ValueError(f"vert_weight: expected a device tensor ({nvo},) or ({P}, {nvo}) (no CPU fallback)")
    return got


def _fit_result(params, verts, joints, tv, tj, **more):
    """The dict fit_hand returns: rms from the distances of the vertices (of the joints when there is no vertex target) to the target."""
    d = (verts - tv) if tv is not None else (joints - tj)
    rms = (d * d).sum(-1).mean(-1).sqrt()
    return {"pose": params[0], "betas": params[1], "trans": params[2], "verts": verts, "joints": joints, "rms": rms, **more}


def _fit_setup(model, target_verts, target_joints, init, steps, vert_weight, prior, flat_hand_mean, seal, count="steps"):
    """The checks and the start that fit_hand and fit_hand_lm share -> (P, nvo, tv, tj, w, params, offset): the targets detached and contiguous,
    the weights as (nvo, 1) or (P, nvo, 1) or None, the three parameter tensors (clones of init, or the rigid start) and what flat_hand_mean=False
    adds to pose[3:] (0.0 or hands_mean on the device).  `count` is what the caller calls `steps` in its refusal."""
    nvo, dev = _model_seal(model, seal)[0], model.device
    first = target_verts if target_verts is not None else target_joints
    P = first.shape[0] if torch.is_tensor(first) and first.dim() == 3 else None
    tv, tj = _targets(model, nvo, P, target_verts, target_joints, vert_weight, "P")
    if len(prior) != 2 or steps < 0:
        raise ValueError(f"prior: expected (pose weight, betas weight); {count}: at least 0")
    with torch.cuda.device(dev), torch.no_grad():
        w = None
        if vert_weight is not None:
            if tuple(vert_weight.shape) not in ((nvo,), (P, nvo)):
                raise ValueError(f"vert_weight: expected ({nvo},) or ({P}, {nvo}), got {tuple(vert_weight.shape)}")
            w = vert_weight.detach().to(dev, torch.float32)[..., None]
        shapes = ((P, model.nj * 3), (P, model.nb), (P, 3))
        if init is not None:
            params = []
            for t, shape, what in zip(init, shapes, ("init[0] (pose)", "init[1] (betas)", "init[2] (trans)")):
                if not torch.is_tensor(t) or not t.is_cuda:
                    raise ValueError(f"{what}: expected a fp32 device tensor {shape} (no CPU fallback)")
                if t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != dev:
                    raise ValueError(f"{what}: expected a fp32 tensor {shape} on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
                params.append(t.detach().clone().contiguous())
        else:
            params = [torch.zeros(shape, dtype=torch.float32, device=dev) for shape in shapes]
            if P > 0:
                rest_v, rest_j = _skin(model, params[0][:1], params[1][:1], params[2][:1], flat_hand_mean, seal)
                rest, target = (rest_v[0], tv) if tv is not None else (rest_j[0], tj)
                params[0][:, :3], params[2][:] = _rigid_start(rest, rest_j[0, 0], target)
        offset = 0.0
        if not flat_hand_mean and model.nj > 1:
            offset = torch.from_numpy(model.arrays["hands_mean"]).to(dev)
    return P, nvo, tv, tj, w, params, offset


def fit_hand(model, target_verts=None, target_joints=None, init=None, steps=300, lr=0.03, vert_weight=None, prior=(0.0, 0.0), flat_hand_mean=False,
             seal=True):
    """Pose, shape and translation of `model` for a batch of meshes in its topology: target_verts (P, nv + 1, 3) (seal=False: (P, nv, 3))
    and / or target_joints (P, nj, 3), fp32 on the model's device.  Minimises, per pose, mean_v w_v |v - v*|^2 + mean_j |j - j*|^2
    + prior[0] |full[3:]|^2 + prior[1] |betas|^2 (full = pose with hands_mean added unless flat_hand_mean; vert_weight (nv + seal) or
    (P, nv + seal), default ones) by `steps` steps of Adam on the device -- skin_hand's forward and vanerf_mano_skin_backward per step, learning
    rates lr for pose, 2 lr for betas and 0.2 lr for trans -- with nothing read back to the host.  init=(pose, betas, trans) starts from those
    values (tracking); init=None starts from the rigid alignment of the zero-pose mesh onto the target (Kabsch by one batched 3 x 3 SVD; the
    rotation becomes the root's axis-angle, the translation follows from the centroids) and zeros elsewhere.
    -> dict: pose (P, nj*3), betas (P, nb), trans (P, 3), verts, joints (of those parameters) and rms (P), the root mean square distance
    of the vertices (of the joints when there is no vertex target) to the target in the target's unit, a device tensor."""
    P, nvo, tv, tj, w, params, offset = _fit_setup(model, target_verts, target_joints, init, steps, vert_weight, prior, flat_hand_mean, seal)
    dev = model.device
    shapes = ((P, model.nj * 3), (P, model.nb), (P, 3))
    with torch.cuda.device(dev), torch.no_grad():
        verts = torch.empty(P, nvo, 3, dtype=torch.float32, device=dev)
        joints = torch.empty(P, model.nj, 3, dtype=torch.float32, device=dev)
        grads = tuple(torch.empty(shape, dtype=torch.float32, device=dev) for shape in shapes)
        forward = lambda p, b, t: _skin(model, p, b, t, flat_hand_mean, seal, out=(verts, joints))  # noqa: E731
        backward = lambda p, b, gv, gj: _skin_backward(model, p, b, flat_hand_mean, seal, gv, gj, out=grads)  # noqa: E731
        if P > 0:
            _fit(forward, backward, params, tv, tj, w, offset, steps, lr, prior)
        forward(*params)
        return _fit_result(params, verts, joints, tv, tj)


def _fit_two(fit_one, stacked, right, left, target_verts, target_joints, init, vert_weight, seal):
    """What fit_two_hands and fit_two_hands_lm share: the checks, the two fits one after the other -- fit_one(model, target_verts, target_joints,
    init, vert_weight) on the halves -- and the stacking; `stacked` names the per-hand results that become (P, 2, ...)."""
    (nvr, nvl), nj = _two_models(right, left, seal), right.nj
    if not torch.is_tensor(target_verts) or not target_verts.is_cuda:
        raise ValueError(f"target_verts: expected a fp32 device tensor (P, {nvr + nvl}, 3) (no CPU fallback)")
    if target_verts.dim() != 3 or tuple(target_verts.shape[1:]) != (nvr + nvl, 3):
        raise ValueError(f"target_verts: expected (P, {nvr + nvl}, 3), got {tuple(target_verts.shape)}")
    if target_joints is not None and (not torch.is_tensor(target_joints) or target_joints.dim() != 3 or tuple(target_joints.shape[1:]) != (2 * nj, 3)):
        raise ValueError(f"target_joints: expected a fp32 device tensor (P, {2 * nj}, 3) (no CPU fallback)")
    if vert_weight is not None and (not torch.is_tensor(vert_weight) or vert_weight.shape[-1] != nvr + nvl):
        raise ValueError(f"vert_weight: expected a device tensor ({nvr + nvl},) or (P, {nvr + nvl}) (no CPU fallback)")
    fits = []
    for h, (mm, v0, v1) in enumerate(((right, 0, nvr), (left, nvr, nvr + nvl))):
        fits.append(fit_one(mm, target_verts[:, v0:v1], None if target_joints is None else target_joints[:, nj * h:nj * (h + 1)],
                            None if init is None else tuple(t[:, h] for t in init), None if vert_weight is None else vert_weight[..., v0:v1]))
    out = {k: torch.stack([fits[0][k], fits[1][k]], 1) for k in stacked}
    out.update({k: torch.cat([fits[0][k], fits[1][k]], 1) for k in ("verts", "joints")})
    return out


def fit_two_hands(right, left, target_verts, target_joints=None, init=None, steps=300, lr=0.03, vert_weight=None, prior=(0.0, 0.0),
                  flat_hand_mean=False, seal=True):
    """fit_hand for the frame's mesh: target_verts (P, nvr + nvl, 3), right then left, as skin_two_hands and surface.register_surface produce
    it ((P, 1558, 3) for MANO, sealed), optionally target_joints (P, 2 nj, 3); init=(pose (P, 2, nj*3), betas (P, 2, nb), trans (P, 2, 3));
    vert_weight (nvr + nvl) or (P, nvr + nvl).  -> dict: pose (P, 2, nj*3), betas (P, 2, nb), trans (P, 2, 3) -- what skin_two_hands and
    posed.mano_sequence take --, verts (P, nvr + nvl, 3), joints (P, 2 nj, 3) and rms (P, 2), the right hand at index 0."""
    return _fit_two(lambda mm, tv, tj, start, w: fit_hand(mm, tv, tj, start, steps, lr, w, prior, flat_hand_mean, seal), ("pose", "betas", "trans", "rms"),
                    right, left, target_verts, target_joints, init, vert_weight, seal)


# ------------------------------------------------------------------------------------------------
# the same fit by Levenberg-Marquardt
# ------------------------------------------------------------------------------------------------
LM_MAX_UNKNOWNS = 128
LM_DAMPING_FLOOR, LM_TRACE_FLOOR = 1e-12, 1e-9


def _skin_normal(model, pose, betas, trans, tv, tj, w, flat_hand_mean, seal, out=None):
    """vanerf_mano_skin_normal after the checks of its callers: tv (P, nvo, 3) and tj (P, nj, 3) contiguous or None, w (nvo,) or (P, nvo)
    contiguous fp32 or None -> (H (P, n, n), g (P, n), loss (P)); out=(H, g, loss): written in place, None entries are not written."""
    dev, P, n = model.device, pose.shape[0], model.nj * 3 + model.nb + 3
    pp, ps = _rows(pose, model.nj * 3, None, dev, "pose")
    bp, bs = _rows(betas, model.nb, P, dev, "betas")
    tp, ts = _rows(trans, 3, P, dev, "trans")
    nvo, ring, n_ring = _model_seal(model, seal)
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(P, n, n, dtype=torch.float32, device=dev), torch.empty(P, n, dtype=torch.float32, device=dev),
                   torch.empty(P, dtype=torch.float32, device=dev))
        ptr = lambda t: None if t is None else c_void_p(t.data_ptr())  # noqa: E731
        wp, nbytes, _ws = _workspace(lib.vanerf_mano_skin_normal_workspace_bytes, model.nv, model.nj, model.nb, P, dev=dev)
        check(lib.vanerf_mano_skin_normal(c_void_p(model.packed.data_ptr()), model.nv, model.nj, model.nb, pp, ps, bp, bs, tp, ts, P, int(bool(flat_hand_mean)),
                                          ring, n_ring, ptr(tv), nvo * 3, ptr(w), 0 if w is None or w.dim() == 1 else nvo, ptr(tj), model.nj * 3,
                                          wp, nbytes, ptr(out[0]), n * n, ptr(out[1]), n, ptr(out[2]), 1, _stream()))
    return out


def _normal_targets(model, nvo, P, target_verts, target_joints, vert_weight):
    """The targets and weights of skin_normal_equations, checked -> contiguous fp32 tensors or None."""
    dev = model.device
    tv, tj = _targets(model, nvo, P, target_verts, target_joints, vert_weight, P)
    w = None
    if vert_weight is not None:
        if target_verts is None or tuple(vert_weight.shape) not in ((nvo,), (P, nvo)) or vert_weight.device != dev:
            raise ValueError(f"vert_weight: expected ({nvo},) or ({P}, {nvo}) on {dev} beside target_verts, got {tuple(vert_weight.shape)}")
        w = vert_weight.detach().to(torch.float32).contiguous()
    return tv, tj, w


def skin_normal_equations(model, pose, betas, trans, target_verts=None, target_joints=None, vert_weight=None, flat_hand_mean=False, seal=True):
    """vanerf_mano_skin_normal: the normal equations of fit_hand's data term at pose (P, nj*3), betas (P, nb), trans (P, 3).  With the unknowns
    ordered x = (pose, betas, trans), n = 3 nj + nb + 3, the residuals r = (verts - target_verts, joints - target_joints) (either target may be
    None), J = dr/dx and W = (vert_weight / (nv + seal), 1 / nj): -> H = J^T W J (P, n, n), symmetric bit for bit, g = J^T W r (P, n) and
    loss = r^T W r (P), fp32 device tensors.  fit_hand's loss is loss + its priors and the loss's gradient is 2 g."""
    _on_device(pose, betas, trans)
    nvo = _model_seal(model, seal)[0]
    _rows(pose, model.nj * 3, None, model.device, "pose")
    tv, tj, w = _normal_targets(model, nvo, pose.shape[0], target_verts, target_joints, vert_weight)
    return _skin_normal(model, pose.detach(), betas.detach(), trans.detach(), tv, tj, w, flat_hand_mean, seal)


def lm_solve(M, g):
    """vanerf_mano_lm_solve: M (P, n, n) symmetric positive definite (its lower triangle is read) and g (P, n), fp32 device tensors, n <= 128
    -> delta = -M^-1 g (P, n) by a Cholesky factorisation in fp64, one wave per system, and ok (P) int32: 0 where a pivot was not positive or
    not finite, and delta = 0 there.  Nothing is read back."""
    for t, what in ((M, "M"), (g, "g")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError(f"{what}: expected a fp32 device tensor (no CPU fallback)")
    if M.dtype != torch.float32 or M.dim() != 3 or M.shape[1] != M.shape[2] or not 1 <= M.shape[1] <= LM_MAX_UNKNOWNS:
        raise ValueError(f"M: expected a fp32 tensor (P, n, n) with 1 <= n <= {LM_MAX_UNKNOWNS}, got {M.dtype} {tuple(M.shape)}")
    P, n = M.shape[0], M.shape[1]
    if g.dtype != torch.float32 or tuple(g.shape) != (P, n) or g.device != M.device:
        raise ValueError(f"g: expected a fp32 tensor ({P}, {n}) on {M.device}, got {g.dtype} {tuple(g.shape)} on {g.device}")
    M, g = M.contiguous(), g.contiguous()
    with torch.cuda.device(M.device):
        delta, ok = torch.empty(P, n, dtype=torch.float32, device=M.device), torch.empty(P, dtype=torch.int32, device=M.device)
        check(lib.vanerf_mano_lm_solve(c_void_p(M.data_ptr()), n * n, c_void_p(g.data_ptr()), n, n, P, c_void_p(delta.data_ptr()), n,
                                       c_void_p(ok.data_ptr()), _stream()))
    return delta, ok


def fit_hand_lm(model, target_verts=None, target_joints=None, init=None, iterations=10, damping=1e-3, vert_weight=None, prior=(0.0, 0.0),
                flat_hand_mean=False, seal=True):
    """fit_hand by Levenberg-Marquardt: the same arguments, checks, loss, rigid start and results, with `iterations` Gauss-Newton steps in place
    of Adam's.  Per iteration and pose: M = H + the priors' diagonal + lambda (diag H + 1e-9 trace H / n), delta = -M^-1 (g + the priors' share)
    (lm_solve), and one skin_normal_equations call at x + delta; where the loss with its priors went down (and the solve succeeded) the step is
    taken and lambda = max(lambda / 10, 1e-12), elsewhere the state is kept and lambda = 10 lambda; a loss that is not finite rejects.  lambda
    starts at `damping`.  Everything is a device tensor selected by torch.where; nothing is read back.
    -> fit_hand's dict and damping (P), the last lambda, and accepted (P), the count of steps taken."""
    P, nvo, tv, tj, w, params, offset = _fit_setup(model, target_verts, target_joints, init, iterations, vert_weight, prior, flat_hand_mean, seal, "iterations")
    dev, nj3, nb = model.device, model.nj * 3, model.nb
    n = nj3 + nb + 3
    with torch.cuda.device(dev), torch.no_grad():
        w = None if w is None else w[..., 0].contiguous()
        x = torch.cat(params, 1)
        split = lambda t: (t[:, :nj3], t[:, nj3:nj3 + nb], t[:, nj3 + nb:])  # noqa: E731  (views: the entry takes row strides)
        pd, off = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
        pd[3:nj3], pd[nj3:nj3 + nb] = float(prior[0]), float(prior[1])
        off[3:nj3] = offset
        lam = torch.full((P,), float(damping), dtype=torch.float32, device=dev)
        accepted = torch.zeros(P, dtype=torch.int64, device=dev)
        if P > 0 and iterations > 0:
            H, g, L = _skin_normal(model, *split(x), tv, tj, w, flat_hand_mean, seal)
            L = L + (pd * (x + off) ** 2).sum(1)
            for _ in range(int(iterations)):
                d = torch.diagonal(H, dim1=1, dim2=2)
                M = H.clone()
                torch.diagonal(M, dim1=1, dim2=2).add_(pd + lam[:, None] * (d + LM_TRACE_FLOOR * d.sum(1, keepdim=True) / n))
                delta, ok = lm_solve(M, g + pd * (x + off))
                x2 = x + delta
                H2, g2, L2 = _skin_normal(model, *split(x2), tv, tj, w, flat_hand_mean, seal)
                L2 = L2 + (pd * (x2 + off) ** 2).sum(1)
                take = (L2 < L) & (ok != 0) & torch.isfinite(L2)
                x, g, L = torch.where(take[:, None], x2, x), torch.where(take[:, None], g2, g), torch.where(take, L2, L)
                H = torch.where(take[:, None, None], H2, H)
                lam = torch.where(take, (lam / 10).clamp_min(LM_DAMPING_FLOOR), lam * 10)
                accepted += take
        params = [t.contiguous() for t in split(x)]
        verts, joints = _skin(model, *params, flat_hand_mean, seal)
        return _fit_result(params, verts, joints, tv, tj, damping=lam, accepted=accepted)


def fit_two_hands_lm(right, left, target_verts, target_joints=None, init=None, iterations=10, damping=1e-3, vert_weight=None, prior=(0.0, 0.0),
                     flat_hand_mean=False, seal=True):
    """fit_two_hands by fit_hand_lm: the same arguments and stacking, two hands one after the other.  -> fit_two_hands' dict, whose pose, betas and
    trans go into skin_two_hands and posed.mano_sequence unchanged, and damping (P, 2), accepted (P, 2)."""
    return _fit_two(lambda mm, tv, tj, start, w: fit_hand_lm(mm, tv, tj, start, iterations, damping, w, prior, flat_hand_mean, seal),
                    ("pose", "betas", "trans", "rms", "damping", "accepted"), right, left, target_verts, target_joints, init, vert_weight, seal)


__all__ = ["MANO_PARENTS", "MANO_SEAL_RING", "ManoModel", "skin_hand", "skin_two_hands", "fit_hand", "fit_two_hands", "skin_normal_equations", "lm_solve",
           "fit_hand_lm", "fit_two_hands_lm"]
