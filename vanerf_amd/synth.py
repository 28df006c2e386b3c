"""Seeded synthetic frames for tests, smoke() and bench.py (no dataset, no MANO pickle).

Shapes follow what the reference renderer consumes: two closed
genus-0 "hands" of 779 vertices / 1554 faces each (the vertex/face counts of a sealed MANO
hand, reference src/dataset.py:35-52, so NV = 1558, NF = 3108 and the twin-vertex roll of
src/networks.py:30-32 is valid), 42 key points, a 256x256 source image and the three feature
maps the image encoders produce (src/model.py:971-972).
"""
import math

import numpy as np
import torch

NV_HAND = 779
NF_HAND = 1554


def uv_sphere(rings=21, segs=37):
    """Unit sphere, outward CCW winding: rings*segs + 2 vertices, 2*segs*rings faces."""
    verts = [(0.0, 0.0, 1.0)]
    for r in range(1, rings + 1):
        th = math.pi * r / (rings + 1)
        for s in range(segs):
            ph = 2.0 * math.pi * s / segs
            verts.append((math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)))
    verts.append((0.0, 0.0, -1.0))
    faces = []
    ring0 = lambda r: 1 + r * segs
    for s in range(segs):
        faces.append((0, ring0(0) + s, ring0(0) + (s + 1) % segs))
    for r in range(rings - 1):
        for s in range(segs):
            a, b = ring0(r) + s, ring0(r) + (s + 1) % segs
            c, d = ring0(r + 1) + s, ring0(r + 1) + (s + 1) % segs
            faces.append((a, c, d))
            faces.append((a, d, b))
    last = len(verts) - 1
    for s in range(segs):
        faces.append((last, ring0(rings - 1) + (s + 1) % segs, ring0(rings - 1) + s))
    return np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)


def two_hand_mesh(seed=0, radius=0.05, offset=0.04, depth=1.0, bumpy=True):
    """(1558,3) float32 vertices, (3108,3) int64 faces; hand 1 is a translated copy of hand 0's topology."""
    rng = np.random.RandomState(seed)
    sv, sf = uv_sphere()
    assert sv.shape[0] == NV_HAND and sf.shape[0] == NF_HAND
    hands = []
    for h, cx in enumerate((-offset, offset)):
        v = sv.copy()
        if bumpy:  # low-frequency radial displacement keeps the surface closed and star-shaped
            amp = rng.uniform(0.05, 0.15, size=3)
            frq = rng.randint(1, 4, size=3)
            ph = rng.uniform(0, 2 * math.pi, size=3)
            r = 1.0 + amp[0] * np.sin(frq[0] * np.arctan2(v[:, 1], v[:, 0]) + ph[0]) * (1 - v[:, 2] ** 2) \
                + amp[1] * np.sin(frq[1] * math.pi * v[:, 2] + ph[1]) * (1 - v[:, 2] ** 2)
            v = v * r[:, None]
            v = v * np.array([1.0, 1.3, 0.7])
        v = v * radius + np.array([cx, 0.003 * (2 * h - 1), depth])
        hands.append(v)
    verts = np.concatenate(hands, 0).astype(np.float32)
    faces = np.concatenate([sf, sf + NV_HAND], 0)
    return verts, faces


# ---------------------------------------------------------------------------------------------------------------------
# closed meshes that are NOT star-shaped (tests/test_mesh_geometry.py): thin lobes with deep gaps, a handle, a cavity.  All are centred at the
# origin; the tests place them (offset, scale).  Vertices float32, faces int64, outward CCW winding (an inner cavity wall keeps the winding of
# the sphere it copies: a point inside both shells is wound twice and counts as outside by parity).
# ---------------------------------------------------------------------------------------------------------------------
def _fingered(sv, seed):
    phi0 = np.random.RandomState(seed).uniform(0.0, 2.0 * math.pi)
    phi = np.arctan2(sv[:, 1], sv[:, 0])
    r = 0.35 + 0.65 * np.abs(np.cos(2.5 * (phi + phi0))) ** 6 * (1.0 - sv[:, 2] ** 2)
    return sv * r[:, None] * np.array([1.0, 1.0, 0.3]) * 0.07


def fingered_hand(seed=0):
    """(779,3) / (1554,3): the topology of uv_sphere() with radius 0.35 + 0.65 |cos(2.5 (phi + phi0(seed)))|^6 (1 - z^2), flattened by
    (1, 1, 0.3), times 0.07 m -- a palm with five thin lobes and deep gaps between them (the surfaces of two lobes lie millimetres apart)."""
    sv, sf = uv_sphere()
    return _fingered(sv, seed).astype(np.float32), sf.copy()


def two_fingered_hands(seed=0):
    """(1558,3) / (3108,3): two fingered hands 6 cm apart along x -- the counts of two_hand_mesh, so the mesh can stand in a frame.  Lobes of the
    two hands may interpenetrate; a point inside both is outside by parity."""
    sv, sf = uv_sphere()
    hands = [_fingered(sv, 2 * seed + h) + np.array([cx, 0.0, 0.0]) for h, cx in enumerate((-0.03, 0.03))]
    return np.concatenate(hands, 0).astype(np.float32), np.concatenate([sf, sf + NV_HAND], 0)


def fingered_hand_fine(seed=0):
    """(2402,3) / (4800,3): the fingered hand on uv_sphere(40, 60) (the accelerated query's LDS tables exceed the 64 KB default limit)."""
    sv, sf = uv_sphere(40, 60)
    return _fingered(sv, seed).astype(np.float32), sf


def torus(n_major=48, n_minor=20, major=1.0, minor=0.3):
    """(n_major * n_minor, 3) / (2 * n_major * n_minor, 3): a torus about the z axis (genus 1, not star-shaped); 960 / 1 920 by default."""
    u = 2.0 * math.pi * np.arange(n_major) / n_major
    v = 2.0 * math.pi * np.arange(n_minor) / n_minor
    uu, vv = np.meshgrid(u, v, indexing="ij")
    rad = major + minor * np.cos(vv)
    verts = np.stack([rad * np.cos(uu), rad * np.sin(uu), minor * np.sin(vv)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % n_major) * n_minor + (j % n_minor)
    faces = []
    for i in range(n_major):
        for j in range(n_minor):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces.append((a, b, c))
            faces.append((a, c, d))
    return verts.astype(np.float32), np.asarray(faces, dtype=np.int64)


def nested_shells():
    """(244,3) / (480,3): uv_sphere(10, 12) and a copy of it scaled 0.55 and shifted by (0.1, 0.05, 0) inside it.  The inner cavity is outside."""
    sv, sf = uv_sphere(10, 12)
    inner = sv * 0.55 + np.array([0.1, 0.05, 0.0])
    return np.concatenate([sv, inner], 0).astype(np.float32), np.concatenate([sf, sf + sv.shape[0]], 0)


def mano_like_model(seed, nv=778, nj=16, nb=10, parents=None):
    """A seeded model of MANO's shapes for vanerf_amd.mano (no licensed file): a dict of numpy arrays under smplx's names, ready for
    ManoModel.from_arrays(**model).  v_template (nv, 3): the points of fingered_hand(seed) (past 779 they repeat, shifted by a millimetre per
    round); shapedirs (nv, 3, nb) with sigma 2 mm and posedirs ((nj-1)*9, nv*3) with sigma 1 mm; J_regressor (nj, nv): per joint up to eight
    vertices with non-negative weights that sum to 1; weights (nv, nj): per vertex up to four joints, likewise; hands_mean ((nj-1)*3) with
    sigma 0.2 rad.  parents: default the wrist with fingers of three joints each, parents[j] = 0 if (j - 1) % 3 == 0 else j - 1, which is
    MANO's tree at nj = 16."""
    rng = np.random.RandomState(seed)
    base, _ = fingered_hand(seed)
    i = np.arange(nv)
    v_template = (base[i % NV_HAND].astype(np.float64) + 1e-3 * (i // NV_HAND)[:, None]).astype(np.float32)
    shapedirs = (2e-3 * rng.standard_normal((nv, 3, nb))).astype(np.float32)
    posedirs = (1e-3 * rng.standard_normal(((nj - 1) * 9, nv * 3))).astype(np.float32)
    J_regressor = np.zeros((nj, nv), dtype=np.float64)
    for j in range(nj):
        ids = rng.choice(nv, size=min(8, nv), replace=False)
        J_regressor[j, ids] = rng.dirichlet(np.ones(len(ids)))
    weights = np.zeros((nv, nj), dtype=np.float64)
    for v in range(nv):
        ids = rng.choice(nj, size=min(4, nj), replace=False)
        weights[v, ids] = rng.dirichlet(np.ones(len(ids)))
    hands_mean = (0.2 * rng.standard_normal((nj - 1) * 3)).astype(np.float32)
    if parents is None:
        parents = [-1] + [0 if (j - 1) % 3 == 0 else j - 1 for j in range(1, nj)]
    return {"v_template": v_template, "shapedirs": shapedirs, "posedirs": posedirs, "J_regressor": J_regressor.astype(np.float32),
            "weights": weights.astype(np.float32), "parents": np.asarray(parents, dtype=np.int32), "hands_mean": hands_mean}


def look_at_extrinsic(eye, target, up=(0.0, -1.0, 0.0)):
    """World->camera 4x4 (x right, y down, z forward)."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 0)
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ eye
    return E.astype(np.float32)


def make_frame(seed=0, tar_h=64, tar_w=64, src_hw=256, orbit_deg=8.0, device="cpu", half_mask=False,
               focal_src=1500.0):
    """One synthetic frame: dict with every tensor `batch_render_pifu_nerf` needs (B = V = 1).

    Keys mirror the reference call (src/model.py:1102-1120, 313-317, 345-349):
      img_in (1,3,256,256), feat_geo [(1,64,32,32),(1,8,128,128)], feat_tex (1,8,64,64),
      cam_in, cam_tar, targets{vert_world, face_world, tar_cam}, sp_data{extrin,kpt3d},
      src_foreground_mask (1,1,1,256,256), bounds (1,2,3).
    """
    g = torch.Generator().manual_seed(seed)
    verts_np, faces_np = two_hand_mesh(seed)
    verts = torch.from_numpy(verts_np)[None]
    faces = torch.from_numpy(faces_np)[None].float()  # reference passes faces as float and calls .long()
    centre = verts[0].mean(0)

    kpts = []
    for h in range(2):
        c = verts[0, h * NV_HAND:(h + 1) * NV_HAND].mean(0)
        kpts.append(c[None] + 0.03 * torch.randn(21, 3, generator=g))
    kpt3d = torch.cat(kpts, 0)[None]

    znear, zfar = 0.71, 1.42
    # source camera: identity extrinsic, principal point at the image centre
    K_src = torch.eye(4)
    K_src[0, 0] = K_src[1, 1] = focal_src
    K_src[0, 2] = K_src[1, 2] = src_hw / 2.0
    E_src = torch.eye(4)
    cam_in = {
        "KRT": (K_src @ E_src)[None], "K": K_src[None], "Rt": E_src[None, :3, :4], "extrin": E_src[None],
        "znear": znear, "zfar": zfar, "width": src_hw, "height": src_hw, "nml_scale": 100.0,
    }
    # target camera: orbit about the scene centre
    ang = math.radians(orbit_deg)
    dist = float(centre[2])
    eye = np.array([centre[0].item() + dist * math.sin(ang), centre[1].item() - 0.02, centre[2].item() - dist * math.cos(ang)])
    E_tar = torch.from_numpy(look_at_extrinsic(eye, centre.numpy()))
    K_tar = torch.eye(4)
    f_tar = focal_src * tar_w / src_hw * 0.9
    K_tar[0, 0] = K_tar[1, 1] = f_tar
    K_tar[0, 2] = tar_w / 2.0
    K_tar[1, 2] = tar_h / 2.0
    cam_tar = {
        "K": K_tar[None], "RT": E_tar[None], "KRT": (K_tar @ E_tar)[None],
        "width": tar_w, "height": tar_h, "nml_scale": 100.0, "znear": znear, "zfar": zfar,
    }
    bmin = verts[0].min(0)[0].clone()
    bmax = verts[0].max(0)[0].clone()
    bmin[2] -= 0.05
    bmax[2] += 0.05
    bounds = torch.stack([bmin, bmax], 0)[None]

    img = torch.rand(1, 3, src_hw, src_hw, generator=g)
    mask = torch.ones(1, 1, 1, src_hw, src_hw)
    if half_mask:
        mask[..., : src_hw // 2 - 9] = 0.0
    feat_geo = [torch.rand(1, 64, 32, 32, generator=g) * 2 - 1, torch.rand(1, 8, 128, 128, generator=g) * 2 - 1]
    feat_tex = torch.rand(1, 8, 64, 64, generator=g) * 2 - 1
    targets = {
        "vert_world": verts, "face_world": faces,
        "tar_cam": {"tar_R": E_tar[None, :3, :3], "tar_T": E_tar[None, :3, 3],
                    "tar_focal": torch.tensor([[f_tar, f_tar]]), "tar_princpt": torch.tensor([[tar_w / 2.0, tar_h / 2.0]])},
    }
    frame = {
        "img_in": img, "feat_geo": feat_geo, "feat_tex": feat_tex, "cam_in": cam_in, "cam_tar": cam_tar,
        "targets": targets, "sp_data": {"extrin": E_src[None].clone(), "kpt3d": kpt3d},
        "src_foreground_mask": mask, "bounds": bounds, "hand_type": torch.ones(1, 2),
    }
    return to_device(frame, device)


def pose_source_camera(frame, yaw, pitch, roll, dist, focal_xy, princpt):
    """A copy of `frame` whose SOURCE camera is posed and off-centre (make_frame's is the identity with the principal point at the image
    centre and one focal length, which hides a transposed rotation, a dropped translation and an x/y swap): it looks at the mesh centre from
    `dist` away, eye = centre + dist (sin yaw cos pitch, sin pitch, -cos yaw cos pitch), then rolls about its optical axis,
    E = Rz(roll) @ look_at; angles in degrees, focal_xy = (fx, fy) and princpt = (cx, cy) in source pixels.  cam_in's KRT / K / Rt / extrin
    and sp_data's extrin are replaced consistently; every other entry is shared with `frame` and the source view stays 256 x 256."""
    dev = frame["cam_in"]["KRT"].device
    centre = frame["targets"]["vert_world"][0].mean(0).cpu().numpy().astype(np.float64)
    a, b, r = math.radians(yaw), math.radians(pitch), math.radians(roll)
    eye = centre + dist * np.array([math.sin(a) * math.cos(b), math.sin(b), -math.cos(a) * math.cos(b)])
    Rz = np.eye(4)
    Rz[:2, :2] = [[math.cos(r), -math.sin(r)], [math.sin(r), math.cos(r)]]
    E = torch.from_numpy((Rz @ look_at_extrinsic(eye, centre).astype(np.float64)).astype(np.float32))
    K = torch.eye(4)
    K[0, 0], K[1, 1] = float(focal_xy[0]), float(focal_xy[1])
    K[0, 2], K[1, 2] = float(princpt[0]), float(princpt[1])
    E, K = E.to(dev), K.to(dev)
    out = dict(frame)
    out["cam_in"] = dict(frame["cam_in"], KRT=(K @ E)[None], K=K[None], Rt=E[None, :3, :4], extrin=E[None])
    out["sp_data"] = dict(frame["sp_data"], extrin=E[None].clone())
    return out


# the two posed source cameras of tests/test_posed_source.py and of the reference fixtures tests/golden/*_posed.npz (oracle/gen_golden.py)
SOURCE_POSES = {"A": dict(yaw=25.0, pitch=-10.0, roll=12.0, dist=1.05, focal_xy=(1150.0, 1230.0), princpt=(101.0, 149.0)),
                "B": dict(yaw=-40.0, pitch=20.0, roll=-35.0, dist=1.05, focal_xy=(1100.0, 1100.0), princpt=(140.0, 110.0))}


def p3d_tar_cam(cam_tar):
    """targets['tar_cam'] in pytorch3d's convention, as the reference's dataset builds it from the OpenCV target camera
    (src/dataset.py:501-503): tar_R = (F R_cv)^T, tar_T = F t_cv with F = diag(-1, -1, 1); focal and principal point from K.
    render_vis with this camera registers with cam_tar["KRT"]."""
    RT, K = cam_tar["RT"], cam_tar["K"]
    flip = torch.tensor([-1.0, -1.0, 1.0], dtype=RT.dtype, device=RT.device)
    return {"tar_R": (flip[:, None] * RT[:, :3, :3]).transpose(1, 2).contiguous(), "tar_T": (flip * RT[:, :3, 3]).contiguous(),
            "tar_focal": torch.stack([K[:, 0, 0], K[:, 1, 1]], 1), "tar_princpt": torch.stack([K[:, 0, 2], K[:, 1, 2]], 1)}


def to_tr_batch(frame):
    """The dict VANeRFLightningModule.decode_batch hands to the renderer (reference src/model.py:213-262), filled from a synthetic frame."""
    return {"im": frame["img_in"], "cam": frame["cam_in"], "hand_type": frame["hand_type"], "targets": frame["targets"], "sp_data": frame["sp_data"],
            "src_foreground_mask": frame["src_foreground_mask"],
            "dr_data": {"tar": None, "cam_tar": frame["cam_tar"], "objcenter": None, "bounds": frame["bounds"], "mask_at_box": None}}


def to_device(obj, device):
    if isinstance(obj, torch.Tensor):
        return obj.to(device)
    if isinstance(obj, dict):
        return {k: to_device(v, device) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(to_device(v, device) for v in obj)
    return obj


# state_dict keys / shapes of the per-sample networks (reference VANeRF.state_dict(), shipped config)
HOT_SHAPES = {
    "sigmoid_beta": (1,),
    "geo_vis_fusion.fconv_at.0.weight": (10, 196, 1), "geo_vis_fusion.fconv_at.2.weight": (3, 10, 1),
    "geo_vis_fusion.fconv_ated.0.weight": (64, 196, 1), "geo_vis_fusion.fconv_ated.2.weight": (64, 64, 1),
    "geo_vis_fusion.fconv_at1.0.weight": (10, 28, 1), "geo_vis_fusion.fconv_at1.2.weight": (3, 10, 1),
    "geo_vis_fusion.fconv_ated1.0.weight": (8, 28, 1), "geo_vis_fusion.fconv_ated1.2.weight": (8, 8, 1),
    "tex_vis_fusion.fconv.0.weight": (96, 96, 1), "tex_vis_fusion.fconv.2.weight": (40, 96, 1),
    "tex_vis_fusion.fconv_at.0.weight": (96, 96, 1), "tex_vis_fusion.fconv_at.2.weight": (6, 96, 1),
    "ibr_compress_gfeat.weight": (24, 128), "ibr_compress_gfeat.bias": (24,),
    "mlp_geo.layers1.layers.0.linear.weight_v": (128, 358), "mlp_geo.layers1.layers.1.linear.weight_v": (128, 128),
    "mlp_geo.layers1.layers.2.linear.weight_v": (120, 136), "mlp_geo.layers1.layers.3.linear.weight": (64, 120),
    "mlp_geo.layers2.layers.0.linear.weight_v": (64, 128), "mlp_geo.layers2.layers.1.linear.weight_v": (64, 64),
    "mlp_geo.layers2.layers.2.linear.weight": (2, 64),
}


def make_hot_weights(seed=0):
    """'Trained-like' random weights for the per-sample networks: activations are O(0.1-1) at every layer, both
    sides of every ReLU / Softplus knee / validity branch are exercised and the density head produces alpha > 0 for
    roughly half of the samples.  (The reference's own init leaves alpha == 0 everywhere and colours ~1e-2, which
    would make a 1e-4 absolute parity bar meaningless.)  Returns {state_dict key: fp32 tensor}."""
    g = torch.Generator().manual_seed(1000 + seed)
    sd = {}
    for k, shp in HOT_SHAPES.items():
        if k == "sigmoid_beta":
            sd[k] = torch.full(shp, 0.1)
            continue
        fan_in = shp[1] if len(shp) > 1 else shp[0]
        if k.endswith("bias"):
            sd[k] = 0.05 * torch.randn(shp, generator=g)
        else:
            sd[k] = torch.randn(shp, generator=g) * math.sqrt(2.0 / fan_in)
    for k in list(sd):
        if k.endswith("weight_v"):
            base = k[: -len("weight_v")]
            sd[base + "weight_g"] = 0.25 + 0.5 * torch.rand(sd[k].shape[0], 1, generator=g)
            sd[base + "bias"] = 0.04 * torch.randn(sd[k].shape[0], generator=g)
    sd["mlp_geo.layers1.layers.3.linear.weight"] *= 0.7
    sd["mlp_geo.layers1.layers.3.linear.bias"] = 0.05 * torch.randn(64, generator=g)
    for i in (0, 1):  # the pooled latent is small (mean ~0.05, variance ~1e-3): give the density head some gain
        sd[f"mlp_geo.layers2.layers.{i}.linear.weight_g"] = 2.0 + 2.0 * torch.rand(64, 1, generator=g)
        sd[f"mlp_geo.layers2.layers.{i}.linear.bias"] = 0.1 * torch.randn(64, generator=g)
    w_last = sd["mlp_geo.layers2.layers.2.linear.weight"]
    w_last -= w_last.mean(1, keepdim=True)  # inputs are post-softplus (positive): zero-mean rows keep rad centred
    sd["mlp_geo.layers2.layers.2.linear.weight"] = w_last * 1.2
    sd["mlp_geo.layers2.layers.2.linear.bias"] = torch.tensor([0.28, -0.47])
    sd["geo_vis_fusion.fconv_at.2.weight"] *= 2.0
    sd["geo_vis_fusion.fconv_at1.2.weight"] *= 2.0
    sd["tex_vis_fusion.fconv_at.2.weight"] *= 2.0
    sd["tex_vis_fusion.fconv.2.weight"] *= 0.6
    return sd


def make_texframe_weights():
    """Per-frame TexVisFusion conv stack with the reference's init recipe (src/model.py:669-698): torch.manual_seed(125)
    before each module, normal_(0, 0.02); LayerNorm affine = (1, 0)."""
    shapes = {"fconv_gt.0.weight": (779, 42, 3), "fconv_gt.3.weight": (1558, 779, 3), "fconv3.0.weight": (21, 8, 3, 3),
              "fconv3.3.weight": (42, 21, 3, 3), "fconv4.0.weight": (21, 3, 3, 3), "fconv4.3.weight": (42, 21, 3, 3)}
    ln = {"fconv_gt.1": (18,), "fconv_gt.4": (18,), "fconv3.1": (64, 64), "fconv3.4": (64, 64), "fconv4.1": (256, 256), "fconv4.4": (256, 256)}
    sd = {}
    state = torch.get_rng_state()
    for k, s in shapes.items():
        torch.manual_seed(125)
        sd["tex_vis_fusion." + k] = torch.empty(s).normal_(0.0, 0.02)
    torch.set_rng_state(state)
    for k, s in ln.items():
        sd[f"tex_vis_fusion.{k}.weight"] = torch.ones(s)
        sd[f"tex_vis_fusion.{k}.bias"] = torch.zeros(s)
    return sd


def make_full_weights(seed=0):
    sd = make_hot_weights(seed)
    sd.update(make_texframe_weights())
    sd.update(make_ibr_weights(seed))
    return sd


IBR_SHAPES = {
    "ray_encoder.0": (16, 4), "ray_encoder.2": (40, 16), "base_layer.0": (64, 120), "base_layer.2": (32, 64),
    "vis_layer1.0": (32, 32), "vis_layer1.2": (33, 32), "vis_layer2.0": (32, 32), "vis_layer2.2": (1, 32),
    "out_layer.0": (16, 37), "out_layer.2": (8, 16), "out_layer.4": (1, 8),
}


def make_ibr_weights(seed=0):
    """IBRRenderingHead parameters (src/model.py:1575-1591).  At V = 1 the head returns rgb_feat[..., :3] exactly
    (softmax over one view), so these only matter to the oracle's restatement and to state_dict completeness."""
    g = torch.Generator().manual_seed(2000 + seed)
    sd = {"mlp_tex.ani_al": torch.tensor(0.2)}
    for k, (o, i) in IBR_SHAPES.items():
        sd[f"mlp_tex.{k}.weight"] = torch.randn(o, i, generator=g) * math.sqrt(2.0 / i)
        sd[f"mlp_tex.{k}.bias"] = torch.zeros(o)
    return sd


# ---------------------------------------------------------------------------------------------------------------------
# weight families: the same keys and shapes as make_full_weights, other kinds of numbers (tests/test_weight_families.py)
# ---------------------------------------------------------------------------------------------------------------------
# the state_dict entries the packed weight streams are built from (VANeRF._PACKED_PREFIXES is this tuple)
PACKED_PREFIXES = ("geo_vis_fusion.", "mlp_geo.", "ibr_compress_gfeat.", "tex_vis_fusion.fconv.", "tex_vis_fusion.fconv_at.", "sigmoid_beta")
WEIGHT_FAMILIES = ("wide", "ties", "sparse", "gains")
WIDE_DECADES = 6.0
# two planted magnitudes per row.  2^-130 (1 + 2^-4 + 2^-9): an fp32 subnormal; its high bf16 part is a bf16 subnormal (step 2^-133) and the
# remainder lies below half a step, so its low part is +-0.  2^-121 (1 + 2^-4 + 2^-9): normal, high part 2^-121 + 2^-125 (step 2^-128), low
# part 2^-130: a bf16 subnormal that is not zero -- a packer that flushes subnormals loses it.
WIDE_TINY = (2.0 ** -130 * (1.0 + 2.0 ** -4 + 2.0 ** -9), 2.0 ** -121 * (1.0 + 2.0 ** -4 + 2.0 ** -9))
SPARSE_ZERO_SHARE = 0.9
GAINS_RANGE = (0.05, 30.0)
GAINS_BETAS = (0.5, 0.02, 1e-3)  # by seed % 3; the last lies below sdf_activation's clamp (2e-3)
_HEAD_BIAS = "mlp_geo.layers2.layers.2.linear.bias"
# rad = W x + b of the density head re-centred per family and seed: minus the median of W x over the valid samples of the posed test
# frame (fp64 oracle, 2 000 points near the mesh of pose A; tests/test_weight_families.py asserts the share of alpha > 0 this gives).
# A seed without an entry is refused: its share of alpha > 0 is not assured until an entry is tuned for it.
_HEAD_RAD_BIAS = {"wide": (0.9011, -0.2202, 0.0395), "ties": (-0.5902, 0.3138, 0.1246), "sparse": (-0.2520, 0.0704, 0.1943),
                  "gains": (-3339.3, 2084.8, 1438.4)}


def _family_matrices(sd):
    """The packed entries that are matrices (conv / linear weights, weight-norm directions) and those that are biases."""
    packed = [k for k in sd if k.startswith(PACKED_PREFIXES)]
    return [k for k in packed if k.endswith(("weight", "weight_v"))], [k for k in packed if k.endswith("bias")]


def _norm_as_packed(v):
    """||v|| of every row as the packers compute it: the squares summed in double in index order, the root rounded to fp32."""
    return v.double().pow(2).cumsum(1)[:, -1].sqrt().float()


def sparse_zero_lines(shape, weight_norm):
    """How many all-zero output rows / input columns the 'sparse' family gives a matrix: two of each; fewer rows where two would leave
    nothing (one of 3 rows, none of 2), and no zero row in a weight-norm direction (its norm divides)."""
    rows = 0 if weight_norm else max(0, min(2, shape[0] - 2))
    return rows, 2


def make_weight_family(name, seed=0, sigmoid_beta=None):
    """make_full_weights(seed) with the entries of the packed streams (PACKED_PREFIXES) rewritten, same keys and shapes, fp32:

    "wide"   magnitudes log-uniform over WIDE_DECADES decades within every matrix (|w| in [1e-6 s, s], the recipe's signs, s chosen to
             keep the matrix's root mean square), two elements per row at +-WIDE_TINY: an fp32 subnormal, and a small normal number whose low bf16
             part is a subnormal.
    "ties"   every weight and bias snapped to a value whose bf16 rounding is a decision -- by element index mod 3: exactly half-way
             between two bf16 neighbours (low half 0x8000; both parities of the lower neighbour occur); one fp32 ulp either side of such
             a tie (0x7fff / 0x8001); a bf16 significand of all ones below a tie or above it (0x..7f8000 / 0x..7fffff), so that the
             rounding carries into the next exponent.  Weight-norm rows are first scaled to the recipe's folded size and get
             weight_g = ||v|| as the packers compute it: the fold multiplies by exactly 1 and the folded value is the snapped one.
    "sparse" SPARSE_ZERO_SHARE exact zeros (an eighth of them -0.0), exactly sparse_zero_lines() all-zero output rows and input columns per
             matrix (every other row and column keeps a value), the remaining values scaled by (1 - share)^-1/4 (half of what would keep the
             variance: the fp32 oracle itself misses 1e-4 on rad at the full factor); half the biases 0.
    "gains"  the recipe's matrices with weight_g log-uniform over GAINS_RANGE per row and sigmoid_beta = GAINS_BETAS[seed % 3] (or the
             argument).
    In every family the density head's second bias is re-centred (_HEAD_RAD_BIAS) so that alpha > 0 on a share of the samples."""
    if name not in WEIGHT_FAMILIES:
        raise ValueError(f"weight family must be one of {WEIGHT_FAMILIES}")
    if not 0 <= seed < len(_HEAD_RAD_BIAS[name]):
        raise ValueError(f"weight family {name!r} has a tuned density-head bias for seeds 0..{len(_HEAD_RAD_BIAS[name]) - 1} only")
    sd = make_full_weights(seed)
    g = torch.Generator().manual_seed(3000 + 10 * seed + WEIGHT_FAMILIES.index(name))
    mats, biases = _family_matrices(sd)
    for k in mats:
        w = sd[k]
        m = w.reshape(w.shape[0], -1).clone()
        wn = k.endswith("weight_v")
        if name == "wide":
            s = m.pow(2).mean().sqrt() * math.sqrt(2.0 * WIDE_DECADES * math.log(10.0))  # E w^2 of the log-uniform law is s^2 / (2 D ln 10)
            sign = torch.where(m < 0, -1.0, 1.0)
            m = sign * s * 10.0 ** (-WIDE_DECADES * torch.rand(m.shape, generator=g))
            rows = torch.arange(m.shape[0])
            col = torch.randint(0, m.shape[1], (m.shape[0],), generator=g)
            for c, tiny in ((col, WIDE_TINY[0]), ((col + 1 + torch.randint(0, m.shape[1] - 1, col.shape, generator=g)) % m.shape[1], WIDE_TINY[1])):
                m[rows, c] = sign[rows, c] * tiny
        elif name == "ties":
            if wn:
                m = m * (sd[k[:-1] + "g"].reshape(-1, 1) / m.norm(2, dim=1, keepdim=True))
            m = _snap_to_ties(m)
            if wn:
                sd[k[:-1] + "g"] = _norm_as_packed(m).reshape(-1, 1)
        elif name == "sparse":
            keep = torch.rand(m.shape, generator=g) >= SPARSE_ZERO_SHARE
            n_rows, n_cols = sparse_zero_lines(m.shape, wn)
            rows = torch.randperm(m.shape[0], generator=g)[:n_rows]
            cols = torch.randperm(m.shape[1], generator=g)[:n_cols]
            keep[rows] = False
            keep[:, cols] = False
            # no other empty row or column (a weight-norm row must keep a norm; and the counts are then exact): one value put back
            live_r = torch.ones(m.shape[0], dtype=torch.bool)
            live_c = torch.ones(m.shape[1], dtype=torch.bool)
            live_r[rows], live_c[cols] = False, False
            live_r, live_c = live_r.nonzero().view(-1), live_c.nonzero().view(-1)
            for r in live_r[~keep[live_r].any(1)]:
                keep[r, live_c[torch.randint(0, live_c.numel(), (1,), generator=g)]] = True
            for c in live_c[~keep[:, live_c].any(0)]:
                keep[live_r[torch.randint(0, live_r.numel(), (1,), generator=g)], c] = True
            zero = torch.where(torch.rand(m.shape, generator=g) < 0.125, -0.0, 0.0)
            m = torch.where(keep, m * (1.0 - SPARSE_ZERO_SHARE) ** -0.25, zero)
        sd[k] = m.reshape(w.shape).contiguous()
    for k in biases:
        if name == "ties":
            sd[k] = _snap_to_ties(sd[k].reshape(1, -1)).reshape(-1)
        elif name == "sparse":
            b = sd[k].clone()
            zero = torch.randperm(b.numel(), generator=g)[: (b.numel() + 1) // 2]
            b[zero] = 0.0
            b[zero[::4]] = -0.0
            sd[k] = b
    if name == "gains":
        lo, hi = GAINS_RANGE
        for k in [k for k in sd if k.endswith("weight_g")]:
            sd[k] = lo * (hi / lo) ** torch.rand(sd[k].shape, generator=g)
        sd["sigmoid_beta"] = torch.tensor([GAINS_BETAS[seed % 3] if sigmoid_beta is None else sigmoid_beta])
    elif sigmoid_beta is not None:
        sd["sigmoid_beta"] = torch.tensor([float(sigmoid_beta)])
    head = sd[_HEAD_BIAS].clone()
    head[1] = _HEAD_RAD_BIAS[name][seed]
    sd[_HEAD_BIAS] = _snap_to_ties(head.reshape(1, -1)).reshape(-1) if name == "ties" else head
    return sd


def _snap_to_ties(m):
    """fp32 values of (rows, n) -> a 'bf16 rounding is a decision' pattern just above the value cut to bf16 (kinds 0, 1) or just below its
    power of two (kind 2: magnitudes shrink, activations stay in the recipe's range), by column index mod 3, and the row's parity for the
    side: 0 an exact tie, 1 a tie -+ one fp32 ulp, 2 an all-ones bf16 significand at / above the tie (the rounding carries)."""
    bits = m.contiguous().view(torch.int32).clone()
    top = bits & ~0xffff  # sign, exponent and the seven significand bits a bf16 keeps (truncated)
    tiny = (top & 0x7f800000) == 0
    top = torch.where(tiny, (top & ~0x7fffffff) | 0x3c000000, top)  # (nothing smaller than 2^-7: zeros / subnormals have no tie to speak of)
    kind = (torch.arange(m.shape[1]) % 3)[None].expand_as(bits)
    side = ((torch.arange(m.shape[0])[:, None] + torch.arange(m.shape[1])[None] // 3) % 2).expand_as(bits)
    low = torch.where(kind == 0, 0x8000, torch.where(kind == 1, torch.where(side == 0, 0x7fff, 0x8001), torch.where(side == 0, 0x8000, 0xffff)))
    top = torch.where(kind == 2, (top - 0x00800000) | 0x007f0000, top)  # the binade below, all ones: rounds up to the value's own power of two
    return (top | low.to(torch.int32)).view(torch.float32)
