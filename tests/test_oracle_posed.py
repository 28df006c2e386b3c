"""The CPU oracle under posed, off-centre source cameras (synth.pose_source_camera), and the helpers tests/test_posed_source.py shares.

Every other fixture and test renders from make_frame's source camera: identity extrinsic, principal point at the image centre, one focal
length.  With it R == R^T and t == 0 in `extrin`, KRT's fourth column is zero, kpt_cam == kpt3d and fx == fy, cx == cy: a transposed
rotation, a dropped translation or an x/y swap changes nothing.  The two poses of synth.SOURCE_POSES break every one of these symmetries:

  pose | yaw, pitch, roll (deg) | fx, fy     | cx, cy
  A    |  25, -10,  12          | 1150, 1230 | 101, 149
  B    | -40,  20, -35          | 1100, 1100 | 140, 110

(camera 1.05 from the mesh centre, looking at it, rolled about its optical axis).  Here: the oracle reproduces the reference's own query
and whole pass on pose A (tests/golden/query_posed.npz, pass_16x16_s16_posed.npz, written by `python -m oracle.gen_golden --posed`) under the
host-independent criterion of tests/oracle_criterion.py, floored at the tolerances of tests/test_oracle_golden.py; its fp32 and fp64 evaluations agree on both poses; and the pose is visible in its outputs, so
that the GPU tests which take it as their reference cannot pass vacuously."""
import math

import pytest
import torch

from oracle import vanerf_oracle as orc
from tests.oracle_criterion import both, hold, hold_pass, remarch64, ulp32
from tests.test_hip_parity import _points_near_mesh as near_mesh_points  # (oracle/gen_golden.py draws query_posed.npz's points the same way)
from tests.test_oracle_fp64 import cast, reference
from tests.test_oracle_golden import _texframe_weights
from vanerf_amd import synth

POSES = (("A", 3), ("B", 5))  # pose name, frame seed (half of the source view masked in both)
N_POINTS = 2048 + 5


def posed_frame(pose, seed, hw=64, half=True):
    return synth.pose_source_camera(synth.make_frame(seed=seed, tar_h=hw, tar_w=hw, half_mask=half), **synth.SOURCE_POSES[pose])


def mesh_queries(frame, pts):
    """The oracle's discrete inputs of the per-sample pass: q_sdf (n,), q_vis (n,) bool, vert_vis (NV,)."""
    verts = frame["targets"]["vert_world"]
    xy01, z01 = orc.source_vert_xyz01(verts, frame["cam_in"])
    q_sdf, q_vis, vert_vis, _ = orc.cal_vis_sdf_batch(verts, frame["targets"]["face_world"].long(), pts[None], xy01, z01)
    return q_sdf[0], q_vis[0, :, 0], vert_vis[0, :, 0]


def decision_margins(frame, pts):
    """fp64 distance of every point to the validity decisions of VANeRF.query (src/model.py:789-803): |x|, |y| <= 1.01, z >= -1, fg > 0.1.
    Returns (margin (n,), xy (n, 2), z (n,), fg (n,)), all float64."""
    fr = cast(frame, torch.float64)
    xy, z = orc.project(pts.double()[None], fr["cam_in"])
    fg = orc.feat_sample(fr["src_foreground_mask"].view(1, 1, *fr["src_foreground_mask"].shape[-2:]), xy)[0, :, 0]
    xy, z = xy[0], z[0, :, 0]
    m = torch.minimum((1.01 - xy.abs()).abs().min(-1)[0], torch.minimum((z + 1.0).abs(), (fg - 0.1).abs()))
    return m, xy, z, fg


def border_band_points(frame):
    """32 points whose source-view x or y lands in (1.0, 1.01) or (-1.01, -1.0) -- beyond the last pixel centre, inside the eps band of the
    validity test, where every bilinear gather clamps onto the border -- at depths inside [znear, zfar]: un-projected through the frame's
    source camera in fp64 (pixel (u, v) at depth d -> world R^T (d K^-1 (u, v, 1) - t)), then rounded to fp32."""
    cam = frame["cam_in"]
    K, E = cam["K"][0].double(), cam["extrin"][0].double()
    W, H = float(cam["width"]), float(cam["height"])
    pts = []
    for axis in (0, 1):
        for sign in (1.0, -1.0):
            for i in range(8):
                band = sign * (1.002 + 0.006 * (i % 2))
                other = (-0.55, -0.1, 0.35, 0.8)[i // 2]
                ndc = (band, other) if axis == 0 else (other, band)
                u, v = 0.5 * (ndc[0] + 1.0) * (W - 1.0), 0.5 * (ndc[1] + 1.0) * (H - 1.0)
                d = (0.93, 1.0, 1.08, 1.17)[(i + axis) % 4]
                c = d * (torch.inverse(K[:3, :3]) @ torch.tensor([u, v, 1.0], dtype=torch.float64))
                pts.append(E[:3, :3].t() @ (c - E[:3, 3]))
    return torch.stack(pts).float().contiguous()


@pytest.fixture(scope="module")
def sd_full(golden, hot_weights):
    sd = dict(hot_weights)
    sd.update(_texframe_weights(golden))
    return sd


@pytest.fixture(scope="module")
def evaluations(sd_full):
    """Per pose: the frame, the points, and the oracle's per-sample pass in fp64 and fp32 (computed once for this module)."""
    out = {}
    for pose, seed in POSES:
        frame = posed_frame(pose, seed)
        pts = near_mesh_points(frame, N_POINTS, seed=2)
        q_sdf, q_vis, vert_vis = mesh_queries(frame, pts)
        out[pose] = dict(frame=frame, pts=pts, q=(q_sdf, q_vis, vert_vis), r64=reference(sd_full, frame, pts, q_sdf, q_vis, vert_vis),
                         r32=reference(sd_full, frame, pts, q_sdf, q_vis, vert_vis, dtype=torch.float32))
    return out


def test_pose_source_camera_replaces_the_camera_and_nothing_else():
    base = synth.make_frame(seed=3, tar_h=64, tar_w=64, half_mask=True)
    fr = synth.pose_source_camera(base, **synth.SOURCE_POSES["A"])
    cam, E = fr["cam_in"], fr["cam_in"]["extrin"][0]
    assert torch.equal(base["cam_in"]["extrin"][0], torch.eye(4)) and torch.equal(base["sp_data"]["extrin"][0], torch.eye(4))  # a copy
    for k in base:
        if k not in ("cam_in", "sp_data"):
            assert fr[k] is base[k], k
    assert all(fr["cam_in"][k] is base["cam_in"][k] or fr["cam_in"][k] == base["cam_in"][k] for k in ("znear", "zfar", "width", "height", "nml_scale"))
    assert fr["sp_data"]["kpt3d"] is base["sp_data"]["kpt3d"] and cam["width"] == cam["height"] == 256
    assert torch.equal(fr["sp_data"]["extrin"], cam["extrin"]) and torch.equal(cam["Rt"][0], E[:3, :4]) and torch.equal(cam["KRT"][0], cam["K"][0] @ E)
    R, t = E[:3, :3].double(), E[:3, 3].double()
    assert (R @ R.t() - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6 and abs(torch.det(R).item() - 1.0) < 1e-6
    assert (R - R.t()).abs().max() > 0.1 and t.abs().min() > 0.05  # neither symmetric nor at the origin
    K = cam["K"][0]
    assert (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) == (1150.0, 1230.0, 101.0, 149.0) and cam["KRT"][0, :3, 3].abs().min() > 0.1
    centre = base["targets"]["vert_world"][0].mean(0).double()
    c_cam = R @ centre + t  # the camera looks at the mesh centre from 1.05 away
    assert c_cam[:2].abs().max() < 1e-6 and abs(c_cam[2].item() - 1.05) < 1e-6
    a, b = math.radians(25.0), math.radians(-10.0)
    eye = centre + 1.05 * torch.tensor([math.sin(a) * math.cos(b), math.sin(b), -math.cos(a) * math.cos(b)], dtype=torch.float64)
    assert (-R.t() @ t - eye).abs().max() < 1e-6


def test_query_posed_vs_reference(golden, sd_full):
    """VANeRF.query of the reference on pose A (tests/golden/query_posed.npz) under the criterion of tests/oracle_criterion.py, floor 2e-6
    (test_query_whole's tolerance).  `extrin` is the golden's bit for bit.  KRT = K @ E is an fp32 matmul of the host: each entry must lie
    of the golden's within 2 ulp of that entry's sum of absolute products |K||E| (observed: 7.6e-6 on an entry of 960, a quarter of that
    bound), and the oracle is then fed the golden's KRT, so that it sees exactly the reference's inputs; points, q_sdf, q_vis, vert_vis and
    validity stay bit-exact.  Against the golden directly `out` failed on every host but the writer's: the reference's own fp32 result is
    1.1e-5 from the exact value.  CPU machine and MI355X host alike (torch 2.10, AVX512 kernels on both):

      tensor | |o32 - golden| | D        | H        | D/H  | bar
      out    | 1.812e-5       | 1.103e-5 | 2.036e-5 | 0.54 | 6.12e-5

    `extrin`'s rotation transposed in the oracle's spatial encoder: D 0.13."""
    g = golden("query_posed")
    frame = posed_frame("A", 3)
    cam = frame["cam_in"]
    assert torch.equal(frame["sp_data"]["extrin"], g["extrin"]) and torch.equal(cam["extrin"], g["extrin"])
    sum_abs = cam["K"].double().abs() @ cam["extrin"].double().abs()  # |K||E|: an fp32 product in any order lands within a few ulp of it
    krt_err = (cam["KRT"].double() - g["KRT"].double()).abs()
    print(f"KRT: max |host - golden| {krt_err.max().item():.3e}, largest share of 2 ulp(|K||E|) {(krt_err / (2.0 * ulp32(sum_abs))).max().item():.2f}")
    assert (krt_err <= 2.0 * ulp32(sum_abs)).all()
    frame["cam_in"] = dict(cam, KRT=g["KRT"])  # from here on the oracle sees exactly the reference's inputs
    assert torch.equal(near_mesh_points(frame, N_POINTS, seed=2), g["pts"][0])
    q_sdf, q_vis, vert_vis = mesh_queries(frame, g["pts"][0])
    assert torch.equal(q_sdf, g["q_sdf"][0]) and torch.equal(q_vis, g["q_vis"][0, :, 0]) and torch.equal(vert_vis, g["vert_vis"][0, :, 0])
    view = torch.nn.functional.normalize(torch.ones_like(g["pts"]), dim=-1)

    def whole(sd, frame, pts, q_sdf, view):
        out, valid = orc.query(sd, pts, frame["cam_in"], frame["targets"], frame["feat_geo"], frame["feat_tex"], g["vert_vis"],
                               g["q_vis"], q_sdf, frame["sp_data"], frame["img_in"], view, frame["src_foreground_mask"])
        assert torch.equal(valid, g["valid"])
        assert 0.05 < valid.float().mean() < 0.95
        return out

    o32, o64 = both(whole, sd_full, frame, g["pts"], g["q_sdf"], view)
    assert o32.dtype == torch.float32 and o64.dtype == torch.float64
    hold("query_posed:out", g["out"], o32, o64, 2e-6)


def test_whole_pass_posed_vs_reference(golden, sd_full):
    """VANeRF.batch_render_pifu_nerf of the reference on pose A, 16 x 16 rays, 16 + 16 samples, under the criterion: the fp32 pass, then its
    own samples re-marched in fp64 (remarch64); floor 2e-6 (test_whole_pass's tolerance), coarse outputs with every element inside the bar,
    fine outputs -- behind the u = 1.0 tie of importance_sample (tests/test_oracle_golden.py) -- under assert_close_frac's cap of 1e-3, of
    which the reference needs none here.  CPU machine and MI355X host alike:

      output      | |o32 - golden| | D       | H       | D/H  | bar
      tex_fg      | 4.26e-6        | 4.52e-6 | 5.17e-6 | 0.87 | 1.56e-5
      depth       | 7.15e-7        | 4.77e-7 | 3.71e-7 | 1.29 | 2.00e-6
      alpha       | 5.96e-8        | 5.96e-8 | 5.96e-8 | 1.00 | 2.00e-6
      tex_fg_fine | 4.35e-6        | 4.44e-6 | 5.10e-6 | 0.87 | 1.54e-5
      depth_fine  | 7.15e-7        | 1.06e-6 | 3.94e-7 | 2.69 | 2.00e-6
      alpha_fine  | 1.19e-7        | 1.19e-7 | 5.96e-8 | 2.00 | 2.00e-6
      sdf         | 3.17e-6        | 2.38e-6 | 1.99e-6 | 1.19 | 5.98e-6

    (depth_fine: D also holds the reference's own, slightly different fine depths; the floor covers it.)"""
    g = golden("pass_16x16_s16_posed")
    frame = posed_frame("A", 3)
    S = int(g["S"])
    assert (S, int(g["level"]), g["stride_xy"].tolist()) == (16, 3, [1, 2])
    out = orc.batch_render(sd_full, frame, int(g["level"]), g["stride_xy"].long()[None, None], S, S, want={})
    assert torch.equal(out["vert_vis"], g["vert_vis"])
    hold_pass("pass_16x16_s16_posed", g, out, remarch64(sd_full, frame, out), 2e-6, 2e-6, 1e-3)
    assert out["depth_fine"].std() > 1e-3 and 0.05 < out["coarse"]["vert_vis"].mean() < 0.95


@pytest.mark.parametrize("pose", [p for p, _ in POSES])
def test_fp32_and_fp64_oracle_agree_on_posed_cameras(evaluations, pose):
    """Same validity, raw outputs within 1e-4 (observed 2.3e-5; identity camera 1.4e-5): the reference is well conditioned on these poses and
    the project's 1e-4 bar keeps its room.  No point sits within 1e-5 of a validity decision, so no kernel may disagree on one."""
    e = evaluations[pose]
    assert torch.equal(e["r64"]["valid"], e["r32"]["valid"])
    assert 0.05 < e["r64"]["valid"].float().mean() < 0.95
    err = (e["r32"]["raw"].double() - e["r64"]["raw"]).abs().max().item()
    print(f"pose {pose}: max |fp32 - fp64| of the oracle's raw outputs {err:.2e}, valid {e['r64']['valid'].float().mean().item():.3f}")
    assert err <= 1e-4
    assert decision_margins(e["frame"], e["pts"])[0].min() > 1e-5


@pytest.mark.parametrize("pose", [p for p, _ in POSES])
def test_the_pose_is_visible_in_the_oracle(evaluations, sd_full, pose):
    """fp64: the posed frame's outputs differ from the un-posed frame's by more than 1e-2, and `extrin` with its rotation transposed changes
    them by more than 1e-3 -- what a kernel with R^T for R would compute is not within the bar of this reference."""
    e = evaluations[pose]
    frame, pts, (q_sdf, q_vis, vert_vis), r64 = e["frame"], e["pts"], e["q"], e["r64"]
    plain = synth.make_frame(seed=dict(POSES)[pose], tar_h=64, tar_w=64, half_mask=True)
    r_plain = reference(sd_full, plain, pts, *mesh_queries(plain, pts))
    both = r64["valid"] & r_plain["valid"]
    assert both.float().mean() > 0.02
    assert (r64["raw"] - r_plain["raw"])[both].abs().max() > 1e-2
    ext_t = frame["sp_data"]["extrin"].clone()
    ext_t[:, :3, :3] = frame["sp_data"]["extrin"][:, :3, :3].transpose(1, 2)
    r_t = reference(sd_full, dict(frame, sp_data=dict(frame["sp_data"], extrin=ext_t)), pts, q_sdf, q_vis, vert_vis)
    assert torch.equal(r_t["valid"], r64["valid"])  # (validity reads KRT alone)
    diff = (r_t["raw"] - r64["raw"])[r64["valid"]].abs().max().item()
    print(f"pose {pose}: transposed rotation in extrin moves the raw outputs by {diff:.2e}")
    assert diff > 1e-3


def test_border_band_points_lie_in_the_band():
    frame = posed_frame("A", 3, half=False)
    pts = border_band_points(frame)
    m, xy, z, fg = decision_margins(frame, pts)
    big = xy.abs().max(-1)[0]
    assert pts.shape == (32, 3) and ((big > 1.0 + 1e-5) & (big < 1.01 - 1e-5)).all() and (xy.abs().min(-1)[0] < 0.9).all()
    assert (z.abs() < 0.5).all() and (fg == 1.0).all() and m.min() > 1e-5
    for axis in (0, 1):
        assert (xy[:, axis] > 1.0).sum() == 8 and (xy[:, axis] < -1.0).sum() == 8
