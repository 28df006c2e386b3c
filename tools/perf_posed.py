"""The baked hand in another pose (vanerf_amd/posed.py, csrc/pose_warp.hip) on the synthetic two-hand frame, from device
events, each figure the median of `--reps` windows after a warm-up of every shape.  The frame is baked at `--size` grid points, the pose is
the frame's vertices under a smooth bend, the cameras are a get_360cameras orbit of `--views` views at `--image` x `--image`.  Per sample count:
  * the stages of render_posed_volume one by one: pose_transforms, the MeshAccel of the posed mesh, ray setup + sample points, the mesh query
    (face and sdf), and the march alone (march_volume_posed on those inputs), with the share of empty samples;
  * render_posed_views for the whole group (accel built per call, and handed in), per group and per view;
  * in the same run: render_baked_views (section 0g: no pose, no mesh query) and the exact pass (64 + 64 samples) on the same cameras.
--dump FILE marches seeded host-made inputs instead (no network, no timing) and writes the group's colour, depth and alpha at the first sample
count to FILE (.npz): two builds of the library (VANERF_HIP_LIB; e.g. one with -DVANERF_POSED_NO_SKIP) are compared bit for bit through it.
--surface times the geometry path instead, per sample count on posed_samples of the group: march_surface_posed and
march_volume_posed on the SAME prepared samples, the mesh query, render_posed_surface_views per view, and the share of found rays with found == 3.
Kernel times: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf_posed.py (volume_render_posed_kernel, pose_transforms_kernel)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vanerf_amd import baked, posed, synth  # noqa: E402
from vanerf_amd import renderer as R  # noqa: E402
from vanerf_amd.config import default_config  # noqa: E402
from vanerf_amd.mask_at_box import frame_bounds  # noqa: E402
from vanerf_amd.model import VANeRF, get_360cameras  # noqa: E402
from vanerf_amd.novel_views import camera_to_cam_tar  # noqa: E402


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def median_ms(fn, calls, reps):
    fn()  # warm-up of this shape
    t = [window(fn, calls) for _ in range(reps)]
    return statistics.median(t), min(t), max(t)


def bent(verts, amount=0.25):
    """The frame's vertices under a smooth bend: x moves by amount (y - cy)^2 / extent, z by half of that with the sign of x - cx."""
    c = verts.mean(0)
    ext = float((verts.max(0).values - verts.min(0).values).max())
    u = (verts - c) / ext
    return (verts + amount * ext * torch.stack([u[:, 1] ** 2, torch.zeros_like(u[:, 0]), 0.5 * u[:, 1] ** 2 * torch.sign(u[:, 0])], 1)).contiguous()


def dump(a):
    """--dump: the group's colour, depth and alpha at the first sample count from SEEDED inputs made on the host -- the frame's mesh and its bend,
    random voxels on bake_volume's grid, sigmoid_beta = 0.01 -- so that two processes march the same bits (a bake does not qualify: the image
    encoders' convolutions are picked per process)."""
    from vanerf_amd import surface
    frame_cpu = synth.make_frame(seed=3, tar_h=a.image, tar_w=a.image)
    verts = frame_cpu["targets"]["vert_world"][0].cuda().contiguous()
    faces = frame_cpu["targets"]["face_world"][0].to(device="cuda", dtype=torch.int32).contiguous()
    wide = frame_cpu["bounds"][0].double() + torch.tensor([[-baked.CLIP_PAD], [baked.CLIP_PAD]], dtype=torch.float64)
    origin, spacing, (nx, ny, nz) = surface.grid_spec(wide, voxel_size=float((wide[1] - wide[0]).max()) / (a.size - 1))
    vox = torch.rand(nz, ny, nx, 4, generator=torch.Generator().manual_seed(0))
    vox[..., 0] = vox[..., 0] * 0.07 - 0.02
    vol = baked.BakedVolume(vox.cuda(), origin, spacing, (nx, ny, nz), frame_cpu["bounds"][0], 0.01, verts=verts, znear=0.71, zfar=1.42)
    headpose = torch.eye(4)
    headpose[:3, 3] = verts.mean(0).cpu()
    cams = [camera_to_cam_tar(c) for c in get_360cameras(headpose[:3, :4].cuda(), 4.0 * a.image, 1.0, 1.0, a.image, a.image, 0.71, 1.42, n_frames=a.views)]
    with torch.no_grad():
        o = posed.render_posed_volume(vol, faces, bent(verts), cams, samples=a.samples[0], reach=a.reach)
    empty = (o["sdf"] > a.reach) | ~torch.isfinite(o["sdf"])
    print(f"grid {nx} x {ny} x {nz}, {a.views} views, {a.samples[0]} samples: {100 * float(empty.float().mean()):.1f} % of the samples are empty, "
          f"{100 * float((o['alpha'] > 0.5).float().mean()):.1f} % of the rays end with alpha above 0.5")
    np.savez(a.dump, **{k: o[k].cpu().numpy() for k in ("color", "depth", "alpha")})
    print(f"wrote {a.dump}")


def surface(a, vol, faces, pose, cams, fmt):
    """--surface: the march of section 0k next to the colour march of the same prepared samples, the query both wait for, and whole frames."""
    V, Rn = len(cams), a.image * a.image
    accel = R.MeshAccel(pose, faces)
    no_vis = torch.zeros(pose.shape[0], device="cuda")
    for S in a.samples:
        p = posed.posed_samples(vol, faces, pose, cams, samples=S, accel=accel)
        tail = (p.T, p.face, p.sdf, p.rays_d, p.cam_pos, p.z, p.hit)
        found = posed.march_surface_posed(vol, *tail, refine=a.refine, reach=a.reach, row_rays=p.row_rays)[3]
        seen = int((found != 0).sum())
        print(f"{S:3d} samples: {seen} of {found.numel()} rays found ({100 * seen / found.numel():.1f} %); found == 1 / 2 / 3: "
              + " / ".join(str(int((found == k).sum())) for k in (1, 2, 3)) + f"; found == 3 on {100 * int((found == 3).sum()) / max(seen, 1):.2f} % of the found rays")
        t_s = median_ms(lambda: posed.march_surface_posed(vol, *tail, refine=a.refine, reach=a.reach, row_rays=p.row_rays), a.calls, a.reps)
        print(f"{S:3d} samples: surface march (march_surface_posed, refine {a.refine}): {fmt(t_s)} per group, {t_s[0] / V:8.3f} ms per view")
        t_c = median_ms(lambda: posed.march_volume_posed(vol, *tail, a.reach, row_rays=p.row_rays), a.calls, a.reps)
        print(f"{S:3d} samples: colour march of the same samples (march_volume_posed): {fmt(t_c)} per group, {t_c[0] / V:8.3f} ms per view; "
              f"surface / colour = {t_s[0] / t_c[0]:.2f}", flush=True)
        pts = R.sample_points(p.rays_d.view(-1, 3), p.cam_pos, p.z.view(-1, S), rays_per_view=Rn)
        t = median_ms(lambda: R.mesh_query_accel(accel, pose, faces, no_vis, pts, want_face=True, want_knn=False, grid=(a.image, V * a.image, S)), a.calls, a.reps)
        print(f"{S:3d} samples: mesh query (face, sdf) of {pts.shape[0] / 1e6:.1f} M points: {fmt(t)} per group, {t[0] / V:8.3f} ms per view", flush=True)
        del pts
        t = median_ms(lambda: posed.render_posed_surface_views(vol, faces, pose, cams, S, refine=a.refine, reach=a.reach, accel=accel), a.calls, a.reps)
        print(f"{S:3d} samples: render_posed_surface_views with accel= handed in, group of {V}: {fmt(t)} per group, {t[0] / V:8.3f} ms per view")
        t = median_ms(lambda: posed.render_posed_surface_views(vol, faces, pose, cams, S, refine=a.refine, reach=a.reach, prepared=p), a.calls, a.reps)
        print(f"{S:3d} samples: render_posed_surface_views with prepared= handed in (march + images): {fmt(t)} per group, {t[0] / V:8.3f} ms per view", flush=True)
        del p, tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--reach", type=float, default=posed.REACH)
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--dump", default=None)
    ap.add_argument("--surface", action="store_true")
    ap.add_argument("--refine", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_posed.py measures on the GPU: no device found")
    if a.dump:
        return dump(a)
    torch.manual_seed(0)
    cfg = default_config()
    cfg["models"]["VANeRF"]["mfma_precision"] = a.precision
    net = VANeRF(cfg).cuda().eval()
    net.load_state_dict(synth.make_full_weights(0), strict=False)
    frame_cpu = synth.make_frame(seed=3, tar_h=a.image, tar_w=a.image)
    trb = synth.to_tr_batch(synth.to_device(frame_cpu, "cuda"))
    headpose = torch.eye(4)
    headpose[:3, 3] = frame_cpu["targets"]["vert_world"][0].mean(0)
    V = a.views
    cams = [camera_to_cam_tar(c) for c in get_360cameras(headpose[:3, :4].cuda(), 4.0 * a.image, 1.0, 1.0, a.image, a.image, 0.71, 1.42, n_frames=V)]
    kw = cfg["models"]["VANeRF"]["dr_kwargs"]
    fmt = lambda t: f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"  # noqa: E731

    def exact():
        return net.render_pifu_nerf_views(trb["im"], trb["cam"], trb["hand_type"], trb["targets"], cams, sp_data=dict(trb["sp_data"]), fine=True, uniform=True,
                                          sample_per_ray_c=kw["sample_per_ray_c"], sample_per_ray_f=kw["sample_per_ray_f"],
                                          src_foreground_mask=trb["src_foreground_mask"], bounds=trb["dr_data"]["bounds"])

    with torch.no_grad():
        vol = baked.bake_volume(net, trb, resolution=a.size)
        faces = posed._frame_faces(trb, vol.voxels.device)
        pose = bent(vol.verts)
        nx, ny, nz = vol.dims
        print(f"{a.image} x {a.image}, {V} orbit views [{a.precision}]; grid {nx} x {ny} x {nz}; {faces.shape[0]} faces; reach {a.reach}; "
              f"the bend moves the vertices by up to {1e3 * float((pose - vol.verts).norm(dim=1).max()):.1f} mm", flush=True)
        if a.surface:
            return surface(a, vol, faces, pose, cams, fmt)
        t = median_ms(lambda: posed.pose_transforms(vol.verts, pose, faces), 20, a.reps)
        print(f"pose_transforms: {fmt(t)}")
        t = median_ms(lambda: R.MeshAccel(pose, faces), 20, a.reps)
        print(f"MeshAccel of the posed mesh: {fmt(t)}", flush=True)
        t = median_ms(exact, 1, a.reps)
        print(f"exact pass ({kw['sample_per_ray_c']} + {kw['sample_per_ray_f']} samples), group of {V}: {fmt(t)} per group, {t[0] / V:8.3f} ms per view", flush=True)
        T, accel = posed.pose_transforms(vol.verts, pose, faces), R.MeshAccel(pose, faces)
        no_vis = torch.zeros(pose.shape[0], device="cuda")
        Rn = a.image * a.image
        for S in a.samples:
            t = median_ms(lambda: baked.render_baked_views(vol, cams, S), a.calls, a.reps)
            print(f"{S:3d} samples: render_baked_views (no pose), group of {V}: {fmt(t)} per group, {t[0] / V:8.3f} ms per view", flush=True)

            def rays_and_points():
                rays = R.ray_setup_views(cams, frame_bounds(pose), 0, 0, 1, a.image, a.image, S)
                return rays, R.sample_points(rays["rays_d"].view(-1, 3), rays["cam_pos"], rays["z"].view(-1, S), rays_per_view=Rn)

            t = median_ms(rays_and_points, a.calls, a.reps)
            print(f"{S:3d} samples: ray setup + sample points: {fmt(t)} per group, {t[0] / V:8.3f} ms per view")
            rays, pts = rays_and_points()
            query = lambda: R.mesh_query_accel(accel, pose, faces, no_vis, pts, want_face=True, want_knn=False, grid=(a.image, V * a.image, S))  # noqa: E731
            t = median_ms(query, a.calls, a.reps)
            print(f"{S:3d} samples: mesh query (face, sdf) of {pts.shape[0] / 1e6:.1f} M points: {fmt(t)} per group, {t[0] / V:8.3f} ms per view", flush=True)
            sdf, _, face = query()
            face, sdf = face.view(V, Rn, S), sdf.view(V, Rn, S)
            empty = (face < 0) | (face >= faces.shape[0]) | ~torch.isfinite(sdf) | (sdf > a.reach)
            rounds = empty.view(V, Rn, -1, min(S, 64)).all(-1) if S % min(S, 64) == 0 else empty.all(-1)
            print(f"{S:3d} samples: {100 * float(empty.float().mean()):.1f} % of the samples are empty, {100 * float(rounds.float().mean()):.1f} % of the rounds of 64 wholly")
            march = lambda: posed.march_volume_posed(vol, T, face, sdf, rays["rays_d"], rays["cam_pos"], rays["z"], rays["hit"], a.reach, row_rays=a.image)  # noqa: E731
            t = median_ms(march, a.calls, a.reps)
            print(f"{S:3d} samples: march alone (march_volume_posed): {fmt(t)} per group, {t[0] / V:8.3f} ms per view", flush=True)
            del rays, pts, face, sdf, empty, rounds
            t = median_ms(lambda: posed.render_posed_views(vol, faces, pose, cams, S, a.reach), a.calls, a.reps)
            print(f"{S:3d} samples: render_posed_views, group of {V}: {fmt(t)} per group, {t[0] / V:8.3f} ms per view")
            t = median_ms(lambda: posed.render_posed_views(vol, faces, pose, cams, S, a.reach, accel=accel), a.calls, a.reps)
            print(f"{S:3d} samples: render_posed_views with accel= handed in: {fmt(t)} per group, {t[0] / V:8.3f} ms per view", flush=True)


if __name__ == "__main__":
    main()
