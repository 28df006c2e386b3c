"""Extent of the 64-point groups the mesh query works on (benchmark view).  By index -- depth k of an 8x8-pixel tile: 90 % span < 1.5 cm, the
tiles on the silhouette of the bounding box (rays that hit it next to rays that miss it) up to 0.5 m.  Behind the tile-split experiment recorded
in DESIGN.md section 8.  --order: also the radius the kernel's tile search works with (max |p - tc|, tc = the centre of the group's box; one depth
per group) for the coarse samples and the importance samples (z_new of a whole pass) by index, and for both cut into 64-slot slabs of the
tile-order table (vanerf_mesh_tile_order), DESIGN.md section 4."""
import os, sys, torch
sys.path.insert(0, ".")
from vanerf_amd import renderer as R, synth
frame = synth.make_frame(seed=11, tar_h=512, tar_w=334, orbit_deg=15.0)
rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 0, 0, 1, 334, 512, 64, device="cuda")
pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"]).view(512, 334, 64, 3)
t = pts[:512, :328].reshape(64, 8, 41, 8, 64, 3).permute(0, 2, 4, 1, 3, 5).reshape(64, 41, 64, 64, 3)
ext = (t.max(3)[0] - t.min(3)[0]).max(-1)[0]
print("tile extent quantiles (m):", [round(float(ext.flatten().quantile(q)), 5) for q in (0.01, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0)])
v = frame["targets"]["vert_world"][0]
print("mesh extent:", (v.max(0)[0] - v.min(0)[0]).tolist())
thr = 0.1 * float(max(v.max(0)[0][1] - v.min(0)[0][1], v.max(0)[0][2] - v.min(0)[0][2]))
print("threshold", thr)
for b in (4, 12, 13, 16, 21, 30, 49):
    e = ext[b]
    print(f"block {b}: fraction of tiles x depths above the threshold {float((e > thr).float().mean()):.3f}, median extent {float(e.median()):.4f}, max {float(e.max()):.3f}")

if "--order" in sys.argv:
    def radii(p, table):
        """p (n, 3) points, table (groups, 64) sample indices (-1: none) -> the radius of every group about the centre of its box."""
        named = table >= 0
        g = p[table.clamp_min(0).long()]  # (groups, 64, 3)
        big = torch.full_like(g, float("inf"))
        lo, hi = torch.where(named[..., None], g, big).min(1)[0], torch.where(named[..., None], g, -big).max(1)[0]
        d = (g - 0.5 * (lo + hi)[:, None]).norm(dim=-1)
        return torch.where(named, d, torch.zeros_like(d)).max(1)[0][named.any(1)]

    def report(tag, r):
        q = [1e3 * float(r.quantile(x)) for x in (0.5, 0.9, 0.99)] + [1e3 * float(r.max())]
        print(f"{tag:34s} radius mm q50 / q90 / q99 / max: " + " / ".join(f"{x:.2f}" for x in q) + f"   above 25 mm: {100 * float((r > 0.025).float().mean()):.2f} %")

    sd = synth.make_full_weights(0)
    fd = synth.to_device(frame, "cuda")
    sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
    fdat = R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
    os.environ["VANERF_MESH_TILE_ORDER"] = "0"  # (the pass that makes z_new: its outputs do not depend on the setting)
    z_new = R.render_pass(R.PackedWeights(sd, mode="bf16x3"), fdat, frame["cam_tar"], frame["bounds"], 0, 0, 1, 334, 512, 64, 64)["z_new"].contiguous()
    for tag, z in (("coarse", rays["z"]), ("fine (z_new)", z_new)):
        p = R.sample_points(rays["rays_d"], rays["cam_pos"], z)
        # the index grouping as a table: equal depths (a stable sort keeps index order, ray-major), regrouped so that slab k = sample k of the rays
        by_index = R.mesh_tile_order(torch.zeros_like(z), 334, 512).view(-1, 64, 64).transpose(1, 2).reshape(-1, 64)
        report(f"{tag}, by index", radii(p, by_index))
        report(f"{tag}, 64-slot slabs of the table", radii(p, R.mesh_tile_order(z, 334, 512).view(-1, 64)))
