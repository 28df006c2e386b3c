"""render_vis (vanerf_render_vis) on a synthetic two-hand frame, 20 calls at 256x256: the time per call from device events.  Kernel times:
rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf_vis_render.py  (vis_vertex_kernel, vis_raster_kernel)."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vanerf_amd import renderer, synth

frame = synth.make_frame(seed=3, tar_h=256, tar_w=256)
fd = synth.to_device(frame, "cuda")
sd = {k: v.cuda() for k, v in synth.make_texframe_weights().items()}
fdat = renderer.FrameData(sd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
cam = {k: v[0].contiguous() for k, v in synth.p3d_tar_cam(fd["cam_tar"]).items()}
args = (fdat.verts3, fdat.faces, fdat.vert_vis, cam["tar_R"], cam["tar_T"], cam["tar_focal"], cam["tar_princpt"], 256, 256)
for _ in range(3):
    renderer.render_vis(*args)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    rgb, vis = renderer.render_vis(*args)
e1.record()
torch.cuda.synchronize()
print(f"render_vis 256x256, NV {fdat.verts3.shape[0]}, NF {fdat.faces.shape[0]}: {1e3 * e0.elapsed_time(e1) / 20:.1f} us per call (20 calls, device events); "
      f"{int((vis == 0).sum())} pixels with vis 0")
