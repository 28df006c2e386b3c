"""Two builds of the library compute the same bits in the per-sample kernels: vanerf_query_order, the instantiations of query_kernel
(fp32, bf16x3 without a table, texel, lean under VANERF_TEXEL_PRODUCTS=0, hoisted under VANERF_LEAN_STREAM=0 -- each without and with the
work order -- and the training spill forward with its xs / aux buffers; a library from before the texel level ignores its switch and runs the
lean level in both cases: "texel" then differs, "lean" must not) on the half-masked 128 x 128 frame of tests/test_lean_stream.py at 16 samples per ray (262 144 samples:
at least three rounds per block, with full -> full, full -> short and short -> full hand-overs).
usage: query_bits.py LIB_A LIB_B     one fresh child process per library (VANERF_HIP_LIB), digests compared; exit status 1 on any difference"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digests():
    import ctypes

    import torch

    sys.path.insert(0, ROOT)
    from vanerf_amd import hip_backward as HB, renderer as R, synth
    from vanerf_amd._ffi import check, lib

    def dig(t):
        return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]

    sd = synth.make_full_weights(0)
    frame = synth.make_frame(seed=5, tar_h=128, tar_w=128, orbit_deg=40.0, half_mask=True)
    fd = synth.to_device(frame, "cuda")
    sdd = {k: v.cuda() for k, v in sd.items() if k.startswith("tex_vis_fusion.")}
    fdat = R.FrameData(sdd, fd["img_in"], fd["feat_geo"], fd["feat_tex"], fd["src_foreground_mask"], fd["cam_in"], fd["targets"], fd["sp_data"])
    rays = R.ray_setup(frame["cam_tar"], frame["bounds"], 0, 0, 1, 128, 128, 16, device="cuda")
    pts = R.sample_points(rays["rays_d"], rays["cam_pos"], rays["z"])
    q_sdf, q_vis, knn = R.mesh_query_accel(fdat.accel, fdat.verts3, fdat.faces, fdat.vert_vis, pts)
    order = R.query_order(fdat, pts)
    res = {"n": pts.shape[0], "order": dig(order)}
    w0, w1 = R.PackedWeights(sd, mode="fp32"), R.PackedWeights(sd, mode="bf16x3")
    table = fdat.vertex_products(w1)
    cases = [("fp32", w0, None, {}), ("bf16x3", w1, None, {}), ("texel", w1, table, {}), ("lean", w1, table, {"VANERF_TEXEL_PRODUCTS": "0"}),
             ("hoisted", w1, table, {"VANERF_LEAN_STREAM": "0"})]
    for name, w, vp, switches in cases:
        for var in ("VANERF_LEAN_STREAM", "VANERF_TEXEL_PRODUCTS"):
            os.environ.pop(var, None)
        os.environ.update(switches)
        for o in (None, order):
            c0 = w.short_groups()
            out, valid = R.query_samples(w, fdat, pts, q_sdf, q_vis, knn, want_valid=True, order=o, vertex_products=vp)
            key = name + ("+order" if o is not None else "")
            res[key] = {"out": dig(out), "valid": dig(valid), "short_groups": int(w.short_groups() - c0), "finite": bool(torch.isfinite(out).all())}
    for var in ("VANERF_LEAN_STREAM", "VANERF_TEXEL_PRODUCTS"):
        os.environ.pop(var, None)
    n = 65536  # one block of the training step
    ws = HB.workspace(n, pts.device)
    for t in (ws.xs, ws.aux, ws.raw, ws.valid):
        t.zero_()
    P, qw = HB._ptr, R._queue_word(pts.device)
    p, s, v, k = (t[:n].contiguous() for t in (pts, q_sdf, q_vis, knn))
    check(lib.vanerf_query_forward_spill(w0.handle, ctypes.byref(fdat.c), P(p), P(s), P(v), P(k), n, ws.block, P(ws.raw), P(ws.valid), P(ws.xs), P(ws.aux),
                                         P(qw), R._stream()))
    torch.cuda.synchronize()
    res["spill"] = {"raw": dig(ws.raw), "valid": dig(ws.valid), "xs": dig(ws.xs), "aux": dig(ws.aux)}
    return res


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        print("DIGESTS " + json.dumps(digests()))
        sys.exit(0)
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    got = []
    for path in sys.argv[1:]:
        env = dict(os.environ, VANERF_HIP_LIB=os.path.abspath(path))
        text = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, capture_output=True, text=True).stdout
        got.append(json.loads([l for l in text.splitlines() if l.startswith("DIGESTS ")][-1][8:]))
    a, b = got
    bad = 0
    for key in a:
        same = a[key] == b.get(key)
        bad += not same
        print(("same      " if same else "DIFFERENT ") + key, a[key], "" if same else b.get(key))
    print("every output, flag, order, short-group count and spill buffer is bitwise equal" if not bad else f"{bad} entries differ")
    sys.exit(1 if bad else 0)
