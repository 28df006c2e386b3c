"""Two builds of the library compute the same bits in the per-ray wave kernels (csrc/wave_ray.h, csrc/volume_field.h): the composite forward
(every dispatch width and the serial fallback, one table and two, with and without `contrib`, sigmoid_beta by number and by handle), its
backward (with d_beta; all four upstream gradients and colour alone), march_volume, march_surface and march_volume_posed.  The inputs are
small and drawn on the CPU from seeded generators: 37 rays for the composite (tests/test_composite_widths.py's count); for the marches a
7 x 6 x 5 grid with a few 1e30 voxels and 2 views of 5 x 3 rays -- odd in both directions, so waves leave at both edges of the 2 x 2 tile --
two of them with hit = 0; for the posed march 4 faces' records, with empty samples, one whole round of 64 empty and one face out of range.
usage: ray_bits.py LIB_A LIB_B     one fresh child process per library (VANERF_HIP_LIB), digests compared; exit status 1 on any difference"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RAYS = 37
FORWARD_S = (1, 64, 65, 128, 192, 193, 256, 257)
FORWARD_TWO = ((40, 24), (100, 93), (200, 57))
BACKWARD_S = (64, 129, 192, 256)
BACKWARD_TWO = ((100, 93),)
BETA = 0.05
DIMS, ORIGIN, SPACING = (7, 6, 5), (-0.12, -0.1, 0.9), (0.04, 0.04, 0.05)
VIEWS, ROW_RAYS, ROWS = 2, 5, 3
MARCH_S = (1, 64, 130)
NF = 4


def composite_tables(rng, S, Sn=0):
    """One table of S samples per ray, or tables of S and Sn in a random merged order -> rgba, z, msdf, rgba_n, sdf_n, src (numpy)."""
    import numpy as np

    def table(n):
        q = rng.random((RAYS, n, 5), dtype=np.float32)
        q[..., 0] = q[..., 0] * 0.08 - 0.03
        return q, (rng.random((RAYS, n), dtype=np.float32) * 0.02 - 0.01)

    rgba, msdf = table(S)
    z = np.sort(rng.random((RAYS, S + Sn), dtype=np.float32) * 0.5 + 0.75, axis=1)
    if not Sn:
        return rgba, z, msdf, None, None, None
    rgba_n, sdf_n = table(Sn)
    src = np.empty((RAYS, S + Sn), dtype=np.int32)
    for r in range(RAYS):
        from_a = np.zeros(S + Sn, dtype=bool)
        from_a[rng.choice(S + Sn, S, replace=False)] = True
        src[r, from_a] = np.arange(S)
        src[r, ~from_a] = ~np.arange(Sn)
    return rgba, z, msdf, rgba_n, sdf_n, src


def march_inputs(rng, S):
    """voxels (nz, ny, nx, 4): a sphere's signed distance around the grid centre (most rays cross it), random colours, three 1e30 voxels; the
    rays of two cameras, one in front of the grid and one beside it, with S depths from in front of the grid to behind it."""
    import numpy as np
    nx, ny, nz = DIMS
    gz, gy, gx = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in (nz, ny, nx)), indexing="ij")
    p = np.stack([ORIGIN[0] + gx * SPACING[0], ORIGIN[1] + gy * SPACING[1], ORIGIN[2] + gz * SPACING[2]], -1)
    centre = np.array([0.0, 0.0, 1.0])
    vox = np.empty((nz, ny, nx, 4), dtype=np.float32)
    vox[..., 0] = np.linalg.norm(p - centre, axis=-1) - 0.095
    vox[..., 1:] = rng.random((nz, ny, nx, 3), dtype=np.float32)
    vox[0, 0, 0, 0] = vox[nz - 1, 2, nx - 1, 0] = vox[2, ny - 1, 3, 0] = 1e30
    R = ROW_RAYS * ROWS
    eyes = np.array([[0.01, -0.02, 0.0], [0.95, 0.03, 1.01]])
    rays_d = np.empty((VIEWS, R, 3), dtype=np.float32)
    for v in range(VIEWS):
        ys, xs = np.meshgrid(np.linspace(-0.06, 0.06, ROWS), np.linspace(-0.08, 0.08, ROW_RAYS), indexing="ij")
        side = np.stack([xs, ys, np.zeros_like(xs)], -1) if v == 0 else np.stack([np.zeros_like(xs), ys, xs], -1)
        d = (centre + side.reshape(R, 3)) - eyes[v]
        rays_d[v] = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    cam_pos = np.concatenate([eyes, np.zeros((VIEWS, 1))], 1).astype(np.float32)
    z = (0.8 + 0.4 * np.sort(rng.random((VIEWS, R, S), dtype=np.float32), axis=-1)).astype(np.float32)
    hit = np.ones((VIEWS, R), dtype=np.uint8)
    hit[0, 3] = hit[1, 11] = 0
    return vox, rays_d, cam_pos, z, hit


def posed_inputs(rng, S):
    """T (NF, 12): the identity and three maps near it; face with -1 (empty) and one NF (out of range), sdf on both sides of reach = 0.03;
    at S > 64 the first round of one ray is empty as a whole."""
    import numpy as np
    R = ROW_RAYS * ROWS
    T = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32), (NF, 1))
    T[1:] += (rng.random((NF - 1, 12), dtype=np.float32) - 0.5) * 0.04
    face = rng.integers(0, NF, (VIEWS, R, S)).astype(np.int32)
    face[rng.random((VIEWS, R, S)) < 0.15] = -1
    face[1, 7, S // 2] = NF
    sdf = (rng.random((VIEWS, R, S), dtype=np.float32) * 0.08 - 0.02).astype(np.float32)
    if S > 64:
        face[0, 6, :64] = -1
    return T, face, sdf


def digests():
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from vanerf_amd import baked, posed, renderer as R, synth

    def dig(t):
        return None if t is None else hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]

    def dev(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    sd = dict(synth.make_full_weights(0))
    sd["sigmoid_beta"] = torch.tensor([BETA])
    handle = R.PackedWeights(sd, mode="fp32")
    res = {}
    names = ("color", "depth", "alpha", "contrib", "sdf")
    # 1. composite forward
    for S, Sn in [(S, 0) for S in FORWARD_S] + list(FORWARD_TWO):
        t = [dev(a) for a in composite_tables(np.random.default_rng(100 + S + Sn), S, Sn)]
        rgba, z, msdf, rgba_n, sdf_n, src = t
        for how, beta in (("number", BETA), ("handle", handle)):
            for want in ((True, False) if not Sn else (True,)):
                out = R._composite(rgba, z, msdf, rgba_n, sdf_n, src, beta, want)
                res[f"composite {S}+{Sn} {how}{'' if want else ' no contrib'}"] = {k: dig(o) for k, o in zip(names, out)}
    # 2. composite backward
    for S, Sn in [(S, 0) for S in BACKWARD_S] + list(BACKWARD_TWO):
        rng = np.random.default_rng(200 + S + Sn)
        rgba, z, msdf, rgba_n, sdf_n, src = (dev(a) for a in composite_tables(rng, S, Sn))
        g = {"g_color": dev(rng.standard_normal((RAYS, 3), dtype=np.float32)), "g_depth": dev(rng.standard_normal(RAYS, dtype=np.float32)),
             "g_alpha": dev(rng.standard_normal(RAYS, dtype=np.float32)), "g_sdf": dev(rng.standard_normal(RAYS, dtype=np.float32))}
        for what, grads in (("all four", g), ("colour only", {"g_color": g["g_color"]})):
            out = R.composite_backward(handle, rgba, z, msdf, rgba_n=rgba_n, sdf_n=sdf_n, src=src, **grads)
            res[f"backward {S}+{Sn} {what}"] = {k: dig(o) for k, o in zip(("d_rgba", "d_rgba_n", "d_beta"), out)}
    # 3 - 5. the marches
    f3 = lambda t: tuple(float(np.float32(x)) for x in t)
    for S in MARCH_S:
        rng = np.random.default_rng(300 + S)
        vox, rays_d, cam_pos, z, hit = march_inputs(rng, S)
        T, face, sdf = posed_inputs(rng, S)
        rays = tuple(dev(a) for a in (rays_d, cam_pos, z, hit))
        for how, beta in (("number", BETA), ("handle", handle)):
            vol = baked.BakedVolume(voxels=dev(vox), origin=f3(ORIGIN), spacing=f3(SPACING), dims=DIMS, bounds=torch.zeros(2, 3), beta=beta)
            out = baked.march_volume(vol, *rays, row_rays=ROW_RAYS)
            res[f"march_volume S={S} {how}"] = {k: dig(o) for k, o in zip(("color", "depth", "alpha"), out)}
            for reach in (0.03, float("inf")):
                out = posed.march_volume_posed(vol, dev(T), dev(face), dev(sdf), *rays, reach=reach, row_rays=ROW_RAYS)
                res[f"march_volume_posed S={S} reach={reach} {how}"] = {k: dig(o) for k, o in zip(("color", "depth", "alpha"), out)}
        for iso in (0.0, 0.01):
            for refine in (0, 2):
                out = baked.march_surface(vol, *rays, iso=iso, refine=refine, row_rays=ROW_RAYS)
                res[f"march_surface S={S} iso={iso} refine={refine}"] = {k: dig(o) for k, o in zip(("depth", "normal", "color", "found"), out)}
                res[f"march_surface S={S} iso={iso} refine={refine}"]["crossings"] = int((out[3] == 1).sum())
    torch.cuda.synchronize()
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
    n = sum(len(v) for v in a.values())
    print(f"all {n} outputs of {len(a)} cases of the composite, its backward and the three marches are bitwise equal" if not bad else f"{bad} cases differ")
    sys.exit(1 if bad else 0)
