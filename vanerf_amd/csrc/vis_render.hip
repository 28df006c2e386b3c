// vis_render.hip -- render_vis (src/render_vis.py:181-226): the mesh coloured by per-vertex visibility, rasterised and Phong-shaded in
// the target camera, thresholded into the discriminator's visibility image.
// The semantics are restated from pytorch3d 0.7.5 (PerspectiveCameras(in_ndc=False), MeshRasterizer with blur_radius 0 and
// faces_per_pixel 1, SoftPhongShader with the default Materials, PointLights at (0,0,-3), softmax_rgb_blend with sigma = gamma = 1e-4);
// pytorch3d is not a dependency, so parity against it is unpinned (as for the mesh queries, mesh_kernels.hip).  The restatement the tests
// hold these kernels to is the fp64 `ref_render` of tests/test_vis_render.py.  Built with -ffp-contract=off.
#include "common.h"
#include "vertex_normal.h"

using namespace vanerf;

namespace {

constexpr int VR_VERT_FLOATS = 16; // scratch record per vertex, see vanerf_render_vis in the header
constexpr int VR_BLOCK = 256;
constexpr int VR_T = 16;           // pixel tile edge: one block per 16 x 16 tile

__device__ __forceinline__ float dot3(float3 a, float3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// Vertex pass: one wave per vertex.  Lane 0 projects the vertex; the wave sums the normals of the vertex's faces (wave_normal_sum,
// vertex_normal.h, which vanerf_vertex_normals shares) -- no atomics, the same bits every call.  A face with a vertex index outside [0, nv) is
// left out here and draws nothing in the raster pass.
__global__ __launch_bounds__(VR_BLOCK) void vis_vertex_kernel(const float* __restrict__ V, int nv, const int32_t* __restrict__ F, int nf,
                                                              const float* __restrict__ vert_vis, const float* __restrict__ Rm,
                                                              const float* __restrict__ Tv, const float* __restrict__ focal,
                                                              const float* __restrict__ princpt, int H, int W, float* __restrict__ scratch)
{
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * (VR_BLOCK / 64) + (threadIdx.x >> 6);
    if (v >= nv) return; // whole waves leave together
    float3 n = wave_normal_sum(V, nv, F, nf, v, lane);
    if (lane != 0) return;
    n = normalize_eps(n);
    const float3 p = make_float3(V[3 * v], V[3 * v + 1], V[3 * v + 2]);
    // row-vector convention: Xv = p @ R + T.  In fp64, rounded once at the end: with world coordinates of ~1 m and focal lengths of ~1e3 px an
    // fp32 transform moves a vertex by ~1e-4 px, i.e. ~4e-5 in the barycentrics of a 3-pixel face (and in the colour of a half-visible face).
    double r[9], t[3];
    for (int k = 0; k < 9; ++k) r[k] = (double)Rm[k];
    for (int k = 0; k < 3; ++k) t[k] = (double)Tv[k];
    const double px = p.x, py = p.y, pz = p.z;
    const double xv = ((px * r[0] + py * r[3]) + pz * r[6]) + t[0];
    const double yv = ((px * r[1] + py * r[4]) + pz * r[7]) + t[1];
    const double zv = ((px * r[2] + py * r[5]) + pz * r[8]) + t[2];
    const double u = (double)princpt[0] - (double)focal[0] * xv / zv, w = (double)princpt[1] - (double)focal[1] * yv / zv;
    // NDC (+x left, +y up, the shorter side spans [-1, 1]): pixel column c samples u = c + 0.5 at x = (W - 2c - 1) / min(H, W)
    const double m = (double)min(H, W);
    float4* out = reinterpret_cast<float4*>(scratch + (size_t)v * VR_VERT_FLOATS);
    out[0] = make_float4((float)u, (float)w, (float)(((double)W - 2.0 * u) / m), (float)(((double)H - 2.0 * w) / m));
    out[1] = make_float4((float)xv, (float)yv, (float)zv, vert_vis[v]);
    out[2] = make_float4(p.x, p.y, p.z, 0.0f);
    out[3] = make_float4(n.x, n.y, n.z, 0.0f);
}

// squared distance from p to the segment v0 v1 (pytorch3d PointLineDistanceForward)
__device__ __forceinline__ float seg_dist2(float px, float py, float ax, float ay, float bx, float by)
{
    const float dx = bx - ax, dy = by - ay;
    const float l2 = dx * dx + dy * dy;
    if (l2 <= 1e-8f) return (px - bx) * (px - bx) + (py - by) * (py - by);
    float t = (dx * (px - ax) + dy * (py - ay)) / l2;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float qx = px - (ax + t * dx), qy = py - (ay + t * dy);
    return qx * qx + qy * qy;
}

// Raster + shade pass: one thread per pixel, one block per 16 x 16 tile.  Faces stream through LDS 256 at a time in index order; a face is
// staged only if it can cover a pixel centre of the tile -- the argument of raster_kernel (mesh_kernels.hip): a face with all three depths
// positive that is not a needle cannot pass the inside test at a pixel centre further than 1e-3 NDC units from its bounding box, whatever the
// rounding; every other face is staged for every tile.  The per-pixel arithmetic is that of the full scan, so culling changes no bit.
__global__ __launch_bounds__(VR_BLOCK) void vis_raster_kernel(const int32_t* __restrict__ F, int nf, int nv, const float* __restrict__ scratch,
                                                              const float* __restrict__ Rm, const float* __restrict__ Tv, int H, int W,
                                                              float* __restrict__ rgb, float* __restrict__ vis, int32_t* __restrict__ pix_to_face,
                                                              float* __restrict__ zbuf)
{
    __shared__ float s_v[VR_BLOCK][9];
    __shared__ int s_id[VR_BLOCK];
    __shared__ int s_wcnt[VR_BLOCK / 64];
    const int tiles_x = (W + VR_T - 1) / VR_T;
    const int c0 = (blockIdx.x % tiles_x) * VR_T, r0 = (blockIdx.x / tiles_x) * VR_T;
    const int col = c0 + (threadIdx.x & (VR_T - 1)), row = r0 + threadIdx.x / VR_T;
    const float m = (float)min(H, W);
    const float cx = (float)(W - 2 * col - 1) / m, cy = (float)(H - 2 * row - 1) / m;
    const float tol = 1e-3f;
    // NDC x falls with the column, y with the row
    const int c1 = min(c0 + VR_T - 1, W - 1), r1 = min(r0 + VR_T - 1, H - 1);
    const float tx_lo = (float)(W - 2 * c1 - 1) / m - tol, tx_hi = (float)(W - 2 * c0 - 1) / m + tol;
    const float ty_lo = (float)(H - 2 * r1 - 1) / m - tol, ty_hi = (float)(H - 2 * r0 - 1) / m + tol;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float4* S4 = reinterpret_cast<const float4*>(scratch);
    float bestz = INFINITY, bb0 = 0.0f, bb1 = 0.0f, bb2 = 0.0f;
    int bf = -1;
    for (int f0 = 0; f0 < nf; f0 += VR_BLOCK) {
        const int f = f0 + threadIdx.x;
        float v[9];
        bool keep = false;
        if (f < nf) {
            const int i0 = F[3 * f], i1 = F[3 * f + 1], i2 = F[3 * f + 2];
            if (face_ok(i0, i1, i2, nv)) {
                const int ii[3] = {i0, i1, i2};
                for (int c = 0; c < 3; ++c) {
                    const float4 a = S4[(size_t)ii[c] * (VR_VERT_FLOATS / 4)], b = S4[(size_t)ii[c] * (VR_VERT_FLOATS / 4) + 1];
                    v[3 * c + 0] = a.z;
                    v[3 * c + 1] = a.w;
                    v[3 * c + 2] = b.z;
                }
                const float area = (v[6] - v[0]) * (v[4] - v[1]) - (v[7] - v[1]) * (v[3] - v[0]);
                const float xlo = fminf(v[0], fminf(v[3], v[6])), xhi = fmaxf(v[0], fmaxf(v[3], v[6]));
                const float ylo = fminf(v[1], fminf(v[4], v[7])), yhi = fmaxf(v[1], fmaxf(v[4], v[7]));
                const bool ordinary = v[2] > 0.0f && v[5] > 0.0f && v[8] > 0.0f && fabsf(area) > 1e-4f * ((xhi - xlo) * (yhi - ylo));
                const bool off_tile = xlo > tx_hi || xhi < tx_lo || ylo > ty_hi || yhi < ty_lo;
                keep = !(fabsf(area) <= 1e-8f) && !(ordinary && off_tile); // (the first: the early-out of the loop below)
            }
        }
        const unsigned long long msk = __ballot(keep);
        __syncthreads(); // the previous pass's readers are done
        if (lane == 0) s_wcnt[wave] = __popcll(msk);
        __syncthreads();
        int at = __popcll(msk & ((1ull << lane) - 1ull)), cnt = 0;
        for (int w = 0; w < VR_BLOCK / 64; ++w) {
            if (w < wave) at += s_wcnt[w];
            cnt += s_wcnt[w];
        }
        if (keep) {
            for (int k = 0; k < 9; ++k) s_v[at][k] = v[k];
            s_id[at] = f;
        }
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const float* v0 = &s_v[k][0]; const float* v1 = &s_v[k][3]; const float* v2 = &s_v[k][6];
            // both windings are drawn (cull_backfaces False): the weights are edge functions over the signed area
            const float area = (v2[0] - v0[0]) * (v1[1] - v0[1]) - (v2[1] - v0[1]) * (v1[0] - v0[0]);
            if (fabsf(area) <= 1e-8f) continue;
            const float w0 = ((cx - v1[0]) * (v2[1] - v1[1]) - (cy - v1[1]) * (v2[0] - v1[0])) / area;
            const float w1 = ((cx - v2[0]) * (v0[1] - v2[1]) - (cy - v2[1]) * (v0[0] - v2[0])) / area;
            const float w2 = ((cx - v0[0]) * (v1[1] - v0[1]) - (cy - v0[1]) * (v1[0] - v0[0])) / area;
            const float t0 = w0 * (v1[2] * v2[2]), t1 = w1 * (v0[2] * v2[2]), t2 = w2 * (v0[2] * v1[2]);
            const float den = (t0 + t1) + t2;
            if (den == 0.0f) continue;
            const float b0 = t0 / den, b1 = t1 / den, b2 = t2 / den;
            const float pz = (b0 * v0[2] + b1 * v1[2]) + b2 * v2[2];
            if (pz < 0.0f) continue;
            if (!(b0 > 0.0f && b1 > 0.0f && b2 > 0.0f)) continue;
            if (pz < bestz) { bestz = pz; bf = s_id[k]; bb0 = b0; bb1 = b1; bb2 = b2; } // index order: the lower face wins a tie
        }
    }
    if (col >= W || row >= H) return;
    const int npix = H * W, pix = row * W + col;
    float r = 1.0f, g = 1.0f, b = 1.0f; // background (1, 1, 1): no face -> prob 0, delta = 1
    if (bf >= 0) {
        const int ids[3] = {F[3 * bf], F[3 * bf + 1], F[3 * bf + 2]};
        const float bw[3] = {bb0, bb1, bb2};
        float tex = 0.0f, d2 = INFINITY;
        float3 p = make_float3(0.0f, 0.0f, 0.0f), n = p;
        float nx[3], ny[3];
        for (int c = 0; c < 3; ++c) { // interpolate_face_attributes with the perspective-corrected barycentrics
            const float4* rec = S4 + (size_t)ids[c] * (VR_VERT_FLOATS / 4);
            const float4 a = rec[0], q = rec[1], wp = rec[2], vn = rec[3];
            nx[c] = a.z; ny[c] = a.w;
            tex += bw[c] * q.w;
            p.x += bw[c] * wp.x; p.y += bw[c] * wp.y; p.z += bw[c] * wp.z;
            n.x += bw[c] * vn.x; n.y += bw[c] * vn.y; n.z += bw[c] * vn.z;
        }
        n = normalize_eps(n);
        // Phong (pytorch3d phong_shading): ambient 0.5, diffuse 0.3, specular 0.2, shininess 64; light at (0, 0, -3), camera centre -T R^T
        const float3 l = normalize_eps(make_float3(0.0f - p.x, 0.0f - p.y, -3.0f - p.z));
        const float3 C = make_float3(-((Tv[0] * Rm[0] + Tv[1] * Rm[1]) + Tv[2] * Rm[2]), -((Tv[0] * Rm[3] + Tv[1] * Rm[4]) + Tv[2] * Rm[5]),
                                     -((Tv[0] * Rm[6] + Tv[1] * Rm[7]) + Tv[2] * Rm[8]));
        const float3 e = normalize_eps(make_float3(C.x - p.x, C.y - p.y, C.z - p.z));
        const float nl = dot3(n, l);
        const float diffuse = 0.3f * fmaxf(nl, 0.0f);
        const float3 refl = make_float3(2.0f * nl * n.x - l.x, 2.0f * nl * n.y - l.y, 2.0f * nl * n.z - l.z);
        float s = nl > 0.0f ? fmaxf(dot3(e, refl), 0.0f) : 0.0f;
        for (int k = 0; k < 6; ++k) s = s * s; // ^64
        const float spec = 0.2f * s;
        const float col_c = (0.5f + diffuse) * tex + spec;
        // softmax_rgb_blend, K = 1: prob = sigmoid(-dists / sigma) with dists = -(squared NDC distance to the nearest edge) inside the face
        for (int c = 0; c < 3; ++c) d2 = fminf(d2, seg_dist2(cx, cy, nx[c], ny[c], nx[(c + 1) % 3], ny[(c + 1) % 3]));
        const float sigma = 1e-4f, gamma = 1e-4f, eps = 1e-10f, znear = 1.0f, zfar = 100.0f;
        const float prob = 1.0f / (1.0f + expf(-(d2 / sigma)));
        const float z_inv = (zfar - bestz) / (zfar - znear);
        const float z_inv_max = fmaxf(z_inv, eps);
        const float wnum = prob * expf((z_inv - z_inv_max) / gamma);
        const float delta = fmaxf(expf((eps - z_inv_max) / gamma), eps);
        const float den = wnum + delta;
        const float c_out = (wnum * col_c + delta) / den; // the three channels share the colour (the texture is vert_vis on every channel)
        r = g = b = c_out;
    }
    rgb[pix] = r;
    rgb[npix + pix] = g;
    rgb[2 * npix + pix] = b;
    // src/render_vis.py:221-226: mean over the channels of rgb * 255, thresholded at 50
    const float mean = ((r * 255.0f + g * 255.0f) + b * 255.0f) / 3.0f;
    vis[pix] = mean >= 50.0f ? 1.0f : 0.0f;
    if (pix_to_face) pix_to_face[pix] = bf;
    if (zbuf) zbuf[pix] = bf >= 0 ? bestz : -1.0f;
}

} // namespace

extern "C" int vanerf_render_vis(const float* verts, int nv, const int32_t* faces, int nf, const float* vert_vis, const float* R, const float* T,
                                 const float* focal, const float* princpt, int H, int W, float* scratch, int64_t scratch_bytes, float* rgb,
                                 float* vis, int32_t* pix_to_face, float* zbuf, void* stream)
{
    return guarded([&] {
        if (!verts || !faces || !vert_vis || !R || !T || !focal || !princpt || !scratch || !rgb || !vis)
            throw_error("vanerf_render_vis: null argument");
        if (nv <= 0 || nf <= 0 || nf > (1 << 28) || H <= 0 || W <= 0 || H > 4096 || W > 4096)
            throw_error("vanerf_render_vis: nv=%d nf=%d H=%d W=%d (positive; nf <= 2^28, H and W <= 4096)", nv, nf, H, W);
        const int64_t need = (int64_t)nv * VR_VERT_FLOATS * (int64_t)sizeof(float);
        if (scratch_bytes < need) throw_error("vanerf_render_vis: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
        if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0) throw_error("vanerf_render_vis: scratch must be 16-byte aligned");
        hipStream_t st = (hipStream_t)stream;
        const int vblocks = (nv + VR_BLOCK / 64 - 1) / (VR_BLOCK / 64);
        hipLaunchKernelGGL(vis_vertex_kernel, dim3((unsigned)vblocks), dim3(VR_BLOCK), 0, st, verts, nv, faces, nf, vert_vis, R, T, focal, princpt, H, W,
                           scratch);
        const int tiles = ((W + VR_T - 1) / VR_T) * ((H + VR_T - 1) / VR_T);
        hipLaunchKernelGGL(vis_raster_kernel, dim3((unsigned)tiles), dim3(VR_BLOCK), 0, st, faces, nf, nv, scratch, R, T, H, W, rgb, vis, pix_to_face,
                           zbuf);
        HIP_CHECK(hipGetLastError());
    });
}
