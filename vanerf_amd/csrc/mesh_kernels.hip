// mesh_kernels.hip -- mesh-geometry inputs of the per-sample networks:
//   cal_vis_sdf_batch   src/lib/dataset/mesh_util.py:498-524 (kaolin point_to_mesh_distance / check_sign)
//   get_visibility      src/lib/dataset/mesh_util.py:284-318 (pytorch3d rasterize_meshes)
//   knn_points (K=1)    src/networks.py:28
// The arithmetic is the operation-for-operation twin of oracle/mesh_oracle.c (third-party semantics, parity
// unpinned against the reference; bit-exact against the oracle).  Built with -ffp-contract=off.
// This file holds the exhaustive kernels and the visibility raster.  The per-triangle arithmetic is in mesh_device.h; the accelerated
// cal_vis_sdf_batch / knn_points is mesh_accel_query.hip, on the tables that mesh_accel_build.hip makes.
#include "mesh_device.h"

using namespace vanerf;

namespace {

constexpr int MQ_BLOCK = 256;
constexpr int MQ_TILE = 512; // triangles staged per LDS tile

__global__ __launch_bounds__(MQ_BLOCK) void mesh_query_kernel(const float* __restrict__ V, const int32_t* __restrict__ F, int nf,
                                                              const float* __restrict__ vert_vis, const float* __restrict__ P,
                                                              long long n, float* __restrict__ sdf, uint8_t* __restrict__ vis,
                                                              int32_t* __restrict__ face)
{
    __shared__ float s_tri[MQ_TILE][9];
    __shared__ int s_idx[MQ_TILE][3];
    const long long i = (long long)blockIdx.x * MQ_BLOCK + threadIdx.x;
    const bool live = i < n;
    const long long ii = live ? i : n - 1;
    const f3 p = {P[3 * ii], P[3 * ii + 1], P[3 * ii + 2]};
    float best = INFINITY;
    int bf = 0, cnt = 0, cnt0 = 0; // cnt0: crossings by the earlier tie rule, for a point at distance exactly 0 (edges_agree)
    for (int f0 = 0; f0 < nf; f0 += MQ_TILE) {
        const int m = min(MQ_TILE, nf - f0);
        __syncthreads();
        for (int k = threadIdx.x; k < m * 3; k += MQ_BLOCK) {
            const int f = k / 3, c = k % 3;
            const int vi = F[3 * (f0 + f) + c];
            s_idx[f][c] = vi;
            s_tri[f][3 * c + 0] = V[3 * vi]; s_tri[f][3 * c + 1] = V[3 * vi + 1]; s_tri[f][3 * c + 2] = V[3 * vi + 2];
        }
        __syncthreads();
        for (int f = 0; f < m; ++f) {
            const f3 a = {s_tri[f][0], s_tri[f][1], s_tri[f][2]}, b = {s_tri[f][3], s_tri[f][4], s_tri[f][5]},
                     c = {s_tri[f][6], s_tri[f][7], s_tri[f][8]};
            const float d = point_tri_dist2(p, a, b, c);
            if (d < best) { best = d; bf = f0 + f; }
            // +x ray parity (oracle/mesh_oracle.c:point_inside)
            const int i0 = s_idx[f][0], i1 = s_idx[f][1], i2 = s_idx[f][2];
            float E0, E1, E2;
            bool by_index;
            const bool agree = edges_agree(a, b, c, i0, i1, i2, p.y, p.z, E0, E1, E2, by_index);
            if ((agree || by_index) && crosses_beyond(E0, E1, E2, a, b, c, p.x)) { cnt += agree; cnt0 += by_index; }
        }
    }
    if (!live) return;
    const float dist = sqrtf(best + 1e-6f);
    if (best == 0.0f) cnt = cnt0;
    sdf[i] = (cnt & 1) ? -dist : dist;
    if (face) face[i] = bf;
    vis[i] = face_visible(V, F, vert_vis, bf, p);
}

// get_visibility: one thread per raster pixel, one block per 16 x 16 pixel tile.  Faces are streamed through LDS 256 at a time; a face is
// staged only if it can cover a pixel centre of the tile (front facing, not degenerate, bounding box within 1e-3 units of the tile -- the
// inside test of a pixel further than that from the box of an ordinary face fails in fp32 whatever the rounding; faces with a vertex behind
// the camera plane and needles are staged for every tile).  The staged faces keep their order (the first of equal depths wins, as in the full scan),
// and the per-pixel arithmetic is unchanged, so the result is the full scan's, bit for bit (13 x fewer tests on the two-hand mesh).
constexpr int RV_BLOCK = 256;
constexpr int RV_T = 16;

__global__ __launch_bounds__(RV_BLOCK) void raster_kernel(const float* __restrict__ xy01, const float* __restrict__ z01,
                                                          const int32_t* __restrict__ F, int nf, int S, int32_t* __restrict__ pix_to_face)
{
    __shared__ float s_v[RV_BLOCK][9];
    __shared__ int s_id[RV_BLOCK];
    __shared__ int s_wcnt[RV_BLOCK / 64];
    const int tiles_x = (S + RV_T - 1) / RV_T;
    const int px0 = (blockIdx.x % tiles_x) * RV_T, py0 = (blockIdx.x / tiles_x) * RV_T;
    const int px = px0 + (threadIdx.x & (RV_T - 1)), py = py0 + threadIdx.x / RV_T;
    const bool live = px < S && py < S;
    const float cx = -1.0f + (2.0f * (float)px + 1.0f) / (float)S;
    const float cy = -1.0f + (2.0f * (float)py + 1.0f) / (float)S;
    const float tol = 1e-3f;
    const float tx_lo = -1.0f + (2.0f * (float)px0 + 1.0f) / (float)S - tol, tx_hi = -1.0f + (2.0f * (float)min(px0 + RV_T - 1, S - 1) + 1.0f) / (float)S + tol;
    const float ty_lo = -1.0f + (2.0f * (float)py0 + 1.0f) / (float)S - tol, ty_hi = -1.0f + (2.0f * (float)min(py0 + RV_T - 1, S - 1) + 1.0f) / (float)S + tol;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float bestz = INFINITY;
    int bf = -1;
    for (int f0 = 0; f0 < nf; f0 += RV_BLOCK) {
        const int f = f0 + threadIdx.x;
        float v[9];
        bool keep = false;
        if (f < nf) {
            for (int c = 0; c < 3; ++c) {
                const int vi = F[3 * f + c];
                v[3 * c + 0] = (xy01[2 * vi] + 1.0f) / 2.0f;
                v[3 * c + 1] = (xy01[2 * vi + 1] + 1.0f) / 2.0f;
                v[3 * c + 2] = (z01[vi] + 1.0f) / 2.0f;
            }
            const float area = (v[6] - v[0]) * (v[4] - v[1]) - (v[7] - v[1]) * (v[3] - v[0]);
            const float xlo = fminf(v[0], fminf(v[3], v[6])), xhi = fmaxf(v[0], fmaxf(v[3], v[6]));
            const float ylo = fminf(v[1], fminf(v[4], v[7])), yhi = fmaxf(v[1], fmaxf(v[4], v[7]));
            // the box test only speaks for an ordinary face: all three depths positive (then the signs of the perspective-corrected weights are
            // the signs of the edge functions) and not a needle (area against its box: the edge functions of a needle cancel to rounding noise)
            const bool ordinary = v[2] > 0.0f && v[5] > 0.0f && v[8] > 0.0f && area > 1e-4f * ((xhi - xlo) * (yhi - ylo));
            const bool off_tile = xlo > tx_hi || xhi < tx_lo || ylo > ty_hi || yhi < ty_lo;
            keep = !(area < 0.0f) && !(fabsf(area) <= 1e-8f) && !(ordinary && off_tile); // (the first two: the early-outs of the loop below)
        }
        const unsigned long long m = __ballot(keep);
        __syncthreads(); // the previous pass's readers are done
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int at = __popcll(m & ((1ull << lane) - 1ull)), cnt = 0;
        for (int w = 0; w < RV_BLOCK / 64; ++w) {
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
            const float area = (v2[0] - v0[0]) * (v1[1] - v0[1]) - (v2[1] - v0[1]) * (v1[0] - v0[0]);
            if (area < 0.0f) continue;
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
            if (pz < bestz) { bestz = pz; bf = s_id[k]; }
        }
    }
    if (live) pix_to_face[py * S + px] = bf;
}

__global__ void mark_visible_kernel(const int32_t* __restrict__ pix_to_face, int npix, const int32_t* __restrict__ F, int nf,
                                    float* __restrict__ vert_vis)
{
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    int f = pix_to_face[pix];
    if (f < 0) f = nf - 1; // faces[-1] through the background id (mesh_util.py:314)
    vert_vis[F[3 * f]] = 1.0f; vert_vis[F[3 * f + 1]] = 1.0f; vert_vis[F[3 * f + 2]] = 1.0f;
}

__global__ __launch_bounds__(256) void knn1_kernel(const float4* __restrict__ verts, int nv, const float* __restrict__ pts, long long n,
                                                   int32_t* __restrict__ idx)
{
    extern __shared__ float4 s_vv[];
    for (int i = threadIdx.x; i < nv; i += blockDim.x) s_vv[i] = verts[i];
    __syncthreads();
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float qx = pts[3 * i], qy = pts[3 * i + 1], qz = pts[3 * i + 2];
    float best = INFINITY;
    int bi = 0;
    for (int j = 0; j < nv; ++j) {
        const float4 v = s_vv[j];
        const float dx = qx - v.x, dy = qy - v.y, dz = qz - v.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (d < best) { best = d; bi = j; }
    }
    idx[i] = bi;
}

} // namespace

extern "C" int vanerf_vertex_visibility(const float* vert_xy01, const float* vert_z01, int nv, const int32_t* faces, int nf,
                                        int raster, int32_t* pix_to_face, float* vert_vis, void* stream)
{
    return guarded([&] {
        if (!vert_xy01 || !vert_z01 || !faces || !pix_to_face || !vert_vis) throw_error("vanerf_vertex_visibility: null argument");
        if (nv <= 0 || nf <= 0 || raster <= 0 || raster > 4096) throw_error("vanerf_vertex_visibility: nv=%d nf=%d raster=%d", nv, nf, raster);
        hipStream_t st = (hipStream_t)stream;
        const int npix = raster * raster;
        HIP_CHECK(hipMemsetAsync(vert_vis, 0, sizeof(float) * nv, st));
        const int tiles = (raster + RV_T - 1) / RV_T;
        hipLaunchKernelGGL(raster_kernel, dim3((unsigned)(tiles * tiles)), dim3(RV_BLOCK), 0, st, vert_xy01, vert_z01, faces, nf, raster, pix_to_face);
        hipLaunchKernelGGL(mark_visible_kernel, dim3((npix + 255) / 256), dim3(256), 0, st, pix_to_face, npix, faces, nf, vert_vis);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_mesh_query(const float* verts, int nv, const int32_t* faces, int nf, const float* vert_vis, const float* pts,
                                 int64_t n, float* sdf, uint8_t* vis, int32_t* face, void* stream)
{
    return guarded([&] {
        if (n == 0) return;
        if (!verts || !faces || !vert_vis || !pts || !sdf || !vis) throw_error("vanerf_mesh_query: null argument");
        if (nv <= 0 || nf <= 0 || n < 0) throw_error("vanerf_mesh_query: nv=%d nf=%d n=%lld", nv, nf, (long long)n);
        if (n == 0) return;
        hipLaunchKernelGGL(mesh_query_kernel, dim3((unsigned)((n + MQ_BLOCK - 1) / MQ_BLOCK)), dim3(MQ_BLOCK), 0, (hipStream_t)stream,
                           verts, faces, nf, vert_vis, pts, (long long)n, sdf, vis, face);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_knn1(const float* verts4, int nv, const float* pts, int64_t n, int32_t* idx, void* stream)
{
    return guarded([&] {
        if (n == 0) return;
        if (!verts4 || !pts || !idx) throw_error("vanerf_knn1: null argument");
        if (nv <= 0 || nv > 8192 || n < 0) throw_error("vanerf_knn1: nv=%d n=%lld", nv, (long long)n);
        if (n == 0) return;
        hipLaunchKernelGGL(knn1_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), sizeof(float4) * nv, (hipStream_t)stream,
                           reinterpret_cast<const float4*>(verts4), nv, pts, (long long)n, idx);
        HIP_CHECK(hipGetLastError());
    });
}
