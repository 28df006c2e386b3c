// mano_skin_backward.hip -- the vector-Jacobian product of vanerf_mano_skin (the definition is the comment of
// vanerf_mano_skin in the header, steps 1-7): gradients of the vertices and joints -> gradients of pose, betas and trans, on the device, for a
// batch of poses.  Stateless: what the forward computed is recomputed from pose and betas by the forward's own functions (mano_forward.h).
// The restatement the tests hold these kernels to is the torch code of tests/test_mano_backward_cpu.py under fp64 autograd.
//
// Three launches per call, all on the caller's stream:
//   mano_bwd_joint_forward_kernel  one wave per pose, fp64: joint_forward(); A (nj x 12) and the pose feature ((nj-1) x 9) rounded once to
//                                  fp32 into the workspace.
//   mano_bwd_vertex_kernel         one block per pose and chunk of 256 vertices.  Phase 1, one lane per vertex, fp32: vertex_forward() for
//                                  x = v_posed and T = sum_j w A_j, the seal's share folded into the ring vertices' gradient g,
//                                  g_x = T^R^T g; g_x, g and x staged in LDS.  Phase 2, one wave per output value (or per joint's twelve):
//                                  lanes over the chunk's vertices with coalesced reads of the [row][k][v] tables, fp32 products summed in
//                                  fp64, a butterfly over the wave, one fp64 partial per (pose, chunk, value) into the workspace.
//   mano_bwd_joint_kernel          one wave per pose, fp64: joint_forward(), the chunks' partials summed in chunk order, the chain in reverse
//                                  (j = nj-1 .. 1 into parents[j]), the Rodrigues backward per joint, J_shapedirs^T . dJ; rounded once to fp32.
// A and the pose feature sit in LDS and are read with wave-uniform indices.  No atomics, no device-side state, every requested output
// element written, every sum in one fixed order: a pose's gradient bits depend neither on P nor on its row in the batch.
#include "common.h"
#include "mano_forward.h"
#include "mano_tables.h"

#include <cmath>
#include <cstdint>

using namespace vanerf;
using namespace vanerf::mano;

namespace {

constexpr int BW_CHUNK = MV_BLOCK;                                                                 // vertices per block of the vertex kernel
constexpr int BW_MAX_OUT = MANO_MAX_NJ * 12 + (MANO_MAX_NJ - 1) * 9 + MANO_MAX_NB + 3;            // values reduced over the vertices, per pose
static_assert(BW_CHUNK == 256, "phase 2 of mano_bwd_vertex_kernel gives a lane four vertices of a chunk");

inline int n_out(int nj, int nb) { return nj * 12 + (nj - 1) * 9 + nb + 3; } // dA, then df, then the direct part of grad_betas, then grad_trans

__global__ __launch_bounds__(64) void mano_bwd_joint_forward_kernel(const ManoTables t, int nj, int nb, const float* __restrict__ pose, int64_t pose_stride,
                                                                   const float* __restrict__ betas, int64_t betas_stride, int flat_hand_mean,
                                                                   float* __restrict__ ws)
{
    __shared__ double sr[MANO_MAX_NJ][3], sR[MANO_MAX_NJ][9], sJ[MANO_MAX_NJ][3], sG[MANO_MAX_NJ][12];
    const size_t p = blockIdx.x;
    float* A = ws + p * (size_t)(nj * 12 + (nj - 1) * 9);
    joint_forward(t, nj, nb, pose + p * pose_stride, betas + p * betas_stride, flat_hand_mean, threadIdx.x, sr, sR, sJ, sG, A, A + nj * 12);
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// vertices: one block per pose and chunk of 256 vertices
// ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BW_CHUNK) void mano_bwd_vertex_kernel(const ManoTables t, int nv, int nj, int nb, int nchunk, const float* __restrict__ betas,
                                                                  int64_t betas_stride, const float* __restrict__ ws,
                                                                  const float* __restrict__ grad_verts, int64_t gv_stride, const IntList64 ring,
                                                                  int n_ring, double* __restrict__ partial)
{
    __shared__ float sA[MANO_MAX_NJ * 12], sf[(MANO_MAX_NJ - 1) * 9 + 1], sb[MANO_MAX_NB], st[9][BW_CHUNK];
    const size_t p = blockIdx.x / (unsigned)nchunk;
    const int ch = (int)(blockIdx.x % (unsigned)nchunk);
    const int rows = (nj - 1) * 9, wsf = nj * 12 + rows, tid = threadIdx.x;
    for (int i = tid; i < wsf + nb; i += BW_CHUNK) {
        if (i < nj * 12) sA[i] = ws[p * wsf + i];
        else if (i < wsf) sf[i - nj * 12] = ws[p * wsf + i];
        else sb[i - wsf] = betas[p * betas_stride + (i - wsf)];
    }
    __syncthreads();
    const size_t n = (size_t)nv;
    const int v = ch * BW_CHUNK + tid;
    float g[3] = {0.0f, 0.0f, 0.0f}, x[3] = {0.0f, 0.0f, 0.0f}, gx[3] = {0.0f, 0.0f, 0.0f};
    if (v < nv) {
        float T[12]; // (only T's rotation is read: its translation's sums are dead code)
        vertex_forward<1>(t, v, nv, nj, nb, PoseValues{sA, sf, sb, nullptr, 0}, &x, &T, nullptr);
        // g: the vertex's own gradient, and 1 / n_ring of the sealed vertex's for every time the ring names this vertex
        const float* gv = grad_verts + p * gv_stride;
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = gv[(size_t)v * 3 + k];
        if (n_ring > 0) {
            const float inv = 1.0f / (float)n_ring;
            const float s0 = gv[n * 3] * inv, s1 = gv[n * 3 + 1] * inv, s2 = gv[n * 3 + 2] * inv;
#pragma unroll
            for (int u = 0; u < MANO_MAX_RING; ++u) {
                if (u < n_ring && ring.v[u] == v) {
                    g[0] = g[0] + s0;
                    g[1] = g[1] + s1;
                    g[2] = g[2] + s2;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) gx[c] = (T[c] * g[0] + T[4 + c] * g[1]) + T[8 + c] * g[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        st[k][tid] = gx[k];
        st[3 + k][tid] = g[k];
        st[6 + k][tid] = x[k];
    }
    __syncthreads();
    // phase 2: a lane takes the chunk's vertices lane, lane + 64, lane + 128, lane + 192; a wave one output value (or one joint) at a time
    const int wave = tid >> 6, lane = tid & 63, v0 = ch * BW_CHUNK;
    float rgx[4][3], rg[4][3], rx[4][3];
    bool ok[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        ok[m] = v0 + lane + 64 * m < nv;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            rgx[m][k] = st[k][lane + 64 * m];
            rg[m][k] = st[3 + k][lane + 64 * m];
            rx[m][k] = st[6 + k][lane + 64 * m];
        }
    }
    double* out = partial + (p * (size_t)nchunk + ch) * (size_t)(wsf + nb + 3);
    // df = posedirs . g_x, then the direct part of grad_betas = shapedirs^T . g_x
    for (int it = wave; it < rows + nb; it += 4) {
        const float* tab = it < rows ? t.pd + (size_t)(it * 3) * n : t.sd + (size_t)((it - rows) * 3) * n;
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const size_t vv = (size_t)(v0 + lane + 64 * m);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float tv = ok[m] ? tab[(size_t)k * n + vv] : 0.0f;
                acc = acc + (double)(tv * rgx[m][k]);
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) out[nj * 12 + it] = acc;
    }
    // dA_j = sum over v of w_vj g (x, 1)^T
    for (int j = wave; j < nj; j += 4) {
        double acc[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) acc[e] = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float w = ok[m] ? t.wt[(size_t)j * n + (size_t)(v0 + lane + 64 * m)] : 0.0f;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float wg = w * rg[m][r];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[r * 4 + c] = acc[r * 4 + c] + (double)(wg * rx[m][c]);
                acc[r * 4 + 3] = acc[r * 4 + 3] + (double)wg;
            }
        }
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            const double a = wave_sum(acc[e]);
            if (lane == 0) out[j * 12 + e] = a;
        }
    }
    // grad_trans = sum over v of g
    if (wave == 3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < 4; ++m) acc = acc + (double)rg[m][k];
            acc = wave_sum(acc);
            if (lane == 0) out[wsf + nb + k] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// joints: one wave per pose, fp64
// ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void mano_bwd_joint_kernel(const ManoTables t, int nj, int nb, const float* __restrict__ pose, int64_t pose_stride,
                                                           const float* __restrict__ betas, int64_t betas_stride, int flat_hand_mean,
                                                           const double* __restrict__ partial, int nchunk, const float* __restrict__ grad_joints,
                                                           int64_t gj_stride, float* __restrict__ grad_pose, int64_t gp_stride,
                                                           float* __restrict__ grad_betas, int64_t gb_stride, float* __restrict__ grad_trans,
                                                           int64_t gt_stride)
{
    __shared__ double sr[MANO_MAX_NJ][3], sR[MANO_MAX_NJ][9], sJ[MANO_MAX_NJ][3], sG[MANO_MAX_NJ][12];
    __shared__ double sdG[MANO_MAX_NJ][12], sdR[MANO_MAX_NJ][9], sdJ[MANO_MAX_NJ][3], sgj[MANO_MAX_NJ][3], sIn[BW_MAX_OUT];
    const size_t p = blockIdx.x;
    const int lane = threadIdx.x;
    joint_forward(t, nj, nb, pose + p * pose_stride, betas + p * betas_stride, flat_hand_mean, lane, sr, sR, sJ, sG, nullptr, nullptr);
    const int rows = (nj - 1) * 9, nout = nj * 12 + rows + nb + 3;
    // the vertex side's sums: the chunks' partials in chunk order (zeros when no vertex gradient came in)
    for (int o = lane; o < nout; o += 64) {
        double s = 0.0;
        if (partial)
            for (int c = 0; c < nchunk; ++c) s = s + partial[(p * (size_t)nchunk + c) * (size_t)nout + o];
        sIn[o] = s;
    }
    if (lane < nj)
        for (int k = 0; k < 3; ++k) sgj[lane][k] = grad_joints ? (double)grad_joints[p * gj_stride + 3 * lane + k] : 0.0;
    __syncthreads();
    // A_j = [G^R | G^t - G^R J_j], joint_j = G^t + trans
    if (lane < nj) {
        const double* dA = sIn + lane * 12;
        const double* G = sG[lane];
        for (int r = 0; r < 3; ++r) {
            sdG[lane][r * 4 + 3] = dA[r * 4 + 3] + sgj[lane][r];
            for (int c = 0; c < 3; ++c) sdG[lane][r * 4 + c] = dA[r * 4 + c] - dA[r * 4 + 3] * sJ[lane][c];
        }
        for (int c = 0; c < 3; ++c) sdJ[lane][c] = -((G[c] * dA[3] + G[4 + c] * dA[7]) + G[8 + c] * dA[11]);
    }
    __syncthreads();
    // the chain in reverse: G_j^R = Gp^R R_j, G_j^t = Gp^R (J_j - J_par) + Gp^t; every child of a joint comes before the joint itself
    for (int j = nj - 1; j >= 1; --j) {
        const int par = parent_of(t, j);
        const double* Gp = sG[par];
        const double* dG = sdG[j];
        if (lane < 9) {
            const int r = lane / 3, c = lane % 3;
            sdR[j][lane] = (Gp[r] * dG[c] + Gp[4 + r] * dG[4 + c]) + Gp[8 + r] * dG[8 + c];
            const double l = sJ[j][c] - sJ[par][c];
            const double add = ((dG[r * 4] * sR[j][c * 3] + dG[r * 4 + 1] * sR[j][c * 3 + 1]) + dG[r * 4 + 2] * sR[j][c * 3 + 2]) + dG[r * 4 + 3] * l;
            sdG[par][r * 4 + c] = sdG[par][r * 4 + c] + add;
        } else if (lane < 12) {
            const int k = lane - 9;
            const double dl = (Gp[k] * dG[3] + Gp[4 + k] * dG[7]) + Gp[8 + k] * dG[11];
            sdJ[j][k] = sdJ[j][k] + dl;
            sdJ[par][k] = sdJ[par][k] - dl;
            sdG[par][k * 4 + 3] = sdG[par][k * 4 + 3] + dG[k * 4 + 3];
        }
        __syncthreads();
    }
    if (lane < 9) sdR[0][lane] = sdG[0][(lane / 3) * 4 + lane % 3]; // the root: L_0 = [R_0 | J_0]
    else if (lane < 12) sdJ[0][lane - 9] = sdJ[0][lane - 9] + sdG[0][(lane - 9) * 4 + 3];
    __syncthreads();
    // Rodrigues backward, lane j: R = I + sin(a) K + (1 - cos(a)) K K, K = skew(r / a), a = |r + 1e-8|
    if (grad_pose && lane < nj) {
        double M[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) M[e] = sdR[lane][e] + (lane >= 1 ? sIn[nj * 12 + (lane - 1) * 9 + e] : 0.0);
        const double* r = sr[lane];
        const RodriguesTerms q = rodrigues_terms(r);
        const double a = q.a, s = q.s, co = q.co, c1 = q.c1;
        const double *e = q.e, *K = q.K, *K2 = q.K2;
        double dK[9], ds = 0.0, dc1 = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            ds = ds + M[e] * K[e];
            dc1 = dc1 + M[e] * K2[e];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double mkt = (M[i * 3] * K[k * 3] + M[i * 3 + 1] * K[k * 3 + 1]) + M[i * 3 + 2] * K[k * 3 + 2]; // (M K^T)[i][k]
                const double ktm = (K[i] * M[k] + K[3 + i] * M[3 + k]) + K[6 + i] * M[6 + k];                         // (K^T M)[i][k]
                dK[i * 3 + k] = s * M[i * 3 + k] + c1 * (mkt + ktm);
            }
        const double dd0 = dK[7] - dK[5], dd1 = dK[2] - dK[6], dd2 = dK[3] - dK[1];
        const double da = (ds * co + dc1 * s) - ((dd0 * r[0] + dd1 * r[1]) + dd2 * r[2]) / (a * a);
        float* o = grad_pose + p * gp_stride + 3 * lane;
        o[0] = (float)(dd0 / a + da * (e[0] / a));
        o[1] = (float)(dd1 / a + da * (e[1] / a));
        o[2] = (float)(dd2 / a + da * (e[2] / a));
    }
    // grad_betas = shapedirs^T . g_x + J_shapedirs^T . dJ
    if (grad_betas && lane < nb) {
        double s = sIn[nj * 12 + rows + lane];
        for (int j = 0; j < nj; ++j)
            for (int k = 0; k < 3; ++k) s = s + t.Js[(j * 3 + k) * nb + lane] * sdJ[j][k];
        grad_betas[p * gb_stride + lane] = (float)s;
    }
    // grad_trans = sum of the vertices' gradients + sum of the joints'
    if (grad_trans && lane >= 32 && lane < 35) {
        const int k = lane - 32;
        double s = sIn[nj * 12 + rows + nb + k];
        for (int j = 0; j < nj; ++j) s = s + sgj[j][k];
        grad_trans[p * gt_stride + k] = (float)s;
    }
}

int64_t bw_partial_bytes(int nv, int nj, int nb, int P)
{
    const int64_t nchunk = ((int64_t)nv + BW_CHUNK - 1) / BW_CHUNK;
    return (int64_t)P * nchunk * n_out(nj, nb) * 8;
}

} // namespace

extern "C" int64_t vanerf_mano_skin_backward_workspace_bytes(int nv, int nj, int nb, int P)
{
    return size_query([&] {
        const char* who = "vanerf_mano_skin_backward_workspace_bytes";
        check_sizes(who, nv, nj, nb);
        if (P < 0) throw_error("%s: P=%d poses (at least 0)", who, P);
        return bw_partial_bytes(nv, nj, nb, P) + (int64_t)P * ws_floats(nj) * 4; // the fp64 partials first, then A and the pose feature
    });
}

extern "C" int vanerf_mano_skin_backward(const void* packed, int nv, int nj, int nb, const float* pose, int64_t pose_stride, const float* betas,
                                         int64_t betas_stride, int P, int flat_hand_mean, const int32_t* ring, int n_ring, const float* grad_verts,
                                         int64_t grad_verts_stride, const float* grad_joints, int64_t grad_joints_stride, void* workspace,
                                         int64_t workspace_bytes, float* grad_pose, int64_t grad_pose_stride, float* grad_betas,
                                         int64_t grad_betas_stride, float* grad_trans, int64_t grad_trans_stride, void* stream)
{
    return guarded([&] {
        const char* who = "vanerf_mano_skin_backward";
        check_sizes(who, nv, nj, nb);
        if (P < 0) throw_error("%s: P=%d poses (at least 0)", who, P);
        const IntList64 rg = ring_list(who, ring, n_ring, nv);
        check_stride(who, "pose", pose_stride, nj * 3);
        check_stride(who, "betas", betas_stride, nb);
        if (grad_verts) check_stride(who, "grad_verts", grad_verts_stride, ((int64_t)nv + (n_ring > 0 ? 1 : 0)) * 3);
        if (grad_joints) check_stride(who, "grad_joints", grad_joints_stride, nj * 3);
        if (grad_pose) check_stride(who, "grad_pose", grad_pose_stride, nj * 3);
        if (grad_betas) check_stride(who, "grad_betas", grad_betas_stride, nb);
        if (grad_trans) check_stride(who, "grad_trans", grad_trans_stride, 3);
        if (P == 0) return;
        if (!packed || !pose || !betas) throw_error("%s: null argument", who);
        if (!grad_verts && !grad_joints) throw_error("%s: null argument (grad_verts and grad_joints are both null: nothing to differentiate)", who);
        if ((uintptr_t)packed & 15) throw_error("%s: packed must be 16-byte aligned", who);
        if (!grad_pose && !grad_betas && !grad_trans) return; // nothing wanted
        const int64_t part = bw_partial_bytes(nv, nj, nb, P), need = grad_verts ? part + (int64_t)P * ws_floats(nj) * 4 : 0;
        if (need > 0 && !workspace) throw_error("%s: null argument (workspace)", who);
        if (workspace_bytes < need)
            throw_error("%s: workspace_bytes=%lld, %d poses need %lld (vanerf_mano_skin_backward_workspace_bytes)", who, (long long)workspace_bytes, P, (long long)need);
        if (need > 0 && ((uintptr_t)workspace & 7)) throw_error("%s: workspace must be 8-byte aligned", who);
        const int nchunk = (nv + BW_CHUNK - 1) / BW_CHUNK;
        const unsigned b_v = blocks_of(who, (int64_t)P * nchunk, 1);
        const ManoTables t = mano_tables(packed, nv, nj, nb);
        double* partial = grad_verts ? static_cast<double*>(workspace) : nullptr;
        if (grad_verts) {
            float* ws = reinterpret_cast<float*>(static_cast<char*>(workspace) + part);
            hipLaunchKernelGGL(mano_bwd_joint_forward_kernel, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, t, nj, nb, pose, pose_stride, betas,
                               betas_stride, flat_hand_mean, ws);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(mano_bwd_vertex_kernel, dim3(b_v), dim3(BW_CHUNK), 0, (hipStream_t)stream, t, nv, nj, nb, nchunk, betas, betas_stride, ws,
                               grad_verts, grad_verts_stride, rg, n_ring, partial);
            HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(mano_bwd_joint_kernel, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, t, nj, nb, pose, pose_stride, betas, betas_stride,
                           flat_hand_mean, partial, nchunk, grad_joints, grad_joints_stride, grad_pose, grad_pose_stride, grad_betas, grad_betas_stride,
                           grad_trans, grad_trans_stride);
        HIP_CHECK(hipGetLastError());
    });
}
