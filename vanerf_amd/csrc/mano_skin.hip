// mano_skin.hip -- linear blend skinning of a MANO-shaped model for a batch of poses (the comment of vanerf_mano_skin in
// the header): pose, shape and translation parameters -> the frame's vertices and joints, on the device, no host read.  The restatement the
// tests hold these kernels to is the numpy code of tests/test_mano_skin_cpu.py.
//
// Three stages per call, all on the caller's stream:
//   mano_joint_kernel   one wave per pose: joint_forward() of mano_forward.h.  All fp64, as the small fp64 cores of vis_vertex_kernel and
//                       pose_transforms_kernel.  A (nj x 12) and the pose feature ((nj - 1) x 9, R_j - I) are rounded once to fp32 into the
//                       workspace; the joints are rounded once into the output.
//   mano_vertex_kernel  one lane per vertex and MANO_POSES_PER_LANE poses per lane: vertex_forward() of mano_forward.h.  A, the pose feature,
//                       betas and trans of the block's poses sit in LDS.  A pose's bits depend neither on P nor on its place in the batch.
//   mano_seal_kernel    the appended wrist vertex: the fp32 sum of the WRITTEN ring vertices in the ring's order, from the left, times 1 / n.
// The pack (once per model) transposes the tables and folds J_regressor into the template and the shape directions in fp64, so that J costs
// 3 nj nb products per pose instead of a pass over the vertices.  No atomics, no device-side state; every output element is written.
#include "common.h"
#include "mano_forward.h"
#include "mano_tables.h"

#include <cmath>
#include <cstdint>

using namespace vanerf;
using namespace vanerf::mano;

#ifndef MANO_POSES_PER_LANE
#define MANO_POSES_PER_LANE 4 // poses a lane of mano_vertex_kernel carries (tools/perf_mano.py times builds with another count)
#endif

namespace {

constexpr int PP = MANO_POSES_PER_LANE;
static_assert(PP >= 1 && PP <= 16, "MANO_POSES_PER_LANE: 1 .. 16");

// (the packed model's layout, the limits and the entries' host-side helpers: mano_tables.h; the forward's arithmetic: mano_forward.h)

// ------------------------------------------------------------------------------------------------------------------------------------------
// pack
// ------------------------------------------------------------------------------------------------------------------------------------------
// One thread per value of the transposed fp32 tables.
__global__ __launch_bounds__(MV_BLOCK) void mano_pack_tables_kernel(const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                                                                   const float* __restrict__ posedirs, const float* __restrict__ weights, int nv, int nj,
                                                                   int nb, float* __restrict__ vt, float* __restrict__ sd, float* __restrict__ pd,
                                                                   float* __restrict__ wt)
{
    const size_t i = (size_t)blockIdx.x * MV_BLOCK + threadIdx.x;
    const size_t n_vt = (size_t)3 * nv, n_sd = (size_t)nb * 3 * nv, n_pd = (size_t)(nj - 1) * 9 * 3 * nv, n_wt = (size_t)nj * nv;
    if (i < n_vt) {
        const size_t k = i / nv, v = i % nv;
        vt[i] = v_template[v * 3 + k];
    } else if (i < n_vt + n_sd) {
        const size_t o = i - n_vt, b = o / ((size_t)3 * nv), k = o / nv % 3, v = o % nv;
        sd[o] = shapedirs[(v * 3 + k) * nb + b];
    } else if (i < n_vt + n_sd + n_pd) {
        const size_t o = i - n_vt - n_sd, row = o / ((size_t)3 * nv), k = o / nv % 3, v = o % nv;
        pd[o] = posedirs[row * ((size_t)3 * nv) + v * 3 + k];
    } else if (i < n_vt + n_sd + n_pd + n_wt) {
        const size_t o = i - n_vt - n_sd - n_pd, j = o / nv, v = o % nv;
        wt[o] = weights[v * nj + j];
    }
}

// One thread per value of the joint tables: (j, k, c), c = 0 the template and c = 1 + b shape direction b; the sum over the vertices in
// fp64, from vertex 0 upwards.  The first threads also write hands_mean as doubles and the parents.
__global__ __launch_bounds__(64) void mano_pack_joints_kernel(const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                                                             const float* __restrict__ J_regressor, const float* __restrict__ hands_mean,
                                                             const IntList32 parents, int nv, int nj, int nb, double* __restrict__ Jt,
                                                             double* __restrict__ Js, double* __restrict__ hm, int32_t* __restrict__ par)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < nj * 3) hm[i] = i < 3 ? 0.0 : (double)hands_mean[i - 3];
    if (i < nj) {
        int32_t p = -1;
#pragma unroll
        for (int u = 0; u < MANO_MAX_NJ; ++u) p = u == i ? parents.v[u] : p; // (compile-time indices: the list stays in scalar registers)
        par[i] = p;
    }
    if (i >= nj * 3 * (nb + 1)) return;
    const int c = i % (nb + 1), k = i / (nb + 1) % 3, j = i / (nb + 1) / 3;
    const float* reg = J_regressor + (size_t)j * nv;
    double s = 0.0;
    for (int v = 0; v < nv; ++v) {
        const double x = c == 0 ? (double)v_template[(size_t)v * 3 + k] : (double)shapedirs[((size_t)v * 3 + k) * nb + (c - 1)];
        s = s + (double)reg[v] * x;
    }
    if (c == 0) Jt[j * 3 + k] = s;
    else Js[(j * 3 + k) * nb + (c - 1)] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// joints: one wave per pose, fp64
// ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void mano_joint_kernel(const ManoTables t, int nj, int nb, const float* __restrict__ pose, int64_t pose_stride,
                                                       const float* __restrict__ betas, int64_t betas_stride, const float* __restrict__ trans,
                                                       int64_t trans_stride, int flat_hand_mean, float* __restrict__ ws, float* __restrict__ joints,
                                                       int64_t joints_stride)
{
    __shared__ double sr[MANO_MAX_NJ][3], sR[MANO_MAX_NJ][9], sJ[MANO_MAX_NJ][3], sG[MANO_MAX_NJ][12];
    const size_t p = blockIdx.x;
    const int lane = threadIdx.x;
    float* A = ws + p * (size_t)(nj * 12 + (nj - 1) * 9);
    joint_forward(t, nj, nb, pose + p * pose_stride, betas + p * betas_stride, flat_hand_mean, lane, sr, sR, sJ, sG, A, A + nj * 12);
    if (lane < nj)
        for (int k = 0; k < 3; ++k) joints[p * joints_stride + 3 * lane + k] = (float)(sG[lane][k * 4 + 3] + (double)trans[p * trans_stride + k]);
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// vertices: one lane per vertex, PP poses per lane, fp32
// ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MV_BLOCK) void mano_vertex_kernel(const ManoTables t, int nv, int nj, int nb, int nvb, const float* __restrict__ betas,
                                                              int64_t betas_stride, const float* __restrict__ trans, int64_t trans_stride, int P,
                                                              const float* __restrict__ ws, float* __restrict__ verts, int64_t verts_stride)
{
    extern __shared__ float sm[]; // per pose of the block: A [nj][12], pose feature [(nj-1)*9], betas [nb], trans [3]
    const int wsf = nj * 12 + (nj - 1) * 9, per = wsf + nb + 3;
    const size_t p0 = (size_t)(blockIdx.x / nvb) * PP;
    const int vb = blockIdx.x % nvb;
    for (int i = threadIdx.x; i < PP * per; i += MV_BLOCK) {
        const int q = i / per, o = i % per;
        size_t p = p0 + q;
        p = p < (size_t)P ? p : (size_t)P - 1; // past the batch: the last pose again, computed and not written
        sm[i] = o < wsf ? ws[p * wsf + o] : o < wsf + nb ? betas[p * betas_stride + (o - wsf)] : trans[p * trans_stride + (o - wsf - nb)];
    }
    __syncthreads();
    const int v = vb * MV_BLOCK + threadIdx.x;
    if (v >= nv) return;
    float x[PP][3], T[PP][12], pos[PP][3];
    vertex_forward<PP>(t, v, nv, nj, nb, PoseValues{sm, sm + nj * 12, sm + wsf, sm + wsf + nb, per}, x, T, pos);
#pragma unroll
    for (int q = 0; q < PP; ++q) {
        if (p0 + q < (size_t)P) { // (block-uniform)
            float* o = verts + (p0 + q) * verts_stride + (size_t)v * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = pos[q][k];
        }
    }
}

// The appended vertex: one thread per pose and coordinate; the ring's ids are kernel arguments read with compile-time indices.
__global__ __launch_bounds__(MV_BLOCK) void mano_seal_kernel(float* __restrict__ verts, int64_t verts_stride, int nv, int P, const IntList64 ring, int n_ring)
{
    const size_t i = (size_t)blockIdx.x * MV_BLOCK + threadIdx.x;
    if (i >= (size_t)P * 3) return;
    float* rowp = verts + (i / 3) * verts_stride;
    const int k = (int)(i % 3);
    float s = rowp[(size_t)ring.v[0] * 3 + k];
#pragma unroll
    for (int u = 1; u < MANO_MAX_RING; ++u)
        if (u < n_ring) s = s + rowp[(size_t)ring.v[u] * 3 + k];
    rowp[(size_t)nv * 3 + k] = s * (1.0f / (float)n_ring);
}

} // namespace

extern "C" int64_t vanerf_mano_packed_bytes(int nv, int nj, int nb)
{
    return size_query([&] {
        check_sizes("vanerf_mano_packed_bytes", nv, nj, nb);
        return mano_layout(nv, nj, nb).bytes;
    });
}

extern "C" int64_t vanerf_mano_workspace_bytes(int nj, int P)
{
    return size_query([&] {
        if (nj < 1 || nj > MANO_MAX_NJ) throw_error("vanerf_mano_workspace_bytes: nj=%d joints (1 .. %d)", nj, MANO_MAX_NJ);
        if (P < 0) throw_error("vanerf_mano_workspace_bytes: P=%d poses (at least 0)", P);
        return (int64_t)P * ws_floats(nj) * 4;
    });
}

extern "C" int vanerf_mano_poses_per_lane(void) { return PP; }

extern "C" int vanerf_mano_pack(const float* v_template, const float* shapedirs, const float* posedirs, const float* J_regressor, const float* weights,
                                const int32_t* parents, const float* hands_mean, int nv, int nj, int nb, void* packed, int64_t packed_bytes, void* stream)
{
    return guarded([&] {
        const char* who = "vanerf_mano_pack";
        if (!v_template || !shapedirs || !J_regressor || !weights || !parents || !packed) throw_error("%s: null argument", who);
        check_sizes(who, nv, nj, nb);
        if (nj > 1 && (!posedirs || !hands_mean)) throw_error("%s: null argument (posedirs and hands_mean are needed with nj=%d)", who, nj);
        if (parents[0] != -1) throw_error("%s: parents[0]=%d (the root has parent -1)", who, parents[0]);
        IntList32 par;
        for (int j = 0; j < MANO_MAX_NJ; ++j) par.v[j] = -1;
        for (int j = 1; j < nj; ++j) {
            if (parents[j] < 0 || parents[j] >= j) throw_error("%s: parents[%d]=%d (expected 0 <= parents[j] < j)", who, j, parents[j]);
            par.v[j] = parents[j];
        }
        const ManoLayout L = mano_layout(nv, nj, nb);
        if (packed_bytes < L.bytes) throw_error("%s: packed_bytes=%lld, the model needs %lld (vanerf_mano_packed_bytes)", who, (long long)packed_bytes, (long long)L.bytes);
        if ((uintptr_t)packed & 15) throw_error("%s: packed must be 16-byte aligned", who);
        const ManoTables t = mano_tables(packed, nv, nj, nb);
        const int64_t n_float = (L.bytes - L.vt) / 4;
        const unsigned b_tab = blocks_of(who, n_float, MV_BLOCK), b_j = blocks_of(who, (int64_t)nj * 3 * (nb + 1), 64);
        hipLaunchKernelGGL(mano_pack_tables_kernel, dim3(b_tab), dim3(MV_BLOCK), 0, (hipStream_t)stream, v_template, shapedirs, posedirs, weights, nv, nj, nb,
                           const_cast<float*>(t.vt), const_cast<float*>(t.sd), const_cast<float*>(t.pd), const_cast<float*>(t.wt));
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(mano_pack_joints_kernel, dim3(b_j), dim3(64), 0, (hipStream_t)stream, v_template, shapedirs, J_regressor, hands_mean, par, nv, nj, nb,
                           const_cast<double*>(t.Jt), const_cast<double*>(t.Js), const_cast<double*>(t.hm), const_cast<int32_t*>(t.parents));
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_mano_skin(const void* packed, int nv, int nj, int nb, const float* pose, int64_t pose_stride, const float* betas,
                                int64_t betas_stride, const float* trans, int64_t trans_stride, int P, int flat_hand_mean, const int32_t* ring, int n_ring,
                                void* workspace, int64_t workspace_bytes, float* verts, int64_t verts_stride, float* joints, int64_t joints_stride, void* stream)
{
    return guarded([&] {
        const char* who = "vanerf_mano_skin";
        check_sizes(who, nv, nj, nb);
        if (P < 0) throw_error("%s: P=%d poses (at least 0)", who, P);
        const IntList64 rg = ring_list(who, ring, n_ring, nv);
        check_stride(who, "pose", pose_stride, nj * 3);
        check_stride(who, "betas", betas_stride, nb);
        check_stride(who, "trans", trans_stride, 3);
        check_stride(who, "verts", verts_stride, ((int64_t)nv + (n_ring > 0 ? 1 : 0)) * 3);
        check_stride(who, "joints", joints_stride, nj * 3);
        if (P == 0) return;
        if (!packed || !pose || !betas || !trans || !workspace || !verts || !joints) throw_error("%s: null argument", who);
        if ((uintptr_t)packed & 15) throw_error("%s: packed must be 16-byte aligned", who);
        const int64_t need = (int64_t)P * ws_floats(nj) * 4;
        if (workspace_bytes < need) throw_error("%s: workspace_bytes=%lld, %d poses need %lld (vanerf_mano_workspace_bytes)", who, (long long)workspace_bytes, P, (long long)need);
        const int nvb = (nv + MV_BLOCK - 1) / MV_BLOCK;
        const unsigned b_v = blocks_of(who, (int64_t)((P + PP - 1) / PP) * nvb, 1);
        const unsigned b_s = blocks_of(who, (int64_t)P * 3, MV_BLOCK);
        const ManoTables t = mano_tables(packed, nv, nj, nb);
        float* ws = static_cast<float*>(workspace);
        hipLaunchKernelGGL(mano_joint_kernel, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, t, nj, nb, pose, pose_stride, betas, betas_stride, trans,
                           trans_stride, flat_hand_mean, ws, joints, joints_stride);
        HIP_CHECK(hipGetLastError());
        const size_t lds = (size_t)PP * (ws_floats(nj) + nb + 3) * sizeof(float);
        hipLaunchKernelGGL(mano_vertex_kernel, dim3(b_v), dim3(MV_BLOCK), lds, (hipStream_t)stream, t, nv, nj, nb, nvb, betas, betas_stride, trans, trans_stride,
                           P, ws, verts, verts_stride);
        HIP_CHECK(hipGetLastError());
        if (n_ring > 0) {
            hipLaunchKernelGGL(mano_seal_kernel, dim3(b_s), dim3(MV_BLOCK), 0, (hipStream_t)stream, verts, verts_stride, nv, P, rg, n_ring);
            HIP_CHECK(hipGetLastError());
        }
    });
}
