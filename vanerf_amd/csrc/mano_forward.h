// mano_forward.h -- the forward of MANO skinning as device code, one copy: the fp64 joint chain and the fp32 per-vertex forward that
// mano_skin.hip writes out and that mano_skin_backward.hip and mano_skin_normal.hip recompute, with the small device helpers the three share.
// Whoever calls these functions gets the forward's bits: the order of every product and sum is fixed here and nowhere else.
#pragma once
#include "mano_tables.h"

#include <cmath>

namespace vanerf {
namespace mano {

__device__ __forceinline__ int parent_of(const ManoTables& t, int j) // j >= 1; clamped (checked at the pack; a foreign buffer must not index outside the block's LDS)
{
    const int par = t.parents[j];
    return par < 0 ? 0 : (par > j - 1 ? j - 1 : par);
}

__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = x + __shfl_xor(x, o, 64); // a butterfly: the same order of additions whatever the data
    return x;
}

// What the derivatives of one joint's Rodrigues formula start from: R = I + sin(a) K + (1 - cos(a)) K K, K = skew(d), d = r / a, a = |e|,
// e = r + 1e-8 (the constant enters the norm only).
struct RodriguesTerms {
    double e[3], a, d[3], s, co, c1, K[9], K2[9];
};

__device__ __forceinline__ RodriguesTerms rodrigues_terms(const double* r)
{
    RodriguesTerms q;
#pragma unroll
    for (int k = 0; k < 3; ++k) q.e[k] = r[k] + 1e-8;
    q.a = sqrt((q.e[0] * q.e[0] + q.e[1] * q.e[1]) + q.e[2] * q.e[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) q.d[k] = r[k] / q.a;
    q.s = sin(q.a);
    q.co = cos(q.a);
    q.c1 = 1.0 - q.co;
    const double K[9] = {0.0, -q.d[2], q.d[1], q.d[2], 0.0, -q.d[0], -q.d[1], q.d[0], 0.0};
#pragma unroll
    for (int i = 0; i < 9; ++i) q.K[i] = K[i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) q.K2[i * 3 + k] = (K[i * 3] * K[k] + K[i * 3 + 1] * K[3 + k]) + K[i * 3 + 2] * K[6 + k];
    return q;
}

// Steps 1, 3, 5 and J of step 2 for one pose, by one wave of 64 lanes.  Lane j: Rodrigues of joint j and J_j from the fp64 joint tables; then
// the chain joint by joint (parents[j] < j, so a loop over j is every tree's order), element (row, col) of G_j on lane 4 row + col.  Leaves
// the full axis-angle (sr), R, J and G in LDS; A and the pose feature (R_j - I, j >= 1) go to `A` / `pf`, rounded once to fp32, when given.
// Ends behind a barrier.
__device__ __forceinline__ void joint_forward(const ManoTables& t, int nj, int nb, const float* __restrict__ pose, const float* __restrict__ betas,
                                              int flat_hand_mean, int lane, double (*sr)[3], double (*sR)[9], double (*sJ)[3], double (*sG)[12],
                                              float* __restrict__ A, float* __restrict__ pf)
{
    if (lane < nj) {
        double r[3];
        for (int k = 0; k < 3; ++k) {
            r[k] = (double)pose[3 * lane + k] + (flat_hand_mean ? 0.0 : t.hm[3 * lane + k]);
            sr[lane][k] = r[k];
        }
        const double e0 = r[0] + 1e-8, e1 = r[1] + 1e-8, e2 = r[2] + 1e-8; // the constant enters the norm only
        const double angle = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        const double dx = r[0] / angle, dy = r[1] / angle, dz = r[2] / angle;
        const double s = sin(angle), c1 = 1.0 - cos(angle);
        // R - I = sin K + (1 - cos) K^2 with K = skew(d); r = 0 gives d = 0 and R = I exactly
        double m[9];
        m[0] = c1 * -(dz * dz + dy * dy);
        m[1] = s * -dz + c1 * (dx * dy);
        m[2] = s * dy + c1 * (dx * dz);
        m[3] = s * dz + c1 * (dx * dy);
        m[4] = c1 * -(dz * dz + dx * dx);
        m[5] = s * -dx + c1 * (dy * dz);
        m[6] = s * -dy + c1 * (dx * dz);
        m[7] = s * dx + c1 * (dy * dz);
        m[8] = c1 * -(dx * dx + dy * dy);
        for (int e = 0; e < 9; ++e) {
            sR[lane][e] = (e % 4 == 0 ? 1.0 : 0.0) + m[e];
            if (pf && lane >= 1) pf[(lane - 1) * 9 + e] = (float)m[e];
        }
        for (int k = 0; k < 3; ++k) {
            double sum = 0.0;
            for (int b = 0; b < nb; ++b) sum = sum + t.Js[(lane * 3 + k) * nb + b] * (double)betas[b];
            sJ[lane][k] = t.Jt[lane * 3 + k] + sum;
        }
    }
    __syncthreads();
    const int row = (lane >> 2) % 3, col = lane & 3;
    for (int j = 0; j < nj; ++j) {
        if (lane < 12) {
            double g;
            if (j == 0) {
                g = col < 3 ? sR[0][row * 3 + col] : sJ[0][row];
            } else {
                const int par = parent_of(t, j);
                const double* G = sG[par];
                double l0, l1, l2;
                if (col < 3) { l0 = sR[j][col]; l1 = sR[j][3 + col]; l2 = sR[j][6 + col]; }
                else { l0 = sJ[j][0] - sJ[par][0]; l1 = sJ[j][1] - sJ[par][1]; l2 = sJ[j][2] - sJ[par][2]; }
                g = (G[row * 4] * l0 + G[row * 4 + 1] * l1) + G[row * 4 + 2] * l2;
                if (col == 3) g = g + G[row * 4 + 3];
            }
            sG[j][row * 4 + col] = g;
        }
        __syncthreads();
    }
    if (A && lane < nj) {
        const double* G = sG[lane];
        for (int k = 0; k < 3; ++k) {
            for (int c = 0; c < 3; ++c) A[lane * 12 + k * 4 + c] = (float)G[k * 4 + c];
            A[lane * 12 + k * 4 + 3] = (float)(G[k * 4 + 3] - ((G[k * 4] * sJ[lane][0] + G[k * 4 + 1] * sJ[lane][1]) + G[k * 4 + 2] * sJ[lane][2]));
        }
    }
}

// Where the values of a lane's poses sit in LDS (read with wave-uniform indices): pose q's A [nj][12] at A + q * stride, its pose feature
// [(nj-1)*9], betas [nb] and trans [3] likewise.  trans is read only where the posed vertex is asked for.
struct PoseValues {
    const float *A, *pf, *betas, *trans;
    int stride;
};

// Steps 2, 4, 6 and 7 for vertex v (0 <= v < nv) and NP poses, by one lane: every value of the transposed tables ([row][k][v]: consecutive
// lanes read consecutive vertices) serves all NP poses.  fp32, every product and sum its own IEEE operation (-ffp-contract=off), in one fixed
// order.  -> x = v_posed, T = sum_j w_vj A_j and, when `pos` is given, the posed vertex with trans added last.
template <int NP>
__device__ __forceinline__ void vertex_forward(const ManoTables& t, int v, int nv, int nj, int nb, const PoseValues& in, float (*x)[3], float (*T)[12],
                                               float (*pos)[3])
{
    const size_t n = (size_t)nv;
    float acc[NP][3];
    const float t0 = t.vt[v], t1 = t.vt[n + v], t2 = t.vt[2 * n + v];
    // v_shaped = v_template + (sum over b, from b = 0, of shapedirs_b betas_b)
#pragma unroll
    for (int q = 0; q < NP; ++q) acc[q][0] = acc[q][1] = acc[q][2] = 0.0f;
    for (int b = 0; b < nb; ++b) {
        const float x0 = t.sd[(size_t)(b * 3) * n + v], x1 = t.sd[(size_t)(b * 3 + 1) * n + v], x2 = t.sd[(size_t)(b * 3 + 2) * n + v];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const float be = in.betas[q * in.stride + b];
            acc[q][0] = acc[q][0] + x0 * be;
            acc[q][1] = acc[q][1] + x1 * be;
            acc[q][2] = acc[q][2] + x2 * be;
        }
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        x[q][0] = t0 + acc[q][0];
        x[q][1] = t1 + acc[q][1];
        x[q][2] = t2 + acc[q][2];
        acc[q][0] = acc[q][1] = acc[q][2] = 0.0f;
    }
    // v_posed = v_shaped + (sum over the rows, from row 0, of posedirs_row feature_row)
    const int rows = (nj - 1) * 9;
    for (int r = 0; r < rows; ++r) {
        const float x0 = t.pd[(size_t)(r * 3) * n + v], x1 = t.pd[(size_t)(r * 3 + 1) * n + v], x2 = t.pd[(size_t)(r * 3 + 2) * n + v];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const float f = in.pf[q * in.stride + r];
            acc[q][0] = acc[q][0] + x0 * f;
            acc[q][1] = acc[q][1] + x1 * f;
            acc[q][2] = acc[q][2] + x2 * f;
        }
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        x[q][0] = x[q][0] + acc[q][0];
        x[q][1] = x[q][1] + acc[q][1];
        x[q][2] = x[q][2] + acc[q][2];
    }
    // T = sum over j, from j = 0, of w_vj A_j
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int e = 0; e < 12; ++e) T[q][e] = 0.0f;
    for (int j = 0; j < nj; ++j) {
        const float w = t.wt[(size_t)j * n + v];
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int e = 0; e < 12; ++e) T[q][e] = T[q][e] + w * in.A[q * in.stride + j * 12 + e];
    }
    if (pos) {
#pragma unroll
        for (int q = 0; q < NP; ++q)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float o = ((T[q][4 * k] * x[q][0] + T[q][4 * k + 1] * x[q][1]) + T[q][4 * k + 2] * x[q][2]) + T[q][4 * k + 3];
                pos[q][k] = o + in.trans[q * in.stride + k];
            }
    }
}

} // namespace mano
} // namespace vanerf
