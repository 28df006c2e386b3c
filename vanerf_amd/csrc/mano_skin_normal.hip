// mano_skin_normal.hip -- the normal equations of fitting a MANO-shaped model to a mesh, and the small SPD solve a Levenberg-Marquardt step
// needs (the definition is the comment of vanerf_mano_skin in the header, steps 1-7, differentiated exactly as
// vanerf_mano_skin_backward differentiates it).  With x = (pose, betas, trans), n = 3 nj + nb + 3 unknowns, the residuals r = (v - v*, j - j*),
// their Jacobian J = dr/dx and the weights W = (w_v / nv_out, 1 / nj), vanerf_mano_skin_normal writes H = J^T W J, g = J^T W r and
// loss = r^T W r per pose.  Stateless: the forward is recomputed by the forward's own functions (mano_forward.h).  The restatement the tests
// hold these kernels to is the torch code of tests/test_mano_lm_cpu.py (forward-mode autograd in fp64).
//
// The tangents.  A pose parameter (a, axis) turns everything below joint a about that joint: with D = G_par(a)^R (dR_a / dr_axis) G_a^R^-1,
// dA_j = D [A_j^R | A_j^t - G_a^t] for EVERY descendant j of a (a itself included) and zero elsewhere.  So the table a pose needs is D (three
// 3 x 3 per joint) and G_a^t, whatever the depth of the tree -- a chain of 32 costs what a star does -- and a vertex's column is
// D (S_a - W_a G_a^t) + T^R (posedirs^T dR_a), S_a = sum over the descendants j of w_vj A_j (x, 1) and W_a = the sum of those w_vj.
// A shape coefficient moves x (shapedirs) and the translation parts: dA_j^t = dG_j^t - G_j^R (J_regressor . shapedirs)_j.
//
// Three launches per call, all on the caller's stream:
//   mano_nrm_joint_kernel   one wave per pose, fp64: joint_forward(); the Rodrigues derivative, D, G^t, dA^t / dbetas, each rounded once to
//                           fp32 into the workspace beside A and the pose feature; the joints' residual rows (dG_j^t / dx and j - j*) in fp64.
//   mano_nrm_vertex_kernel  one block of one wave per pose and chunk of 64 vertices.  Phase 1, one lane per vertex, fp32: vertex_forward() for
//                           x = v_posed, T and the vertex, the 3 x (n + 1) block of (J | r) into an LDS panel [column][row] (rows
//                           k * 64 + lane: conflict-free writes).  Phase 2: the lower triangle of panel^T diag(W) panel in 32 x 32 tiles of the
//                           exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) over the 192 rows in row order: fp32 products w * b, then per element the
//                           chain fmaf(a, w b, acc) in fp32 (the loss, one entry, is added in fp64 instead: a lane's three rows, then a butterfly).
//                           One packed triangle per (pose, chunk) into the workspace.  The sealed vertex is one more chunk: a lane per ring
//                           occurrence recomputes that vertex, the rows are added in the ring's order (the forward's sum) and scaled.
//   mano_nrm_reduce_kernel  one block per pose: per entry of the triangle the chunks' partials in chunk order in fp64, the joints' rows added in
//                           fp64, rounded once; H's upper triangle is a copy of the lower.
// and one for vanerf_mano_lm_solve: one wave per pose, the matrix in LDS in fp64, Cholesky column by column, two triangular solves.
// Tangent tables sit in LDS and are read with wave-uniform indices; no per-lane array is indexed at run time.  No atomics, no device-side
// state; every sum has one fixed order: a pose's bits depend neither on P nor on its row in the batch.
#include "common.h"
#include "mano_forward.h"
#include "mano_tables.h"

#include <cmath>
#include <cstdint>

using namespace vanerf;
using namespace vanerf::mano;

namespace {

constexpr int NQ_CHUNK = 64;             // vertices per block of the vertex kernel: one lane each
constexpr int NQ_ROWS = 3 * NQ_CHUNK;    // residual rows of a chunk
constexpr int NQ_RS = NQ_ROWS + 2;       // floats between two columns of the panel: column c at bank 2 c, so the 64 operand reads of an MFMA step hit 64 banks
constexpr int LM_MAX_N = 128;

// The per-pose fp32 tables the joint stage hands the vertex stage (offsets in floats).
struct TanLayout {
    int A, pf, D, Gt, dF, dAt, total;
};

__host__ __device__ inline TanLayout tan_layout(int nj, int nb)
{
    TanLayout L;
    L.A = 0;                        // [nj][12]
    L.pf = L.A + nj * 12;           // [(nj-1)*9]       R_j - I
    L.D = L.pf + (nj - 1) * 9;      // [nj][3][9]       G_par^R dR_j/dr_axis G_j^R^-1
    L.Gt = L.D + nj * 27;           // [nj][3]          G_j^t
    L.dF = L.Gt + nj * 3;           // [nj-1][3][9]     dR_j/dr_axis, j >= 1
    L.dAt = L.dF + (nj - 1) * 27;   // [nj][nb][3]      dA_j^t / dbetas_b
    L.total = (L.dAt + nj * nb * 3 + 3) / 4 * 4;
    return L;
}

__host__ __device__ inline int tri_size(int ne) { return ne * (ne + 1) / 2; }

__device__ __forceinline__ unsigned ancestors_of(const ManoTables& t, int j) // bit a: a is j or above it
{
    unsigned m = 1u << j;
    for (int q = j; q > 0;) {
        q = parent_of(t, q);
        m |= 1u << q;
    }
    return m;
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// joints: one wave per pose, fp64
// ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void mano_nrm_joint_kernel(const ManoTables t, int nj, int nb, const float* __restrict__ pose, int64_t pose_stride,
                                                           const float* __restrict__ betas, int64_t betas_stride, const float* __restrict__ trans,
                                                           int64_t trans_stride, int flat_hand_mean, const float* __restrict__ target_joints,
                                                           int64_t tj_stride, float* __restrict__ tan, double* __restrict__ jj)
{
    __shared__ double sr[MANO_MAX_NJ][3], sR[MANO_MAX_NJ][9], sJ[MANO_MAX_NJ][3], sG[MANO_MAX_NJ][12];
    __shared__ double sD[MANO_MAX_NJ][27], sdGt[MANO_MAX_NJ][MANO_MAX_NB][3];
    __shared__ unsigned sAnc[MANO_MAX_NJ];
    const size_t p = blockIdx.x;
    const int lane = threadIdx.x;
    const TanLayout L = tan_layout(nj, nb);
    float* out = tan + p * (size_t)L.total;
    joint_forward(t, nj, nb, pose + p * pose_stride, betas + p * betas_stride, flat_hand_mean, lane, sr, sR, sJ, sG, out + L.A, out + L.pf);
    if (lane < nj) {
        sAnc[lane] = ancestors_of(t, lane);
        // the Rodrigues derivative: R = I + sin(a) K + (1 - cos(a)) K K, K = skew(d), d = r / a, a = |r + 1e-8|;
        // da/dr_x = e_x / a, dd_i/dr_x = (delta_ix - d_i e_x / a) / a
        const RodriguesTerms q = rodrigues_terms(sr[lane]);
        const double a = q.a, s = q.s, co = q.co, c1 = q.c1;
        const double *e = q.e, *d = q.d, *K = q.K, *K2 = q.K2;
        double Gp[9], Ga[9];
        const int par = lane >= 1 ? parent_of(t, lane) : 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                Gp[i * 3 + k] = lane >= 1 ? sG[par][i * 4 + k] : (i == k ? 1.0 : 0.0);
                Ga[i * 3 + k] = sG[lane][i * 4 + k];
            }
        // G_a^R^-1 by cofactors, not the transpose: with the 1e-8 in the angle |d| is not 1 and R not orthogonal, to 1e-8 |r|
        double Gi[9];
        Gi[0] = Ga[4] * Ga[8] - Ga[5] * Ga[7];
        Gi[1] = Ga[2] * Ga[7] - Ga[1] * Ga[8];
        Gi[2] = Ga[1] * Ga[5] - Ga[2] * Ga[4];
        Gi[3] = Ga[5] * Ga[6] - Ga[3] * Ga[8];
        Gi[4] = Ga[0] * Ga[8] - Ga[2] * Ga[6];
        Gi[5] = Ga[2] * Ga[3] - Ga[0] * Ga[5];
        Gi[6] = Ga[3] * Ga[7] - Ga[4] * Ga[6];
        Gi[7] = Ga[1] * Ga[6] - Ga[0] * Ga[7];
        Gi[8] = Ga[0] * Ga[4] - Ga[1] * Ga[3];
        const double det = (Ga[0] * Gi[0] + Ga[1] * Gi[3]) + Ga[2] * Gi[6];
#pragma unroll
        for (int q = 0; q < 9; ++q) Gi[q] = Gi[q] / det;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const double ex = e[x] / a;
            double dd[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) dd[i] = ((i == x ? 1.0 : 0.0) - d[i] * ex) / a;
            const double Kx[9] = {0.0, -dd[2], dd[1], dd[2], 0.0, -dd[0], -dd[1], dd[0], 0.0};
            double dR[9], M1[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double kxk = (Kx[i * 3] * K[k] + Kx[i * 3 + 1] * K[3 + k]) + Kx[i * 3 + 2] * K[6 + k];
                    const double kkx = (K[i * 3] * Kx[k] + K[i * 3 + 1] * Kx[3 + k]) + K[i * 3 + 2] * Kx[6 + k];
                    dR[i * 3 + k] = ((co * ex) * K[i * 3 + k] + s * Kx[i * 3 + k]) + ((s * ex) * K2[i * 3 + k] + c1 * (kxk + kkx));
                }
#pragma unroll
            for (int q = 0; q < 9; ++q)
                if (lane >= 1) out[L.dF + ((lane - 1) * 3 + x) * 9 + q] = (float)dR[q];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) M1[i * 3 + k] = (Gp[i * 3] * dR[k] + Gp[i * 3 + 1] * dR[3 + k]) + Gp[i * 3 + 2] * dR[6 + k];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double v = (M1[i * 3] * Gi[k] + M1[i * 3 + 1] * Gi[3 + k]) + M1[i * 3 + 2] * Gi[6 + k];
                    sD[lane][x * 9 + i * 3 + k] = v;
                    out[L.D + (lane * 3 + x) * 9 + i * 3 + k] = (float)v;
                }
        }
        for (int k = 0; k < 3; ++k) out[L.Gt + lane * 3 + k] = (float)sG[lane][k * 4 + 3];
    }
    __syncthreads();
    // dG_j^t / dbetas_b down the chain, element (b, k) on lane 3 b + k
    for (int j = 0; j < nj; ++j) {
        if (lane < nb * 3) {
            const int b = lane / 3, k = lane % 3;
            double g;
            if (j == 0) {
                g = t.Js[k * nb + b];
            } else {
                const int par = parent_of(t, j);
                const double* G = sG[par];
                const double l0 = t.Js[(j * 3) * nb + b] - t.Js[(par * 3) * nb + b], l1 = t.Js[(j * 3 + 1) * nb + b] - t.Js[(par * 3 + 1) * nb + b],
                             l2 = t.Js[(j * 3 + 2) * nb + b] - t.Js[(par * 3 + 2) * nb + b];
                g = ((G[k * 4] * l0 + G[k * 4 + 1] * l1) + G[k * 4 + 2] * l2) + sdGt[par][b][k];
            }
            sdGt[j][b][k] = g;
        }
        __syncthreads();
    }
    for (int i = lane; i < nj * nb * 3; i += 64) {
        const int j = i / (nb * 3), b = i / 3 % nb, k = i % 3;
        const double* G = sG[j];
        out[L.dAt + i] = (float)(sdGt[j][b][k] - ((G[k * 4] * t.Js[(j * 3) * nb + b] + G[k * 4 + 1] * t.Js[(j * 3 + 1) * nb + b]) + G[k * 4 + 2] * t.Js[(j * 3 + 2) * nb + b]));
    }
    // the joints' rows of (J | r): joint_j = G_j^t + trans
    if (jj) {
        const int n = 3 * nj + nb + 3, ne = n + 1;
        double* o = jj + p * (size_t)(3 * nj * ne);
        for (int i = lane; i < 3 * nj * ne; i += 64) {
            const int row = i / ne, c = i % ne, j = row / 3, k = row % 3;
            double v = 0.0;
            if (c < 3 * nj) {
                const int a = c / 3, x = c % 3;
                if (a != j && ((sAnc[j] >> a) & 1u)) {
                    const double* D = sD[a] + x * 9;
                    const double d0 = sG[j][3] - sG[a][3], d1 = sG[j][7] - sG[a][7], d2 = sG[j][11] - sG[a][11];
                    v = (D[k * 3] * d0 + D[k * 3 + 1] * d1) + D[k * 3 + 2] * d2;
                }
            } else if (c < 3 * nj + nb) {
                v = sdGt[j][c - 3 * nj][k];
            } else if (c < n) {
                v = c - 3 * nj - nb == k ? 1.0 : 0.0;
            } else {
                const float jf = (float)(sG[j][k * 4 + 3] + (double)trans[p * trans_stride + k]); // the joint as the forward writes it
                v = (double)jf - (double)target_joints[p * tj_stride + row];
            }
            o[i] = v;
        }
    }
}

// The lower triangle of panel^T diag(w) panel for one wave, in 32 x 32 tiles of v_mfma_f32_32x32x2_f32 (exact fp32: per element a k-ordered chain
// acc = fmaf(a, b, acc), one rounding per step).  Lane l holds A[i = l & 31][k = l >> 5] = panel[row r + k][column 32 ti + i] and
// B[k][j = l & 31] = w[r + k] * panel[r + k][32 tj + j] (an fp32 product); an instruction takes two rows, k = 0 first.  NT column blocks of 32.
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int NT>
__device__ __forceinline__ void panel_product(const float* __restrict__ Pt, const float* __restrict__ sW, int lane, int n, int ne, float* __restrict__ out)
{
    f32x16 acc[NT * (NT + 1) / 2];
#pragma unroll
    for (int t = 0; t < NT * (NT + 1) / 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;
    const int col = lane & 31, kh = lane >> 5;
    for (int r = 0; r < NQ_ROWS; r += 2) {
        const float w = sW[r + kh];
        float a[NT], b[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            a[t] = Pt[(32 * t + col) * NQ_RS + r + kh];
            b[t] = w * a[t];
        }
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj <= ti; ++tj) acc[ti * (ti + 1) / 2 + tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ti], b[tj], acc[ti * (ti + 1) / 2 + tj], 0, 0, 0);
    }
    // C / D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int c = 32 * ti + (e & 3) + 8 * (e >> 2) + 4 * kh, c2 = 32 * tj + col;
                if (c < ne && c2 <= c && c2 < n) out[c * (c + 1) / 2 + c2] = acc[ti * (ti + 1) / 2 + tj][e]; // (c2 == n: the loss, written by the caller)
            }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// vertices: one wave per pose and chunk of 64 vertices; the last chunk of a sealed call is the appended vertex
// ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NQ_CHUNK) void mano_nrm_vertex_kernel(const ManoTables t, int nv, int nj, int nb, int nchunk, int nblk,
                                                                  const float* __restrict__ betas, int64_t betas_stride, const float* __restrict__ trans,
                                                                  int64_t trans_stride, const float* __restrict__ tan, const float* __restrict__ target_verts,
                                                                  int64_t tv_stride, const float* __restrict__ vert_weight, int64_t vw_stride,
                                                                  const IntList64 ring, int n_ring, float* __restrict__ partial)
{
    extern __shared__ float sm[];
    const TanLayout L = tan_layout(nj, nb);
    const int n = 3 * nj + nb + 3, ne = n + 1, nt = (ne + 31) / 32, ncp = 32 * nt;
    const int tabf = (L.total + nb + 3 + 3) / 4 * 4;
    float* sT = sm;                                             // the tangent tables, then betas, then trans
    float* sW = sm + tabf;                                      // [192] the rows' weights
    unsigned* sAnc = reinterpret_cast<unsigned*>(sW + NQ_ROWS); // [32]
    float* Pt = sW + NQ_ROWS + MANO_MAX_NJ;                     // [ncp][NQ_RS] the panel (J | r), by column
    const size_t p = blockIdx.x / (unsigned)nblk;
    const int ch = (int)(blockIdx.x % (unsigned)nblk), lane = threadIdx.x;
    for (int i = lane; i < L.total + nb + 3; i += NQ_CHUNK)
        sT[i] = i < L.total ? tan[p * (size_t)L.total + i] : i < L.total + nb ? betas[p * betas_stride + (i - L.total)] : trans[p * trans_stride + (i - L.total - nb)];
    if (lane < nj) sAnc[lane] = ancestors_of(t, lane);
    for (int c = ne; c < ncp; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) Pt[c * NQ_RS + k * NQ_CHUNK + lane] = 0.0f;
    __syncthreads();
    const bool is_seal = ch == nchunk;
    const size_t nvs = (size_t)nv;
    const int nvo = nv + (n_ring > 0 ? 1 : 0);
    int v;
    bool live;
    if (!is_seal) {
        v = ch * NQ_CHUNK + lane;
        live = v < nv;
        v = live ? v : nv - 1; // past the mesh: the last vertex again, with weight zero
    } else {
        live = lane < n_ring;
        v = ring.v[0];
#pragma unroll
        for (int u = 1; u < MANO_MAX_RING; ++u)
            if (u == lane && u < n_ring) v = ring.v[u]; // (compile-time indices: the list stays in scalar registers)
    }
    // x = v_posed, T and the vertex
    float x[3], T[12], pos[3];
    vertex_forward<1>(t, v, nv, nj, nb, PoseValues{sT + L.A, sT + L.pf, sT + L.total, sT + L.total + nb, 0}, &x, &T, &pos);
    // the rows' weights, the residual column and the identity of trans
    {
        float w = 0.0f;
        if (!is_seal) {
            if (live) w = (vert_weight ? vert_weight[p * vw_stride + v] : 1.0f) / (float)nvo;
        } else if (lane == 0) {
            w = (vert_weight ? vert_weight[p * vw_stride + nv] : 1.0f) / (float)nvo;
        }
        const float* tv = target_verts + p * tv_stride + (size_t)v * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sW[k * NQ_CHUNK + lane] = w;
            Pt[n * NQ_RS + k * NQ_CHUNK + lane] = is_seal ? pos[k] : pos[k] - tv[k]; // (the seal's chunk: the position; its target comes after the sum)
#pragma unroll
            for (int k2 = 0; k2 < 3; ++k2) Pt[(3 * nj + nb + k2) * NQ_RS + k * NQ_CHUNK + lane] = k == k2 ? 1.0f : 0.0f;
        }
    }
    // betas: T^R shapedirs_b + sum_j w_vj dA_j^t/db
    for (int b = 0; b < nb; ++b) {
        const float s0 = t.sd[(size_t)(b * 3) * nvs + v], s1 = t.sd[(size_t)(b * 3 + 1) * nvs + v], s2 = t.sd[(size_t)(b * 3 + 2) * nvs + v];
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        for (int j = 0; j < nj; ++j) {
            const float w = t.wt[(size_t)j * nvs + v];
            const float* dA = sT + L.dAt + (j * nb + b) * 3;
            a0 = a0 + w * dA[0];
            a1 = a1 + w * dA[1];
            a2 = a2 + w * dA[2];
        }
        float* col = Pt + (3 * nj + b) * NQ_RS + lane;
        col[0] = ((T[0] * s0 + T[1] * s1) + T[2] * s2) + a0;
        col[NQ_CHUNK] = ((T[4] * s0 + T[5] * s1) + T[6] * s2) + a1;
        col[2 * NQ_CHUNK] = ((T[8] * s0 + T[9] * s1) + T[10] * s2) + a2;
    }
    // pose: joint a turns what hangs below it about itself
    for (int a = 0; a < nj; ++a) {
        float S0 = 0.0f, S1 = 0.0f, S2 = 0.0f, Ws = 0.0f;
        for (int j = a; j < nj; ++j) {
            const unsigned anc = __builtin_amdgcn_readfirstlane(sAnc[j]);
            if (!((anc >> a) & 1u)) continue; // (wave-uniform)
            const float w = t.wt[(size_t)j * nvs + v];
            const float* A = sT + L.A + j * 12;
            S0 = S0 + w * (((A[0] * x[0] + A[1] * x[1]) + A[2] * x[2]) + A[3]);
            S1 = S1 + w * (((A[4] * x[0] + A[5] * x[1]) + A[6] * x[2]) + A[7]);
            S2 = S2 + w * (((A[8] * x[0] + A[9] * x[1]) + A[10] * x[2]) + A[11]);
            Ws = Ws + w;
        }
        const float* Gt = sT + L.Gt + a * 3;
        const float u0 = S0 - Ws * Gt[0], u1 = S1 - Ws * Gt[1], u2 = S2 - Ws * Gt[2];
        float dx[3][3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) dx[ax][0] = dx[ax][1] = dx[ax][2] = 0.0f;
        if (a >= 1) {
            for (int e = 0; e < 9; ++e) {
                const size_t r = (size_t)((a - 1) * 9 + e) * 3;
                const float p0 = t.pd[r * nvs + v], p1 = t.pd[(r + 1) * nvs + v], p2 = t.pd[(r + 2) * nvs + v];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const float f = sT[L.dF + ((a - 1) * 3 + ax) * 9 + e];
                    dx[ax][0] = dx[ax][0] + p0 * f;
                    dx[ax][1] = dx[ax][1] + p1 * f;
                    dx[ax][2] = dx[ax][2] + p2 * f;
                }
            }
        }
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const float* D = sT + L.D + (a * 3 + ax) * 9;
            float* col = Pt + (3 * a + ax) * NQ_RS + lane;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float c = (D[3 * k] * u0 + D[3 * k + 1] * u1) + D[3 * k + 2] * u2;
                if (a >= 1) c = c + ((T[4 * k] * dx[ax][0] + T[4 * k + 1] * dx[ax][1]) + T[4 * k + 2] * dx[ax][2]);
                col[k * NQ_CHUNK] = c;
            }
        }
    }
    __syncthreads();
    if (is_seal) {
        // the appended vertex: s = row[ring[0]], s = s + row[ring[u]], times 1 / n_ring -- the forward's sum, on every column
        const float inv = 1.0f / (float)n_ring;
        for (int c = lane; c < ne; c += NQ_CHUNK) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float* rowp = Pt + c * NQ_RS + k * NQ_CHUNK;
                float s = rowp[0];
                for (int u = 1; u < n_ring; ++u) s = s + rowp[u];
                s = s * inv;
                if (c == n) s = s - target_verts[p * tv_stride + nvs * 3 + k];
                rowp[0] = s;
            }
        }
        __syncthreads();
    }
    float* out = partial + (p * (size_t)nblk + ch) * (size_t)tri_size(ne);
    // the chunk's loss: fp32 products w r, times r and added in fp64 (k from 0 per lane, then a butterfly over the wave), rounded once
    {
        double l = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float rr = Pt[n * NQ_RS + k * NQ_CHUNK + lane];
            l = l + (double)(sW[k * NQ_CHUNK + lane] * rr) * (double)rr;
        }
        l = wave_sum(l);
        if (lane == 0) out[tri_size(ne) - 1] = (float)l;
    }
    // phase 2: the rest of the lower triangle of panel^T diag(w) panel on the matrix cores
    switch (nt) { // (block-uniform)
    case 1: panel_product<1>(Pt, sW, lane, n, ne, out); break;
    case 2: panel_product<2>(Pt, sW, lane, n, ne, out); break;
    case 3: panel_product<3>(Pt, sW, lane, n, ne, out); break;
    default: panel_product<4>(Pt, sW, lane, n, ne, out); break;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// reduce: one block per pose
// ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mano_nrm_reduce_kernel(int n, int nj, int nblk, const float* __restrict__ partial, const double* __restrict__ jj,
                                                             float* __restrict__ H, int64_t H_stride, float* __restrict__ g, int64_t g_stride,
                                                             float* __restrict__ loss, int64_t loss_stride)
{
    const size_t p = blockIdx.x;
    const int ne = n + 1, ntri = tri_size(ne);
    const float* part = partial ? partial + p * (size_t)nblk * ntri : nullptr;
    const double* rowsj = jj ? jj + p * (size_t)(3 * nj * ne) : nullptr;
    for (int idx = threadIdx.x; idx < ne * ne; idx += 256) {
        const int c = idx / ne, c2 = idx % ne;
        if (c2 > c) continue;
        double s = 0.0;
        if (part)
            for (int b = 0; b < nblk; ++b) s = s + (double)part[(size_t)b * ntri + c * (c + 1) / 2 + c2];
        if (rowsj) {
            double a = 0.0;
            for (int r = 0; r < 3 * nj; ++r) a = a + rowsj[r * ne + c] * rowsj[r * ne + c2];
            s = s + a / (double)nj;
        }
        const float o = (float)s;
        if (c < n) {
            if (H) {
                H[p * H_stride + (size_t)c * n + c2] = o;
                H[p * H_stride + (size_t)c2 * n + c] = o;
            }
        } else if (c2 < n) {
            if (g) g[p * g_stride + c2] = o;
        } else if (loss) {
            loss[p * loss_stride] = o;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// the solve: delta = -M^-1 g by Cholesky in fp64, one wave per pose, the lower triangle of M in LDS
// ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void mano_lm_solve_kernel(const float* __restrict__ M, int64_t M_stride, const float* __restrict__ g, int64_t g_stride, int n,
                                                          float* __restrict__ delta, int64_t delta_stride, int32_t* __restrict__ ok)
{
    extern __shared__ double sl[];
    const int ns = n | 1, lane = threadIdx.x; // an odd row stride: a column's elements fall into different banks
    double* Lm = sl;
    double* b = sl + (size_t)n * ns;
    const size_t p = blockIdx.x;
    for (int idx = lane; idx < n * n; idx += 64) {
        const int i = idx / n, j = idx % n;
        if (j <= i) Lm[i * ns + j] = (double)M[p * M_stride + idx];
    }
    for (int i = lane; i < n; i += 64) b[i] = -(double)g[p * g_stride + i];
    __syncthreads();
    bool fail = false;
    for (int j = 0; j < n; ++j) {
        for (int i = j + lane; i < n; i += 64) {
            double s = Lm[i * ns + j];
            for (int k = 0; k < j; ++k) s = s - Lm[i * ns + k] * Lm[j * ns + k];
            Lm[i * ns + j] = s;
        }
        __syncthreads();
        const double piv = Lm[j * ns + j];
        if (!(piv > 0.0) || !(piv < INFINITY)) { // (the same value on every lane)
            fail = true;
            break;
        }
        const double d = sqrt(piv);
        __syncthreads();
        for (int i = j + lane; i < n; i += 64) Lm[i * ns + j] = i == j ? d : Lm[i * ns + j] / d;
        __syncthreads();
    }
    if (!fail) {
        for (int j = 0; j < n; ++j) { // L y = -g
            const double y = b[j] / Lm[j * ns + j];
            __syncthreads();
            for (int i = j + 1 + lane; i < n; i += 64) b[i] = b[i] - Lm[i * ns + j] * y;
            if (lane == 0) b[j] = y;
            __syncthreads();
        }
        for (int j = n - 1; j >= 0; --j) { // L^T delta = y
            const double xj = b[j] / Lm[j * ns + j];
            __syncthreads();
            for (int i = lane; i < j; i += 64) b[i] = b[i] - Lm[j * ns + i] * xj;
            if (lane == 0) b[j] = xj;
            __syncthreads();
        }
        int bad = 0;
        for (int i = lane; i < n; i += 64) bad |= !isfinite((float)b[i]);
        fail = __any(bad) != 0;
    }
    for (int i = lane; i < n; i += 64) delta[p * delta_stride + i] = fail ? 0.0f : (float)b[i];
    if (lane == 0) ok[p] = fail ? 0 : 1;
}

struct NrmSizes {
    int64_t jj, partial, tan, total;
};

NrmSizes nrm_sizes(int nv, int nj, int nb, int P)
{
    const int64_t ne = 3 * nj + nb + 4, nblk = ((int64_t)nv + NQ_CHUNK - 1) / NQ_CHUNK + 1;
    NrmSizes s;
    s.jj = (int64_t)P * 3 * nj * ne * 8;                // the joints' rows, fp64
    s.partial = (int64_t)P * nblk * tri_size((int)ne) * 4; // a packed triangle per pose and chunk (the seal's included)
    s.partial = (s.partial + 7) / 8 * 8;
    s.tan = (int64_t)P * tan_layout(nj, nb).total * 4;
    s.total = s.jj + s.partial + s.tan;
    return s;
}

} // namespace

extern "C" int64_t vanerf_mano_skin_normal_workspace_bytes(int nv, int nj, int nb, int P)
{
    return size_query([&] {
        const char* who = "vanerf_mano_skin_normal_workspace_bytes";
        check_sizes(who, nv, nj, nb);
        if (P < 0) throw_error("%s: P=%d poses (at least 0)", who, P);
        return nrm_sizes(nv, nj, nb, P).total;
    });
}

extern "C" int vanerf_mano_skin_normal(const void* packed, int nv, int nj, int nb, const float* pose, int64_t pose_stride, const float* betas,
                                       int64_t betas_stride, const float* trans, int64_t trans_stride, int P, int flat_hand_mean, const int32_t* ring,
                                       int n_ring, const float* target_verts, int64_t target_verts_stride, const float* vert_weight,
                                       int64_t vert_weight_stride, const float* target_joints, int64_t target_joints_stride, void* workspace,
                                       int64_t workspace_bytes, float* H, int64_t H_stride, float* g, int64_t g_stride, float* loss, int64_t loss_stride,
                                       void* stream)
{
    return guarded([&] {
        const char* who = "vanerf_mano_skin_normal";
        check_sizes(who, nv, nj, nb);
        if (P < 0) throw_error("%s: P=%d poses (at least 0)", who, P);
        const IntList64 rg = ring_list(who, ring, n_ring, nv);
        const int64_t nvo = (int64_t)nv + (n_ring > 0 ? 1 : 0), n = 3 * nj + nb + 3;
        check_stride(who, "pose", pose_stride, nj * 3);
        check_stride(who, "betas", betas_stride, nb);
        check_stride(who, "trans", trans_stride, 3);
        if (target_verts) check_stride(who, "target_verts", target_verts_stride, nvo * 3);
        if (vert_weight && vert_weight_stride != 0 && vert_weight_stride < nvo)
            throw_error("%s: vert_weight_stride=%lld is neither 0 (one shared row) nor at least a row's %lld floats", who, (long long)vert_weight_stride, (long long)nvo);
        if (target_joints) check_stride(who, "target_joints", target_joints_stride, nj * 3);
        if (H && H_stride < n * n) throw_error("%s: H_stride=%lld is below a matrix's %lld floats", who, (long long)H_stride, (long long)(n * n));
        if (g) check_stride(who, "g", g_stride, n);
        if (loss && loss_stride < 1) throw_error("%s: loss_stride=%lld (at least 1)", who, (long long)loss_stride);
        if (P == 0) return;
        if (!packed || !pose || !betas || !trans) throw_error("%s: null argument", who);
        if (!target_verts && !target_joints) throw_error("%s: null argument (target_verts and target_joints are both null: nothing to fit)", who);
        if (vert_weight && !target_verts) throw_error("%s: vert_weight without target_verts", who);
        if ((uintptr_t)packed & 15) throw_error("%s: packed must be 16-byte aligned", who);
        if (!workspace) throw_error("%s: null argument (workspace)", who);
        const NrmSizes sz = nrm_sizes(nv, nj, nb, P);
        if (workspace_bytes < sz.total)
            throw_error("%s: workspace_bytes=%lld, %d poses need %lld (vanerf_mano_skin_normal_workspace_bytes)", who, (long long)workspace_bytes, P, (long long)sz.total);
        if ((uintptr_t)workspace & 15) throw_error("%s: workspace must be 16-byte aligned", who);
        if (!H && !g && !loss) return; // nothing wanted
        const int nchunk = (nv + NQ_CHUNK - 1) / NQ_CHUNK, nblk = nchunk + (n_ring > 0 ? 1 : 0);
        const unsigned b_v = blocks_of(who, (int64_t)P * nblk, 1);
        const ManoTables t = mano_tables(packed, nv, nj, nb);
        double* jj = target_joints ? static_cast<double*>(workspace) : nullptr;
        float* partial = target_verts ? reinterpret_cast<float*>(static_cast<char*>(workspace) + sz.jj) : nullptr;
        float* tan = reinterpret_cast<float*>(static_cast<char*>(workspace) + sz.jj + sz.partial);
        hipLaunchKernelGGL(mano_nrm_joint_kernel, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, t, nj, nb, pose, pose_stride, betas, betas_stride, trans,
                           trans_stride, flat_hand_mean, target_joints, target_joints_stride, tan, jj);
        HIP_CHECK(hipGetLastError());
        if (target_verts) {
            const TanLayout L = tan_layout(nj, nb);
            const int ne = (int)n + 1, ncp = (ne + 31) / 32 * 32, tabf = (L.total + nb + 3 + 3) / 4 * 4;
            const size_t lds = (size_t)(tabf + NQ_ROWS + MANO_MAX_NJ + ncp * NQ_RS) * sizeof(float);
            if (lds > 64 * 1024)
                HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(mano_nrm_vertex_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(mano_nrm_vertex_kernel, dim3(b_v), dim3(NQ_CHUNK), lds, (hipStream_t)stream, t, nv, nj, nb, nchunk, nblk, betas, betas_stride, trans,
                               trans_stride, tan, target_verts, target_verts_stride, vert_weight, vert_weight_stride, rg, n_ring, partial);
            HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(mano_nrm_reduce_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, (int)n, nj, nblk, partial, jj, H, H_stride, g, g_stride,
                           loss, loss_stride);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_mano_lm_solve(const float* M, int64_t M_stride, const float* g, int64_t g_stride, int n, int P, float* delta, int64_t delta_stride,
                                    int32_t* ok, void* stream)
{
    return guarded([&] {
        const char* who = "vanerf_mano_lm_solve";
        if (n < 1 || n > LM_MAX_N) throw_error("%s: n=%d unknowns (1 .. %d)", who, n, LM_MAX_N);
        if (P < 0) throw_error("%s: P=%d systems (at least 0)", who, P);
        if (M_stride < (int64_t)n * n) throw_error("%s: M_stride=%lld is below a matrix's %d floats", who, (long long)M_stride, n * n);
        check_stride(who, "g", g_stride, n);
        check_stride(who, "delta", delta_stride, n);
        if (P == 0) return;
        if (!M || !g || !delta || !ok) throw_error("%s: null argument", who);
        const size_t lds = ((size_t)n * (n | 1) + n) * sizeof(double);
        if (lds > 64 * 1024)
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(mano_lm_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(mano_lm_solve_kernel, dim3((unsigned)P), dim3(64), lds, (hipStream_t)stream, M, M_stride, g, g_stride, n, delta, delta_stride, ok);
        HIP_CHECK(hipGetLastError());
    });
}
