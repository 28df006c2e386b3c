// surface_lines.hip -- the learned surface along lines (the comments of vanerf_vertex_normals ... vanerf_line_refine in the
// header): sample f = alpha + mesh_sdf on n lines base + t dir, bracket the crossing of f = iso nearest to t = 0 on each line and refine it
// with further field values.  surface.register_surface runs it on the lines through the MANO vertices along their normals.  The
// restatement the tests hold these kernels to is the fp64 numpy code of tests/test_surface_register.py.  Built with -ffp-contract=off.
//
// Every output is a function of its own line alone, computed in a fixed order: no atomics, no LDS, no device globals, the same bits every call.
#include "common.h"
#include "vertex_normal.h"

#include <cfloat>
#include <climits>
#include <cmath>

using namespace vanerf;

namespace {

constexpr int SL_BLOCK = 256;
constexpr int SL_WAVES = SL_BLOCK / 64;
constexpr int SL_F4 = VANERF_LINE_STATE_FLOATS / 4; // float4s of a record
constexpr long long SL_MAX_POINTS = 0x7fffffffLL;

static_assert(VANERF_LINE_STATE_FLOATS == 16 && VANERF_LS_TA == 0 && VANERF_LS_TB == 1 && VANERF_LS_GA == 2 && VANERF_LS_GB == 3 &&
              VANERF_LS_RGB_A == 4 && VANERF_LS_FOUND == 7 && VANERF_LS_RGB_B == 8 && VANERF_LS_T_EST == 11 && VANERF_LS_RGB_EST == 12 &&
              VANERF_LS_T_NEXT == 15, "the kernels below write the record as four float4s in this order");

// A field value as the extractor reads it (surface.hip): non-finite -> +FLT_MAX (outside).
__device__ __forceinline__ float field_read(float v) { return fabsf(v) <= FLT_MAX ? v : FLT_MAX; }

// fminf(fmaxf(w, lo), hi): a NaN quotient (both differences overflowed) reads as lo, as in the extractor.
__device__ __forceinline__ float clampf(float w, float lo, float hi) { return fminf(fmaxf(w, lo), hi); }

// Where iso lies between the ends a and b of a bracket, as a weight in [0, 1].  Exactly one of ga, gb is below iso, so gb != ga.
__device__ __forceinline__ float cross_weight(float ga, float gb, float iso) { return clampf((iso - ga) / (gb - ga), 0.0f, 1.0f); }

struct Bracket {
    float ta, tb, ga, gb;
    float3 ca, cb;
};

// The record of a found line from its bracket: w, t_est, rgb_est and t_next, the same expressions after the bracket and after every refinement.
__device__ __forceinline__ void store_found(float4* __restrict__ rec, const Bracket& B, float iso)
{
    const float w = cross_weight(B.ga, B.gb, iso), width = B.tb - B.ta;
    const float t_est = fmaf(w, width, B.ta), t_next = fmaf(clampf(w, 0.125f, 0.875f), width, B.ta);
    rec[0] = make_float4(B.ta, B.tb, B.ga, B.gb);
    rec[1] = make_float4(B.ca.x, B.ca.y, B.ca.z, 1.0f);
    rec[2] = make_float4(B.cb.x, B.cb.y, B.cb.z, t_est);
    rec[3] = make_float4(B.ca.x + w * (B.cb.x - B.ca.x), B.ca.y + w * (B.cb.y - B.ca.y), B.ca.z + w * (B.cb.z - B.ca.z), t_next);
}

__global__ __launch_bounds__(SL_BLOCK) void vertex_normals_kernel(const float* __restrict__ V, int nv, const int32_t* __restrict__ F, int nf,
                                                                  float* __restrict__ normals)
{
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * SL_WAVES + (threadIdx.x >> 6);
    if (v >= nv) return; // whole waves leave together
    float3 n = wave_normal_sum(V, nv, F, nf, v, lane);
    if (lane != 0) return;
    n = normalize_eps(n);
    normals[3 * v] = n.x;
    normals[3 * v + 1] = n.y;
    normals[3 * v + 2] = n.z;
}

// One thread per point, line-major: consecutive threads write consecutive points.
__global__ __launch_bounds__(SL_BLOCK) void line_points_kernel(const float* __restrict__ base, const float* __restrict__ dir, long long total, int K,
                                                               float t0, float dt, const float* __restrict__ t_dev, float* __restrict__ pts)
{
    const long long p = (long long)blockIdx.x * SL_BLOCK + threadIdx.x;
    if (p >= total) return;
    const long long i = p / K;
    float t;
    bool on_line = true;
    if (t_dev) { // K == 1
        t = t_dev[i];
        on_line = fabsf(t) <= FLT_MAX; // a non-finite t is read as 0: the base itself, bit for bit
    } else {
        t = fmaf((float)(int)(p - i * K), dt, t0);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float b = base[3 * i + j];
        pts[3 * p + j] = on_line ? fmaf(t, dir[3 * i + j], b) : b;
    }
}

// One wave per line, lanes over samples, K > 64 in rounds of 64 (coalesced reads of f).  Lane j of a round looks at the pair (k - 1, k) that ends
// at its own sample k = 64 round + j: with m the ballot of the inside flags, the crossings of the round are the bits of m ^ (m << 1 | carry),
// carry being the inside flag of the sample before the round -- m ^ (m >> 1) seen from the upper end of each pair, the last bit carried across
// rounds.  A round without a crossing costs the ballot alone (whole-wave branch).  Each lane keeps the best (|tc|, pair) of its own pairs
// (ascending, so a tie keeps the lower pair), a fixed xor butterfly takes the minimum of (|tc|, pair) over the lanes, and lane 0 writes the
// record from the two samples of that pair.  (Keeping all four rounds of a line in registers, loaded up front, and taking the two samples from
// the lanes that hold them instead of reading them again measured the same: 0.081 against 0.075 ms for 200 000 lines of 128 samples.)
__global__ __launch_bounds__(SL_BLOCK) void line_bracket_kernel(const float* __restrict__ f, const float* __restrict__ rgb, int n, int K, float t0,
                                                                float dt, float iso, float* __restrict__ state)
{
    const int lane = threadIdx.x & 63;
    const int line = blockIdx.x * SL_WAVES + (threadIdx.x >> 6);
    if (line >= n) return; // whole waves leave together
    const float* __restrict__ row = f + (size_t)line * K;
    float best = INFINITY;
    int best_k = INT_MAX; // the lower sample of the best pair; INT_MAX: none
    float g_carry = FLT_MAX;
    unsigned long long carry = 0;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const float g = k < K ? field_read(row[k]) : FLT_MAX;
        const unsigned long long m = __ballot(k < K && g < iso);
        // pairs that exist: k >= 1 and k < K
        const int left = K - k0; // samples of this round, >= 1
        unsigned long long pairs = left >= 64 ? ~0ull : (1ull << left) - 1ull;
        if (k0 == 0) pairs &= ~1ull;
        const unsigned long long x = (m ^ (m << 1 | carry)) & pairs;
        float g_lo = __shfl_up(g, 1);
        if (lane == 0) g_lo = g_carry;
        if (x != 0) { // the same in every lane
            if (x >> lane & 1ull) {
                const float w = cross_weight(g_lo, g, iso);
                const float a = fabsf(fmaf(w, dt, fmaf((float)(k - 1), dt, t0)));
                if (best_k == INT_MAX || a < best) { best = a; best_k = k - 1; }
            }
        }
        carry = m >> 63;
        g_carry = __shfl(g, 63);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const float o = __shfl_xor(best, s);
        const int ok = __shfl_xor(best_k, s);
        if (ok != INT_MAX && (best_k == INT_MAX || o < best || (o == best && ok < best_k))) { best = o; best_k = ok; }
    }
    if (lane != 0) return;
    float4* __restrict__ rec = reinterpret_cast<float4*>(state) + (size_t)line * SL_F4;
    if (best_k == INT_MAX) {
        rec[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        rec[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        rec[2] = make_float4(0.0f, 0.0f, 0.0f, NAN);
        rec[3] = make_float4(0.0f, 0.0f, 0.0f, NAN);
        return;
    }
    Bracket B;
    B.ta = fmaf((float)best_k, dt, t0);
    B.tb = fmaf((float)(best_k + 1), dt, t0);
    B.ga = field_read(row[best_k]);
    B.gb = field_read(row[best_k + 1]);
    B.ca = B.cb = make_float3(0.0f, 0.0f, 0.0f);
    if (rgb) {
        const float* __restrict__ c = rgb + 3 * ((size_t)line * K + best_k);
        B.ca = make_float3(c[0], c[1], c[2]);
        B.cb = make_float3(c[3], c[4], c[5]);
    }
    store_found(rec, B, iso);
}

// One thread per line: the new sample replaces the end of the bracket on its own side of iso.
__global__ __launch_bounds__(SL_BLOCK) void line_refine_kernel(const float* __restrict__ f_new, const float* __restrict__ rgb_new, int n, float iso,
                                                               float* __restrict__ state)
{
    const int i = blockIdx.x * SL_BLOCK + threadIdx.x;
    if (i >= n) return;
    float4* __restrict__ rec = reinterpret_cast<float4*>(state) + (size_t)i * SL_F4;
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    if (r1.w != 1.0f) return; // no crossing on this line: the record stays as it is
    Bracket B = {r0.x, r0.y, r0.z, r0.w, make_float3(r1.x, r1.y, r1.z), make_float3(r2.x, r2.y, r2.z)};
    const float g = field_read(f_new[i]), t = r3.w;
    const bool to_a = (g < iso) == (B.ga < iso);
    if (to_a) { B.ta = t; B.ga = g; } else { B.tb = t; B.gb = g; }
    if (rgb_new) {
        const float3 c = make_float3(rgb_new[3 * (size_t)i], rgb_new[3 * (size_t)i + 1], rgb_new[3 * (size_t)i + 2]);
        if (to_a) B.ca = c; else B.cb = c;
    }
    store_found(rec, B, iso);
}

void check_aligned(const char* who, const void* p, const char* name, unsigned align)
{
    if (reinterpret_cast<uintptr_t>(p) % align != 0) throw_error("%s: %s must be %u-byte aligned", who, name, align);
}

unsigned blocks_of(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

} // namespace

extern "C" int vanerf_line_state_floats(void) { return VANERF_LINE_STATE_FLOATS; }

extern "C" int vanerf_vertex_normals(const float* verts, int nv, const int32_t* faces, int nf, float* normals, void* stream)
{
    return guarded([&] {
        if (!verts || !faces || !normals) throw_error("vanerf_vertex_normals: null argument");
        if (nv <= 0 || nf <= 0 || nf > (1 << 28)) throw_error("vanerf_vertex_normals: nv=%d nf=%d (positive; nf <= 2^28)", nv, nf);
        hipLaunchKernelGGL(vertex_normals_kernel, dim3(blocks_of(nv, SL_WAVES)), dim3(SL_BLOCK), 0, (hipStream_t)stream, verts, nv, faces, nf, normals);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_line_points(const float* base, const float* dir, int n, int K, float t0, float dt, const float* t_dev, float* pts, void* stream)
{
    return guarded([&] {
        if (n < 0) throw_error("vanerf_line_points: n=%d is negative", n);
        if (K < 1 || K > VANERF_LINE_MAX_SAMPLES) throw_error("vanerf_line_points: K=%d outside [1, %d]", K, VANERF_LINE_MAX_SAMPLES);
        if (t_dev) {
            if (K != 1) throw_error("vanerf_line_points: K=%d with t_dev (one parameter per line: K must be 1)", K);
        } else if (!std::isfinite(t0) || !std::isfinite(dt) || !(dt > 0.0f)) {
            throw_error("vanerf_line_points: t0 must be finite and dt finite and positive (t0 %g, dt %g)", (double)t0, (double)dt);
        }
        const long long total = (long long)n * K;
        if (total > SL_MAX_POINTS) throw_error("vanerf_line_points: n K = %lld points, at most 2^31 - 1", total);
        if (n == 0) return;
        if (!base || !dir || !pts) throw_error("vanerf_line_points: null argument");
        hipLaunchKernelGGL(line_points_kernel, dim3(blocks_of(total, SL_BLOCK)), dim3(SL_BLOCK), 0, (hipStream_t)stream, base, dir, total, K, t0, dt,
                           t_dev, pts);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_line_bracket(const float* f, const float* rgb, int n, int K, float t0, float dt, float iso, float* state, void* stream)
{
    return guarded([&] {
        if (n < 0) throw_error("vanerf_line_bracket: n=%d is negative", n);
        if (K < 2 || K > VANERF_LINE_MAX_SAMPLES) throw_error("vanerf_line_bracket: K=%d outside [2, %d]", K, VANERF_LINE_MAX_SAMPLES);
        if (!std::isfinite(t0) || !std::isfinite(dt) || !(dt > 0.0f))
            throw_error("vanerf_line_bracket: t0 must be finite and dt finite and positive (t0 %g, dt %g)", (double)t0, (double)dt);
        if (!std::isfinite(iso)) throw_error("vanerf_line_bracket: iso must be finite");
        if ((long long)n * K > SL_MAX_POINTS) throw_error("vanerf_line_bracket: n K = %lld samples, at most 2^31 - 1", (long long)n * K);
        if (n == 0) return;
        if (!f || !state) throw_error("vanerf_line_bracket: null argument");
        check_aligned("vanerf_line_bracket", state, "state", 16);
        hipLaunchKernelGGL(line_bracket_kernel, dim3(blocks_of(n, SL_WAVES)), dim3(SL_BLOCK), 0, (hipStream_t)stream, f, rgb, n, K, t0, dt, iso, state);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_line_refine(const float* f_new, const float* rgb_new, int n, float iso, float* state, void* stream)
{
    return guarded([&] {
        if (n < 0) throw_error("vanerf_line_refine: n=%d is negative", n);
        if (!std::isfinite(iso)) throw_error("vanerf_line_refine: iso must be finite");
        if (n == 0) return;
        if (!f_new || !state) throw_error("vanerf_line_refine: null argument");
        check_aligned("vanerf_line_refine", state, "state", 16);
        hipLaunchKernelGGL(line_refine_kernel, dim3(blocks_of(n, SL_BLOCK)), dim3(SL_BLOCK), 0, (hipStream_t)stream, f_new, rgb_new, n, iso, state);
        HIP_CHECK(hipGetLastError());
    });
}
