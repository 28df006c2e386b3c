// sample_math.h -- the per-sample arithmetic around the layer stack of query_kernel.hip: activations, grid_sample taps and gathers, the
// projection into the source view with its validity mask (shared with query_order.hip: ONE definition, so both take the same decision)
// and the boundary weight.  Built with -ffp-contract=off; fused multiply-adds are spelled fmaf().
#pragma once
#include "common.h"
#include "mfma_chain.h"

namespace vanerf {
namespace {

using vanerf_chain::f32x16;

// ---------------------------------------------------------------------------------------------
// elementwise helpers
// ---------------------------------------------------------------------------------------------
// 1 / (1 + exp(-x)) on v_exp_f32 / v_rcp_f32 (1 ulp each; the gates and boundary weights they feed are compared at 1e-4)
__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504f)); }

// max(x, 0) as ONE v_med3_f32: fmaxf() costs two instructions (the backend first canonicalises the MFMA result)
__device__ __forceinline__ float relu_f(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 3.0e38f); }

// torch.nn.Softplus(beta=100, threshold=20) (src/utils.py:656): x if 100x > 20 else log1p(exp(100x))/100, evaluated as
// max(x,0) + ln2/100 * log2(1 + exp2(-|x| * 100 log2(e))) on the raw v_exp_f32 / v_log_f32 (1 + e is in [1,2]: no denormal or
// range handling).  Above the threshold the correction is < 2.1e-11 and x + it rounds to x (x > 0.2), so no select is
// needed.  |error| < 1e-8 against fp64 over x in [-0.5, 0.5] (tools/probe_trig.hip).  6 VALU instructions, 2 transcendental.
__device__ __forceinline__ float softplus100(float x)
{
    const float e = __builtin_amdgcn_exp2f(fabsf(x) * -144.269504f);
    return fmaf(__builtin_amdgcn_logf(1.0f + e), 6.93147181e-3f, relu_f(x));
}

template <int NB> __device__ __forceinline__ void relu(f32x16 (&a)[NB])
{
#pragma unroll
    for (int ob = 0; ob < NB; ++ob)
#pragma unroll
        for (int r = 0; r < 16; ++r) a[ob][r] = relu_f(a[ob][r]);
}

template <int NB> __device__ __forceinline__ void softplus(f32x16 (&a)[NB])
{
#pragma unroll
    for (int ob = 0; ob < NB; ++ob)
#pragma unroll
        for (int r = 0; r < 16; ++r) a[ob][r] = softplus100(a[ob][r]);
}

// Activation at the point of use.  An activation output is consumed exactly once, as a B operand of the next layer.  The fp32 kernel
// applies the activation to a whole accumulator block right after its layer (VALU time adds to fp32-MFMA time wherever it stands); the
// split-bf16 kernel applies it when the operand is gathered, inside the software pipeline of run_layer_b, where VALU work runs beside
// the MFMAs of the previous k-step.  Same function, same values, same results.
enum Act { ACT_RELU = 1, ACT_SOFTPLUS = 2 };
template <int MODE, int ACT> __device__ __forceinline__ float lazy_act(float v)
{
    if constexpr (MODE == 0) return v; // already applied in bulk
    else if constexpr (ACT == ACT_RELU) return relu_f(v);
    else return softplus100(v);
}

// ---------------------------------------------------------------------------------------------
// grid_sample(bilinear, border, align_corners=True) (src/utils.py:136-151)
// ---------------------------------------------------------------------------------------------
struct Bilin {
    int o00, o01, o10, o11; // pixel offsets y*W + x of the nw, ne, sw, se taps
    float w00, w01, w10, w11;
};

__device__ __forceinline__ Bilin bilin_setup(float x, float y, int H, int W, float wm1, float hm1)
{
    float ix = ((x + 1.0f) / 2.0f) * wm1;
    float iy = ((y + 1.0f) / 2.0f) * hm1;
    ix = fminf(wm1, fmaxf(ix, 0.0f));
    iy = fminf(hm1, fmaxf(iy, 0.0f));
    float fx = floorf(ix), fy = floorf(iy);
    float wx1 = ix - fx, wx0 = (fx + 1.0f) - ix;
    float wy1 = iy - fy, wy0 = (fy + 1.0f) - iy;
    int x0 = (int)fx, y0 = (int)fy;
    int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1); // out-of-range taps carry weight 0
    Bilin b;
    b.o00 = y0 * W + x0; b.o01 = y0 * W + x1; b.o10 = y1 * W + x0; b.o11 = y1 * W + x1;
    b.w00 = wx0 * wy0; b.w01 = wx1 * wy0; b.w10 = wx0 * wy1; b.w11 = wx1 * wy1;
    return b;
}

__device__ __forceinline__ float bilin_mix(const Bilin& b, float v00, float v01, float v10, float v11)
{
    return ((v00 * b.w00 + v01 * b.w01) + v10 * b.w10) + v11 * b.w11;
}

// Load through a wave-uniform base pointer plus a 32-bit BYTE offset: the form `global_load v, v_off, s[base]` needs the
// zero-extended 32-bit offset to be in bytes already (an element offset would have to be widened before the shift: two 64-bit
// VALU adds per load).
template <class T> __device__ __forceinline__ T ld_off(const void* __restrict__ base, unsigned byte_off)
{
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}

// C4 = number of float4 groups to gather from a channel-last map with `C` channels, starting at channel coff.
template <int C4> __device__ __forceinline__ void gather(const float* __restrict__ map, const Bilin& b, int C, int coff, float (&dst)[C4 * 4])
{
    const unsigned o00 = (unsigned)(b.o00 * C + coff) * 4u, o01 = (unsigned)(b.o01 * C + coff) * 4u, o10 = (unsigned)(b.o10 * C + coff) * 4u,
                   o11 = (unsigned)(b.o11 * C + coff) * 4u;
#pragma unroll
    for (int i = 0; i < C4; ++i) {
        const float4 a = ld_off<float4>(map, o00 + 16 * i), c = ld_off<float4>(map, o01 + 16 * i), d = ld_off<float4>(map, o10 + 16 * i),
                     e = ld_off<float4>(map, o11 + 16 * i);
        dst[4 * i + 0] = bilin_mix(b, a.x, c.x, d.x, e.x);
        dst[4 * i + 1] = bilin_mix(b, a.y, c.y, d.y, e.y);
        dst[4 * i + 2] = bilin_mix(b, a.z, c.z, d.z, e.z);
        dst[4 * i + 3] = bilin_mix(b, a.w, c.w, d.w, e.w);
    }
}

template <int C4> __device__ __forceinline__ void load_row(const float* __restrict__ table, unsigned elem_off, float (&dst)[C4 * 4])
{
#pragma unroll
    for (int i = 0; i < C4; ++i) {
        const float4 a = ld_off<float4>(table, elem_off * 4u + 16 * i);
        dst[4 * i] = a.x; dst[4 * i + 1] = a.y; dst[4 * i + 2] = a.z; dst[4 * i + 3] = a.w;
    }
}

// NB accumulator blocks straight from a table row in D-register order: 4 NB loads of 16 bytes
template <int NB> __device__ __forceinline__ void load_acc(const float* __restrict__ table, unsigned elem_off, f32x16 (&acc)[NB])
{
#pragma unroll
    for (int ob = 0; ob < NB; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 a = ld_off<float4>(table, (elem_off + 16u * ob + 4u * i) * 4u);
            acc[ob][4 * i] = a.x; acc[ob][4 * i + 1] = a.y; acc[ob][4 * i + 2] = a.z; acc[ob][4 * i + 3] = a.w;
        }
}

// Projection of a sample into the source view and its validity mask (src/model.py:780-803).  ONE definition, used by query_kernel
// and by the validity partition (query_order.hip), so that both always take the same decision.
struct Projected { float x, y, zn, mask; };
__device__ __forceinline__ Projected project_and_mask(const VanerfFrame& F, float wm1, float hm1, float px, float py, float pz)
{
    const float vx = fmaf(pz, F.KRT[2], fmaf(py, F.KRT[1], px * F.KRT[0])) + F.KRT[3];
    const float vy = fmaf(pz, F.KRT[6], fmaf(py, F.KRT[5], px * F.KRT[4])) + F.KRT[7];
    const float vz = fmaf(pz, F.KRT[10], fmaf(py, F.KRT[9], px * F.KRT[8])) + F.KRT[11];
    Projected r;
    r.x = 2.0f * ((vx / vz) / (F.width - 1.0f)) - 1.0f;
    r.y = 2.0f * ((vy / vz) / (F.height - 1.0f)) - 1.0f;
    r.zn = 2.0f * (vz - F.znear) / (F.zfar - F.znear) - 1.0f;
    const float eps = 1e-2f;
    const bool in_img = (r.x >= -1.0f - eps) && (r.x <= 1.0f + eps) && (r.y >= -1.0f - eps) && (r.y <= 1.0f + eps) && (r.zn >= -1.0f);
    const Bilin bi = bilin_setup(r.x, r.y, F.hi, F.wi, wm1, hm1);
    const float fg = bilin_mix(bi, ld_off<float>(F.mask, 4u * bi.o00), ld_off<float>(F.mask, 4u * bi.o01), ld_off<float>(F.mask, 4u * bi.o10),
                               ld_off<float>(F.mask, 4u * bi.o11));
    r.mask = (in_img && fg > 0.1f) ? 1.0f : 0.0f;
    return r;
}

// Boundary weight of a projected sample (src/model.py:804-821): 0 for a masked-out sample, otherwise p / (p + 1e-6) of the product of three
// sigmoids of the distance to the nearest face of the view volume.
__device__ __forceinline__ float boundary_weight(const Projected& pr)
{
    float ux = 0.5f * pr.x + 0.5f, uy = 0.5f * pr.y + 0.5f, uz = 0.5f * pr.zn + 0.5f;
    float dx = fminf(ux, 1.0f - ux), dy = fminf(uy, 1.0f - uy), dz = fminf(uz, 1.0f - uz);
    float wx = sigmoid_f(5.0f * (dx * 10.0f - 1.0f)), wy = sigmoid_f(5.0f * (dy * 10.0f - 1.0f)),
          wz = sigmoid_f(5.0f * (dz * 10.0f - 1.0f));
    float p = (wx * wy) * wz * pr.mask;
    return p / (p + 1e-6f);
}

} // namespace
} // namespace vanerf
