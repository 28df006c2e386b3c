// pack_math.h -- the arithmetic of the weight packer that the host (weights_pack.cpp) and the device (weights_update.hip) must do bit for bit
// alike: both call these.  (-ffp-contract=off everywhere: no product below is fused unless it says fmaf.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace vanerf {

// torch.nn.utils.weight_norm, dim=0: W[o][:] = v[o][:] * (g[o] / ||v[o][:]||_2) (src/utils.py:674-675).  torch's norm accumulates in fp32
// (vectorised); here in double, in index order (the product of two floats is exact in double): error << 1 ulp of W.
__host__ __device__ inline float weight_norm_scale(const float* v, int kin, float g)
{
    double sum = 0.0;
    for (int k = 0; k < kin; ++k) sum += (double)v[k] * (double)v[k];
    return g / (float)sqrt(sum);
}

// One folded matrix of the lean stream in eff: F[o][c] = sum_k A[o][a0 + k] B[k][c], A at eff + a with rows of kin_a, B [n][nc] at eff + b,
// F [nout][nc] at eff + dst.  Element idx = o * nc + c is one fmaf chain in ascending k.
struct FoldProduct { unsigned a, b, dst; int kin_a, a0, n, nc, nout; };
__host__ __device__ inline float folded_element(const float* eff, const FoldProduct& p, unsigned idx)
{
    const float* a = eff + p.a + (size_t)(idx / (unsigned)p.nc) * p.kin_a + p.a0;
    const float* b = eff + p.b + idx % (unsigned)p.nc;
    float acc = 0.0f;
    for (int k = 0; k < p.n; ++k) acc = fmaf(a[k], b[(size_t)k * p.nc], acc);
    return acc;
}

__host__ __device__ inline unsigned bf16_rne(float f)
{
    const unsigned u = __builtin_bit_cast(unsigned, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u; // NaN stays NaN (the rounding add would carry a full payload over into -0.0); torch's constant
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__host__ __device__ inline unsigned bf16_part(float v, int part) // 0: v rounded to bf16, 1: what that left, rounded to bf16
{
    const unsigned hi = bf16_rne(v);
    return part ? bf16_rne(v - __builtin_bit_cast(float, hi << 16)) : hi;
}

// the gathers of the placement tables (streams.h): one float, one word of a bf16x3 stream
__host__ __device__ inline float placed_f32(const float* eff, int id) { return id ? eff[id - 1] : 0.0f; }
__host__ __device__ inline unsigned placed_bf16x3(const float* eff, int a, int id1)
{
    const int part = (a >> 30) & 1;
    return bf16_part(placed_f32(eff, a & 0x3fffffff), part) | (bf16_part(placed_f32(eff, id1), part) << 16);
}

} // namespace vanerf
