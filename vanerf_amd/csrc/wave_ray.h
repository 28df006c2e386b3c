// wave_ray.h -- what "one wave per ray" means, written once for the kernels that work that way: the composite and its backward
// (render_kernels.hip), the march through the baked volume (volume_render.hip), its posed form (pose_warp.hip) and the surface search
// (volume_surface.hip).  Lanes hold samples; the transmittance is an exclusive prefix product over the lanes with a fixed shuffle pattern,
// the per-ray sums a fixed xor butterfly in fp64.  No atomics, no device-side state, no LDS.  Every file that includes this is built with
// -ffp-contract=off: every product and sum below is its own IEEE operation, and the same one in every kernel that calls it.
#pragma once
#include "common.h"

#include <cstdint>
#include <type_traits>

namespace vanerf {

// The pixel tile of a block of the per-view kernels: its waves take neighbouring pixels, so their gathers share cache lines.
constexpr int RAY_TX = 2, RAY_TY = 2;
constexpr int RAY_WAVES = RAY_TX * RAY_TY;

// Block (bx, by) of view block_y takes the TX x TY pixels at (TX bx, TY by) of the view's row_rays-wide ray grid, one wave per pixel: a
// block never straddles two views.  False: the wave's pixel is past the edge and the wave leaves whole.  (`wave` is wave-uniform: the
// caller keeps it under readfirstlane.)
template <int TX, int TY>
__device__ __forceinline__ bool tile_ray(unsigned block_x, unsigned block_y, int wave, int row_rays, int rays_per_view, int& v, size_t& r)
{
    const int tiles_x = (row_rays + TX - 1) / TX;
    const int px = (int)(block_x % tiles_x) * TX + (wave % TX);
    const int py = (int)(block_x / tiles_x) * TY + (wave / TX);
    if (px >= row_rays || py >= rays_per_view / row_rays) return false;
    v = block_y;
    r = (size_t)v * (size_t)rays_per_view + (size_t)py * (size_t)row_rays + (size_t)px;
    return true;
}

// the grid of tile_ray's blocks for V views of `rows` rows of row_rays rays
inline dim3 tile_blocks(int row_rays, int rows, int V)
{
    return dim3((unsigned)(((row_rays + RAY_TX - 1) / RAY_TX) * ((rows + RAY_TY - 1) / RAY_TY)), (unsigned)V);
}

// Exclusive multiplicative scan of x over the 64 lanes: `before` is the product of the lanes in front of this one (1 for lane 0), `all`
// the product of all 64.
struct ProductScan {
    float before, all;
};
__device__ __forceinline__ ProductScan exclusive_product_scan(float x, int lane)
{
    float incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float u = __shfl_up(incl, d);
        if (lane >= d) incl *= u;
    }
    ProductScan s;
    s.before = __shfl_up(incl, 1);
    if (lane == 0) s.before = 1.0f;
    s.all = __shfl(incl, 63);
    return s;
}

// sigmoid(-x / beta) of sdf_activation.  The density is sdf_sigmoid(a, beta) / beta and a sample's opacity 1 - expf(-density * dist).
__device__ __forceinline__ float sdf_sigmoid(float x, float beta) { return 1.0f / (1.0f + expf(-(-x / beta))); }

// the distance from sample i of a ray's S depths zr to the next one; the last sample reaches to infinity (rgba2out's 1e10)
__device__ __forceinline__ float sample_dist(const float* zr, int i, int S, float zi) { return i + 1 < S ? zr[i + 1] - zi : 1e10f; }

// rgba2out's sums over the samples of a ray, accumulated in fp64 from fp32 products so that the result does not depend on the summation
// order; SDF: the weighted sdf channel as well (the composite; the marches carry none).
template <bool SDF>
struct RaySums {
    double cr = 0, cg = 0, cb = 0, ca = 0, cs = 0, cd = 0;

    __device__ __forceinline__ void add(float red, float green, float blue, float s, float w, float zi)
    {
        cr += (double)(red * w); cg += (double)(green * w); cb += (double)(blue * w);
        ca += (double)w;
        if (SDF) cs += (double)(s * w);
        cd += (double)(zi * w);
    }
    __device__ __forceinline__ void butterfly() // every lane ends with the wave's sums
    {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            cr += __shfl_xor(cr, d); cg += __shfl_xor(cg, d); cb += __shfl_xor(cb, d);
            ca += __shfl_xor(ca, d);
            if (SDF) cs += __shfl_xor(cs, d);
            cd += __shfl_xor(cd, d);
        }
    }
    template <class Index> // (int in the composite, size_t in the marches: the index arithmetic each of them had)
    __device__ __forceinline__ void store(float* color, float* depth, float* alpha, float* sdf, Index r) const
    {
        const float acc = (float)ca;
        color[3 * r] = (float)cr; color[3 * r + 1] = (float)cg; color[3 * r + 2] = (float)cb;
        alpha[r] = acc;
        if (SDF) sdf[r] = (float)cs / (acc + 1e-8f);
        depth[r] = (float)cd / (acc + 1e-8f);
    }
};

// The ray of this wave in a march over the RAY_TX x RAY_TY tile, or false when there is nothing to march: the pixel is past the edge, or
// the ray misses the box (hit == 0) and its outputs are zero.  Both are whole-wave decisions.
__device__ __forceinline__ bool march_ray(const uint8_t* hit, int rays_per_view, int row_rays, int lane, float* color, float* depth, float* alpha,
                                          int& v, size_t& r)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (!tile_ray<RAY_TX, RAY_TY>(blockIdx.x, blockIdx.y, wave, row_rays, rays_per_view, v, r)) return false;
    if (!hit[r]) {
        if (lane == 0) { color[3 * r] = 0.0f; color[3 * r + 1] = 0.0f; color[3 * r + 2] = 0.0f; depth[r] = 0.0f; alpha[r] = 0.0f; }
        return false;
    }
    return true;
}

// The round loop of a march: lane l of round k holds sample 64 k + l of the ray's S depths zr, the transmittance is carried from round to
// round, so any S >= 1 runs through the one loop.  sample(i, zi, c, q) is called by every lane of every round (it may ballot) and leaves
// the opacity c and q = (f, r, g, b) of sample i, or does not touch them (c = 0: an empty sample, or i >= S); it takes the distance to the
// next sample from sample_dist itself, so that a sample it skips loads nothing.  Returns the wave's sums, in every lane.
template <class Sample>
__device__ __forceinline__ RaySums<false> march_rounds(const float* zr, int S, int lane, Sample sample)
{
    RaySums<false> sums;
    float carry = 1.0f; // the transmittance in front of this round's first sample
    for (int i0 = 0; i0 < S; i0 += 64) { // (S is uniform: every lane runs every round)
        const int i = i0 + lane;
        float c = 0.0f, zi = 0.0f;
        float4 q = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i < S) zi = zr[i];
        sample(i, zi, c, q);
        const ProductScan keep = exclusive_product_scan(1.0f - c, lane); // of 1 - c over the lanes, behind the rounds before
        const float T = carry * keep.before;
        carry = carry * keep.all;
        const float w = c * T;
        if (i < S) sums.add(q.y, q.z, q.w, 0.0f, w, zi);
    }
    sums.butterfly();
    return sums;
}

// The S samples of ray r in merged depth order, gathered from one or two per-ray tables (the coarse samples and the newly drawn importance
// samples): without `src` sample i is entry i of table a, otherwise src >= 0 names entry src of table a and src < 0 entry ~src of table b.
struct SampleTables {
    const float *qa, *ma, *qb, *mb;
    const int32_t* sr;

    __device__ __forceinline__ SampleTables(const float* rgba, const float* msdf, const float* rgba_b, const float* msdf_b, const int32_t* src, int Sa,
                                            int Sb, int S, int r)
    {
        qa = rgba + (size_t)r * Sa * 5;
        ma = msdf + (size_t)r * Sa;
        qb = rgba_b ? rgba_b + (size_t)r * Sb * 5 : nullptr;
        mb = msdf_b ? msdf_b + (size_t)r * Sb : nullptr;
        sr = src ? src + (size_t)r * S : nullptr;
    }
    // where sample i came from: >= 0 entry of table a, < 0 entry ~ of table b
    __device__ __forceinline__ int origin(int i) const { return sr ? sr[i] : i; }
    // the five channels q and the mesh sdf m of the sample that came from k
    __device__ __forceinline__ void fetch(int k, const float*& q, float& m) const
    {
        if (k >= 0) { q = qa + 5 * k; m = ma[k]; } else { q = qb + 5 * (~k); m = mb[~k]; }
    }
};

// The composite kernels hold SPL = 1 .. 4 samples per lane: f(std::integral_constant<int, SPL>) for the narrowest that takes S <= 256.
template <class F>
inline void dispatch_spl(int S, F f)
{
    if (S <= 64) f(std::integral_constant<int, 1>{});
    else if (S <= 128) f(std::integral_constant<int, 2>{});
    else if (S <= 192) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 4>{});
}

} // namespace vanerf
