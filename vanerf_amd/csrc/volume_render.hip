// volume_render.hip -- the learned field baked into a voxel grid, and rays marched through it (the comments of
// vanerf_volume_pack / vanerf_volume_render in the header).  At one source view the colour does not depend on the viewing direction and the
// density is a function of f = alpha + mesh_sdf alone, so (f, r, g, b) on a regular grid holds everything an orbit of cameras needs: a view is
// then trilinear gathers and a composite, with no network and no mesh query.  An approximation of the pass (grid resolution, uniform samples),
// never a replacement of it.  The restatement the tests hold these kernels to is the numpy code of tests/test_baked_volume.py.
//
// The render kernel restates composite_wave_kernel's pattern (render_kernels.hip): one wave per ray, lanes over samples, the transmittance an
// exclusive prefix product over the lanes with a fixed shuffle pattern, the sums a fixed xor butterfly in fp64 -- here in rounds of 64 samples
// with the transmittance carried from round to round, so any S >= 1 runs through the one kernel.  No atomics, no device-side state, no LDS.
// Built with -ffp-contract=off: every product and sum below is its own IEEE operation.
#include "common.h"

#include <cfloat>
#include <cmath>
#include <cstdint>

using namespace vanerf;

namespace {

constexpr int VP_BLOCK = 256;
constexpr float VOL_OUTSIDE = 1e30f; // what a non-finite f is stored as: sigmoid(-1e30 / beta) is exactly 0, and eight weights that sum to 1
                                     // can neither overflow it nor meet an infinity (0 * inf)

__global__ __launch_bounds__(VP_BLOCK) void volume_pack_kernel(const float* __restrict__ f, const float* __restrict__ rgb, long long n,
                                                               float4* __restrict__ voxels)
{
    const long long i = (long long)blockIdx.x * VP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float v = f[i], r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    float4 o;
    o.x = fabsf(v) <= FLT_MAX ? v : VOL_OUTSIDE; // (NaN compares false)
    o.y = fabsf(r) <= FLT_MAX ? r : 0.0f;
    o.z = fabsf(g) <= FLT_MAX ? g : 0.0f;
    o.w = fabsf(b) <= FLT_MAX ? b : 0.0f;
    voxels[i] = o;
}

struct VolGrid {
    float o[3], s[3];
    int nx, ny, nz;
};

constexpr int VR_TX = 2, VR_TY = 2;          // the pixel tile of a block: its waves take neighbouring pixels, so their gathers share cache lines
constexpr int VR_WAVES = VR_TX * VR_TY;

// Grid coordinate of p on one axis, clamped onto the grid (border padding, as feat_sample pads: the ray clip widens the bounds by 0.01, so
// samples just outside the grid are the normal case), as the lower corner i0 of its cell and the weight w of the upper one.
// fmaxf(NaN, 0) is 0: a NaN coordinate reads cell 0 with weight 0, never an address outside the grid.
__device__ __forceinline__ void cell_of(float p, float origin, float spacing, int n, int& i0, float& w)
{
    float u = (p - origin) / spacing;
    u = fminf(fmaxf(u, 0.0f), (float)(n - 1));
    i0 = min((int)floorf(u), n - 2);
    w = u - (float)i0;
}

// (1 - w) a + w b per channel: with 1e30 entries the difference b - a must not be formed
__device__ __forceinline__ float4 blend(float w, const float4& a, const float4& b)
{
    const float k = 1.0f - w;
    float4 o;
    o.x = k * a.x + w * b.x; o.y = k * a.y + w * b.y; o.z = k * a.z + w * b.z; o.w = k * a.w + w * b.w;
    return o;
}

// One wave per ray, lane l of round k holds sample 64 k + l.  Block (bx, by) of view blockIdx.y takes the VR_TX x VR_TY pixels at
// (VR_TX bx, VR_TY by) of the view's row_rays-wide ray grid: a block never straddles two views, and a wave past the edge leaves whole.
__global__ __launch_bounds__(64 * VR_WAVES) void volume_render_kernel(const float4* __restrict__ voxels, const VolGrid G, float beta,
                                                                      const float* __restrict__ beta_dev, const float* __restrict__ rays_d,
                                                                      const float* __restrict__ cam_pos, const float* __restrict__ z,
                                                                      const uint8_t* __restrict__ hit, int rays_per_view, int row_rays, int S,
                                                                      float* __restrict__ color, float* __restrict__ depth, float* __restrict__ alpha)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tiles_x = (row_rays + VR_TX - 1) / VR_TX;
    const int px = (int)(blockIdx.x % tiles_x) * VR_TX + (wave % VR_TX);
    const int py = (int)(blockIdx.x / tiles_x) * VR_TY + (wave / VR_TX);
    if (px >= row_rays || py >= rays_per_view / row_rays) return; // whole wave
    const int v = blockIdx.y;
    const size_t r = (size_t)v * (size_t)rays_per_view + (size_t)py * (size_t)row_rays + (size_t)px;
    if (!hit[r]) { // whole wave: the ray misses the box
        if (lane == 0) { color[3 * r] = 0.0f; color[3 * r + 1] = 0.0f; color[3 * r + 2] = 0.0f; depth[r] = 0.0f; alpha[r] = 0.0f; }
        return;
    }
    if (beta_dev) beta = *beta_dev; // a weight handle's device copy of sigmoid_beta, already clamped
    const float ox = cam_pos[4 * v], oy = cam_pos[4 * v + 1], oz = cam_pos[4 * v + 2];
    const float dx = rays_d[3 * r], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
    const float* zr = z + r * (size_t)S;
    const size_t row = (size_t)G.nx, slab = (size_t)G.nx * (size_t)G.ny;
    double cr = 0, cg = 0, cb = 0, ca = 0, cd = 0;
    float carry = 1.0f; // the transmittance in front of this round's first sample
    for (int i0 = 0; i0 < S; i0 += 64) { // (S is uniform: every lane runs every round)
        const int i = i0 + lane;
        float c = 0.0f, zi = 0.0f;
        float4 q = {0.0f, 0.0f, 0.0f, 0.0f};
        if (i < S) {
            zi = zr[i];
            const float dist = i + 1 < S ? zr[i + 1] - zi : 1e10f;
            int ix, iy, iz;
            float wx, wy, wz;
            cell_of(ox + dx * zi, G.o[0], G.s[0], G.nx, ix, wx); // p = o + d z per axis: sample_points_kernel's expression
            cell_of(oy + dy * zi, G.o[1], G.s[1], G.ny, iy, wy);
            cell_of(oz + dz * zi, G.o[2], G.s[2], G.nz, iz, wz);
            const float4* p = voxels + (((size_t)iz * (size_t)G.ny + (size_t)iy) * row + (size_t)ix);
            const float4 v000 = p[0], v100 = p[1], v010 = p[row], v110 = p[row + 1];
            const float4 v001 = p[slab], v101 = p[slab + 1], v011 = p[slab + row], v111 = p[slab + row + 1];
            q = blend(wz, blend(wy, blend(wx, v000, v100), blend(wx, v010, v110)), blend(wy, blend(wx, v001, v101), blend(wx, v011, v111)));
            const float a = q.x;
            const float sg = (1.0f / (1.0f + expf(-(-a / beta)))) / beta; // sigmoid(-a / beta) / beta, composite_kernel's expression
            c = 1.0f - expf(-sg * dist);
        }
        // exclusive multiplicative scan of 1 - c over the lanes, behind the rounds before
        float incl = 1.0f - c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float u = __shfl_up(incl, d);
            if (lane >= d) incl *= u;
        }
        float T = __shfl_up(incl, 1);
        if (lane == 0) T = 1.0f;
        T = carry * T;
        carry = carry * __shfl(incl, 63);
        const float w = c * T;
        if (i < S) {
            cr += (double)(q.y * w); cg += (double)(q.z * w); cb += (double)(q.w * w);
            ca += (double)w; cd += (double)(zi * w);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        cr += __shfl_xor(cr, d); cg += __shfl_xor(cg, d); cb += __shfl_xor(cb, d);
        ca += __shfl_xor(ca, d); cd += __shfl_xor(cd, d);
    }
    if (lane == 0) {
        const float acc = (float)ca;
        color[3 * r] = (float)cr; color[3 * r + 1] = (float)cg; color[3 * r + 2] = (float)cb;
        alpha[r] = acc;
        depth[r] = (float)cd / (acc + 1e-8f);
    }
}

void check_grid(const char* who, const float* origin, const float* spacing, int nx, int ny, int nz)
{
    if (!origin || !spacing) throw_error("%s: null argument", who);
    if (nx < 2 || ny < 2 || nz < 2) throw_error("%s: a grid of (%d, %d, %d) points: every dimension must be at least 2", who, nx, ny, nz);
    if (7LL * nx * ny >= (1LL << 31) || 7LL * nx * ny * nz >= (1LL << 31))
        throw_error("%s: a grid of (%d, %d, %d) points is too large: 7 nx ny nz must stay below 2^31", who, nx, ny, nz);
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin[a])) throw_error("%s: the grid origin must be finite", who);
        if (!(std::isfinite(spacing[a]) && spacing[a] > 0.0f)) throw_error("%s: the grid spacing must be finite and positive", who);
    }
}

} // namespace

extern "C" int vanerf_volume_pack(const float* f, const float* rgb, int64_t n, float* voxels, void* stream)
{
    return guarded([&] {
        if (!f || !rgb || !voxels) throw_error("vanerf_volume_pack: null argument");
        if (n < 0 || n >= (1LL << 31)) throw_error("vanerf_volume_pack: n = %lld outside [0, 2^31)", (long long)n);
        if ((uintptr_t)voxels & 15) throw_error("vanerf_volume_pack: voxels must be 16-byte aligned");
        if (n == 0) return;
        hipLaunchKernelGGL(volume_pack_kernel, dim3((unsigned)((n + VP_BLOCK - 1) / VP_BLOCK)), dim3(VP_BLOCK), 0, (hipStream_t)stream, f, rgb, (long long)n,
                           reinterpret_cast<float4*>(voxels));
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_volume_render(const float* voxels, const float origin[3], const float spacing[3], int nx, int ny, int nz, const VanerfWeights* w,
                                    float beta, const float* rays_d, const float* cam_pos, const float* z, const uint8_t* hit, int R, int rays_per_view,
                                    int row_rays, int S, float* color, float* depth, float* alpha, void* stream)
{
    return guarded([&] {
        if (!voxels || !rays_d || !cam_pos || !z || !hit || !color || !depth || !alpha) throw_error("vanerf_volume_render: null argument");
        check_grid("vanerf_volume_render", origin, spacing, nx, ny, nz);
        if ((uintptr_t)voxels & 15) throw_error("vanerf_volume_render: voxels must be 16-byte aligned");
        if (S < 1) throw_error("vanerf_volume_render: S = %d samples per ray (at least 1)", S);
        if (w && !w->dev_beta) throw_error("vanerf_volume_render: the weight handle carries no sigmoid_beta");
        if (!w && !(std::isfinite(beta) && beta > 0.0f)) throw_error("vanerf_volume_render: beta must be finite and positive");
        if (R < 0 || rays_per_view < 1 || row_rays < 1) throw_error("vanerf_volume_render: R=%d rays_per_view=%d row_rays=%d", R, rays_per_view, row_rays);
        if (R % rays_per_view != 0) throw_error("vanerf_volume_render: R = %d is not a whole number of views of %d rays", R, rays_per_view);
        if (rays_per_view % row_rays != 0)
            throw_error("vanerf_volume_render: rays_per_view = %d is not a whole number of rows of %d rays", rays_per_view, row_rays);
        const int V = R / rays_per_view;
        if (V > 65535) throw_error("vanerf_volume_render: %d views (at most 65535)", V);
        if (R == 0) return;
        if (beta < 2e-3f) beta = 2e-3f; // sdf_activation's clamp, as vanerf_composite applies it (a handle's device copy is clamped already)
        VolGrid G;
        for (int a = 0; a < 3; ++a) { G.o[a] = origin[a]; G.s[a] = spacing[a]; }
        G.nx = nx; G.ny = ny; G.nz = nz;
        const int rows = rays_per_view / row_rays;
        const dim3 blocks((unsigned)(((row_rays + VR_TX - 1) / VR_TX) * ((rows + VR_TY - 1) / VR_TY)), (unsigned)V);
        hipLaunchKernelGGL(volume_render_kernel, blocks, dim3(64 * VR_WAVES), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(voxels), G, beta,
                           w ? w->dev_beta : nullptr, rays_d, cam_pos, z, hit, rays_per_view, row_rays, S, color, depth, alpha);
        HIP_CHECK(hipGetLastError());
    });
}
