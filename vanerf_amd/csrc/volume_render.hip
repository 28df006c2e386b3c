// volume_render.hip -- the learned field baked into a voxel grid, and rays marched through it (the comments of
// vanerf_volume_pack / vanerf_volume_render in the header).  At one source view the colour does not depend on the viewing direction and the
// density is a function of f = alpha + mesh_sdf alone, so (f, r, g, b) on a regular grid holds everything an orbit of cameras needs: a view is
// then trilinear gathers and a composite, with no network and no mesh query.  An approximation of the pass (grid resolution, uniform samples),
// never a replacement of it.  The restatement the tests hold these kernels to is the numpy code of tests/test_baked_volume.py.
//
// The render kernel is one wave per ray, lanes over samples in rounds of 64 (wave_ray.h: the pixel tile, march_rounds, the sums), on the
// trilinear field of volume_field.h.  Built with -ffp-contract=off.
#include "common.h"
#include "volume_field.h"
#include "wave_ray.h"

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

// One wave per ray: march_ray names the ray, march_rounds runs its samples; sample i is the field at p = o + d z per axis
// (sample_points_kernel's expression) under sdf_activation.
__global__ __launch_bounds__(64 * RAY_WAVES) void volume_render_kernel(const float4* __restrict__ voxels, const VolGrid G, float beta,
                                                                       const float* __restrict__ beta_dev, const float* __restrict__ rays_d,
                                                                       const float* __restrict__ cam_pos, const float* __restrict__ z,
                                                                       const uint8_t* __restrict__ hit, int rays_per_view, int row_rays, int S,
                                                                       float* __restrict__ color, float* __restrict__ depth, float* __restrict__ alpha)
{
    const int lane = threadIdx.x & 63;
    int v;
    size_t r;
    if (!march_ray(hit, rays_per_view, row_rays, lane, color, depth, alpha, v, r)) return; // whole wave
    if (beta_dev) beta = *beta_dev; // a weight handle's device copy of sigmoid_beta, already clamped
    const float ox = cam_pos[4 * v], oy = cam_pos[4 * v + 1], oz = cam_pos[4 * v + 2];
    const float dx = rays_d[3 * r], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
    const float* zr = z + r * (size_t)S;
    const RaySums<false> sums = march_rounds(zr, S, lane, [&](int i, float zi, float& c, float4& q) {
        if (i >= S) return;
        const float dist = sample_dist(zr, i, S, zi);
        q = field_at_point(voxels, G, ox + dx * zi, oy + dy * zi, oz + dz * zi);
        const float sg = sdf_sigmoid(q.x, beta) / beta;
        c = 1.0f - expf(-sg * dist);
    });
    if (lane == 0) sums.store(color, depth, alpha, nullptr, r);
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
        const char* who = "vanerf_volume_render";
        if (!voxels || !rays_d || !cam_pos || !z || !hit || !color || !depth || !alpha) throw_error("%s: null argument", who);
        check_grid(who, origin, spacing, nx, ny, nz);
        if ((uintptr_t)voxels & 15) throw_error("%s: voxels must be 16-byte aligned", who);
        if (S < 1) throw_error("%s: S = %d samples per ray (at least 1)", who, S);
        beta = check_beta(who, w, beta);
        const int V = check_ray_grid(who, R, rays_per_view, row_rays);
        if (R == 0) return;
        hipLaunchKernelGGL(volume_render_kernel, tile_blocks(row_rays, rays_per_view / row_rays, V), dim3(64 * RAY_WAVES), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4*>(voxels), make_grid(origin, spacing, nx, ny, nz), beta, w ? w->dev_beta : nullptr, rays_d, cam_pos, z,
                           hit, rays_per_view, row_rays, S, color, depth, alpha);
        HIP_CHECK(hipGetLastError());
    });
}
