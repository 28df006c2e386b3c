// volume_surface.hip -- the surface of the baked volume as a camera sees it (DESIGN.md sections 0h and 0k, the comments of vanerf_volume_surface
// and vanerf_volume_surface_posed in the header): per ray the first crossing of f = iso, outside to inside, along the samples of the pass's own
// rays; the crossing refined by 65-way splits; depth, normal (the gradient of the trilinear field), n . v and the interpolated colour there.
// The field is the trilinear function vanerf_volume_render composites: both read it through volume_field.h.  The restatements the tests hold
// these kernels to are the numpy code of tests/test_baked_surface.py and tests/test_posed_surface_cpu.py.
//
// Two kernels over one search: in the SOURCE pose the ray runs through the volume's own space (IdentityMap), in another pose of the mesh every
// sample is carried into it by the record of its closest face (FaceMap; records, face, sdf and the rule for empty samples are pose_warp.hip's).
// Refinement, normal and stores are templates over that map, and the identity compiles to nothing.
//
// The pattern is volume_render_kernel's: one wave per ray, lanes over samples in rounds of 64, the four waves of a block on a 2 x 2 pixel tile
// of one view (wave_ray.h's tile_ray).  A lane gets its neighbour's value by a shuffle (lane 0: the value carried from the round before),
// "outside there, inside here" is a 64-bit ballot and its lowest set bit the crossing; every branch on it is wave-uniform.  No LDS, no
// atomics, no device-side state.
// Built with -ffp-contract=off: every product and sum below is its own IEEE operation.
#include "common.h"
#include "volume_field.h"
#include "wave_ray.h"

#include <cfloat>
#include <cmath>
#include <cstdint>

using namespace vanerf;

namespace {

constexpr int MAX_REFINE = 4;

// The point map of a search: where the ray's point at depth zz lies in the volume's space, and what a gradient taken there is in the ray's
// space.  The search, the refinement and the surface point below are written once over it.  IdentityMap: the ray runs through the volume's
// own space (sample_points_kernel's expression; the gradient is left alone, so vanerf_volume_surface compiles to what it was).
struct IdentityMap {
    __device__ __forceinline__ void point(const float o[3], const float d[3], float zz, float q[3]) const
    {
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = o[a] + d[a] * zz;
    }
    __device__ __forceinline__ void gradient(float g[3]) const {}
};

// FaceMap: the ray runs through POSED space and one face's record (pose_warp.hip: A row-major, then t) carries its points into the source
// space of the volume, q = A p + t as volume_render_posed_kernel writes it; the gradient of f(A p + t) with respect to p is A^T G.
struct FaceMap {
    float4 t0, t1, t2; // A00 A01 A02 A10 | A11 A12 A20 A21 | A22 tx ty tz

    __device__ __forceinline__ FaceMap(const float4* __restrict__ T, int f) : t0(T[3 * (size_t)f]), t1(T[3 * (size_t)f + 1]), t2(T[3 * (size_t)f + 2]) {}
    __device__ __forceinline__ void point(const float o[3], const float d[3], float zz, float q[3]) const
    {
        const float px = o[0] + d[0] * zz, py = o[1] + d[1] * zz, pz = o[2] + d[2] * zz;
        q[0] = ((t0.x * px + t0.y * py) + t0.z * pz) + t2.y;
        q[1] = ((t0.w * px + t1.x * py) + t1.y * pz) + t2.z;
        q[2] = ((t1.z * px + t1.w * py) + t2.x * pz) + t2.w;
    }
    __device__ __forceinline__ void gradient(float g[3]) const
    {
        const float n0 = (t0.x * g[0] + t0.w * g[1]) + t1.z * g[2];
        const float n1 = (t0.y * g[0] + t1.x * g[1]) + t1.w * g[2];
        const float n2 = (t0.z * g[0] + t1.y * g[1]) + t2.x * g[2];
        g[0] = n0; g[1] = n1; g[2] = n2;
    }
};

// g(zz): f at the image of p = o + d zz
template <class Map>
__device__ __forceinline__ float f_along(const float* __restrict__ voxels, const VolGrid& G, const Map& map, const float o[3], const float d[3], float zz)
{
    float q[3], f;
    map.point(o, d, zz, q);
    field_at<0, 1>(voxels, G, coord_of(q[0], G.o[0], G.s[0], G.nx), coord_of(q[1], G.o[1], G.s[1], G.ny), coord_of(q[2], G.o[2], G.s[2], G.nz), &f);
    return f;
}

// whole wave: a miss, or no crossing
__device__ __forceinline__ void store_nothing(int lane, size_t r, float* __restrict__ depth, float4* __restrict__ normal, float* __restrict__ color,
                                              uint8_t* __restrict__ found)
{
    if (lane == 0) {
        depth[r] = 0.0f; normal[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        color[3 * r] = 0.0f; color[3 * r + 1] = 0.0f; color[3 * r + 2] = 0.0f; found[r] = 0;
    }
}

// `refine` rounds of the 65-way split of the bracket (za, zb), f = ga outside and gb inside, then the linear step -> z*.  Wave-uniform.
template <class Map>
__device__ __forceinline__ float refine_bracket(const float* __restrict__ voxels, const VolGrid& G, const Map& map, const float o[3], const float d[3],
                                                float iso, int refine, int lane, float za, float zb, float ga, float gb)
{
    for (int round = 0; round < refine; ++round) { // a, t_0 .. t_63, b: the first adjacent (outside, inside) pair is the new bracket
        const float t = za + ((float)(lane + 1) / 65.0f) * (zb - za);
        const float gt = f_along(voxels, G, map, o, d, t);
        float gp = __shfl_up(gt, 1), tp = __shfl_up(t, 1);
        if (lane == 0) { gp = ga; tp = za; }
        const unsigned long long cross = __ballot(!(gp < iso) && gt < iso);
        if (cross) {
            const int at = __builtin_ctzll(cross);
            za = __shfl(tp, at); zb = __shfl(t, at); ga = __shfl(gp, at); gb = __shfl(gt, at);
        } else { // (t_63, b): a is outside and b inside, so one pair of the sequence crosses
            za = __shfl(t, 63); ga = __shfl(gt, 63);
        }
    }
    const float w = fminf(fmaxf((iso - ga) / (gb - ga), 0.0f), 1.0f);
    return za + w * (zb - za);
}

// The surface point at depth zs of a found ray, whole wave: colour, normal and n . v there, and the ray's four outputs.  Lanes 0 .. 5 take
// the six points of the central difference, the others the point itself (lane 6's colour is used).
template <class Map>
__device__ __forceinline__ void store_surface_point(const float* __restrict__ voxels, const VolGrid& G, const Map& map, const float o[3], const float d[3],
                                                    float zs, int kind, int lane, size_t r, float* __restrict__ depth, float4* __restrict__ normal,
                                                    float* __restrict__ color, uint8_t* __restrict__ found)
{
    float p[3];
    map.point(o, d, zs, p);
    float u[3] = {coord_of(p[0], G.o[0], G.s[0], G.nx), coord_of(p[1], G.o[1], G.s[1], G.ny), coord_of(p[2], G.o[2], G.s[2], G.nz)};
    const float top[3] = {(float)(G.nx - 1), (float)(G.ny - 1), (float)(G.nz - 1)};
    float span[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float up = fminf(u[a] + 1.0f, top[a]), um = fmaxf(u[a] - 1.0f, 0.0f);
        span[a] = (up - um) * G.s[a];
        if (lane == 2 * a) u[a] = up;
        if (lane == 2 * a + 1) u[a] = um;
    }
    float q[4];
    field_at<0, 4>(voxels, G, u[0], u[1], u[2], q);
    float g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = (__shfl(q[0], 2 * a) - __shfl(q[0], 2 * a + 1)) / span[a];
    const float cr = __shfl(q[1], 6), cg = __shfl(q[2], 6), cb = __shfl(q[3], 6);
    if (lane != 0) return;
    map.gradient(g); // into the ray's space
    float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float m = fmaxf(fmaxf(fabsf(g[0]), fabsf(g[1])), fabsf(g[2]));
    if (m > 0.0f && m <= FLT_MAX) { // (a NaN compares false)
        const float hx = g[0] / m, hy = g[1] / m, hz = g[2] / m; // scaled first: 1e30 voxels cannot overflow the squares
        const float len = sqrtf(hx * hx + hy * hy + hz * hz);
        n.x = hx / len; n.y = hy / len; n.z = hz / len;
        const float dlen = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        n.w = fmaxf(0.0f, -((n.x * d[0] + n.y * d[1] + n.z * d[2]) / dlen)); // (fmaxf(0, NaN) is 0: a zero direction)
    }
    depth[r] = zs;
    normal[r] = n; // one 16-byte store
    color[3 * r] = cr; color[3 * r + 1] = cg; color[3 * r + 2] = cb;
    found[r] = (uint8_t)kind;
}

__global__ __launch_bounds__(64 * RAY_WAVES) void volume_surface_kernel(const float* __restrict__ voxels, const VolGrid G, float iso, int refine,
                                                                       const float* __restrict__ rays_d, const float* __restrict__ cam_pos,
                                                                       const float* __restrict__ z, const uint8_t* __restrict__ hit, int rays_per_view,
                                                                       int row_rays, int S, float* __restrict__ depth, float4* __restrict__ normal,
                                                                       float* __restrict__ color, uint8_t* __restrict__ found)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int v;
    size_t r;
    if (!tile_ray<RAY_TX, RAY_TY>(blockIdx.x, blockIdx.y, wave, row_rays, rays_per_view, v, r)) return; // whole wave
    const float o[3] = {cam_pos[4 * v], cam_pos[4 * v + 1], cam_pos[4 * v + 2]};
    const float d[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
    const float* zr = z + r * (size_t)S;
    const IdentityMap map;

    // 0: nothing, 1: a crossing in (za, zb) with f = ga outside and gb inside, 2: sample 0 is inside (za).  Wave-uniform throughout.
    int kind = 0;
    float za = 0.0f, zb = 0.0f, ga = 0.0f, gb = 0.0f;
    if (hit[r]) {
        float carry_g = 0.0f, carry_z = 0.0f; // the last sample of the round before
        for (int i0 = 0; i0 < S; i0 += 64) { // (S is uniform: every lane runs every round it is reached in)
            const int i = i0 + lane;
            float gi = 0.0f, zi = 0.0f;
            if (i < S) {
                zi = zr[i];
                gi = f_along(voxels, G, map, o, d, zi);
            }
            if (i0 == 0 && __shfl(gi, 0) < iso) { // the clipped ray starts inside the hand
                kind = 2;
                za = __shfl(zi, 0);
                break;
            }
            float gp = __shfl_up(gi, 1), zp = __shfl_up(zi, 1);
            if (lane == 0) { gp = carry_g; zp = carry_z; }
            const unsigned long long cross = __ballot(i >= 1 && i < S && !(gp < iso) && gi < iso); // sample i - 1 outside, sample i inside
            if (cross) {
                const int at = __builtin_ctzll(cross);
                kind = 1;
                za = __shfl(zp, at); zb = __shfl(zi, at); ga = __shfl(gp, at); gb = __shfl(gi, at);
                break;
            }
            carry_g = __shfl(gi, 63); carry_z = __shfl(zi, 63);
        }
    }
    if (kind == 0) return store_nothing(lane, r, depth, normal, color, found);
    const float zs = kind == 1 ? refine_bracket(voxels, G, map, o, d, iso, refine, lane, za, zb, ga, gb) : za;
    store_surface_point(voxels, G, map, o, d, zs, kind, lane, r, depth, normal, color, found);
}

// The same search along a ray through the POSED hand (the comment of vanerf_volume_surface_posed in the header): sample i
// is carried into the volume by the record of its own face, or is EMPTY by volume_render_posed_kernel's rule and then outside.  The march
// carries "was the last sample inside" from round to round instead of its value, because the bracket is re-evaluated under ONE map: the
// face F of the inside end comes by shuffle from the crossing lane, and from there on the record is wave-uniform (the refinement points have
// no mesh query of their own).  kind 3: under F's map the near end is inside already, and the depth is held there.  A round all of whose
// samples are empty issues no gather; its samples are outside with or without the branch.
__global__ __launch_bounds__(64 * RAY_WAVES) void volume_surface_posed_kernel(const float* __restrict__ voxels, const VolGrid G, float iso, int refine,
                                                                             const float* __restrict__ rays_d, const float* __restrict__ cam_pos,
                                                                             const float* __restrict__ z, const uint8_t* __restrict__ hit,
                                                                             int rays_per_view, int row_rays, int S, const float4* __restrict__ T, int nf,
                                                                             const int32_t* __restrict__ face, const float* __restrict__ sdf, float reach,
                                                                             float* __restrict__ depth, float4* __restrict__ normal,
                                                                             float* __restrict__ color, uint8_t* __restrict__ found)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int v;
    size_t r;
    if (!tile_ray<RAY_TX, RAY_TY>(blockIdx.x, blockIdx.y, wave, row_rays, rays_per_view, v, r)) return; // whole wave
    const float o[3] = {cam_pos[4 * v], cam_pos[4 * v + 1], cam_pos[4 * v + 2]};
    const float d[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
    const float* zr = z + r * (size_t)S;
    const int32_t* fr = face + r * (size_t)S;
    const float* sr = sdf + r * (size_t)S;

    // 0: nothing, 1: a crossing in (za, zb) whose far end, f = gb, is inside under face F, 2: sample 0 is inside (za, F).  Wave-uniform.
    int kind = 0, F = 0;
    float za = 0.0f, zb = 0.0f, gb = 0.0f;
    if (hit[r]) {
        int carry_in = 0;     // the last sample of the round before: inside?
        float carry_z = 0.0f; // and its depth
        for (int i0 = 0; i0 < S; i0 += 64) { // (S is uniform: every lane runs every round it is reached in)
            const int i = i0 + lane;
            int fi = -1, in = 0;
            float sd = 0.0f, zi = 0.0f, gi = 0.0f;
            if (i < S) { zi = zr[i]; fi = fr[i]; sd = sr[i]; }
            const bool live = fi >= 0 && fi < nf && fabsf(sd) <= FLT_MAX && sd <= reach; // (NaN compares false; i >= S: fi = -1)
            if (__ballot(live) != 0ull && live) { // (the ballot is wave-uniform: an all-empty round gathers nothing)
                gi = f_along(voxels, G, FaceMap(T, fi), o, d, zi);
                in = gi < iso;
            }
            if (i0 == 0 && __shfl(in, 0)) { // the clipped ray starts inside the hand
                kind = 2;
                za = __shfl(zi, 0); F = __shfl(fi, 0);
                break;
            }
            int ip = __shfl_up(in, 1);
            float zp = __shfl_up(zi, 1);
            if (lane == 0) { ip = carry_in; zp = carry_z; }
            const unsigned long long cross = __ballot(i >= 1 && !ip && in); // sample i - 1 not inside, sample i inside (so i < S)
            if (cross) {
                const int at = __builtin_ctzll(cross);
                kind = 1;
                za = __shfl(zp, at); zb = __shfl(zi, at); gb = __shfl(gi, at); F = __shfl(fi, at);
                break;
            }
            carry_in = __shfl(in, 63); carry_z = __shfl(zi, 63);
        }
    }
    if (kind == 0) return store_nothing(lane, r, depth, normal, color, found);
    const FaceMap map(T, __builtin_amdgcn_readfirstlane(F)); // one record for the whole wave (F is in [0, nf): its sample was live)
    float zs = za;
    if (kind == 1) {
        const float ga = f_along(voxels, G, map, o, d, za); // the near end under F's map, whatever sample k was
        if (ga < iso) kind = 3; // the surface under F's map lies at or in front of sample k: the depth is held at the bracket's near end
        else zs = refine_bracket(voxels, G, map, o, d, iso, refine, lane, za, zb, ga, gb);
    }
    store_surface_point(voxels, G, map, o, d, zs, kind, lane, r, depth, normal, color, found);
}

} // namespace

extern "C" int vanerf_volume_surface(const float* voxels, const float origin[3], const float spacing[3], int nx, int ny, int nz, float iso, int refine,
                                     const float* rays_d, const float* cam_pos, const float* z, const uint8_t* hit, int R, int rays_per_view, int row_rays,
                                     int S, float* depth, float* normal, float* color, uint8_t* found, void* stream)
{
    return guarded([&] {
        const char* who = "vanerf_volume_surface";
        if (!voxels || !rays_d || !cam_pos || !z || !hit || !depth || !normal || !color || !found) throw_error("%s: null argument", who);
        check_grid(who, origin, spacing, nx, ny, nz);
        if ((uintptr_t)voxels & 15) throw_error("%s: voxels must be 16-byte aligned", who);
        if ((uintptr_t)normal & 15) throw_error("%s: normal must be 16-byte aligned", who);
        if (S < 1) throw_error("%s: S = %d samples per ray (at least 1)", who, S);
        if (!std::isfinite(iso)) throw_error("%s: iso must be finite", who);
        if (refine < 0 || refine > MAX_REFINE) throw_error("%s: refine = %d outside [0, %d]", who, refine, MAX_REFINE);
        const int V = check_ray_grid(who, R, rays_per_view, row_rays);
        if (R == 0) return;
        hipLaunchKernelGGL(volume_surface_kernel, tile_blocks(row_rays, rays_per_view / row_rays, V), dim3(64 * RAY_WAVES), 0, (hipStream_t)stream, voxels,
                           make_grid(origin, spacing, nx, ny, nz), iso, refine, rays_d, cam_pos, z, hit,
                           rays_per_view, row_rays, S, depth, reinterpret_cast<float4*>(normal), color, found);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_volume_surface_posed(const float* voxels, const float origin[3], const float spacing[3], int nx, int ny, int nz, float iso, int refine,
                                           const float* rays_d, const float* cam_pos, const float* z, const uint8_t* hit, int R, int rays_per_view,
                                           int row_rays, int S, const float* T, int nf, const int32_t* face, const float* sdf, float reach, float* depth,
                                           float* normal, float* color, uint8_t* found, void* stream)
{
    return guarded([&] {
        const char* who = "vanerf_volume_surface_posed";
        if (!voxels || !rays_d || !cam_pos || !z || !hit || !T || !face || !sdf || !depth || !normal || !color || !found) throw_error("%s: null argument", who);
        check_grid(who, origin, spacing, nx, ny, nz);
        if (((uintptr_t)voxels & 15) || ((uintptr_t)T & 15)) throw_error("%s: voxels and T must be 16-byte aligned", who);
        if ((uintptr_t)normal & 15) throw_error("%s: normal must be 16-byte aligned", who);
        if (S < 1) throw_error("%s: S = %d samples per ray (at least 1)", who, S);
        if (nf < 1) throw_error("%s: nf = %d faces (at least 1)", who, nf);
        if (std::isnan(reach)) throw_error("%s: reach must not be NaN (+inf disables it)", who);
        if (!std::isfinite(iso)) throw_error("%s: iso must be finite", who);
        if (refine < 0 || refine > MAX_REFINE) throw_error("%s: refine = %d outside [0, %d]", who, refine, MAX_REFINE);
        const int V = check_ray_grid(who, R, rays_per_view, row_rays);
        if (R == 0) return;
        hipLaunchKernelGGL(volume_surface_posed_kernel, tile_blocks(row_rays, rays_per_view / row_rays, V), dim3(64 * RAY_WAVES), 0, (hipStream_t)stream,
                           voxels, make_grid(origin, spacing, nx, ny, nz), iso, refine, rays_d, cam_pos, z, hit, rays_per_view, row_rays, S,
                           reinterpret_cast<const float4*>(T), nf, face, sdf, reach, depth, reinterpret_cast<float4*>(normal), color, found);
        HIP_CHECK(hipGetLastError());
    });
}
