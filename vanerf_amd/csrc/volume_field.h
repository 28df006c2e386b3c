// volume_field.h -- the baked field, written once: voxels (nz, ny, nx) of (f, r, g, b) on a regular grid, read by trilinear interpolation
// with border padding.  volume_render.hip and pose_warp.hip composite this function and volume_surface.hip finds its level set, so the three
// agree bit for bit by construction: the same u, clamp, cell and (1 - w) a + w b order.  The restatement the tests hold it to is the numpy
// code of tests/test_baked_volume.py.  Built with -ffp-contract=off: every product and sum below is its own IEEE operation.
// The host half checks and packs what the three entries share: the grid, sigmoid_beta and the ray layout that wave_ray.h's pixel tile takes.
#pragma once
#include "common.h"

#include <cmath>

namespace vanerf {

struct VolGrid {
    float o[3], s[3];
    int nx, ny, nz;
};

// The grid coordinate of p on one axis, clamped onto the grid (border padding, as feat_sample pads: the ray clip widens the bounds by
// 0.01, so samples just outside the grid are the normal case).  fmaxf(NaN, 0) is 0: a NaN coordinate reads cell 0 with weight 0, never an
// address outside the grid.
__device__ __forceinline__ float coord_of(float p, float origin, float spacing, int n)
{
    const float u = (p - origin) / spacing;
    return fminf(fmaxf(u, 0.0f), (float)(n - 1));
}

// the lower corner i0 of u's cell and the weight w of the upper one (u already clamped)
__device__ __forceinline__ void cell_of(float u, int n, int& i0, float& w)
{
    i0 = min((int)floorf(u), n - 2);
    w = u - (float)i0;
}

// (1 - w) a + w b: with 1e30 entries the difference b - a must not be formed
__device__ __forceinline__ float blend(float w, float a, float b) { return (1.0f - w) * a + w * b; }
__device__ __forceinline__ float4 blend(float w, const float4& a, const float4& b)
{
    const float k = 1.0f - w;
    float4 o;
    o.x = k * a.x + w * b.x; o.y = k * a.y + w * b.y; o.z = k * a.z + w * b.z; o.w = k * a.w + w * b.w;
    return o;
}

// The cell of the clamped grid coordinate (ux, uy, uz): its lower corner `at`, counted in voxels, and the weights of the upper corners.
struct Cell {
    size_t at;
    float wx, wy, wz;
};
__device__ __forceinline__ Cell cell_at(const VolGrid& G, float ux, float uy, float uz)
{
    int ix, iy, iz;
    Cell c;
    cell_of(ux, G.nx, ix, c.wx);
    cell_of(uy, G.ny, iy, c.wy);
    cell_of(uz, G.nz, iz, c.wz);
    c.at = ((size_t)iz * (size_t)G.ny + (size_t)iy) * (size_t)G.nx + (size_t)ix;
    return c;
}

// The interpolation over a cell's eight corners: corner(k) is what the voxel k voxels behind the lower corner holds, a float or a float4.
template <class Corner>
__device__ __forceinline__ auto trilinear(const VolGrid& G, const Cell& c, Corner corner)
{
    const size_t row = (size_t)G.nx, slab = (size_t)G.nx * (size_t)G.ny;
    const auto v000 = corner(0), v100 = corner(1), v010 = corner(row), v110 = corner(row + 1);
    const auto v001 = corner(slab), v101 = corner(slab + 1), v011 = corner(slab + row), v111 = corner(slab + row + 1);
    return blend(c.wz, blend(c.wy, blend(c.wx, v000, v100), blend(c.wx, v010, v110)), blend(c.wy, blend(c.wx, v001, v101), blend(c.wx, v011, v111)));
}

// (f, r, g, b) at the clamped grid coordinate (ux, uy, uz): eight 16-byte loads
__device__ __forceinline__ float4 field_at(const float4* voxels, const VolGrid& G, float ux, float uy, float uz)
{
    const Cell c = cell_at(G, ux, uy, uz);
    const float4* p = voxels + c.at;
    return trilinear(G, c, [&](size_t k) { return p[k]; });
}

// channels C0 .. C0 + NC - 1 of the same function; NC == 1 reads one float per corner (the crossing search reads f alone)
template <int C0, int NC>
__device__ __forceinline__ void field_at(const float* voxels, const VolGrid& G, float ux, float uy, float uz, float* out)
{
    const Cell c = cell_at(G, ux, uy, uz);
    const float* p = voxels + (4 * c.at + C0);
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) out[ch] = trilinear(G, c, [&](size_t k) { return p[4 * k + ch]; });
}

// the field at the world point (x, y, z)
__device__ __forceinline__ float4 field_at_point(const float4* voxels, const VolGrid& G, float x, float y, float z)
{
    return field_at(voxels, G, coord_of(x, G.o[0], G.s[0], G.nx), coord_of(y, G.o[1], G.s[1], G.ny), coord_of(z, G.o[2], G.s[2], G.nz));
}

// ------------------------------------------------------------------------------------------------
// host side: what vanerf_volume_render, vanerf_volume_surface and vanerf_volume_render_posed check and pack alike
// ------------------------------------------------------------------------------------------------
inline void check_grid(const char* who, const float* origin, const float* spacing, int nx, int ny, int nz)
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

inline VolGrid make_grid(const float* origin, const float* spacing, int nx, int ny, int nz)
{
    VolGrid G;
    for (int a = 0; a < 3; ++a) { G.o[a] = origin[a]; G.s[a] = spacing[a]; }
    G.nx = nx; G.ny = ny; G.nz = nz;
    return G;
}

// R rays as whole views of rays_per_view rays in rows of row_rays -> the number of views (blockIdx.y carries the view)
inline int check_ray_grid(const char* who, int R, int rays_per_view, int row_rays)
{
    if (R < 0 || rays_per_view < 1 || row_rays < 1) throw_error("%s: R=%d rays_per_view=%d row_rays=%d", who, R, rays_per_view, row_rays);
    if (R % rays_per_view != 0) throw_error("%s: R = %d is not a whole number of views of %d rays", who, R, rays_per_view);
    if (rays_per_view % row_rays != 0) throw_error("%s: rays_per_view = %d is not a whole number of rows of %d rays", who, rays_per_view, row_rays);
    const int V = R / rays_per_view;
    if (V > 65535) throw_error("%s: %d views (at most 65535)", who, V);
    return V;
}

// sigmoid_beta of a march, by handle (the kernel reads the device copy, already clamped) or by value -> the value the kernel gets
inline float check_beta(const char* who, const VanerfWeights* w, float beta)
{
    if (w && !w->dev_beta) throw_error("%s: the weight handle carries no sigmoid_beta", who);
    if (!w && !(std::isfinite(beta) && beta > 0.0f)) throw_error("%s: beta must be finite and positive", who);
    return beta < 2e-3f ? 2e-3f : beta; // sdf_activation's clamp, as vanerf_composite applies it
}

} // namespace vanerf
