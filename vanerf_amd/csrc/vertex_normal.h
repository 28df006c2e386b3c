// vertex_normal.h -- the vertex normal of a triangle mesh as one wave computes it, shared by the vertex pass of render_vis (vis_render.hip) and
// vanerf_vertex_normals (surface_lines.hip) so that both leave the same bits.  Both files are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vanerf {

__device__ __forceinline__ bool face_ok(int i0, int i1, int i2, int nv)
{
    return (unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv;
}

// x / max(|x|, 1e-6) (torch.nn.functional.normalize, eps 1e-6)
__device__ __forceinline__ float3 normalize_eps(float3 a)
{
    const float n = fmaxf(sqrtf((a.x * a.x + a.y * a.y) + a.z * a.z), 1e-6f);
    return make_float3(a.x / n, a.y / n, a.z / n);
}

// The sum of the normals of vertex v's faces (Meshes.verts_normals_packed: n_f = cross(v2 - v1, v0 - v1) added into each corner), by one whole
// wave: lane l takes faces l, l + 64, ... in ascending order, then a fixed butterfly over the lanes -- no atomics, the same bits every call, in
// every lane.  A face with a vertex index outside [0, nv) is left out.  The caller normalises (normalize_eps).
__device__ __forceinline__ float3 wave_normal_sum(const float* __restrict__ V, int nv, const int32_t* __restrict__ F, int nf, int v, int lane)
{
    float3 n = make_float3(0.0f, 0.0f, 0.0f);
    for (int f = lane; f < nf; f += 64) {
        const int i0 = F[3 * f], i1 = F[3 * f + 1], i2 = F[3 * f + 2];
        if ((i0 != v && i1 != v && i2 != v) || !face_ok(i0, i1, i2, nv)) continue;
        const float3 a = make_float3(V[3 * i0], V[3 * i0 + 1], V[3 * i0 + 2]);
        const float3 b = make_float3(V[3 * i1], V[3 * i1 + 1], V[3 * i1 + 2]);
        const float3 c = make_float3(V[3 * i2], V[3 * i2 + 1], V[3 * i2 + 2]);
        const float3 e1 = make_float3(c.x - b.x, c.y - b.y, c.z - b.z), e2 = make_float3(a.x - b.x, a.y - b.y, a.z - b.z);
        const float3 nf3 = make_float3(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
        // a face that names the vertex twice adds its normal twice (index_add over the three corners)
        const float k = (float)((i0 == v) + (i1 == v) + (i2 == v));
        n.x += k * nf3.x; n.y += k * nf3.y; n.z += k * nf3.z;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        n.x += __shfl_xor(n.x, m);
        n.y += __shfl_xor(n.y, m);
        n.z += __shfl_xor(n.z, m);
    }
    return n;
}

} // namespace vanerf
