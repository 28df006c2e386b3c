// mesh_device.h -- device helpers shared by the mesh translation units (mesh_kernels.hip, mesh_accel_query.hip, mesh_accel_build.hip): the
// per-triangle arithmetic that the exhaustive and the accelerated query must share operation for operation (the twin of oracle/mesh_oracle.c,
// built with -ffp-contract=off), and the wave-level primitives of the searches.
// (A branch-free point_tri_dist2 with one shared division was measured: bit-exact, but 7 % slower -- the lanes of a wave mostly
// agree on the Voronoi region, so the branches are cheap.)
#pragma once
#include "common.h"

namespace vanerf {
namespace {

struct f3 { float x, y, z; };
__device__ __forceinline__ f3 sub3(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot3(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ f3 madd3(f3 a, f3 d, float t) { return {a.x + d.x * t, a.y + d.y * t, a.z + d.z * t}; }

// squared distance from p to triangle (a, b, c); q = the closest point of the triangle
__device__ __forceinline__ float point_tri_dist2_q(f3 p, f3 a, f3 b, f3 c, f3& q)
{
    const f3 ab = sub3(b, a), ac = sub3(c, a), ap = sub3(p, a);
    const float d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0.0f && d2 <= 0.0f) {
        q = a;
    } else {
        const f3 bp = sub3(p, b);
        const float d3 = dot3(ab, bp), d4 = dot3(ac, bp);
        if (d3 >= 0.0f && d4 <= d3) {
            q = b;
        } else {
            const float vc = d1 * d4 - d3 * d2;
            if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
                q = madd3(a, ab, d1 / (d1 - d3));
            } else {
                const f3 cp = sub3(p, c);
                const float d5 = dot3(ab, cp), d6 = dot3(ac, cp);
                if (d6 >= 0.0f && d5 <= d6) {
                    q = c;
                } else {
                    const float vb = d5 * d2 - d1 * d6;
                    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
                        q = madd3(a, ac, d2 / (d2 - d6));
                    } else {
                        const float va = d3 * d6 - d5 * d4;
                        const float e1 = d4 - d3, e2 = d5 - d6;
                        if (va <= 0.0f && e1 >= 0.0f && e2 >= 0.0f) {
                            q = madd3(b, sub3(c, b), e1 / (e1 + e2));
                        } else {
                            const float den = 1.0f / ((va + vb) + vc);
                            const float v = vb * den, w = vc * den;
                            q.x = (a.x + ab.x * v) + ac.x * w;
                            q.y = (a.y + ab.y * v) + ac.y * w;
                            q.z = (a.z + ab.z * v) + ac.z * w;
                        }
                    }
                }
            }
        }
    }
    const f3 r = sub3(p, q);
    return dot3(r, r);
}

__device__ __forceinline__ float point_tri_dist2(f3 p, f3 a, f3 b, f3 c)
{
    f3 q;
    return point_tri_dist2_q(p, a, b, c, q);
}

// canonical (index-ordered) edge function in the (y,z) plane, see oracle/mesh_oracle.c:edge_side
__device__ __forceinline__ float edge_fn(f3 va, f3 vb, int ia, int ib, float qy, float qz)
{
    const bool fwd = ia < ib;
    const f3 lo = fwd ? va : vb, hi = fwd ? vb : va;
    const float e = (hi.y - lo.y) * (qz - lo.z) - (hi.z - lo.z) * (qy - lo.y);
    return fwd ? e : -e;
}

// the side of an edge whose function ties (== 0): as if q were moved by (eps^2, eps) in (y,z), the same displaced point for every edge
__device__ __forceinline__ bool edge_tie_side(f3 va, f3 vb, int ia, int ib)
{
    const bool fwd = ia < ib;
    const f3 lo = fwd ? va : vb, hi = fwd ? vb : va;
    const float dy = hi.y - lo.y, dz = hi.z - lo.z;
    return fwd == ((dy > 0.0f) || (dy == 0.0f && dz < 0.0f));
}

// do the three edge functions of triangle (a, b, c) put (qy, qz) on one side (oracle/mesh_oracle.c:point_inside)?  E0..E2 are the weights of
// a, b, c.  Ties are rare (the +x ray meets an edge's line exactly): all of them are settled in one branch, the common path compares once per edge.
// `by_index` is the answer of the earlier tie rule (a tie goes to the traversal from the lower to the higher vertex index), which a point at
// distance exactly 0 keeps: its sign has no meaning, and the fixtures recorded that one.
__device__ __forceinline__ bool edges_agree(f3 a, f3 b, f3 c, int i0, int i1, int i2, float qy, float qz, float& E0, float& E1, float& E2, bool& by_index)
{
    E0 = edge_fn(b, c, i1, i2, qy, qz);
    E1 = edge_fn(c, a, i2, i0, qy, qz);
    E2 = edge_fn(a, b, i0, i1, qy, qz);
    bool s0 = E0 > 0.0f, s1 = E1 > 0.0f, s2 = E2 > 0.0f;
    bool agree = (s0 && s1 && s2) || (!s0 && !s1 && !s2);
    by_index = agree;
    if (__builtin_expect(E0 == 0.0f || E1 == 0.0f || E2 == 0.0f, 0)) {
        const bool o0 = E0 == 0.0f ? i1 < i2 : s0, o1 = E1 == 0.0f ? i2 < i0 : s1, o2 = E2 == 0.0f ? i0 < i1 : s2;
        by_index = (o0 && o1 && o2) || (!o0 && !o1 && !o2);
        if (E0 == 0.0f) s0 = edge_tie_side(b, c, i1, i2);
        if (E1 == 0.0f) s1 = edge_tie_side(c, a, i2, i0);
        if (E2 == 0.0f) s2 = edge_tie_side(a, b, i0, i1);
        agree = (s0 && s1 && s2) || (!s0 && !s1 && !s2);
    }
    return agree;
}

// The accelerated kernel's first pass over a point's triangles: the earlier tie rule (a tie goes to the traversal from the lower to the higher
// vertex index) at the price it always had, plus a note in `tie` that some edge function was exactly 0.  Only a point with such a note that
// does not lie on the surface is counted again with edges_agree (mesh_query_accel_kernel): ties stay out of the common path altogether.
__device__ __forceinline__ bool edge_side_by_index(f3 va, f3 vb, int ia, int ib, float qy, float qz, float& E, bool& tie)
{
    const bool fwd = ia < ib;
    const f3 lo = fwd ? va : vb, hi = fwd ? vb : va;
    float e = (hi.y - lo.y) * (qz - lo.z) - (hi.z - lo.z) * (qy - lo.y);
    if (!fwd) e = -e;
    E = e;
    tie |= e == 0.0f;
    return (e > 0.0f) || (e == 0.0f && fwd);
}

// +x ray parity (oracle/mesh_oracle.c:point_inside): does the ray from p cross the plane of (a, b, c) beyond p?  E0..E2 are the edge
// functions at (p.y, p.z), the weights of a, b, c; the caller has checked that they agree in sign.
__device__ __forceinline__ bool crosses_beyond(float E0, float E1, float E2, f3 a, f3 b, f3 c, float px)
{
    const float den = (E0 + E1) + E2;
    if (den == 0.0f) return false;
    const float xh = ((E0 * a.x + E1 * b.x) + E2 * c.x) / den;
    return xh > px;
}

// barycentric_coordinates_of_projection (mesh_util.py:321-356) on face bf (the closest one): the interpolated vertex visibility at the
// projection of p, thresholded
__device__ __forceinline__ bool face_visible(const float* __restrict__ V, const int32_t* __restrict__ F, const float* __restrict__ vert_vis, int bf, f3 p)
{
    const int i0 = F[3 * bf], i1 = F[3 * bf + 1], i2 = F[3 * bf + 2];
    const f3 v0 = {V[3 * i0], V[3 * i0 + 1], V[3 * i0 + 2]}, v1 = {V[3 * i1], V[3 * i1 + 1], V[3 * i1 + 2]},
             v2 = {V[3 * i2], V[3 * i2 + 1], V[3 * i2 + 2]};
    const f3 u = sub3(v1, v0), v = sub3(v2, v0);
    const f3 nrm = {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
    float s = dot3(nrm, nrm);
    if (s == 0.0f) s = 1e-6f;
    const float inv = 1.0f / s;
    const f3 wv = sub3(p, v0);
    const f3 c1 = {u.y * wv.z - u.z * wv.y, u.z * wv.x - u.x * wv.z, u.x * wv.y - u.y * wv.x};
    const f3 c2 = {wv.y * v.z - wv.z * v.y, wv.z * v.x - wv.x * v.z, wv.x * v.y - wv.y * v.x};
    const float b2 = dot3(c1, nrm) * inv;
    const float b1 = dot3(c2, nrm) * inv;
    const float w0 = (1.0f - b1) - b2;
    const float sv = (w0 * vert_vis[i0] + b1 * vert_vis[i1]) + b2 * vert_vis[i2];
    return sv >= 0.1f;
}

// Wave-wide reductions on the DPP path (quad swaps, half-row / row mirrors, row broadcasts; the result is read from lane 63 into a scalar
// register): six VALU moves instead of the six LDS round trips of __shfl_xor's ds_bpermute, and no address registers.  The searches of mesh_accel_query.hip
// reduce a few dozen times per 64 points and are bound by exactly this kind of dependent latency.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xF, false); } // masked-off rows keep v
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_f(float v) { return __int_as_float(dpp_i<CTRL, ROW_MASK>(__float_as_int(v))); }
#define VANERF_WAVE_REDUCE(T, DPP, OP)                                                                                                   \
    v = OP(v, DPP<0xB1>(v));        /* quad_perm [1,0,3,2] */                                                                             \
    v = OP(v, DPP<0x4E>(v));        /* quad_perm [2,3,0,1] */                                                                             \
    v = OP(v, DPP<0x141>(v));       /* row_half_mirror */                                                                                 \
    v = OP(v, DPP<0x140>(v));       /* row_mirror: every lane holds its row of 16 */                                                      \
    v = OP(v, DPP<0x142, 0xA>(v));  /* row_bcast15 into rows 1, 3 */                                                                      \
    v = OP(v, DPP<0x143, 0xC>(v));  /* row_bcast31 into rows 2, 3: lane 63 holds all 64 */
__device__ __forceinline__ float wave_min_f(float v) { VANERF_WAVE_REDUCE(float, dpp_f, fminf) return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
__device__ __forceinline__ float wave_max_f(float v) { VANERF_WAVE_REDUCE(float, dpp_f, fmaxf) return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }
__device__ __forceinline__ int wave_min_i(int v) { VANERF_WAVE_REDUCE(int, dpp_i, min) return __builtin_amdgcn_readlane(v, 63); }
#undef VANERF_WAVE_REDUCE

// a value that is the same in every lane, moved to a scalar register (the tile's box, centre, radius: they live through the whole search)
__device__ __forceinline__ float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

__device__ __forceinline__ float box_dist2(f3 p, const float* b)
{
    const float dx = fmaxf(fmaxf(b[0] - p.x, p.x - b[3]), 0.0f);
    const float dy = fmaxf(fmaxf(b[1] - p.y, p.y - b[4]), 0.0f);
    const float dz = fmaxf(fmaxf(b[2] - p.z, p.z - b[5]), 0.0f);
    return (dx * dx + dy * dy) + dz * dz;
}

} // namespace
} // namespace vanerf
