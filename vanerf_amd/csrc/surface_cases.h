// surface_cases.h -- the tables of marching tetrahedra (surface.hip), derived at compile time from the geometry of the split; plain C++17.
//
// Corners of a cell carry the code c = dx | dy << 1 | dz << 2.  The cell is split into the six Kuhn tetrahedra around its main diagonal:
// tetrahedron t walks from corner 0 to corner 7 along the axes in the order TET_PERM[t], v0 = 0, v1 = v0 + e_p0, v2 = v1 + e_p1, v3 = 7.
// det(v1 - v0, v2 - v0, v3 - v0) = det(e_p0, e_p1, e_p2) = the sign of the permutation (positive spacings).
//
// A tetrahedron's sign case is m = sum of (vertex k inside) << k.  For a positively oriented tetrahedron (a, b, c, d) -- any even
// permutation of (v0, v1, v2, v3) -- with the cut points P_xy on its edges:
//   only a inside:   (P_ab, P_ac, P_ad).  With P_ax = a + t_x (x - a) and D = det(b - a, c - a, d - a) > 0 the normal n = (P_ac - P_ab) x (P_ad - P_ab)
//                    has n . (x - a) = t_y t_z D > 0 for each of x = b, c, d ({y, z} the other two): it points from a to the outside.
//   only a outside:  the same triangle reversed.
//   a, b inside:     moving b through the surface in the first case splits P_ab into P_bc (beside P_ac, on face abc) and P_bd (beside P_ad, on
//                    face abd): the polygon (P_ac, P_ad, P_bd, P_bc), cut along P_ac - P_bd, keeps the orientation.
// A case word holds the number of triangles in bits 0-1 and six 3-bit edge numbers from bit 2 (two triangles of three); edges are numbered
// (01, 02, 03, 12, 13, 23).  A negatively oriented tetrahedron swaps the last two corners of every triangle.
#pragma once
#include <cstdint>

namespace vanerf {
namespace surface {

constexpr int TET_PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
constexpr int EDGE_A[6] = {0, 0, 0, 1, 1, 2}, EDGE_B[6] = {1, 2, 3, 2, 3, 3};

constexpr int tet_corner(int t, int k)
{
    int c = 0;
    for (int j = 0; j < k; ++j) c |= 1 << TET_PERM[t][j];
    return c;
}

constexpr bool tet_positive(int t)
{
    int inv = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) inv += TET_PERM[t][i] > TET_PERM[t][j];
    return inv % 2 == 0;
}

constexpr int edge_of(int a, int b)
{
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    for (int e = 0; e < 6; ++e)
        if (EDGE_A[e] == lo && EDGE_B[e] == hi) return e;
    return -1;
}

constexpr bool even4(int a, int b, int c, int d)
{
    const int p[4] = {a, b, c, d};
    int inv = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j) inv += p[i] > p[j];
    return inv % 2 == 0;
}

constexpr uint32_t pack_tri(int e0, int e1, int e2, int slot) { return (uint32_t)(e0 | e1 << 3 | e2 << 6) << (2 + 9 * slot); }

constexpr uint32_t tet_case(int m)
{
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int k = 0; k < 4; ++k) {
        if (m >> k & 1) in[ni++] = k;
        else out[no++] = k;
    }
    if (ni == 0 || ni == 4) return 0;
    if (ni == 2) {
        const int a = in[0], b = in[1];
        int c = out[0], d = out[1];
        if (!even4(a, b, c, d)) { const int s = c; c = d; d = s; }
        return 2u | pack_tri(edge_of(a, c), edge_of(a, d), edge_of(b, d), 0) | pack_tri(edge_of(a, c), edge_of(b, d), edge_of(b, c), 1);
    }
    const int a = ni == 1 ? in[0] : out[0];
    const int* o = ni == 1 ? out : in;
    const int b = o[0];
    int c = o[1], d = o[2];
    if (!even4(a, b, c, d)) { const int s = c; c = d; d = s; }
    if (ni == 3) { const int s = c; c = d; d = s; }
    return 1u | pack_tri(edge_of(a, b), edge_of(a, c), edge_of(a, d), 0);
}

// for tetrahedron t, six bits per edge e: the corner code of its lower end (bits 0-2) and the direction code to its upper end (bits 3-5)
constexpr uint64_t tet_edges(int t)
{
    uint64_t w = 0;
    for (int e = 0; e < 6; ++e) {
        const int ca = tet_corner(t, EDGE_A[e]), cb = tet_corner(t, EDGE_B[e]);
        w |= (uint64_t)(ca | (cb ^ ca) << 3) << (6 * e);
    }
    return w;
}

} // namespace surface
} // namespace vanerf
