// mano_tables.h -- what mano_skin.hip (the forward), mano_skin_backward.hip and mano_skin_normal.hip share on the host: the limits of a
// MANO-shaped model, the layout of the buffer vanerf_mano_pack writes, and the small helpers of their entries.  Host code only; the kernels
// take ManoTables by value (the device code the three share is mano_forward.h).
#pragma once
#include "common.h"

#include <cstdint>

namespace vanerf {
namespace mano {

constexpr int MANO_MAX_NJ = 32;
constexpr int MANO_MAX_NB = 16;
constexpr int MANO_MAX_RING = 64;
constexpr int MV_BLOCK = 256;

// The packed model: a host-side description of one device buffer.  fp64 tables first (the buffer is 16-byte aligned), then parents, then the
// transposed fp32 tables.
struct ManoTables {
    const double* Jt;      // [nj][3]        J_regressor . v_template
    const double* Js;      // [nj][3][nb]    J_regressor . shapedirs
    const double* hm;      // [nj][3]        hands_mean as doubles, zeros for the root
    const int32_t* parents; // [nj]
    const float* vt;       // [3][nv]
    const float* sd;       // [nb][3][nv]
    const float* pd;       // [(nj-1)*9][3][nv]
    const float* wt;       // [nj][nv]
};

struct ManoLayout {
    int64_t Jt, Js, hm, parents, vt, sd, pd, wt, bytes;
};

inline ManoLayout mano_layout(int nv, int nj, int nb)
{
    ManoLayout L;
    int64_t at = 0;
    L.Jt = at; at += (int64_t)nj * 3 * 8;
    L.Js = at; at += (int64_t)nj * 3 * nb * 8;
    L.hm = at; at += (int64_t)nj * 3 * 8;
    L.parents = at; at += (int64_t)((nj + 3) / 4 * 4) * 4;
    L.vt = at; at += (int64_t)3 * nv * 4;
    L.sd = at; at += (int64_t)nb * 3 * nv * 4;
    L.pd = at; at += (int64_t)(nj - 1) * 9 * 3 * nv * 4;
    L.wt = at; at += (int64_t)nj * nv * 4;
    L.bytes = (at + 15) / 16 * 16;
    return L;
}

inline ManoTables mano_tables(const void* packed, int nv, int nj, int nb)
{
    const ManoLayout L = mano_layout(nv, nj, nb);
    const char* b = static_cast<const char*>(packed);
    ManoTables t;
    t.Jt = reinterpret_cast<const double*>(b + L.Jt);
    t.Js = reinterpret_cast<const double*>(b + L.Js);
    t.hm = reinterpret_cast<const double*>(b + L.hm);
    t.parents = reinterpret_cast<const int32_t*>(b + L.parents);
    t.vt = reinterpret_cast<const float*>(b + L.vt);
    t.sd = reinterpret_cast<const float*>(b + L.sd);
    t.pd = reinterpret_cast<const float*>(b + L.pd);
    t.wt = reinterpret_cast<const float*>(b + L.wt);
    return t;
}

inline int ws_floats(int nj) { return nj * 12 + (nj - 1) * 9; } // per pose: A, then the pose feature

inline void check_sizes(const char* who, int nv, int nj, int nb)
{
    if (nv < 1) throw_error("%s: nv=%d vertices (at least 1)", who, nv);
    if (nj < 1 || nj > MANO_MAX_NJ) throw_error("%s: nj=%d joints (1 .. %d)", who, nj, MANO_MAX_NJ);
    if (nb < 1 || nb > MANO_MAX_NB) throw_error("%s: nb=%d shape coefficients (1 .. %d)", who, nb, MANO_MAX_NB);
    if ((int64_t)nv * 3 * (int64_t)(nj - 1) * 9 > 0x7fffffffLL) throw_error("%s: posedirs of nv=%d nj=%d has more than 2^31 - 1 values", who, nv, nj);
}

struct IntList32 { int32_t v[MANO_MAX_NJ]; };
struct IntList64 { int32_t v[MANO_MAX_RING]; };

// The seal's ring as a kernel argument, checked; entries from n_ring on are 0 and every reader guards with u < n_ring.
inline IntList64 ring_list(const char* who, const int32_t* ring, int n_ring, int nv)
{
    if (n_ring < 0 || n_ring > MANO_MAX_RING) throw_error("%s: n_ring=%d (0 = no seal .. %d)", who, n_ring, MANO_MAX_RING);
    if (n_ring > 0 && !ring) throw_error("%s: null argument (ring with n_ring=%d)", who, n_ring);
    IntList64 rg;
    for (int u = 0; u < MANO_MAX_RING; ++u) rg.v[u] = 0;
    for (int u = 0; u < n_ring; ++u) {
        if (ring[u] < 0 || ring[u] >= nv) throw_error("%s: ring[%d]=%d names no vertex of nv=%d", who, u, ring[u], nv);
        rg.v[u] = ring[u];
    }
    return rg;
}

inline void check_stride(const char* who, const char* what, int64_t stride, int64_t floats)
{
    if (stride < floats) throw_error("%s: %s_stride=%lld is below a row's %lld floats", who, what, (long long)stride, (long long)floats);
}

// A size query of the C ABI: the bytes `size()` returns, or its refusal as a negative error code.
template <class F>
inline int64_t size_query(F&& size)
{
    int64_t bytes = -1;
    const int rc = guarded([&] { bytes = size(); });
    return rc == VANERF_OK ? bytes : (int64_t)rc;
}

inline unsigned blocks_of(const char* who, int64_t n, int per)
{
    const int64_t b = (n + per - 1) / per;
    if (b > 0x7fffffffLL) throw_error("%s: %lld blocks exceed a launch's 2^31 - 1", who, (long long)b);
    return (unsigned)b;
}

} // namespace mano
} // namespace vanerf
