// surface.hip -- the learned surface as a triangle mesh: a regular grid of points, the signed field f = alpha + mesh_sdf on it, and marching
// tetrahedra over the grid of scalars (the comments of vanerf_grid_points ... vanerf_surface_emit in the header).  The
// restatement the tests hold these kernels to is the fp64 numpy code of tests/test_surface_march.py.
//
// The extractor is two calls with one host read between them.  vanerf_surface_count: one block per brick of 8 x 8 x 8 grid points stages the
// brick's 9^3 values in LDS, flags the active ones of the seven edges every point owns, counts the triangles of the cell at every point, ranks
// both inside the block (ballots over the bits of the per-thread counts, v_mbcnt) and leaves a word per point and two totals per block; one
// more block scans the block totals.  vanerf_surface_emit: the same bricks interpolate the vertices of their own edges and write the triangles
// of their own cells, looking the vertex numbers of the 19 edges of a cell up in the staged words of its eight corners.  Numbers follow the
// order (block, thread, edge) and (block, thread, tetrahedron): no atomics, no device globals, the same bits every call.
//
// Every point, edge, cell and tetrahedron is indexed with 32 bits: 7 nx ny nz < 2^31 is checked on the host.
#include "common.h"
#include "surface_cases.h"

#include <cfloat>
#include <cmath>

using namespace vanerf;
namespace sc = vanerf::surface;

namespace {

constexpr int SF_B = 8;                          // grid points of a brick per axis
constexpr int SF_H = SF_B + 1;                   // with the halo towards +x, +y, +z
constexpr int SF_THREADS = SF_B * SF_B * SF_B;   // one thread per point / cell: eight waves, a wave is one z-layer of the brick
constexpr int SF_STAGE = SF_H * SF_H * SF_H;
constexpr int SF_SCAN = 1024;
constexpr int PT_BLOCK = 256;

struct SfAxes { float o[3], s[3]; };
struct SfDims { int nx, ny, nz, bx, by, bz; };   // grid points and bricks per axis

constexpr uint32_t SF_CASE[16] = {sc::tet_case(0), sc::tet_case(1), sc::tet_case(2), sc::tet_case(3), sc::tet_case(4), sc::tet_case(5),
                                  sc::tet_case(6), sc::tet_case(7), sc::tet_case(8), sc::tet_case(9), sc::tet_case(10), sc::tet_case(11),
                                  sc::tet_case(12), sc::tet_case(13), sc::tet_case(14), sc::tet_case(15)};

// The coordinate of grid index i on an axis: one fused multiply-add, one rounding.  vanerf_grid_points and the extractor share it.
__device__ __forceinline__ float grid_coord(int i, float origin, float spacing) { return fmaf((float)i, spacing, origin); }

// A field value as the extractor reads it: non-finite -> +FLT_MAX (outside).
__device__ __forceinline__ float field_read(float v) { return fabsf(v) <= FLT_MAX ? v : FLT_MAX; }

__device__ __forceinline__ int mbcnt(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// Exclusive prefix of v (0 <= v < 2^BITS) over the block's threads in thread order, and the block's total: a ballot per bit of v inside
// the wave, then the eight waves in order.  s_wave: SF_THREADS / 64 ints of LDS, free again when the call returns.
template <int BITS>
__device__ __forceinline__ int block_prefix(int v, int* s_wave, int& total)
{
    int pre = 0, wsum = 0;
#pragma unroll
    for (int k = 0; k < BITS; ++k) {
        const unsigned long long m = __ballot((v >> k) & 1);
        pre += mbcnt(m) << k;
        wsum += __builtin_popcountll(m) << k;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_wave[wave] = wsum;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < SF_THREADS / 64; ++w) {
        const int c = s_wave[w];
        base += w < wave ? c : 0;
        total += c;
    }
    __syncthreads();
    return base + pre;
}

struct SfThread {
    int gx, gy, gz;    // the thread's grid point
    int own;           // its place in the staged 9^3 arrays
    bool point, cell;  // the point is in the grid; so is the cell it is the lowest corner of
    unsigned inside;   // bit c: corner c of that cell is inside (f < iso); corners outside the grid read as outside
    unsigned edges;    // bit d - 1: the edge from the point towards direction code d exists and has exactly one end inside
};

__device__ __forceinline__ void brick_origin(const SfDims& D, int& x0, int& y0, int& z0)
{
    const int b = blockIdx.x;
    x0 = (b % D.bx) * SF_B;
    y0 = (b / D.bx % D.by) * SF_B;
    z0 = (b / (D.bx * D.by)) * SF_B;
}

// Stages the brick's values, as the extractor reads them, in s_f[SF_STAGE] (places outside the grid: +FLT_MAX) and classifies the thread's point.
__device__ __forceinline__ SfThread stage_and_classify(const float* __restrict__ f, const SfDims& D, float iso, float* s_f)
{
    int x0, y0, z0;
    brick_origin(D, x0, y0, z0);
    for (int s = threadIdx.x; s < SF_STAGE; s += SF_THREADS) {
        const int gx = x0 + s % SF_H, gy = y0 + s / SF_H % SF_H, gz = z0 + s / (SF_H * SF_H);
        const bool in = gx < D.nx && gy < D.ny && gz < D.nz;
        s_f[s] = in ? field_read(f[((size_t)gz * D.ny + gy) * D.nx + gx]) : FLT_MAX;
    }
    __syncthreads();
    SfThread T;
    const int tx = threadIdx.x % SF_B, ty = threadIdx.x / SF_B % SF_B, tz = threadIdx.x / (SF_B * SF_B);
    T.gx = x0 + tx; T.gy = y0 + ty; T.gz = z0 + tz;
    T.own = (tz * SF_H + ty) * SF_H + tx;
    T.point = T.gx < D.nx && T.gy < D.ny && T.gz < D.nz;
    const bool ex = T.gx + 1 < D.nx, ey = T.gy + 1 < D.ny, ez = T.gz + 1 < D.nz;
    T.cell = T.point && ex && ey && ez;
    T.inside = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) T.inside |= (unsigned)(s_f[T.own + (c & 1) + SF_H * (c >> 1 & 1) + SF_H * SF_H * (c >> 2)] < iso) << c;
    T.edges = 0;
#pragma unroll
    for (int d = 1; d < 8; ++d) {
        const bool exists = (!(d & 1) || ex) && (!(d & 2) || ey) && (!(d & 4) || ez);
        T.edges |= (unsigned)(T.point && exists && ((T.inside >> d ^ T.inside) & 1u)) << (d - 1);
    }
    return T;
}

// the sign case of tetrahedron t of a cell whose corners' inside bits are `inside`
template <int t>
__device__ __forceinline__ unsigned tet_mask(unsigned inside)
{
    return (inside & 1u) | (inside >> sc::tet_corner(t, 1) & 1u) << 1 | (inside >> sc::tet_corner(t, 2) & 1u) << 2 | (inside >> 7 & 1u) << 3;
}

__device__ __forceinline__ int cell_triangles(unsigned inside)
{
    const unsigned m[6] = {tet_mask<0>(inside), tet_mask<1>(inside), tet_mask<2>(inside), tet_mask<3>(inside), tet_mask<4>(inside), tet_mask<5>(inside)};
    int n = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int k = __builtin_popcount(m[t]); // 1 or 3 inside: one triangle; 2: two; 0 or 4: none
        n += k == 2 ? 2 : (k == 1 || k == 3 ? 1 : 0);
    }
    return n;
}

// Launch 1 of the count: a word per point (its first vertex's rank in the block | its edge flags << 16) and the block's two totals.
__global__ __launch_bounds__(SF_THREADS) void sf_count_kernel(const float* __restrict__ f, SfDims D, float iso, uint32_t* __restrict__ pinfo,
                                                              uint32_t* __restrict__ bverts, unsigned long long* __restrict__ btris)
{
    __shared__ float s_f[SF_STAGE];
    __shared__ int s_wave[SF_THREADS / 64];
    const SfThread T = stage_and_classify(f, D, iso, s_f);
    int nv, nt;
    const int rank = block_prefix<3>(__builtin_popcount(T.edges), s_wave, nv);
    block_prefix<4>(T.cell ? cell_triangles(T.inside) : 0, s_wave, nt);
    if (T.point) pinfo[((size_t)T.gz * D.ny + T.gy) * D.nx + T.gx] = (uint32_t)rank | T.edges << 16;
    if (threadIdx.x == 0) {
        bverts[blockIdx.x] = (uint32_t)nv;
        btris[blockIdx.x] = (unsigned long long)nt;
    }
}

// Launch 2 of the count, one block: exclusive scans of both block totals in place, the grand totals behind them and into counts[2].
__global__ __launch_bounds__(SF_SCAN) void sf_scan_kernel(uint32_t* __restrict__ bverts, unsigned long long* __restrict__ btris, int nblocks,
                                                          long long* __restrict__ counts)
{
    __shared__ unsigned long long s_v[SF_SCAN], s_t[SF_SCAN];
    const int per = (nblocks + SF_SCAN - 1) / SF_SCAN;
    const int b0 = min((int)threadIdx.x * per, nblocks), b1 = min(b0 + per, nblocks);
    unsigned long long lv = 0, lt = 0;
    for (int b = b0; b < b1; ++b) { lv += bverts[b]; lt += btris[b]; }
    s_v[threadIdx.x] = lv;
    s_t[threadIdx.x] = lt;
    __syncthreads();
    for (int d = 1; d < SF_SCAN; d <<= 1) { // Hillis-Steele inclusive scan
        const bool take = threadIdx.x >= (unsigned)d;
        const unsigned long long v = take ? s_v[threadIdx.x - d] : 0ull, t = take ? s_t[threadIdx.x - d] : 0ull;
        __syncthreads();
        s_v[threadIdx.x] += v;
        s_t[threadIdx.x] += t;
        __syncthreads();
    }
    unsigned long long rv = s_v[threadIdx.x] - lv, rt = s_t[threadIdx.x] - lt; // exclusive prefixes of this thread's chunk
    for (int b = b0; b < b1; ++b) {
        const unsigned long long cv = bverts[b], ct = btris[b];
        bverts[b] = (uint32_t)rv;
        btris[b] = rt;
        rv += cv;
        rt += ct;
    }
    if (threadIdx.x == SF_SCAN - 1) {
        bverts[nblocks] = (uint32_t)s_v[SF_SCAN - 1];
        btris[nblocks] = s_t[SF_SCAN - 1];
        counts[0] = (long long)s_v[SF_SCAN - 1];
        counts[1] = (long long)s_t[SF_SCAN - 1];
    }
}

// The triangles of tetrahedron t of the thread's cell: vertex numbers from the staged words of the cell's corners.
template <int t>
__device__ __forceinline__ void emit_tet(unsigned inside, int own, const int* s_vb, const uint32_t* s_em, long long& at, long long cap,
                                         int32_t* __restrict__ tris)
{
    constexpr uint64_t ED = sc::tet_edges(t);
    const uint32_t cw = SF_CASE[tet_mask<t>(inside)];
    const int n = (int)(cw & 3u);
    for (int i = 0; i < n; ++i) {
        int v[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e = (int)(cw >> (2 + 9 * i + 3 * j) & 7u);
            const int code = (int)(ED >> (6 * e) & 63u), ca = code & 7, d = code >> 3;
            const int at_c = own + (ca & 1) + SF_H * (ca >> 1 & 1) + SF_H * SF_H * (ca >> 2);
            v[j] = s_vb[at_c] + __builtin_popcount(s_em[at_c] & ((1u << (d - 1)) - 1u));
        }
        if (!sc::tet_positive(t)) { const int s = v[1]; v[1] = v[2]; v[2] = s; }
        if (at < cap) {
            tris[3 * at] = v[0];
            tris[3 * at + 1] = v[1];
            tris[3 * at + 2] = v[2];
        }
        ++at;
    }
}

__global__ __launch_bounds__(SF_THREADS) void sf_emit_kernel(const float* __restrict__ f, const float* __restrict__ rgb, SfAxes A, SfDims D, float iso,
                                                             const uint32_t* __restrict__ pinfo, const uint32_t* __restrict__ bverts,
                                                             const unsigned long long* __restrict__ btris, float* __restrict__ verts,
                                                             float* __restrict__ colors, int32_t* __restrict__ tris, long long cap_v, long long cap_t)
{
    __shared__ float s_f[SF_STAGE];
    __shared__ int s_vb[SF_STAGE];       // number of the first vertex of the point
    __shared__ uint32_t s_em[SF_STAGE];  // its edge flags
    __shared__ int s_wave[SF_THREADS / 64];
    int x0, y0, z0;
    brick_origin(D, x0, y0, z0);
    for (int s = threadIdx.x; s < SF_STAGE; s += SF_THREADS) {
        const int gx = x0 + s % SF_H, gy = y0 + s / SF_H % SF_H, gz = z0 + s / (SF_H * SF_H);
        int vb = 0;
        uint32_t em = 0;
        if (gx < D.nx && gy < D.ny && gz < D.nz) {
            const uint32_t w = pinfo[((size_t)gz * D.ny + gy) * D.nx + gx];
            vb = (int)(bverts[((gz / SF_B) * D.by + gy / SF_B) * D.bx + gx / SF_B] + (w & 0xffffu));
            em = w >> 16;
        }
        s_vb[s] = vb;
        s_em[s] = em;
    }
    const SfThread T = stage_and_classify(f, D, iso, s_f); // (its barrier also covers s_vb / s_em)

    // the vertices of the point's own active edges, a = the point itself (the lower linear index), b = a + direction
    if (T.edges) {
        const float pa[3] = {grid_coord(T.gx, A.o[0], A.s[0]), grid_coord(T.gy, A.o[1], A.s[1]), grid_coord(T.gz, A.o[2], A.s[2])};
        const float pn[3] = {grid_coord(T.gx + 1, A.o[0], A.s[0]), grid_coord(T.gy + 1, A.o[1], A.s[1]), grid_coord(T.gz + 1, A.o[2], A.s[2])};
        const float fa = s_f[T.own];
        const size_t ia = ((size_t)T.gz * D.ny + T.gy) * D.nx + T.gx;
        long long k = s_vb[T.own];
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            if (!(T.edges >> (d - 1) & 1u)) continue;
            const float fb = s_f[T.own + (d & 1) + SF_H * (d >> 1 & 1) + SF_H * SF_H * (d >> 2)];
            float t = (iso - fa) / (fb - fa);
            t = fminf(fmaxf(t, 0.0f), 1.0f); // already there for finite operands; FLT_MAX ends can leave the quotient outside or NaN
            if (k < cap_v) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float pb = (d >> j & 1) ? pn[j] : pa[j];
                    const float p = pa[j] + t * (pb - pa[j]);
                    verts[3 * k + j] = fminf(fmaxf(p, pa[j]), pb); // on the edge whatever the last bit of the sum did (spacings are positive)
                }
                if (colors) {
                    const size_t ib = ia + (d & 1) + (size_t)D.nx * (d >> 1 & 1) + (size_t)D.nx * D.ny * (d >> 2);
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float ca = rgb[3 * ia + j], cb = rgb[3 * ib + j];
                        colors[3 * k + j] = ca + t * (cb - ca);
                    }
                }
            }
            ++k;
        }
    }

    // the triangles of the point's cell
    int nt;
    const int rank = block_prefix<4>(T.cell ? cell_triangles(T.inside) : 0, s_wave, nt);
    if (!T.cell) return;
    long long at = (long long)btris[blockIdx.x] + rank;
    emit_tet<0>(T.inside, T.own, s_vb, s_em, at, cap_t, tris);
    emit_tet<1>(T.inside, T.own, s_vb, s_em, at, cap_t, tris);
    emit_tet<2>(T.inside, T.own, s_vb, s_em, at, cap_t, tris);
    emit_tet<3>(T.inside, T.own, s_vb, s_em, at, cap_t, tris);
    emit_tet<4>(T.inside, T.own, s_vb, s_em, at, cap_t, tris);
    emit_tet<5>(T.inside, T.own, s_vb, s_em, at, cap_t, tris);
}

__global__ __launch_bounds__(PT_BLOCK) void grid_points_kernel(SfAxes A, int nx, int ny, int z0, long long n, float* __restrict__ pts)
{
    const long long i = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % nx), y = (int)(i / nx % ny), z = z0 + (int)(i / ((long long)nx * ny));
    pts[3 * i] = grid_coord(x, A.o[0], A.s[0]);
    pts[3 * i + 1] = grid_coord(y, A.o[1], A.s[1]);
    pts[3 * i + 2] = grid_coord(z, A.o[2], A.s[2]);
}

__global__ __launch_bounds__(PT_BLOCK) void field_values_kernel(const float* __restrict__ rgba, const float* __restrict__ mesh_sdf, long long n,
                                                                float* __restrict__ f, float* __restrict__ rgb)
{
    const long long i = (long long)blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    f[i] = rgba[5 * i] + mesh_sdf[i];
    if (rgb) {
        rgb[3 * i] = rgba[5 * i + 2];
        rgb[3 * i + 1] = rgba[5 * i + 3];
        rgb[3 * i + 2] = rgba[5 * i + 4];
    }
}

const char* dims_error(int nx, int ny, int nz)
{
    if (nx < 2 || ny < 2 || nz < 2) return "every dimension must be at least 2";
    if (7LL * nx * ny >= 0x80000000LL || 7LL * nx * ny * nz >= 0x80000000LL) return "7 nx ny nz must stay below 2^31";
    return nullptr;
}

SfDims dims_of(int nx, int ny, int nz) { return {nx, ny, nz, (nx + SF_B - 1) / SF_B, (ny + SF_B - 1) / SF_B, (nz + SF_B - 1) / SF_B}; }

SfAxes axes_of(const char* who, const float* origin, const float* spacing)
{
    SfAxes A;
    for (int j = 0; j < 3; ++j) {
        A.o[j] = origin[j];
        A.s[j] = spacing[j];
        if (!std::isfinite(A.o[j]) || !std::isfinite(A.s[j]) || !(A.s[j] > 0.0f))
            throw_error("%s: origin must be finite and spacing finite and positive (axis %d: origin %g, spacing %g)", who, j, (double)A.o[j], (double)A.s[j]);
    }
    return A;
}

int64_t align16(int64_t n) { return (n + 15) / 16 * 16; }

struct SfScratch {
    uint32_t* pinfo;
    unsigned long long* btris;
    uint32_t* bverts;
};

SfScratch carve(void* scratch, const SfDims& D)
{
    const int64_t n = (int64_t)D.nx * D.ny * D.nz, nb = (int64_t)D.bx * D.by * D.bz;
    char* p = static_cast<char*>(scratch);
    SfScratch S;
    S.pinfo = reinterpret_cast<uint32_t*>(p);
    S.btris = reinterpret_cast<unsigned long long*>(p + align16(4 * n));
    S.bverts = reinterpret_cast<uint32_t*>(p + align16(4 * n) + align16(8 * (nb + 1)));
    return S;
}

} // namespace

extern "C" int vanerf_grid_points(const float* origin, const float* spacing, int nx, int ny, int nz, int z0, int nz_out, float* pts, void* stream)
{
    return guarded([&] {
        if (!origin || !spacing) throw_error("vanerf_grid_points: null argument");
        if (const char* e = dims_error(nx, ny, nz)) throw_error("vanerf_grid_points: nx=%d ny=%d nz=%d: %s", nx, ny, nz, e);
        if (z0 < 0 || nz_out < 0 || (long long)z0 + nz_out > nz) throw_error("vanerf_grid_points: layers [%d, %d + %d) outside [0, %d)", z0, z0, nz_out, nz);
        const SfAxes A = axes_of("vanerf_grid_points", origin, spacing);
        const long long n = (long long)nx * ny * nz_out;
        if (n == 0) return;
        if (!pts) throw_error("vanerf_grid_points: null argument");
        hipLaunchKernelGGL(grid_points_kernel, dim3((unsigned)((n + PT_BLOCK - 1) / PT_BLOCK)), dim3(PT_BLOCK), 0, (hipStream_t)stream, A, nx, ny, z0, n, pts);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_field_values(const float* rgba, const float* mesh_sdf, int64_t n, float* f, float* rgb, void* stream)
{
    return guarded([&] {
        if (n < 0 || n >= 0x7fffffffLL) throw_error("vanerf_field_values: n = %lld outside [0, 2^31 - 1)", (long long)n);
        if (n == 0) return;
        if (!rgba || !mesh_sdf || !f) throw_error("vanerf_field_values: null argument");
        hipLaunchKernelGGL(field_values_kernel, dim3((unsigned)((n + PT_BLOCK - 1) / PT_BLOCK)), dim3(PT_BLOCK), 0, (hipStream_t)stream, rgba, mesh_sdf,
                           (long long)n, f, rgb);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int64_t vanerf_surface_scratch(int nx, int ny, int nz)
{
    if (dims_error(nx, ny, nz)) return 0;
    const SfDims D = dims_of(nx, ny, nz);
    const int64_t n = (int64_t)nx * ny * nz, nb = (int64_t)D.bx * D.by * D.bz;
    return align16(4 * n) + align16(8 * (nb + 1)) + align16(4 * (nb + 1));
}

extern "C" int vanerf_surface_count(const float* f, int nx, int ny, int nz, float iso, void* scratch, int64_t scratch_bytes, int64_t* counts,
                                    void* stream)
{
    return guarded([&] {
        if (const char* e = dims_error(nx, ny, nz)) throw_error("vanerf_surface_count: nx=%d ny=%d nz=%d: %s", nx, ny, nz, e);
        if (!f || !scratch || !counts) throw_error("vanerf_surface_count: null argument");
        if (!std::isfinite(iso)) throw_error("vanerf_surface_count: iso must be finite");
        if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0 || reinterpret_cast<uintptr_t>(counts) % 8 != 0 || reinterpret_cast<uintptr_t>(f) % 4 != 0)
            throw_error("vanerf_surface_count: scratch must be 16-byte, counts 8-byte and f 4-byte aligned");
        const int64_t need = vanerf_surface_scratch(nx, ny, nz);
        if (scratch_bytes < need) throw_error("vanerf_surface_count: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
        const SfDims D = dims_of(nx, ny, nz);
        const SfScratch S = carve(scratch, D);
        const int nb = D.bx * D.by * D.bz;
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(sf_count_kernel, dim3((unsigned)nb), dim3(SF_THREADS), 0, st, f, D, iso, S.pinfo, S.bverts, S.btris);
        hipLaunchKernelGGL(sf_scan_kernel, dim3(1), dim3(SF_SCAN), 0, st, S.bverts, S.btris, nb, reinterpret_cast<long long*>(counts));
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_surface_emit(const float* f, const float* rgb, const float* origin, const float* spacing, int nx, int ny, int nz, float iso,
                                   const void* scratch, int64_t scratch_bytes, int64_t n_verts, int64_t n_tris, float* verts, float* colors,
                                   int32_t* tris, int64_t cap_verts, int64_t cap_tris, void* stream)
{
    return guarded([&] {
        if (const char* e = dims_error(nx, ny, nz)) throw_error("vanerf_surface_emit: nx=%d ny=%d nz=%d: %s", nx, ny, nz, e);
        if (!origin || !spacing) throw_error("vanerf_surface_emit: null argument");
        const SfAxes A = axes_of("vanerf_surface_emit", origin, spacing);
        if (!std::isfinite(iso)) throw_error("vanerf_surface_emit: iso must be finite");
        if (n_verts < 0 || n_tris < 0 || cap_verts < 0 || cap_tris < 0) throw_error("vanerf_surface_emit: negative count or capacity");
        if (cap_verts < n_verts || cap_tris < n_tris)
            throw_error("vanerf_surface_emit: capacity of %lld vertices and %lld triangles, %lld and %lld counted", (long long)cap_verts,
                        (long long)cap_tris, (long long)n_verts, (long long)n_tris);
        if (n_verts == 0 && n_tris == 0) return;
        if (!f || !scratch || !verts || !tris) throw_error("vanerf_surface_emit: null argument");
        if (colors && !rgb) throw_error("vanerf_surface_emit: colors without rgb");
        if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0) throw_error("vanerf_surface_emit: scratch must be 16-byte aligned");
        const int64_t need = vanerf_surface_scratch(nx, ny, nz);
        if (scratch_bytes < need) throw_error("vanerf_surface_emit: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
        const SfDims D = dims_of(nx, ny, nz);
        const SfScratch S = carve(const_cast<void*>(scratch), D);
        hipLaunchKernelGGL(sf_emit_kernel, dim3((unsigned)(D.bx * D.by * D.bz)), dim3(SF_THREADS), 0, (hipStream_t)stream, f, rgb, A, D, iso,
                           (const uint32_t*)S.pinfo, (const uint32_t*)S.bverts, (const unsigned long long*)S.btris, verts, colors, tris,
                           (long long)cap_verts, (long long)cap_tris);
        HIP_CHECK(hipGetLastError());
    });
}
