// mesh_accel_query.hip -- accelerated cal_vis_sdf_batch and knn_points (K=1): identical results to mesh_query_kernel and knn1_kernel
// (mesh_kernels.hip; the same per-triangle arithmetic, mesh_device.h), but
//   * closest face: triangles are Morton-sorted into clusters of CL with an AABB per cluster and a bounding sphere
//     per triangle; a cluster / triangle is skipped only when its distance lower bound exceeds the best distance so
//     far by a safety margin (1e-4 relative: far above fp32 rounding), so the exact minimum and every tie survive;
//     ties resolve to the lowest ORIGINAL face index, as the brute-force scan does;
//   * inside test: a G x G grid over the mesh's (y,z) extent lists the triangles whose (y,z) bounding box touches each
//     cell; the +x ray of a point can only cross triangles of its own cell.
// The structure is built per source frame by vanerf_mesh_accel_build (mesh_accel_build.hip).  The item order of the ordered entry
// (vanerf_mesh_tile_order) is at the end of this file.
#include "mesh_accel.h"
#include "mesh_device.h"

using namespace vanerf;

namespace {

constexpr int MA_BLOCK = 1024; // one block per CU: 16 waves share the LDS copy of the vertex / box tables (53 KB for the two-hand mesh)
// tile searches (below): clusters a wave's candidate list can hold, and the 64-candidate rounds that makes
constexpr int TL_LIST = 160; // measured on the benchmark view with the work queue: 64 -> 2.34 ms, 128 -> 2.00, 160 -> 1.93, 192 -> 1.95, 256 -> 2.16
constexpr int TL_IT = TL_LIST * CL / 64;
constexpr int ND_MAX = 2; // consecutive depths of a pixel tile a wave takes at once (template parameter ND of the kernel): one tile search, ND per-lane evaluations
constexpr int TL_CAND = 40; // triangles (9 floats + original index, padded to 12) a wave's candidate table holds
static_assert(TL_LIST * CL % 64 == 0 && 64 % CL == 0 && MA_MAX_CLUSTERS <= 65536, "candidate lists hold 16-bit cluster ids in whole rounds of 64");

// Diagnostic build only (-DVANERF_MESH_PHASES): s_memtime deltas per phase, summed over waves (tools/perf_mesh.py --phases)
#ifdef VANERF_MESH_PHASES
__device__ unsigned long long g_ma_phase[16];
#define MPH(k) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ph[k] += t_ - tprev; tprev = t_; } while (0)
#define MPH_COUNT(cond, k, v) do { if (cond) ph[k] += (v); } while (0) // the event counters of slots 5-9 and 11-15
#else
#define MPH(k) do { } while (0)
#define MPH_COUNT(cond, k, v) do { } while (0)
#endif

// ---- Bounds of the searches: code that depends on a few values only.  Every kernel stage below that prunes does it through one of these.

// Disc lower bound (squared) of a triangle for point q.  A triangle lies in the plane through its centroid c (unit normal n), within r of c,
//      so with e = q - c, h = n.e:  d^2 >= h^2 + max(0, sqrt(|e|^2 - h^2) - r)^2.  For a sample far from the mesh, where
//      hundreds of triangles are nearly equidistant from q, this keeps the few it is roughly above -- the bounding-sphere
//      bound (|e| - r)^2 it replaces kept every triangle of a patch of radius ~sqrt(2 d r) (5x the exact evaluations).
//      Rounding: n and the dot products are off by <= 1e-6 |e|, the stored centres by <= a = 1e-6 x (largest
//      coordinate) -- the radii are padded by a by the builder -- so |h| is off by delta <= 1e-6 |e| + a and
//      h^2 by 2 |h| delta <= kappa |e|^2 + w with w = 1e5 a^2 (tnorm.w); h^2 is lowered by that much where it adds
//      to the bound and raised where it is subtracted.
// sp = (centroid, radius), tn = (unit normal, w): the triangle's records of A.sphere and A.tnorm.
__device__ __forceinline__ float disc_lb2(const float4 sp, const float4 tn, f3 q)
{
    constexpr float kappa = 3e-5f;
    const float ex = q.x - sp.x, ey = q.y - sp.y, ez = q.z - sp.z;
    const float e2 = (ex * ex + ey * ey) + ez * ez;
    const float h = (tn.x * ex + tn.y * ey) + tn.z * ez;
    const float h2 = h * h;
    const float gr = fmaxf(sqrtf(fmaxf(e2 * (1.0f - kappa) - h2 - tn.w, 0.0f)) - sp.w, 0.0f);
    return fmaxf(h2 - kappa * e2 - tn.w, 0.0f) + gr * gr;
}

// Cylinder lower bound (squared) of a triangle cluster for a point at offset e from the cylinder's centre, L2 = |e|^2.  cd = (mean vertex,
// radius), cn = (axis = mean normal, half height): the cluster's two records of A.cdisc.
__device__ __forceinline__ float cyl_lb2(const float4 cd, const float4 cn, f3 e, float L2)
{
    const float h = (cn.x * e.x + cn.y * e.y) + cn.z * e.z;
    const float dh = fmaxf(fabsf(h) * (1.0f - 1e-5f) - cn.w, 0.0f), dl = fmaxf(sqrtf(fmaxf(L2 - h * h, 0.0f)) * (1.0f - 1e-5f) - cd.w, 0.0f);
    return (dh * dh + dl * dl) * (1.0f - 1e-5f);
}

// Bound on |u - ua| for every unit vector u from a point of the ball (m, R) to tc: e = tc - m, x = R / |e| (padded by the caller), ua the
// reference's unit vector.  |u - ua| <= |u_m - ua| + 1.05 x for x < 1/2 (chord <= angle <= 1.05 sine), and <= 2 always.
__device__ __forceinline__ float ball_du(f3 e, float x, f3 ua)
{
    float du = 2.0f;
    if (x < 0.5f) {
        const float inv = 1.0f / fmaxf(sqrtf(dot3(e, e)), 1e-20f);
        const float ex = e.x * inv - ua.x, ey = e.y * inv - ua.y, ez = e.z * inv - ua.z;
        du = sqrtf((ex * ex + ey * ey) + ez * ez) + 1.05f * x + 1e-5f;
    }
    return du;
}

struct Tri { f3 a, b, c; };
__device__ __forceinline__ Tri load_tri(const float* __restrict__ tri, int t)
{
    const float* r = tri + (size_t)t * 9;
    return Tri{{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, {r[6], r[7], r[8]}};
}

// one row of a wave's candidate table: the corners and the original face index, padded to twelve floats (read back as three float4)
__device__ __forceinline__ void write_cand_row(float* e, const Tri& T, int orig)
{
    e[0] = T.a.x; e[1] = T.a.y; e[2] = T.a.z; e[3] = T.b.x; e[4] = T.b.y; e[5] = T.b.z; e[6] = T.c.x; e[7] = T.c.y; e[8] = T.c.z;
    e[9] = __int_as_float(orig);
}

// The crossings of the +x ray from p among the records [k0, e) of the cells' lists.  `sides(a, b, c, i0, i1, i2, E0, E1, E2)` computes the
// three edge functions and says whether they put (p.y, p.z) on one side.
template <class Sides>
__device__ __forceinline__ int count_crossings(const float* __restrict__ cell_rec, int k0, int e, f3 p, Sides sides)
{
    int cnt = 0;
    for (int k = k0; k < e; ++k) {
        // one 48-byte record per list entry (vertex ids for the canonical edge orientation, then the corners: copies of F and V), so that
        // an entry costs one independent load instead of the chain face id -> vertex ids -> corners
        const float4 r0 = reinterpret_cast<const float4*>(cell_rec)[3 * k], r1 = reinterpret_cast<const float4*>(cell_rec)[3 * k + 1],
                     r2 = reinterpret_cast<const float4*>(cell_rec)[3 * k + 2];
        const int i0 = __float_as_int(r0.x), i1 = __float_as_int(r0.y), i2 = __float_as_int(r0.z);
        const f3 a = {r0.w, r1.x, r1.y}, b = {r1.z, r1.w, r2.x}, c3 = {r2.y, r2.z, r2.w};
        float E0, E1, E2;
        if (sides(a, b, c3, i0, i1, i2, E0, E1, E2) && crosses_beyond(E0, E1, E2, a, b, c3, p.x)) ++cnt;
    }
    return cnt;
}

// A wave takes 64 x ND points at a time.  Its work loop is a sequence of stages, each a lambda of the loop body whose comment says what it reads,
// what it leaves in the wave's LDS (my_list: cluster ids; s_dit: a distance per lane and round; s_cand: the candidate table) and what it returns.
// The state they share: pk[] (the points), tlo / thi / tc / slack / rho (the tile), vbk / vik (1-NN so far), bestk / bfk (closest face so far).
template <int ND> // 1 or ND_MAX: small launches take one depth per item (twice the items: a launch of a few thousand items is bound by the latency of single items)
__global__ __launch_bounds__(MA_BLOCK) void mesh_query_accel_kernel(const VanerfMeshAccel A, const float* __restrict__ V,
                                                                    const int32_t* __restrict__ F, const float* __restrict__ vert_vis,
                                                                    const float* __restrict__ P, long long n, float* __restrict__ sdf,
                                                                    uint8_t* __restrict__ vis, int32_t* __restrict__ face,
                                                                    int32_t* __restrict__ knn, int gnx, int gny, int gS,
                                                                    unsigned long long* __restrict__ queue,
                                                                    const int32_t* __restrict__ item_order)
{
    // dynamic LDS: [nvc*CL] sorted vertices (float4) | [nvc][6] vertex-cluster boxes | [nc][6] triangle-cluster boxes
    extern __shared__ float4 s_dyn[];
    __shared__ unsigned short s_list[MA_BLOCK / 64][TL_LIST]; // per-wave candidate lists of the tile searches
    __shared__ __attribute__((aligned(16))) float s_cand[MA_BLOCK / 64][TL_CAND][12];
    __shared__ float s_dit[MA_BLOCK / 64][TL_IT][64]; // per-wave, per-lane distances of the searches' rounds (registers are the scarce resource here)
    float4* s_vs = s_dyn;
    float* s_vbox = reinterpret_cast<float*>(s_vs + A.nvc * CL);
    float* s_box = s_vbox + A.nvc * 6;
    for (int k = threadIdx.x; k < A.nc * 6; k += MA_BLOCK) s_box[k] = A.cbox[k];
    for (int k = threadIdx.x; k < A.nvc * 6; k += MA_BLOCK) s_vbox[k] = A.vbox[k];
    for (int k = threadIdx.x; k < A.nvc * CL; k += MA_BLOCK) s_vs[k] = reinterpret_cast<const float4*>(A.vsort)[k];
    // (y,z) grid of the inside test: written on the device by vanerf_mesh_accel_build (uniform loads)
    const float grid_y0 = A.grid[0], grid_z0 = A.grid[1], grid_cy = A.grid[2], grid_cz = A.grid[3];
    const int grid_G = __float_as_int(A.grid[4]);
    __syncthreads();
    // Work mapping.  The pruning below is data dependent, so a wave runs the UNION of its lanes' candidate lists.  With the
    // ray-grid hint (gnx x gny rays, gS samples per ray, sample index = ray * gS + depth) a wave takes one depth of an 8 x 8
    // pixel tile: 64 points a few millimetres apart that prune almost identically.  Without the hint (gnx == 0) consecutive
    // lanes take consecutive samples (one whole ray per wave: its points span the bounding box, ~4x more work per wave).
    // With an item order on top of the hint (vanerf_mesh_tile_order: the tile's 64 x gS sample indices sorted by depth, 64 gS slots per tile)
    // depth k of a tile is the k-th 64-slot slab of its table instead: 64 points of one depth range wherever the rays put their k-th sample
    // (importance samples, rays with different clip ranges).  Nothing below locate() knows which grouping it works on: every point's answer
    // is exact, so any table that names every sample once gives the same bits.
    const int lane = threadIdx.x & 63;
    // the lane number as a value the compiler must take afresh: index and address arithmetic on it is then redone where it is used instead of
    // being hoisted out of the work loop into registers that stay occupied for the whole kernel (the kernel lives at the 128-register limit)
    auto lane_now = [&]() { int l = lane; asm volatile("" : "+v"(l)); return l; };
    // Work queue: a wave claims its next 64 points with one atomic.  The cost of a wave's search varies 10x with the tile's distance from
    // the mesh; a fixed assignment left 40 % of the wave slots idle behind the slowest waves (2.45 of 4 waves per SIMD on average).
    auto claim = [&]() {
        unsigned long long v = 0ull;
        if (lane == 0) v = atomicAdd(queue, 1ull);
        return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                           (unsigned)__builtin_amdgcn_readfirstlane((int)v));
    };
    const int ntx = (gnx + 7) >> 3, nty = (gny + 7) >> 3;
    const int gD = (gS + ND - 1) / ND; // depth groups per tile
    const long long nwork = gnx > 0 ? (long long)ntx * nty * gD : (n + 64 * ND - 1) / (64 * ND);
#ifdef VANERF_MESH_PHASES
    unsigned long long ph[16] = {}, tprev = __builtin_amdgcn_s_memtime();
#endif
    for (long long w = claim(); w < nwork; w = claim()) { // ---- stage 1: claim an item
        // ---- stage 2: locate and load the points.
        // every lane keeps a point (the searches below are wave-cooperative): a lane beyond the grid border / the end of the batch
        // repeats a neighbour's point and does not store
        // (the item's depth group and pixel tile: wave-uniform, divided out once; the host checks that the item count fits 32 bits)
        int item_d0 = 0, item_x0 = 0, item_y0 = 0, item_tile = 0;
        if (gnx > 0) {
            const unsigned wu = (unsigned)w, tile = wu / (unsigned)gD;
            item_tile = __builtin_amdgcn_readfirstlane((int)tile);
            item_d0 = __builtin_amdgcn_readfirstlane((int)(wu % (unsigned)gD) * ND);
            item_x0 = __builtin_amdgcn_readfirstlane((int)(tile % (unsigned)ntx) * 8);
            item_y0 = __builtin_amdgcn_readfirstlane((int)(tile / (unsigned)ntx) * 8);
        }
        // sample index of depth k of this item for this lane, and whether the lane stores it (recomputed where needed rather than kept)
        auto locate = [&](int k, bool& act) -> long long {
            long long i;
            if (gnx > 0 && item_order) {
                // slot `lane` of slab d of the tile's table.  A slot without a sample (-1: a ray beyond the grid border; anything outside
                // [0, n) is treated alike) repeats the first sample of its slab -- of the launch, if the slab names none -- and stores nothing.
                const int d = item_d0 + k;
                int idx = item_order[((long long)item_tile * gS + min(d, gS - 1)) * 64 + lane_now()];
                const bool named = (unsigned long long)(unsigned)idx < (unsigned long long)n;
                const unsigned long long m = __ballot(named);
                const int first = __builtin_amdgcn_readlane(idx, m ? __builtin_ctzll(m) : 0);
                act = named && d < gS;
                i = named ? idx : m ? first : 0;
            } else if (gnx > 0) {
                const int d = item_d0 + k;
                const int l = lane_now();
                const int rx = item_x0 + (l & 7), ry = item_y0 + (l >> 3);
                act = rx < gnx && ry < gny && d < gS;
                i = ((long long)min(ry, gny - 1) * gnx + min(rx, gnx - 1)) * gS + min(d, gS - 1);
            } else {
                i = (w * ND + k) * 64 + lane;
                act = i < n;
                i = act ? i : n - 1;
            }
            return i;
        };
        f3 pk[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            bool act;
            const long long i = locate(k, act);
            pk[k] = {P[3 * i], P[3 * i + 1], P[3 * i + 2]};
        }
        MPH(0); // point load
        // ---- stage 3: the tile's box T = [tlo, thi], its centre tc and the slack of the tile searches.
        // Both searches prune per WAVE first: the 64 points of a wave lie in a small box T, and a cluster whose box is farther from
        // T than the largest bound any lane holds cannot matter to any lane.  The lanes test 64 clusters at a time against T (one
        // cluster per lane, __ballot), and only the surviving clusters are then tested by every lane against its own point and
        // bound -- the flat per-lane loop over all boxes this replaces was 2/3 of the kernel's instructions.
        float tlo[3] = {pk[0].x, pk[0].y, pk[0].z}, thi[3] = {pk[0].x, pk[0].y, pk[0].z};
#pragma unroll
        for (int k = 1; k < ND; ++k) {
            tlo[0] = fminf(tlo[0], pk[k].x); tlo[1] = fminf(tlo[1], pk[k].y); tlo[2] = fminf(tlo[2], pk[k].z);
            thi[0] = fmaxf(thi[0], pk[k].x); thi[1] = fmaxf(thi[1], pk[k].y); thi[2] = fmaxf(thi[2], pk[k].z);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) { tlo[a] = wave_min_f(tlo[a]); thi[a] = wave_max_f(thi[a]); }
        auto tile_dist2 = [&](const float* b) { // box-to-box: <= box_dist2(q, b) for every q in T (same monotone fp32 expression)
            const float dx = fmaxf(fmaxf(b[0] - thi[0], tlo[0] - b[3]), 0.0f);
            const float dy = fmaxf(fmaxf(b[1] - thi[1], tlo[1] - b[4]), 0.0f);
            const float dz = fmaxf(fmaxf(b[2] - thi[2], tlo[2] - b[5]), 0.0f);
            return (dx * dx + dy * dy) + dz * dz;
        };
        // ---- Tile searches.  With the ray-grid hint the 64 points of a wave lie within a few millimetres of each other -- less than a
        //      triangle -- so the wave first answers the query for ONE point, the centre tc of its tile, with the lanes working on 64
        //      CANDIDATES at a time (clusters, then the triangles / vertices of the surviving clusters), and only then every lane evaluates,
        //      for its own point, the few candidates that can still matter.  Which ones can (rho = max |p - tc| over the wave, D = the
        //      minimum at tc, attained on t_D at the point q_D, u_t = the unit vector from t's closest point to tc, w = p - tc):
        //        (i)  distances are 1-Lipschitz:  d(p, t*) <= d(p, t_D) <= D + rho  and  d(tc, t*) <= d(p, t*) + rho, so the minimum t* of
        //             a lane has  d(tc, t*) - D <= 2 rho;
        //        (ii) the distance to a convex set is convex:  d(p, t) >= d(tc, t) + u_t.w,  while  d(p, t_D) <= |p - q_D| <=
        //             D + u_D.w + |w|^2 / (2 D);  so t can beat t_D at some p of the tile only if
        //             d(tc, t) - D <= |u_t - u_D| rho + rho^2 / (2 D).
        //      (ii) is what keeps tiles centimetres from the mesh cheap: there dozens of triangles lie within 2 rho of the minimum, but
        //      their u_t are nearly parallel.  `slack` adds 10 um on top of 2 rho and (ii) carries 20 um, two orders of magnitude above the
        //      fp32 rounding of a computed distance at these coordinates (~0.1 um), so every candidate whose COMPUTED distance could win or
        //      tie survives: the per-lane arg-min (ties to the lowest original index) is the exhaustive scan's, bit for bit.  A tile too
        //      large for the candidate tables (rays on the silhouette of the bounding box, samples decimetres from the mesh, launches
        //      without the hint) falls back to the per-lane search below.
        //      Measured and dropped: taking the seed cluster's best triangle as the reference of (ii) from the start, with a cylinder
        //      around each cluster as its lower bound (no search for D first): looser at every level -- 106 instead of 62 listed clusters,
        //      19 instead of 13 per-lane evaluations, 44 % instead of 71 % of the waves within the tables; 4.6 ms against 3.4.
        unsigned short* const my_list = s_list[threadIdx.x >> 6];
        const f3 tc = {0.5f * (tlo[0] + thi[0]), 0.5f * (tlo[1] + thi[1]), 0.5f * (tlo[2] + thi[2])};
        float far2 = 0.0f; // the largest |p - tc|^2 of the lane's points
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const float ex = pk[k].x - tc.x, ey = pk[k].y - tc.y, ez = pk[k].z - tc.z;
            far2 = fmaxf(far2, (ex * ex + ey * ey) + ez * ez);
        }
        const float slack = uni(2.0f * sqrtf(wave_max_f(far2)) * (1.0f + 1e-5f) + 1e-5f);
        const float rho = 0.5f * slack;
        const bool try_tile = gnx > 0 && slack < 0.05f; // (a NaN slack compares false)
        auto sq_plus = [&](float d2) { const float r = sqrtf(d2) + slack; return (r * r) * (1.0f + 1e-4f) + 1e-12f; }; // (i), squared
        // (i) and (ii) for a candidate at distance d from tc whose unit vector differs from u_R by du (R = the reference's distance)
        auto may_win = [&](float d, float R, float du, bool have_uR) {
            const float lim = (have_uR && R > 1e-4f) ? fminf(slack, du * rho * (1.0f + 1e-4f) + (rho * rho) / (2.0f * R) * (1.0f + 1e-4f) + 2e-5f) : slack;
            return d - R <= lim;
        };
        // ---- The wave-level steps that both searches are made of.
        auto mbcnt = [&](unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); };
        // Lists the clusters c of [0, ncl) with keep(c): the lanes test 64 at a time, and the kept ones are appended to my_list in ascending
        // order.  Returns how many there are; only the first TL_LIST are on the list (more: the caller gives up or lists again).  The caller
        // sees to it that the list's previous readers are done; the new list is visible to the wave on return.
        auto list_clusters = [&](int ncl, auto keep) {
            int ns = 0;
            for (int c0 = 0; c0 < ncl; c0 += 64) {
                const int cl_ = min(c0 + lane_now(), ncl - 1);
                const bool kept = c0 + lane < ncl && keep(cl_);
                const unsigned long long m = __ballot(kept);
                const int pos = ns + mbcnt(m);
                if (kept && pos < TL_LIST) my_list[pos] = (unsigned short)cl_;
                ns += __builtin_popcountll(m);
            }
            __builtin_amdgcn_wave_barrier();
            return ns;
        };
        // round `it` of a list: lane l looks at member (triangle or vertex slot) number 64 it + l of the listed clusters (the list stays in LDS;
        // lanes beyond the list read an unused entry), and keeps a distance for it in dit(it)
        auto listed = [&](int it) { const int l = lane_now(); return (int)my_list[it * (64 / CL) + l / CL] * CL + l % CL; };
        float* const dit0 = s_dit[threadIdx.x >> 6][0] + lane;
        auto dit = [&](int it) -> float& { return dit0[it * 64]; };
        // the member that attains d2 in the first round that holds it (the lowest lane of that round); false, and `member` untouched, if none does
        auto first_at = [&](int nt, float d2, int& member) {
            bool have = false;
#pragma nounroll
            for (int it = 0; it * 64 < nt && !have; ++it) {
                const unsigned long long m = __ballot(dit(it) == d2);
                if (m) { member = __builtin_amdgcn_readlane(listed(it), __builtin_ctzll(m)); have = true; }
            }
            return have;
        };
        // the cluster whose box is nearest to tc, the lowest index among equals; 0 for a NaN tile.  Reads `boxes` only.
        auto nearest_cluster = [&](const float* boxes, int ncl) {
            float smin = INFINITY;
            int cm = 0;
            for (int c = lane_now(); c < ncl; c += 64) {
                const float lb = box_dist2(tc, boxes + 6 * c);
                if (lb < smin) { smin = lb; cm = c; }
            }
            cm = wave_min_i(smin == wave_min_f(smin) ? cm : 0x7fffffff);
            return cm == 0x7fffffff ? 0 : cm;
        };
        // Per-lane search for point p, when the tile search does not apply: every lane prunes against its own point and bound.  `eval(c)`
        // evaluates cluster c for p and `bound()` is the lane's squared bound so far.  The seed first, so that every lane holds a bound close
        // to its answer; then the other clusters 64 at a time against T with the wave's largest bound, the survivors by every lane against
        // its own.  Touches no LDS table of the wave.  `faces`: the diagnostic build counts the face search's clusters.
        auto lane_search = [&](const f3& p, const float* boxes, int ncl, int seed, auto bound, auto eval, bool faces) {
            eval(seed);
            const float cap = wave_max_f(bound()) * (1.0f + 1e-4f) + 1e-12f;
            for (int c0 = 0; c0 < ncl; c0 += 64) {
                const int cl_ = c0 + lane;
                unsigned long long m = __ballot(cl_ < ncl && cl_ != seed && tile_dist2(boxes + 6 * min(cl_, ncl - 1)) <= cap);
                while (m) {
                    const int c = c0 + __builtin_ctzll(m);
                    m &= m - 1;
                    MPH_COUNT(faces && lane == 0, 5, 1); // clusters surviving the wave-level test
                    if (box_dist2(p, boxes + 6 * c) > bound() * (1.0f + 1e-4f) + 1e-12f) continue;
                    MPH_COUNT(faces && __builtin_ctzll(__ballot(1)) == lane, 6, 1); // ... whose members some lane looks at
                    eval(c);
                }
            }
        };

        // ---- stage 4: 1-NN vertex (knn_points K=1, src/networks.py:28): clusters of CL Morton-sorted vertices; squared distance
        //      ((dx*dx + dy*dy) + dz*dz), first minimum in ORIGINAL vertex order (oracle/mesh_oracle.c:knn1).  Leaves vbk / vik.
        float vbk[ND];
        int vik[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) { vbk[k] = INFINITY; vik[k] = 0x7fffffff; }
        auto vert_dist2 = [&](f3 q, const float4 v) { const float dx = q.x - v.x, dy = q.y - v.y, dz = q.z - v.z; return (dx * dx + dy * dy) + dz * dz; };
        // The list of a tile decimetres from the mesh, where every vertex cluster of the near side is within 2 rho of the minimum.  As for the
        // faces below: the exact minimum at tc first (all vertices, from LDS), then only the clusters that can hold a vertex passing (ii) -- a
        // vertex of cluster c lies in the ball around its box, so its unit vector differs from the box centre's by at most 1.05 R_c / |tc - m_c|.
        // Leaves the list in my_list and returns its length; -1 if the tile has no usable reference (NaN, or on a vertex).
        auto knn_list_far = [&]() -> int {
            float b = INFINITY;
            int sb = 0;
            for (int j = lane_now(); j < A.nvc * CL; j += 64) {
                const float d = vert_dist2(tc, s_vs[j]);
                if (d < b) { b = d; sb = j; }
            }
            const float D2a = wave_min_f(b), Da = sqrtf(D2a);
            const unsigned long long mD = __ballot(b == D2a);
            if (!mD || !(Da > 1e-4f)) return -1;
            const float4 va = s_vs[__builtin_amdgcn_readlane(sb, __builtin_ctzll(mD))];
            const f3 ua = {(tc.x - va.x) / Da, (tc.y - va.y) / Da, (tc.z - va.z) / Da};
            __builtin_amdgcn_wave_barrier();
            return list_clusters(A.nvc, [&](int cl_) {
                const float* bx = s_vbox + 6 * cl_;
                const f3 e = {tc.x - 0.5f * (bx[0] + bx[3]), tc.y - 0.5f * (bx[1] + bx[4]), tc.z - 0.5f * (bx[2] + bx[5])};
                const float hx = bx[3] - bx[0], hy = bx[4] - bx[1], hz = bx[5] - bx[2];
                const float x = (0.5f * sqrtf((hx * hx + hy * hy) + hz * hz) * (1.0f + 1e-5f) + 1e-7f) / fmaxf(sqrtf(dot3(e, e)), 1e-20f);
                return may_win(sqrtf(box_dist2(tc, bx)), Da, ball_du(e, x, ua), true);
            });
        };
        // Tile search from the vertex cluster cm nearest to tc.  Uses my_list and s_dit; false if the tile does not fit the list (vbk / vik
        // untouched), else vbk / vik hold every lane's exact answer.
        auto knn_tile = [&](int cm) -> bool {
            float U = INFINITY;
            if (lane < CL) U = vert_dist2(tc, s_vs[cm * CL + lane]);
            U = wave_min_f(U);
            const float thr = sq_plus(U);
            int ns = list_clusters(A.nvc, [&](int cl_) { return box_dist2(tc, s_vbox + 6 * cl_) <= thr; });
            if (ns > TL_LIST) ns = knn_list_far();
            if (ns < 0 || ns > TL_LIST) return false;
            const int nt = ns * CL;
            // (the rounds are run-time loops: their distances live in LDS, not in register arrays, and unrolled eight-fold they made the kernel
            //  107 KB of code for a 64 KB instruction cache shared by two CUs)
#pragma nounroll
            for (int it = 0; it * 64 < nt; ++it) {
                dit(it) = INFINITY;
                const int j = it * 64 + lane;
                if (j < nt) dit(it) = vert_dist2(tc, s_vs[listed(it)]);
                U = fminf(U, dit(it));
            }
            const float D2 = uni(wave_min_f(U)), Tf = sq_plus(D2), D = sqrtf(D2);
            // reference: a vertex that attains the minimum at tc (always found: the seed cluster is on the list; if it ever were not, (i) alone decides)
            int slotD = 0;
            const bool have = first_at(nt, D2, slotD);
            const float4 vD = s_vs[slotD];
            const float invD = D > 1e-4f ? 1.0f / D : 0.0f;
            const f3 uD = {uni((tc.x - vD.x) * invD), uni((tc.y - vD.y) * invD), uni((tc.z - vD.z) * invD)};
#pragma nounroll
            for (int it = 0; it * 64 < nt; ++it) {
                bool cand = dit(it) <= Tf;
                if (cand) {
                    const float4 v = s_vs[listed(it)];
                    const float d = sqrtf(dit(it)), inv = 1.0f / fmaxf(d, 1e-20f);
                    const float ex = (tc.x - v.x) * inv - uD.x, ey = (tc.y - v.y) * inv - uD.y, ez = (tc.z - v.z) * inv - uD.z;
                    cand = may_win(d, D, sqrtf((ex * ex + ey * ey) + ez * ez), have);
                }
                unsigned long long m = __ballot(cand);
                const int sl = listed(it);
                while (m) { // every lane evaluates the candidate for its own points
                    const int src = __builtin_ctzll(m);
                    m &= m - 1;
                    const float4 v = s_vs[__builtin_amdgcn_readlane(sl, src)];
                    const int oi = __float_as_int(v.w);
#pragma unroll
                    for (int k = 0; k < ND; ++k) {
                        const float d = vert_dist2(pk[k], v);
                        if (d < vbk[k] || (d == vbk[k] && oi < vik[k])) { vbk[k] = d; vik[k] = oi; }
                    }
                }
            }
            return true;
        };
        const int cm = nearest_cluster(s_vbox, A.nvc);
        if (!(try_tile && knn_tile(cm))) {
#pragma unroll
            for (int k = 0; k < ND; ++k) {
                const f3 p = pk[k];
                float vb = INFINITY;
                int vi = 0x7fffffff;
                lane_search(p, s_vbox, A.nvc, cm, [&]() { return vb; }, [&](int c) {
                    for (int j = 0; j < CL; ++j) {
                        const float4 v = s_vs[c * CL + j];
                        const float d = vert_dist2(p, v);
                        const int oi = __float_as_int(v.w);
                        if (d < vb || (d == vb && oi < vi)) { vb = d; vi = oi; }
                    }
                }, false);
                vbk[k] = vb;
                vik[k] = vi;
            }
        }
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            if (vik[k] == 0x7fffffff) vik[k] = 0; // a NaN point compares false with everything: index 0, like the exhaustive scan
            bool act;
            const long long i = locate(k, act);
            if (knn && act) knn[i] = vik[k];
        }
        MPH(1); // 1-NN

        // ---- stage 5: closest face.  The nearest vertex belongs to some triangle, so its distance bounds the closest-face distance from
        //      above; a cluster / triangle whose LOWER bound (disc_lb2, cyl_lb2, the cluster's box) exceeds min(best, that bound) by the
        //      safety margin cannot hold the minimum or a tie.  Leaves bestk / bfk.
        float bestk[ND];
        int bfk[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) { bestk[k] = INFINITY; bfk[k] = 0x7fffffff; }
        auto tri_dist2 = [&](f3 q, int t) { const Tri T = load_tri(A.tri, t); return point_tri_dist2(q, T.a, T.b, T.c); };
        auto sphere_of = [&](int t) { return reinterpret_cast<const float4*>(A.sphere)[t]; };
        auto tnorm_of = [&](int t) { return reinterpret_cast<const float4*>(A.tnorm)[t]; };
        // lower bound (squared) of cluster cl_ at tc: the axis-aligned box (LDS) and the cylinder around the cluster (axis = mean normal through
        // the mean vertex; global table, one cluster per lane); x = R_c / |tc - m_c| of the ball around the cylinder; returns e = tc - m_c
        auto cluster_lb2 = [&](int cl_, float& lb2, float& x) {
            const float4 cd = reinterpret_cast<const float4*>(A.cdisc)[2 * cl_], cn = reinterpret_cast<const float4*>(A.cdisc)[2 * cl_ + 1];
            const f3 e = {tc.x - cd.x, tc.y - cd.y, tc.z - cd.z};
            const float L2 = dot3(e, e);
            lb2 = fmaxf(box_dist2(tc, s_box + 6 * cl_), cyl_lb2(cd, cn, e, L2));
            x = sqrtf(cd.w * cd.w + cn.w * cn.w) * (1.0f + 1e-5f) / fmaxf(sqrtf(L2), 1e-20f);
            return e;
        };
        // The list of a tile decimetres from the mesh: hundreds of clusters lie within 2 rho of the seed's distance U.  Two stages instead.
        // 1. the exact minimum D at tc: only clusters within the seed's distance U itself can hold it (a short list);
        // 2. the clusters that can hold a triangle passing (ii): every closest point of cluster c lies in the ball (m_c, R_c) around
        //    its cylinder, so  |u_t - u_D| <= |u_m - u_D| + 1.05 R_c / |tc - m_c|  (R_c < |tc - m_c| / 2; chord <= angle <= 1.05 sine),
        //    and d(tc, t) >= the cluster's lower bound: c matters only if  bound_c - D  passes may_win with that difference.
        // Leaves the list of stage 2 in my_list and returns its length, with thr_eval = the threshold (squared) that a listed triangle's
        // bound at tc has to meet; -1 if the tile has no usable reference (NaN; a tile this close to the mesh does not overflow the list).
        auto face_list_far = [&](int cseed, float U, float& thr_eval) -> int {
            const float thr1 = U * (1.0f + 1e-4f) + 1e-12f;
            __builtin_amdgcn_wave_barrier(); // (the first listing's writers are done with the list)
            const int n1 = list_clusters(A.nc, [&](int cl_) { float lb2, x; cluster_lb2(cl_, lb2, x); return lb2 <= thr1; });
            float b1 = INFINITY;
            int t1 = cseed * CL;
            if (lane < CL) { b1 = tri_dist2(tc, cseed * CL + lane); t1 = cseed * CL + lane; }
            if (n1 <= TL_LIST) {
                for (int j = lane_now(); j < n1 * CL; j += 64) {
                    const int t = (int)my_list[j / CL] * CL + j % CL;
                    if (disc_lb2(sphere_of(t), tnorm_of(t), tc) <= thr1) {
                        const float d = tri_dist2(tc, t);
                        if (d < b1) { b1 = d; t1 = t; }
                    }
                }
            } else { // (a flat part of the mesh faces the tile: hundreds of clusters are as near as the seed) every triangle, 64 at a time
                float bw = thr1;
                for (int t0 = 0; t0 < A.nfp; t0 += 64) {
                    const int t = min(t0 + lane, A.nfp - 1);
                    if (disc_lb2(sphere_of(t), tnorm_of(t), tc) <= bw) {
                        const float d = tri_dist2(tc, t);
                        if (d < b1) { b1 = d; t1 = t; }
                    }
                    bw = fminf(bw, wave_min_f(b1) * (1.0f + 1e-4f) + 1e-12f);
                }
            }
            const float D2a = wave_min_f(b1), Da = sqrtf(D2a);
            const unsigned long long mD = __ballot(b1 == D2a);
            if (!mD || !(Da > 1e-4f)) return -1;
            f3 qa;
            { const Tri T = load_tri(A.tri, __builtin_amdgcn_readlane(t1, __builtin_ctzll(mD))); point_tri_dist2_q(tc, T.a, T.b, T.c, qa); }
            const f3 ua = {(tc.x - qa.x) / Da, (tc.y - qa.y) / Da, (tc.z - qa.z) / Da};
            __builtin_amdgcn_wave_barrier(); // (stage 1's readers are done with the list)
            thr_eval = sq_plus(D2a);
            return list_clusters(A.nc, [&](int cl_) {
                float lb2, x;
                const f3 e = cluster_lb2(cl_, lb2, x);
                return may_win(sqrtf(lb2), Da, ball_du(e, x, ua), true);
            });
        };
        // Distances at tc of the nt listed triangles into s_dit: first the disc bounds of all rounds (their loads are independent and overlap),
        // then the exact distances of the triangles whose bound is within thr_eval; INFINITY for the others.  Returns min(U, the lane's distances).
        auto face_dist_at_tc = [&](int nt, float thr_eval, float U) {
#pragma nounroll
            for (int it = 0; it * 64 < nt; ++it) {
                dit(it) = INFINITY;
                const int j = it * 64 + lane;
                if (j < nt) {
                    const int t = listed(it);
                    dit(it) = disc_lb2(sphere_of(t), tnorm_of(t), tc) <= thr_eval ? 0.0f : INFINITY; // 0 = "evaluate me"
                }
            }
#pragma nounroll
            for (int it = 0; it * 64 < nt; ++it) {
                if (dit(it) == 0.0f) dit(it) = tri_dist2(tc, listed(it));
                U = fminf(U, dit(it));
            }
            return U;
        };
        // The candidates among the listed triangles, from s_dit: those that pass (i) get a second look (their closest point, for (ii)); those
        // that pass both are candidates.  Bit `it` of cbits: this lane's triangle of round `it` is one.  The first TL_CAND of them go to the
        // wave's candidate table s_cand.  Returns their number K <= TL_LIST * CL.  (A tile on the surface: every triangle within 2 rho is a
        // candidate; the per-lane search prunes those by each lane's own bound.)
        auto face_candidates = [&](int nt, float Tf, float D, f3 uD, bool have, unsigned& cbits) {
            int K = 0;
#pragma nounroll
            for (int it = 0; it * 64 < nt; ++it) {
                if (__ballot(dit(it) <= Tf)) {
                    bool cand = dit(it) <= Tf;
                    Tri T = {};
                    if (cand) {
                        T = load_tri(A.tri, listed(it));
                        f3 qt;
                        point_tri_dist2_q(tc, T.a, T.b, T.c, qt);
                        const float d = sqrtf(dit(it)), inv = 1.0f / fmaxf(d, 1e-20f);
                        const float ex = (tc.x - qt.x) * inv - uD.x, ey = (tc.y - qt.y) * inv - uD.y, ez = (tc.z - qt.z) * inv - uD.z;
                        cand = may_win(d, D, sqrtf((ex * ex + ey * ey) + ez * ez), have);
                    }
                    const unsigned long long m = __ballot(cand);
                    cbits |= cand ? 1u << it : 0u;
                    const int pos = K + mbcnt(m);
                    if (cand && pos < TL_CAND) write_cand_row(s_cand[threadIdx.x >> 6][pos], T, A.orig[listed(it)]);
                    K += __builtin_popcountll(m);
                }
            }
            return K;
        };
        // candidates [base, base + TL_CAND) of cbits into the candidate table, once its previous readers are done
        auto face_refill = [&](int nt, unsigned cbits, int base) {
            __builtin_amdgcn_wave_barrier(); // the previous batch's readers are done
            int k0 = 0;
#pragma nounroll
            for (int it = 0; it * 64 < nt; ++it) {
                const unsigned long long m = __ballot((cbits >> it) & 1u);
                if (m) {
                    const int pos = k0 + mbcnt(m) - base;
                    if (((m >> lane) & 1ull) && pos >= 0 && pos < TL_CAND) {
                        const int t = listed(it);
                        write_cand_row(s_cand[threadIdx.x >> 6][pos], load_tri(A.tri, t), A.orig[t]);
                    }
                    k0 += __builtin_popcountll(m);
                }
            }
        };
        // every lane evaluates the first kn rows of the candidate table for its own points, into bestk / bfk
        auto face_eval_table = [&](int kn) {
            const float* const ctab = s_cand[threadIdx.x >> 6][0];
#pragma unroll
            for (int q = 0; q < ND; ++q) { // one point after the other: the registers of one exact distance at a time
                __builtin_amdgcn_sched_barrier(0);
                const f3 p = pk[q];
                float best = bestk[q];
                int bf = bfk[q];
                for (int k = 0; k < kn; ++k) {
                    const float4 e0 = reinterpret_cast<const float4*>(ctab + k * 12)[0], e1 = reinterpret_cast<const float4*>(ctab + k * 12)[1],
                                 e2 = reinterpret_cast<const float4*>(ctab + k * 12)[2];
                    const f3 a = {e0.x, e0.y, e0.z}, b = {e0.w, e1.x, e1.y}, c3 = {e1.z, e1.w, e2.x};
                    const float d = point_tri_dist2(p, a, b, c3);
                    const int of = __float_as_int(e2.y);
                    if (d < best || (d == best && of < bf)) { best = d; bf = of; }
                }
                bestk[q] = best;
                bfk[q] = bf;
            }
        };
        // Tile search from the triangle cluster cseed nearest to tc.  Uses my_list, s_dit and s_cand; false if the tile does not fit the list
        // (bestk / bfk untouched), else bestk / bfk hold every lane's exact answer.
        auto face_tile = [&](int cseed) -> bool {
            float U = INFINITY;
            if (lane < CL) U = tri_dist2(tc, cseed * CL + lane);
            U = wave_min_f(U);
            const float thr = sq_plus(U);
            // clusters within thr of tc by BOTH lower bounds: the box and the cylinder.  For a tile centimetres from the mesh the box alone is too
            // loose -- a corner of it sticks out towards the tile by up to half its diagonal -- and lists every cluster of the near side.
            int ns = list_clusters(A.nc, [&](int cl_) {
                if (!(box_dist2(tc, s_box + 6 * cl_) <= thr)) return false;
                const float4 cd = reinterpret_cast<const float4*>(A.cdisc)[2 * cl_], cn = reinterpret_cast<const float4*>(A.cdisc)[2 * cl_ + 1];
                const f3 e = {tc.x - cd.x, tc.y - cd.y, tc.z - cd.z};
                return cyl_lb2(cd, cn, e, dot3(e, e)) <= thr;
            });
            float thr_eval = thr;
            if (ns > TL_LIST) ns = face_list_far(cseed, U, thr_eval);
            if (ns < 0) return false;
            MPH_COUNT(lane == 0 && ns > TL_LIST, 14, 1); // list overflow
            if (ns > TL_LIST) return false;
            MPH_COUNT(lane == 0, 12, ns); // clusters on the list
            const int nt = ns * CL;
            U = face_dist_at_tc(nt, thr_eval, U);
            const float D2 = uni(wave_min_f(U)), Tf = sq_plus(D2), D = sqrtf(D2);
            // reference: (one of) the triangle(s) that attain the minimum at tc, with its closest point q_D
            int tD = cseed * CL;
            const bool have = first_at(nt, D2, tD);
            f3 qD;
            { const Tri T = load_tri(A.tri, tD); point_tri_dist2_q(tc, T.a, T.b, T.c, qD); }
            const float invD = D > 1e-4f ? 1.0f / D : 0.0f;
            const f3 uD = {uni((tc.x - qD.x) * invD), uni((tc.y - qD.y) * invD), uni((tc.z - qD.z) * invD)};
            unsigned cbits = 0u;
            const int K = face_candidates(nt, Tf, D, uD, have, cbits);
            MPH_COUNT(lane == 0 && K > TL_CAND, 15, 1); // more candidates than the table holds: evaluated in batches
            MPH_COUNT(lane == 0, 11, K);                // per-lane evaluations of the tile search
            // a table-full at a time (a tile facing a flat part of the mesh from decimetres away has ~60: any triangle under the tile's
            // footprint can be the closest of one of its points)
            for (int base = 0; base < K; base += TL_CAND) {
                if (base > 0) face_refill(nt, cbits, base);
                __builtin_amdgcn_wave_barrier();
                face_eval_table(min(TL_CAND, K - base));
            }
            return true;
        };
        // The records of a cluster come through wave-uniform (scalar) loads: the cluster index is the same in every lane.  All CL bound
        // records are fetched before the first is used (one scalar-memory latency per cluster instead of one per triangle).
        auto eval_cluster = [&](const f3& p, float& best, int& bf, const float vb, int c) {
            float4 sp[CL], tn[CL];
#pragma unroll
            for (int k = 0; k < CL; ++k) { sp[k] = sphere_of(c * CL + k); tn[k] = tnorm_of(c * CL + k); }
#pragma unroll
            for (int k = 0; k < CL; ++k) {
                if (disc_lb2(sp[k], tn[k], p) > fminf(best, vb) * (1.0f + 1e-4f) + 1e-12f) continue;
                const int t = c * CL + k;
                const float d = tri_dist2(p, t);
                MPH_COUNT(__builtin_ctzll(__ballot(1)) == lane, 7, 1); // exact evaluations (some lane)
                const int of = A.orig[t];
                if (d < best || (d == best && of < bf)) { best = d; bf = of; }
            }
        };
        const int cseed = nearest_cluster(s_box, A.nc);
        const bool tiled = try_tile && face_tile(cseed);
#ifdef VANERF_MESH_PHASES
        if (lane == 0 && !try_tile) ph[13] += 1;
        if (lane == 0) { ph[tiled ? 8 : 9] += 1; const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (tiled) ph[10] += t_ - tprev; }
#endif
        if (!tiled) {
#pragma unroll
            for (int k = 0; k < ND; ++k) {
                const f3 p = pk[k];
                const float vb = vbk[k];
                float best = INFINITY;
                int bf = 0x7fffffff;
                lane_search(p, s_box, A.nc, cseed, [&]() { return fminf(best, vb); }, [&](int c) { eval_cluster(p, best, bf, vb, c); }, true);
                bestk[k] = best;
                bfk[k] = bf;
            }
        }
        MPH(2); // closest face

        // ---- stage 6, per point: inside test, signed distance, visibility, stores
        auto finish_point = [&](int k) {
            const f3 p = pk[k];
            bool act;
            const long long i = locate(k, act);
            const float best = bestk[k];
            // a point without a finite distance (NaN or infinite coordinates) answers face 0, as the exhaustive scan's strict `d < best` leaves it; the
            // sentinel never indexes the face table
            const int bf = (bfk[k] == 0x7fffffff || !(best < INFINITY)) ? 0 : bfk[k];
            // inside test on the (y,z) grid
            const float fy = floorf((p.y - grid_y0) / grid_cy), fz = floorf((p.z - grid_z0) / grid_cz);
            int cy = (int)fy, cz = (int)fz;
            cy = min(max(cy, 0), grid_G - 1);
            cz = min(max(cz, 0), grid_G - 1);
            const int cell = cy * grid_G + cz;
            // A point more than a whole cell outside the mesh's (y,z) extent lies beside every triangle by ~1 mm or more: its edge functions
            // (|edge| x distance against 1e-7 relative rounding) cannot all agree in sign, so the exhaustive scan counts no crossing either.
            // (Points within a cell of the border keep going through the border cells' lists, as before.)
            const bool beside = fy < -1.0f || fy > (float)grid_G || fz < -1.0f || fz > (float)grid_G;
            const int k0 = beside ? 0 : A.cell_start[cell], e = beside ? 0 : A.cell_start[cell + 1];
            // first pass: the earlier tie rule at the price it always had, plus a note that some edge function was exactly 0 (edge_side_by_index)
            bool tie = false;
            int cnt = count_crossings(A.cell_rec, k0, e, p, [&](f3 a, f3 b, f3 c3, int i0, int i1, int i2, float& E0, float& E1, float& E2) {
                const bool s0 = edge_side_by_index(b, c3, i1, i2, p.y, p.z, E0, tie);
                const bool s1 = edge_side_by_index(c3, a, i2, i0, p.y, p.z, E1, tie);
                const bool s2 = edge_side_by_index(a, b, i0, i1, p.y, p.z, E2, tie);
                return (s0 && s1 && s2) || (!s0 && !s1 && !s2);
            });
            // Some edge function tied and the point is not on the surface (where the count above stands, edges_agree): the ray meets an edge's
            // line or a vertex' projection exactly.  Counted again with the ties decided for one displaced point.  Rare: never on ray samples.
            if (__builtin_expect(tie && best != 0.0f, 0))
                cnt = count_crossings(A.cell_rec, k0, e, p, [&](f3 a, f3 b, f3 c3, int i0, int i1, int i2, float& E0, float& E1, float& E2) {
                    bool by_index;
                    return edges_agree(a, b, c3, i0, i1, i2, p.y, p.z, E0, E1, E2, by_index);
                });
            MPH(3); // inside test
            const float dist = sqrtf(best + 1e-6f);
            if (act) sdf[i] = (cnt & 1) ? -dist : dist;
            if (face && act) face[i] = bf;
            const bool visible = face_visible(V, F, vert_vis, bf, p);
            if (act) vis[i] = visible;
        };
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            __builtin_amdgcn_sched_barrier(0); // one point after the other (no interleaving of the unrolled copies: registers)
            finish_point(k);
        }
        MPH(4); // visibility + stores
    }
#ifdef VANERF_MESH_PHASES
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 16; ++k) atomicAdd(&g_ma_phase[k], ph[k]);
#endif
}

} // namespace

// One body for both query entries: vanerf_mesh_query_accel is the NULL-order case (its messages name that entry for either).
extern "C" int vanerf_mesh_query_accel_ordered(const VanerfMeshAccel* accel, const float* verts, int nv, const int32_t* faces, int nf,
                                               const float* vert_vis, const float* pts, int64_t n, float* sdf, uint8_t* vis, int32_t* face,
                                               int32_t* knn_idx, int grid_nx, int grid_ny, int grid_s, void* queue_word,
                                               const int32_t* item_order, void* stream)
{
    return guarded([&] {
        if (n == 0) return; // an empty batch is valid (and has null data pointers)
        if (item_order && grid_nx <= 0) throw_error("vanerf_mesh_query_accel_ordered: an item order needs the ray-grid hint");
        if (item_order && n > 0x7fffffffLL) throw_error("vanerf_mesh_query_accel_ordered: n = %lld does not fit the table's 32-bit sample indices", (long long)n);
        if (!accel || !verts || !faces || !vert_vis || !pts || !sdf || !vis) throw_error("vanerf_mesh_query_accel: null argument");
        const VanerfMeshAccel& A = *accel;
        if (!A.tri || !A.sphere || !A.tnorm || !A.orig || !A.cbox || !A.cdisc || !A.cell_start || !A.cell_tri || !A.cell_rec || !A.grid) throw_error("vanerf_mesh_query_accel: accel has a null pointer");
        if (A.nc <= 0 || A.nc > MA_MAX_CLUSTERS || A.nfp != A.nc * CL || A.nfp < nf) throw_error("vanerf_mesh_query_accel: bad cluster table (nc=%d nfp=%d nf=%d)", A.nc, A.nfp, nf);
        if (nv <= 0 || nf <= 0 || n < 0) throw_error("vanerf_mesh_query_accel: nv=%d nf=%d n=%lld", nv, nf, (long long)n);
        if (!A.vsort || !A.vbox || A.nvc <= 0 || A.nvc > MA_MAX_VCLUSTERS || A.nvc * CL < nv)
            throw_error("vanerf_mesh_query_accel: bad vertex cluster table (nvc=%d nv=%d)", A.nvc, nv);
        const size_t lds = sizeof(float) * ((size_t)A.nvc * CL * 4 + (size_t)A.nvc * 6 + (size_t)A.nc * 6);
        if (lds > 140 * 1024) throw_error("vanerf_mesh_query_accel: mesh too large for the LDS-resident tables (%zu bytes)", lds);
        if (lds > 64 * 1024) { // above the default dynamic-LDS limit (gfx950 has 160 KB per CU)
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(mesh_query_accel_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(mesh_query_accel_kernel<ND_MAX>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        if (n == 0) return;
        if (grid_nx != 0 && (grid_nx < 0 || grid_ny <= 0 || grid_s <= 0 || (long long)grid_nx * grid_ny * grid_s != n))
            throw_error("vanerf_mesh_query_accel: ray-grid hint %d x %d x %d does not match n = %lld", grid_nx, grid_ny, grid_s, (long long)n);
        if (n >= (1ll << 36)) throw_error("vanerf_mesh_query_accel: n = %lld points in one launch (limit 2^36)", (long long)n);
        // as many blocks as the chip holds at once (the work queue hands out the points; its head is the caller's queue_word, zeroed on the stream)
        if (!queue_word || (reinterpret_cast<uintptr_t>(queue_word) & 7u)) throw_error("vanerf_mesh_query_accel: queue_word must be 8 bytes of device memory, 8-byte aligned");
        struct PerDevice { std::atomic<size_t> lds{~(size_t)0}; std::atomic<int> resident{0}; };
        static PerDevice per_device[64]; // host-side cache of the occupancy query, per device (and again when the mesh, hence the LDS footprint, changes)
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        PerDevice& pd = per_device[dev & 63];
        if (pd.resident.load() == 0 || pd.lds.load() != lds) {
            int cus = 256, per_cu = 1;
            HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mesh_query_accel_kernel<ND_MAX>, MA_BLOCK, lds));
            pd.resident.store(cus * (per_cu > 0 ? per_cu : 1));
            pd.lds.store(lds);
        }
        const int resident = pd.resident.load();
        unsigned long long* const queue = static_cast<unsigned long long*>(queue_word);
        HIP_CHECK(hipMemsetAsync(queue, 0, sizeof(unsigned long long), (hipStream_t)stream));
        long long blocks = (n + MA_BLOCK - 1) / MA_BLOCK;
        if (blocks > resident) blocks = resident;
        // Several depths per item only when every wave gets a handful of them: below that a launch is bound by the latency of single items, and
        // twice as many lighter items run better (a 128x128 view at 32 samples: 4 096 items of two depths for 4 096 waves).
        const long long waves = (long long)resident * (MA_BLOCK / 64), items_nd = (n + 64 * ND_MAX - 1) / (64 * ND_MAX);
        if (ND_MAX > 1 && items_nd >= 4 * waves)
            hipLaunchKernelGGL(mesh_query_accel_kernel<ND_MAX>, dim3((unsigned)blocks), dim3(MA_BLOCK), lds, (hipStream_t)stream, A, verts, faces, vert_vis,
                               pts, (long long)n, sdf, vis, face, knn_idx, grid_nx, grid_ny, grid_s, queue, item_order);
        else
            hipLaunchKernelGGL(mesh_query_accel_kernel<1>, dim3((unsigned)blocks), dim3(MA_BLOCK), lds, (hipStream_t)stream, A, verts, faces, vert_vis,
                               pts, (long long)n, sdf, vis, face, knn_idx, grid_nx, grid_ny, grid_s, queue, item_order);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_mesh_query_accel(const VanerfMeshAccel* accel, const float* verts, int nv, const int32_t* faces, int nf,
                                       const float* vert_vis, const float* pts, int64_t n, float* sdf, uint8_t* vis, int32_t* face,
                                       int32_t* knn_idx, int grid_nx, int grid_ny, int grid_s, void* queue_word, void* stream)
{
    return vanerf_mesh_query_accel_ordered(accel, verts, nv, faces, nf, vert_vis, pts, n, sdf, vis, face, knn_idx, grid_nx, grid_ny, grid_s, queue_word,
                                           nullptr, stream);
}

#ifdef VANERF_MESH_PHASES
extern "C" int vanerf_debug_mesh_phases(unsigned long long* out8, int reset)
{
    return guarded([&] {
        HIP_CHECK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_ma_phase), sizeof(unsigned long long) * 16));
        if (reset) { unsigned long long z[16] = {}; HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_ma_phase), z, sizeof z)); }
    });
}
#endif

extern "C" int vanerf_mesh_cluster_size(void) { return CL; }

// ---------------------------------------------------------------------------------------------------------------
// vanerf_mesh_tile_order: the item order of vanerf_mesh_query_accel_ordered.  One block per 8 x 8 pixel tile sorts the tile's 64 S samples by
// the depth they were made from, in LDS, by a merge sort by ranks: every element finds its place in the merged run by a search of the
// sibling run, and the passes go from one pair of LDS arrays (32-bit keys: the depth as an ordered integer; 16-bit index within the tile)
// to the other.  Stable without the index in the key: the first runs are in index order, and of equal keys the one from the earlier run goes
// first (a key of the earlier run counts the sibling's keys below it, a key of the later run those not above it) -- ties keep ray-major
// index order, the table is the same on every run, no atomics.
//   * A ray's depths nearly always ascend already (linspace, sorted importance samples): then the first runs are the rays themselves (6
//     passes instead of log2(64 S)); a tile with a ray that does not (or with a NaN) starts from runs of one element.  Runs need not be
//     powers of two.
//   * The kernel is bound by its LDS reads, counted per WAVE: a loop runs as long as its slowest lane (measured on the benchmark view: 64-bit
//     keys and a bisection per element, 57 reads each, 0.32 ms; 32-bit keys and a search that gallops from the element's own offset, short
//     in most lanes but long in some lane of nearly every wave, 0.26 ms).  So a thread takes four consecutive keys of a run: a bisection
//     for the first -- the same trip count in every lane -- and for the others a gallop upwards from the previous key's rank, which
//     neighbouring rays (samples at nearly the same depths) end within a step or two.
namespace {

constexpr int TO_BLOCK = 1024;
constexpr int TO_MAX_S = 128; // 64 S elements of 2 x (4 + 2) bytes: 96 KB of the CU's 160 KB
static_assert(64 * TO_MAX_S <= 65536, "the index within a tile is kept in 16 bits");

__global__ __launch_bounds__(TO_BLOCK) void mesh_tile_order_kernel(const float* __restrict__ z, int gnx, int gny, int S, int32_t* __restrict__ order)
{
    extern __shared__ unsigned s_tile[]; // [2][64 S] keys, then [2][64 S] 16-bit indices
    const int N = 64 * S;
    // (Measured and dropped: four dwords of padding per 32 keys against the power-of-two strides of the bisections' probes: 0.21 / 0.24 ms
    //  against 0.18 / 0.20 on the coarse / fine depths of the benchmark view.)
    unsigned* src = s_tile;
    unsigned* dst = s_tile + N;
    unsigned short* src_i = reinterpret_cast<unsigned short*>(s_tile + 2 * N);
    unsigned short* dst_i = src_i + N;
    const int ntx = (gnx + 7) >> 3;
    const int x0 = (int)(blockIdx.x % (unsigned)ntx) * 8, y0 = (int)(blockIdx.x / (unsigned)ntx) * 8;
    for (int e = threadIdx.x; e < N; e += TO_BLOCK) {
        const int l = e / S, d = e - l * S;
        const int rx = x0 + (l & 7), ry = y0 + (l >> 3);
        unsigned u = 0xffffffffu; // a ray beyond the grid border: behind every sample
        if (rx < gnx && ry < gny) {
            u = __float_as_uint(z[((long long)ry * gnx + rx) * S + d] + 0.0f); // (-0 becomes +0: they compare equal)
            u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;                         // ascending as unsigned
            u = min(u, 0xfffffffeu);                                            // (only a NaN of the last payload gets there)
        }
        src[e] = u;
        src_i[e] = (unsigned short)e;
    }
    __syncthreads();
    int descends = 0;
    for (int e = threadIdx.x; e < N; e += TO_BLOCK) descends |= (e % S != 0) && src[e - 1] > src[e];
    for (int L = __syncthreads_or(descends) ? 1 : S; L < N; L *= 2) {
        // four consecutive keys of a run per thread (one where the runs are no multiple of four), read in one 16-byte read
        const int E = (L & 3) ? 1 : 4;
        for (int c = threadIdx.x * E; c < N; c += TO_BLOCK * E) {
            unsigned key4[4] = {};
            unsigned idx4[4] = {};
            if (E == 4) {
                const uint4 k = *reinterpret_cast<const uint4*>(src + c);
                const uint2 i = *reinterpret_cast<const uint2*>(src_i + c);
                key4[0] = k.x; key4[1] = k.y; key4[2] = k.z; key4[3] = k.w;
                idx4[0] = i.x & 0xffffu; idx4[1] = i.x >> 16; idx4[2] = i.y & 0xffffu; idx4[3] = i.y >> 16;
            } else {
                key4[0] = src[c];
                idx4[0] = src_i[c];
            }
            const int a0 = c / (2 * L) * (2 * L), b0 = min(a0 + L, N), end = min(a0 + 2 * L, N);
            const bool in_a = c < b0;
            const unsigned* const sib = src + (in_a ? b0 : a0); // the sibling run
            const int len = in_a ? end - b0 : L;
            // a0 + (offset in the own run) + rank: e + rank for a key of the earlier run, a0 + (e - b0) + rank for one of the later
            const int place0 = c - b0 + (in_a ? b0 : a0);
            int lo = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= E) break;
                const unsigned key = key4[j];
                // `below`: the sibling's keys that go in front of this one; the rank is the first index that is not below (they ascend)
                auto below = [&](int i) { return in_a ? sib[i] < key : sib[i] <= key; };
                int hi = len; // the rank is in [lo, hi]
                if (j > 0) {  // gallop up from the previous key's rank: 1, 2, 4, ... until the rank is bracketed
                    for (int step = 1; lo + step - 1 < hi; step *= 2) {
                        const int p = lo + step - 1;
                        if (below(p)) lo = p + 1; else { hi = p; break; }
                    }
                }
                while (lo < hi) { // bisection: the whole sibling run for a thread's first key (the same trip count in every lane)
                    const int mid = (lo + hi) >> 1;
                    if (below(mid)) lo = mid + 1; else hi = mid;
                }
                dst[place0 + j + lo] = key;
                dst_i[place0 + j + lo] = (unsigned short)idx4[j];
            }
        }
        __syncthreads();
        unsigned* const t = src; src = dst; dst = t;
        unsigned short* const ti = src_i; src_i = dst_i; dst_i = ti;
    }
    for (int e = threadIdx.x; e < N; e += TO_BLOCK) {
        const int local = src_i[e], l = local / S, d = local - l * S;
        const int rx = x0 + (l & 7), ry = y0 + (l >> 3);
        order[(long long)blockIdx.x * N + e] = (rx < gnx && ry < gny) ? (ry * gnx + rx) * S + d : -1;
    }
}

} // namespace

extern "C" int vanerf_mesh_tile_order(const float* z, int grid_nx, int grid_ny, int grid_s, int32_t* order, void* stream)
{
    return guarded([&] {
        if (!z || !order) throw_error("vanerf_mesh_tile_order: null argument");
        if (grid_nx <= 0 || grid_ny <= 0 || grid_s <= 0) throw_error("vanerf_mesh_tile_order: grid %d x %d x %d", grid_nx, grid_ny, grid_s);
        if (grid_s > TO_MAX_S) throw_error("vanerf_mesh_tile_order: %d samples per ray (limit %d: a tile is sorted in LDS)", grid_s, TO_MAX_S);
        const long long tiles = (long long)((grid_nx + 7) >> 3) * ((grid_ny + 7) >> 3);
        if (tiles * 64 * grid_s > 0x7fffffffLL) throw_error("vanerf_mesh_tile_order: grid %d x %d x %d does not fit 32-bit sample indices", grid_nx, grid_ny, grid_s);
        const size_t lds = (sizeof(unsigned) + sizeof(unsigned short)) * 2 * 64 * (size_t)grid_s;
        if (lds > 64 * 1024) // above the default dynamic-LDS limit
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(mesh_tile_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(mesh_tile_order_kernel, dim3((unsigned)tiles), dim3(TO_BLOCK), lds, (hipStream_t)stream, z, grid_nx, grid_ny, grid_s, order);
        HIP_CHECK(hipGetLastError());
    });
}
