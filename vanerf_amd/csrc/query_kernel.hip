// query_kernel.hip -- the per-sample hot kernel: VANeRF.query + eval_func for N samples
// (reference src/model.py:748-957, 1140-1160; networks src/networks.py:27-33, 75-106, 281-293;
// src/utils.py:136-151, 633-649, 744-779, 822-880; src/spatial.py:59-117).
//
// One wave = 32 samples.  Lane l works on sample j = l & 31; the two lanes j and j + 32 that share
// a sample split every K dimension between them (half h = l >> 5), see layer_spec.h.  All 20 dense
// layers run as MFMA chains -- query_kernel<0>: v_mfma_f32_32x32x2_f32 on fp32 operands; query_kernel<1>:
// v_mfma_f32_32x32x16_bf16 on split (hi + lo) operands, fp32 accumulate -- whose accumulators stay in registers
// from the bilinear gathers to the final (alpha, sdf, rgb) store: activations never touch LDS or HBM.
// The fp32 kernel uses no LDS beyond its control words: key points come through the scalar cache, weights stream from L2 as pre-permuted
// MFMA A-fragments (weights_pack.cpp).  The split-bf16 kernel owns its CU's LDS: key points, the resident fragments of the last layers and
// the ring the eight waves of a block share the streamed fragments through (see the LDS map in bf16x3_ring.h).  The 1-NN vertex index arrives
// from vanerf_mesh_query_accel.  query_kernel<1, false, 1> is the HOISTED split-bf16 kernel: three first layers start from the per-vertex
// products of vertex_products.hip and run their per-sample k-steps only (layer_spec.h).  query_kernel<1, false, 2> is the LEAN kernel: the
// hoisted one on the lean stream -- two linear layers folded into their consumers, five accumulators started from a bias table, one k-pair
// less in the TexVisFusion input, the two last head layers resident (layer_spec.h).  With a validity partition it hands the all-invalid groups
// behind the partition's boundary to query_short_kernel<2>, a second launch in a shape of its own (three waves per SIMD; same stages, same bits).
//
// The file: QueryParams, the fp32 lane with its spill plumbing, the mode dispatch of the layer runners (mfma_chain.h fp32, bf16x3_ring.h
// split-bf16), the stages of a round in the order they run, the kernel -- its body is the round's protocol and the sequence of stages --,
// the launch entries.  The per-sample arithmetic around the layers is sample_math.h, the validity partition query_order.hip.
//
// Built with -ffp-contract=off: the integer-valued outputs (1-NN index) depend on fp32 compare
// results and must match oracle/mesh_oracle.c bit for bit; fused multiply-adds are spelled fmaf().
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "common.h"
#include "mfma_chain.h"
#include "sample_math.h"
#include "bf16x3_ring.h"

using namespace vanerf;
using namespace vanerf_chain;


namespace {

// Waves per SIMD of the split-bf16 kernel: TWO, as one 8-wave block per CU that owns the CU's LDS.  One in-order wave per SIMD
// issues at most one instruction every ~4 cycles, and a full 32-sample group is ~9 700 instructions around 990 MFMAs: alone, the wave was
// issue-bound at ~54 k cycles per group with NO fragment traffic at all, against 31.7 k cycles of matrix-pipe time ("Round 3:
// what the kernel is now").  A second wave fills the issue slots; it needs the kernel in 256 registers WITHOUT scratch (build.py fails a
// build that spills): key points in LDS instead of 63 VGPRs, gathers issued where they are used, fragment rings kept per output block and
// at most two blocks deep, LDS addresses formed from three window bases (see LAddr).  Cut to 256 registers by the compiler instead, the
// kernel put 155 VGPRs in scratch and its results were not reproducible run to run; this build is reproducible
// (tools/check_mode1_determinism.py).
constexpr int WAVES_PER_SIMD = 2;       // query_kernel<0> and query_kernel<1>
constexpr int WAVES_PER_SIMD_SPILL = 1; // the spill build takes the whole register file: at 256 registers it goes to scratch
// waves per block: the fp32 kernel runs two 4-wave blocks per CU, the split-bf16 kernel ONE 8-wave block per CU (it owns the CU's LDS)
template <int MODE> constexpr int WPB = MODE == 1 ? RING_WAVES : 4;

// Diagnostic build only (-DVANERF_STAMPS): per-phase s_memtime deltas summed per wave into QueryParams::stamps.
// No stamp executes in the product build; stamp values never reach an output element.

#ifdef VANERF_STAMPS
#define STAMP(k)                                                                                  \
    do {                                                                                          \
        unsigned long long t_;                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        phase_cycles[k] += t_ - t_prev;                                                           \
        t_prev = t_;                                                                              \
    } while (0)
constexpr int N_PHASES = 12;
#else
#define STAMP(k) do { } while (0)
#endif

struct QueryParams {
    VanerfFrame f;
    const float* w;
    unsigned wbytes;
    const float* pts;
    const float* qsdf;
    const uint8_t* qvis;
    const float* noise;
    const int32_t* knn_in;
    const int32_t* order;  // optional: slot k of the launch works on sample order[k] (validity partition), else on sample k
    int raw; // 1: write [sdf_pred, rad, r, g, b] (VANeRF.query), 0: eval_func applied ([alpha, sdf, r, g, b])
    long long n;
    float* out;
    uint8_t* valid;
    unsigned long long* stamps; // [waves][N_PHASES] (diagnostic build), else unused
    unsigned* queue;            // work-queue head: next unclaimed 32-sample group (zero before the launch)
    unsigned long long* short_groups; // optional: += number of groups that took the all-invalid short path
    float wm1[4], hm1[4];             // (float)(W - 1), (float)(H - 1) of the image / tex / geo0 / geo1 maps (kept scalar: no per-lane copies)
    const float* vp;                  // hoisted kernel: the table of per-vertex products (vertex_products.hip), else unused
    float *xs, *aux;                  // spill mode (training): X and auxiliary spills, [rows][npad] floats (layer_spec.h)
    long long npad;
};

// precision-mode dispatch: MODE 0 = fp32 MFMA (exact), MODE 1 = split-bf16 x3
template <int MODE, int NB> struct RingSel { using type = Ring<NB>; };
template <int NB> struct RingSel<1, NB> { using type = RingB<NB>; };

// `la`: the lane's place in a fragment -- its index (fp32 kernel) or its LDS / buffer byte offsets (split-bf16 kernel, LAddr)
// fp32 kernel: the lane index, plus (training, spill mode: vanerf_query_forward_spill) where this lane's column of the X / auxiliary
// spills starts -- null pointers in the inference kernel, where every store below folds away
struct LLane {
    int lane;
    // spill mode: buffer stores, offset = voff (this lane's column: 4 (col + h npad)) + a wave-uniform row offset (2 r x 4 npad) -- one s_mul and
    // one store per value (global stores with 64-bit addresses took ~9 instructions each: 19.6 k instructions per group against 9.8 k without
    // the spills).  A lane that must not spill holds voff = SPILL_OFF: beyond both buffers' sizes, so the hardware drops the store.
    WRsrc xs, aux;       // Xs[X_ROWS][npad], Aux[AUX_ROWS][npad]
    unsigned voff, row4; // row4 = 4 npad (bytes per row)
    bool on;             // the kernel's SPILL parameter (a constant: the stores fold away in the other builds)
};
constexpr unsigned SPILL_OFF = 0xfffffff0u;
template <int L, int t> __device__ __forceinline__ void spill_x(const LLane& la, float v)
{
    if (la.on) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), la.xs, la.voff, (unsigned)(x_row_base(L) + 2 * t) * la.row4, 0);
}
template <int K> __device__ __forceinline__ void spill_aux(const LLane& la, float v)
{
    if (la.on) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), la.aux, la.voff, (unsigned)(2 * K) * la.row4, 0);
}
// the fp32 lane of slot g * 32 + (lane & 31), made per round
template <bool SPILL> __device__ __forceinline__ LLane make_llane(int lane, WRsrc xs_rs, WRsrc aux_rs, long long npad, long long g, long long ngroups)
{
    LLane la;
    la.lane = lane; la.voff = SPILL_OFF; la.row4 = 0; la.on = SPILL;
    if constexpr (SPILL) {
        la.xs = xs_rs; la.aux = aux_rs;
        // the row stride, opaque per round: hoisted out of the work loop the ~1 100 row offsets are parked in registers.  (Set on every
        // path: a value that depends on the group index is divergent to the compiler, and a divergent store offset is a waterfall loop.)
        unsigned r4 = (unsigned)npad * 4u;
        asm volatile("" : "+s"(r4));
        la.row4 = r4;
        // column = the slot's own place g * 32 + j (also for lanes beyond n: their output gradient is zero); no column beyond the last group
        if (g < ngroups) la.voff = 4u * ((unsigned)g * 32u + (unsigned)(lane & 31)) + (unsigned)(lane >> 5) * r4;
    }
    return la;
}
template <int MODE> struct LaneSel { using type = LLane; };
template <> struct LaneSel<1> { using type = LAddr; };
__device__ __forceinline__ unsigned lane_of(const LLane& la) { return (unsigned)la.lane; }
template <int MODE, int LEVEL, int NB, int T, int L> __device__ __forceinline__ typename RingSel<MODE, NB>::type ring_start_m(WRsrc rs, const typename LaneSel<MODE>::type& la)
{
    if constexpr (MODE == 0) return ring_start<NB, T>(rs, layer_offset(L), lane_of(la) * NB * 4u);
    else return ring_start_b<LEVEL, NB, T, (L >= LDS_FIRST<LEVEL>), layer_offset_b(L, LEVEL)>(rs, la);
}

template <int MODE, int LEVEL, int NB, int T, int L, class Op>
__device__ __forceinline__ void run_layer_m(f32x16 (&acc)[NB], typename RingSel<MODE, NB>::type& ring, WRsrc rs, const typename LaneSel<MODE>::type& la, Op&& operand)
{
    if constexpr (MODE == 0)
        run_layer<NB, T>(acc, ring, rs, layer_offset(L), lane_of(la) * NB * 4u, [&](auto tc) -> float {
            const float b = operand(tc);
            spill_x<L, decltype(tc)::value>(la, b); // (spill mode only)
            return b;
        });
    else {
        static_assert(MODE == 0 || T == kT_b(L, LEVEL), "the kernel and the packed stream agree on the layer's k-pairs");
        run_layer_b<LEVEL, NB, T, (L >= LDS_FIRST<LEVEL>), layer_offset_b(L, LEVEL)>(acc, ring, rs, la, static_cast<Op&&>(operand));
    }
}

// chain operand t of a layer: register t % 16 of block t / 16 of a previous accumulator array, then the bias step (B operand one_h0: 1 in the h = 0 half)
template <int NSTEPS, int NB, class TC> __device__ __forceinline__ float chain(const f32x16 (&src)[NB], TC, float one_h0)
{
    constexpr int t = TC::value;
    if constexpr (t < NSTEPS) return src[t / 16][t % 16];
    else return one_h0;
}
template <int MODE, int NSTEPS, int NB, class TC> __device__ __forceinline__ float chain_sp(const f32x16 (&src)[NB], TC, float one_h0) // the same through Softplus (lazy_act)
{
    constexpr int t = TC::value;
    if constexpr (t < NSTEPS) return lazy_act<MODE, ACT_SOFTPLUS>(src[t / 16][t % 16]);
    else return one_h0;
}

// ---- The stages of a round, in the order query_kernel runs them.  Each takes what it reads and writes as parameters: the arrays in a stage's
// ---- signature are the registers that are live across it.

// The six per-sample inputs of a group are fetched one group ahead (its index is known from the early claim): their HBM latency
// is otherwise the first thing a group waits for.
struct SampleIn { float px, py, pz, sdf; int knn; unsigned char vis; };
__device__ __forceinline__ SampleIn fetch_at(const QueryParams& P, long long sc) // the inputs of sample sc
{
    SampleIn in;
    in.px = P.pts[3 * sc]; in.py = P.pts[3 * sc + 1]; in.pz = P.pts[3 * sc + 2];
    in.sdf = P.qsdf[sc]; in.knn = P.knn_in[sc]; in.vis = P.qvis[sc];
    return in;
}
__device__ __forceinline__ SampleIn fetch_sample(const QueryParams& P, unsigned grp, int j)
{
    const long long sr = (long long)grp * 32 + j;
    long long sc = sr < P.n ? sr : P.n - 1; // also covers a claim beyond the last group (never used)
    if (P.order) sc = P.order[sc];
    return fetch_at(P, sc);
}

// Block prologue of the split-bf16 kernel, once per launch (it is persistent).  The key points (the fp32 kernel reads them through the scalar cache) ...
__device__ __forceinline__ void key_points_to_lds(const VanerfFrame& F)
{
    if (threadIdx.x < 2 * PE_KPT_PER_HALF) s_dyn[LDS_KPT / 16 + threadIdx.x] = reinterpret_cast<const u32x4*>(F.kpt_cam)[threadIdx.x];
}
// ... one copy of the resident fragments per block (256 blocks x 126 KB from L2), the lean kernel's bias table and phase 0 of the ring
// (BASE_DW, DW, LDS_AT: the part of the stream that stays and where -- the full map's, or the SHORT map's; THREADS: the block's)
template <int LEVEL, unsigned BASE_DW, unsigned DW, unsigned LDS_AT, unsigned THREADS> __device__ __forceinline__ void resident_to_lds(const QueryParams& P)
{
    const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(P.w) + BASE_DW / 4;
    for (unsigned i = threadIdx.x; i < DW / 4; i += THREADS) s_dyn[LDS_AT / 16 + i] = src[i];
    if constexpr (LEVEL >= 2) { // the bias table stands behind the stream's slack (layer_spec.h); here it goes right behind the resident fragments
        const u32x4* __restrict__ bsrc = reinterpret_cast<const u32x4*>(P.w) + (layer_offset_b(NUM_LAYERS, LEVEL) + STREAM_SLACK_DW) / 4;
        if (threadIdx.x < BIAS_TABLE_FLOATS / 4) s_dyn[LDS_BIAS<LEVEL> / 16 + threadIdx.x] = bsrc[threadIdx.x];
    }
}
template <int LEVEL> __device__ __forceinline__ void fill_lds(const QueryParams& P, WRsrc W, int lane, unsigned wv_u)
{
    resident_to_lds<LEVEL, RES_BASE_DW<LEVEL>, RES_DW<LEVEL>, LDS_RES, 64 * RING_WAVES>(P);
    // phase 0 of the ring, once: every full round re-issues it for its successor (see phase_begin)
    const LAddr la0 = make_laddr(lane, wv_u);
    ring_dma<0>(W, la0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The short path's constant latent (wave 0; the layer's fragments -- and the bias table -- are resident by now), see LDS_LAT0
template <int LEVEL> __device__ __forceinline__ void short_path_latent(WRsrc W, int lane, unsigned wv_u)
{
    if (wv_u == 0u) {
        constexpr int T_IBR = kT_b(L_IBR, LEVEL);
        const LAddr la0 = make_laddr(lane, wv_u);
        auto r0 = ring_start_m<1, LEVEL, 1, T_IBR, L_IBR>(W, la0);
        f32x16 lat0[1];
        if constexpr (LEVEL >= 2) load_bias<L_IBR, 1>(lane >> 5, lat0);
        else zero<1>(lat0);
        const float one0 = (lane >> 5) ? 0.0f : 1.0f;
        run_layer_m<1, LEVEL, 1, T_IBR, L_IBR>(lat0, r0, W, la0, [&](auto tc) -> float { return decltype(tc)::value < 64 ? 0.0f : one0; });
        if ((lane & 31) == 0)
            static_for<16>([&](auto rc) { constexpr int r = decltype(rc)::value; reinterpret_cast<lds_u32_t*>((size_t)LDS_LAT0)[(lane >> 5) * 16 + r] = __float_as_uint(lat0[0][r]); });
    }
}

// Inputs of GeoVisFusion scale 0: the lane half's 32 channels of the pixel and of the two vertex rows -- hoisted kernels: the rows' products with
// the two first layers instead of the rows (nn = N0[i], tw = T0[i]: same registers) and a0s = A0[i]
// -- texel level: pix = the bilinear sample of GM (the feature's product with the second layer, same taps, same weights) and a0s = A0[i] + the
// sample of GA
template <bool HOIST, bool TEXEL = false>
__device__ __forceinline__ void geo0_gathers(const QueryParams& P, float x, float y, int h, int nn_idx, int tw_idx, float (&pix)[32], float (&nn)[32],
                                             float (&tw)[32], float (&a0s)[8])
{
    const VanerfFrame& F = P.f;
    const Bilin b0 = bilin_setup(x, y, F.h0, F.w0, P.wm1[2], P.hm1[2]);
    if constexpr (TEXEL) gather<8>(P.vp + VP_GM, b0, (int)VP_N0_ROW, 32 * h, pix);
    else gather<8>(F.geo0, b0, 64, 32 * h, pix);
    if constexpr (HOIST) {
        load_row<2>(P.vp + VP_A0, (unsigned)(nn_idx * (int)VP_A0_ROW + 8 * h), a0s);
        if constexpr (TEXEL) {
            float ga[8];
            gather<2>(P.vp + VP_GA, b0, (int)VP_A0_ROW, 8 * h, ga);
#pragma unroll
            for (int r = 0; r < 8; ++r) a0s[r] += ga[r];
        }
        load_row<8>(P.vp + VP_N0, (unsigned)(nn_idx * (int)VP_N0_ROW + 32 * h), nn);
        load_row<8>(P.vp + VP_T0, (unsigned)(nn_idx * (int)VP_N0_ROW + 32 * h), tw);
    } else {
        load_row<8>(F.vfeat0, (unsigned)(nn_idx * 64 + 32 * h), nn);
        load_row<8>(F.vfeat0, (unsigned)(tw_idx * 64 + 32 * h), tw);
    }
}

__device__ __forceinline__ void geo1_gathers(const QueryParams& P, float x, float y, int h, int nn_idx, int tw_idx, float (&pix8)[4], float (&nn8)[4],
                                             float (&tw8)[4])
{
    const VanerfFrame& F = P.f;
    const Bilin b1 = bilin_setup(x, y, F.h1, F.w1, P.wm1[3], P.hm1[3]);
    gather<1>(F.geo1, b1, 8, 4 * h, pix8);
    load_row<1>(F.vfeat1, (unsigned)(nn_idx * 8 + 4 * h), nn8);
    load_row<1>(F.vfeat1, (unsigned)(tw_idx * 8 + 4 * h), tw8);
}

// Inputs of the texture branch.  row: h = 0 nearest vertex [img3|tex8|gf18], h = 1 twin vertex; bi: the source-image taps
__device__ __forceinline__ void tex_gathers(const QueryParams& P, float x, float y, const Bilin& bi, int h, int nn_idx, int tw_idx, float (&row)[32],
                                            float (&qi)[4], float (&qt)[8])
{
    const VanerfFrame& F = P.f;
    load_row<8>(F.vfeat_tex, (unsigned)((h ? tw_idx : nn_idx) * 32), row);
    gather<1>(F.img, bi, 4, 0, qi);
    const Bilin bt = bilin_setup(x, y, F.ht, F.wt, P.wm1[1], P.hm1[1]);
    gather<2>(F.tex, bt, 8, 0, qt);
}

// one GeoVisFusion scale (src/networks.py:83-94 / 96-104): gates, gated 2-layer MLP.
//   HC = channels per lane half (32 for the 64-channel map, 4 for the 8-channel map), NBO = output blocks,
//   NREG_MID = registers of the last hidden block that carry real channels
// Lean kernel: the scale ends at `mid` (before its ReLU) -- the last layer is folded into the consumer's weights, which reads relu(mid).
template <int MODE, int LEVEL, int HC, int NBO, int NREG_MID, int l_at_a>
__device__ __forceinline__ void geo_scale(WRsrc W, int lane, const typename LaneSel<MODE>::type& la, typename RingSel<MODE, 1>::type& ring_at,
                                          float (&pix)[HC], float (&nn)[HC], float (&tw)[HC], float s0, float s1,
                                          f32x16 (&outacc)[NBO])
{
    constexpr int TIN = 3 * HC + 2;
    constexpr int TOUT = (NBO - 1) * 16 + NREG_MID;
    auto input = [&](auto tc) -> float {
        constexpr int t = decltype(tc)::value;
        if constexpr (t < HC) return pix[t];
        else if constexpr (t < 2 * HC) return nn[t - HC];
        else if constexpr (t < 3 * HC) return tw[t - 2 * HC];
        else if constexpr (t == 3 * HC) return s0;
        else return s1;
    };
    f32x16 at[1];
    zero<1>(at);
    run_layer_m<MODE, LEVEL, 1, TIN, l_at_a>(at, ring_at, W, la, input);
    auto r_gate = ring_start_m<MODE, LEVEL, 1, 6, l_at_a + 1>(W, la);
    auto r_mid = ring_start_m<MODE, LEVEL, NBO, TIN, l_at_a + 2>(W, la);
    if constexpr (MODE == 0) relu<1>(at);
    f32x16 gate[1];
    zero<1>(gate);
    run_layer_m<MODE, LEVEL, 1, 6, l_at_a + 1>(gate, r_gate, W, la, [&](auto tc) -> float { return lazy_act<MODE, ACT_RELU>(at[0][decltype(tc)::value]); });
    // gates live in rows 0..2 = registers 0..2 of the h = 0 lanes
    const float a0 = __shfl(sigmoid_f(gate[0][0]), lane & 31);
    const float a1 = __shfl(sigmoid_f(gate[0][1]), lane & 31);
    const float a2 = __shfl(sigmoid_f(gate[0][2]), lane & 31);
    if constexpr (MODE == 0) { constexpr int A = HC == 32 ? AUX_G0 : AUX_G1; spill_aux<A>(la, a0); spill_aux<A + 1>(la, a1); spill_aux<A + 2>(la, a2); }
#pragma unroll
    for (int t = 0; t < HC; ++t) { pix[t] *= a0; nn[t] *= a1; tw[t] *= a2; }
    if constexpr (LEVEL >= 2) {
        zero<NBO>(outacc);
        run_layer_m<MODE, LEVEL, NBO, TIN, l_at_a + 2>(outacc, r_mid, W, la, input);
    } else {
        f32x16 mid[NBO];
        zero<NBO>(mid);
        run_layer_m<MODE, LEVEL, NBO, TIN, l_at_a + 2>(mid, r_mid, W, la, input);
        auto r_out = ring_start_m<MODE, LEVEL, NBO, TOUT, l_at_a + 3>(W, la);
        if constexpr (MODE == 0) relu<NBO>(mid);
        zero<NBO>(outacc);
        run_layer_m<MODE, LEVEL, NBO, TOUT, l_at_a + 3>(outacc, r_out, W, la,
                             [&](auto tc) -> float { constexpr int t = decltype(tc)::value; return lazy_act<MODE, ACT_RELU>(mid[t / 16][t % 16]); });
    }
}

// Scale 0 of GeoVisFusion in the hoisted kernel.  The two vertex rows' share of both first layers comes from the table of per-vertex
// products: `at` starts from A0[i] (registers 0..7, the rest of the block is rows >= 10), `mid` from a1 N0[i] + a2 T0[i] -- the gates scale the
// products instead of the rows, W (a x) = a (W x) -- and the MFMAs run the 34 per-sample k-pairs [pix32 | (sdf, qvis) | (vis_nn, vis_tw)] only.
// Lean kernel: ends at `mid`, as geo_scale.
// Texel level: `pix` holds the sampled product GM, `a0s` already includes the sampled GA (geo0_gathers); `mid` starts from
// a0 GM + a1 N0 + a2 T0 and both layers run the one step of their two scalar k-pairs.
template <int MODE, int LEVEL>
__device__ __forceinline__ void geo_scale0_vp(WRsrc W, int lane, const typename LaneSel<MODE>::type& la, typename RingSel<MODE, 1>::type& ring_at,
                                              float (&pix)[32], const float (&a0s)[8], const float (&n0)[32], const float (&t0)[32], float s0, float s1,
                                              f32x16 (&outacc)[2])
{
    constexpr int TIN = kT_b(L_GEO_AT0_A, LEVEL);
    static_assert(TIN == (LEVEL == 3 ? 2 : 32 + 2), "[pix32 |] (sdf, qvis) | (vis_nn, vis_tw)");
    auto input = [&](auto tc) -> float {
        constexpr int t = decltype(tc)::value;
        if constexpr (t < TIN - 2) return pix[t];
        else if constexpr (t == TIN - 2) return s0;
        else return s1;
    };
    f32x16 at[1];
    zero<1>(at);
#pragma unroll
    for (int r = 0; r < 8; ++r) at[0][r] = a0s[r];
    run_layer_m<MODE, LEVEL, 1, TIN, L_GEO_AT0_A>(at, ring_at, W, la, input);
    auto r_gate = ring_start_m<MODE, LEVEL, 1, 6, L_GEO_AT0_B>(W, la);
    auto r_mid = ring_start_m<MODE, LEVEL, 2, TIN, L_GEO_ATED0_A>(W, la);
    f32x16 gate[1];
    zero<1>(gate);
    run_layer_m<MODE, LEVEL, 1, 6, L_GEO_AT0_B>(gate, r_gate, W, la, [&](auto tc) -> float { return lazy_act<MODE, ACT_RELU>(at[0][decltype(tc)::value]); });
    const float a0 = __shfl(sigmoid_f(gate[0][0]), lane & 31);
    const float a1 = __shfl(sigmoid_f(gate[0][1]), lane & 31);
    const float a2 = __shfl(sigmoid_f(gate[0][2]), lane & 31);
    if constexpr (LEVEL == 3) {
#pragma unroll
        for (int t = 0; t < 32; ++t) outacc[t / 16][t % 16] = fmaf(a0, pix[t], fmaf(a2, t0[t], a1 * n0[t]));
        run_layer_m<MODE, LEVEL, 2, TIN, L_GEO_ATED0_A>(outacc, r_mid, W, la, input);
    } else if constexpr (LEVEL == 2) {
#pragma unroll
        for (int t = 0; t < 32; ++t) { pix[t] *= a0; outacc[t / 16][t % 16] = fmaf(a2, t0[t], a1 * n0[t]); }
        run_layer_m<MODE, LEVEL, 2, TIN, L_GEO_ATED0_A>(outacc, r_mid, W, la, input);
    } else {
        f32x16 mid[2];
#pragma unroll
        for (int t = 0; t < 32; ++t) { pix[t] *= a0; mid[t / 16][t % 16] = fmaf(a2, t0[t], a1 * n0[t]); }
        run_layer_m<MODE, LEVEL, 2, TIN, L_GEO_ATED0_A>(mid, r_mid, W, la, input);
        auto r_out = ring_start_m<MODE, LEVEL, 2, 32, L_GEO_ATED0_B>(W, la);
        zero<2>(outacc);
        run_layer_m<MODE, LEVEL, 2, 32, L_GEO_ATED0_B>(outacc, r_out, W, la,
                             [&](auto tc) -> float { constexpr int t = decltype(tc)::value; return lazy_act<MODE, ACT_RELU>(mid[t / 16][t % 16]); });
    }
}

// mlp0's fragment ring, started before the layer in front of it runs: fp32 seven one-step slots (slot = k-step % 7), split-bf16 a RingB
struct Mlp0RingF { WFrag<4> f[PE_FEATS]; };
template <int MODE> using Mlp0Ring = std::conditional_t<MODE == 0, Mlp0RingF, RingB<4>>;

// The small second scale, with mlp0's ring (7 x dwordx4) started before it runs (split-bf16: behind it)
template <int MODE, int LEVEL>
__device__ __forceinline__ void geo_scale1(WRsrc W, int lane, const typename LaneSel<MODE>::type& la, float (&pix8)[4], float (&nn8)[4], float (&tw8)[4],
                                           float s0, float s1, f32x16 (&g8)[1], Mlp0Ring<MODE>& ring0)
{
    auto r_at1 = ring_start_m<MODE, LEVEL, 1, 14, L_GEO_AT1_A>(W, la);
    if constexpr (MODE == 0)
        static_for<PE_FEATS>([&](auto fc) { constexpr int f = decltype(fc)::value; ring0.f[f] = wload<4>(W, (layer_offset(L_MLP0) + f * 256) * 4u, lane_of(la) * 16u); });
    geo_scale<MODE, LEVEL, 4, 1, 4, L_GEO_AT1_A>(W, lane, la, r_at1, pix8, nn8, tw8, s0, s1, g8);
    if constexpr (MODE == 1) ring0 = ring_start_b<LEVEL, 4, 180, false, layer_offset_b(L_MLP0, LEVEL)>(W, la);
}

// SpatialEncoder 'rel_z_decay' (src/spatial.py:71-72, 109-117) in source-camera coordinates: the sample there ...
struct Cam3 { float x, y, z; };
__device__ __forceinline__ Cam3 to_source_camera(const VanerfFrame& F, float px, float py, float pz)
{
    Cam3 c;
    c.x = fmaf(pz, F.extrin[2], fmaf(py, F.extrin[1], px * F.extrin[0])) + F.extrin[3];
    c.y = fmaf(pz, F.extrin[6], fmaf(py, F.extrin[5], px * F.extrin[4])) + F.extrin[7];
    c.z = fmaf(pz, F.extrin[10], fmaf(py, F.extrin[9], px * F.extrin[8])) + F.extrin[11];
    return c;
}
// ... and the 7 positional-encoding features of key point i: dz, sin/cos(pi 2^l dz) for l = 0..2, all times the Gaussian decay.
// v_sin_f32 / v_cos_f32 take revolutions, so the arguments are dz/2, dz, 2dz exactly (|error| < 1.6e-7 absolute over
// the hand's extent, tools/probe_trig.hip).  Key points: split-bf16 from LDS (kp_lds: the lane half's table), fp32 through the scalar
// cache (wave-uniform addresses), selected per lane half.
template <int MODE> __device__ __forceinline__ void pe_features(const VanerfFrame& F, unsigned kp_lds, int h, const Cam3& c, int i, float (&feat)[PE_FEATS])
{
    float kx, ky, kz;
    if constexpr (MODE == 1) {
        const u32x4 k = *reinterpret_cast<const lds_u32x4_t*>((size_t)(kp_lds + 16u * i));
        kx = __uint_as_float(k.x); ky = __uint_as_float(k.y); kz = __uint_as_float(k.z);
    } else {
        const float4* __restrict__ kpg = reinterpret_cast<const float4*>(F.kpt_cam);
        const float4 k0 = kpg[i], k1 = kpg[PE_KPT_PER_HALF + i];
        kx = h ? k1.x : k0.x; ky = h ? k1.y : k0.y; kz = h ? k1.z : k0.z;
    }
    const float ddx = c.x - kx, ddy = c.y - ky, ddz = c.z - kz;
    const float d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
    const float wk = __expf(-d2 * F.pe_inv_2sigma2);
    const float dz = F.pe_scale * ddz;
    const float s0 = __builtin_amdgcn_sinf(0.5f * dz), c0 = __builtin_amdgcn_cosf(0.5f * dz);
    const float s1 = __builtin_amdgcn_sinf(dz), c1 = __builtin_amdgcn_cosf(dz);
    const float s2 = __builtin_amdgcn_sinf(2.0f * dz), c2 = __builtin_amdgcn_cosf(2.0f * dz);
    feat[0] = dz * wk; feat[1] = s0 * wk; feat[2] = c0 * wk; feat[3] = s1 * wk; feat[4] = c1 * wk;
    feat[5] = s2 * wk; feat[6] = c2 * wk;
}

// ---- mlp_geo.layers1 (src/utils.py:822-852): [PE294 | geo64] -> 128 -> 128 -> [. | geo8] -> 120 -> 64 ----
// mlp0, fp32 form: the 7 features of key point i (one per lane half) are k-steps 7i..7i+6, their fragments ring slots 0..6
__device__ __forceinline__ void mlp0_f32(const VanerfFrame& F, WRsrc W, const LLane& la, int h, float one_h0, float px, float py, float pz,
                                         Mlp0RingF& ring0, const f32x16 (&g64)[2], f32x16 (&a0)[4])
{
    constexpr unsigned base0 = layer_offset(L_MLP0);
    constexpr int D0 = PE_FEATS;
    const unsigned v4 = lane_of(la) * 16u; // byte offset of the lane in a 4-block fp32 fragment
    zero<4>(a0);
    const Cam3 c = to_source_camera(F, px, py, pz);
    // fully unrolled: as a run-time loop hipcc hoists the seven prefetch loads of an iteration above its first use and
    // waits vmcnt(0) (no prefetch left), and copies the 64 accumulator registers around the back edge
    static_for<PE_KPT_PER_HALF>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        float feat[PE_FEATS];
        pe_features<0>(F, 0u, h, c, i, feat);
        static_for<D0>([&](auto fc) {
            constexpr int f = decltype(fc)::value;
            const WFrag<4> a = ring0.f[f];
            // step 7(i+1)+f; after the last key point these are the first steps of the chain part below
            ring0.f[f] = wload<4>(W, (base0 + ((i + 1) * D0 + f) * 256) * 4u, v4);
            spill_x<L_MLP0, i * D0 + f>(la, feat[f]);
            mfma_step<4>(a0, a, feat[f]);
        });
    });
    constexpr unsigned nextp = base0 + (PE_KPT_PER_HALF + 1) * D0 * 256;
    // remaining 32 + 1 steps: geo64 (two blocks) and the bias; ring slot = step % 7 (147 = 21 * 7)
    constexpr int TREM = 33;
    static_for<TREM>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        const float b = chain<32>(g64, tc, one_h0);
        const WFrag<4> a = ring0.f[t % D0];
        if constexpr (t + D0 < TREM) ring0.f[t % D0] = wload<4>(W, (nextp + t * 256) * 4u, v4);
        spill_x<L_MLP0, PE_KPT_PER_HALF * D0 + t>(la, b);
        mfma_step<4>(a0, a, b);
    });
}

// mlp0, split-bf16 form: k-pairs 0..146 are the features (pair 7i+f = feature f of key point i), 147..178 the geo64 chain,
// 179 the bias.  A bf16 step takes 8 consecutive pairs, so key point i is computed right before the first step
// that needs it (at most two key points are live at a time).
// (lean: the geo pairs hold the folded matrix and read the scale's hidden layer through its ReLU)
template <int LEVEL>
__device__ __forceinline__ void mlp0_b(const VanerfFrame& F, WRsrc W, const LAddr& la, unsigned kp_lds, int h, float one_h0, float px, float py, float pz,
                                       RingB<4>& ring0, const f32x16 (&g64)[2], f32x16 (&a0)[4])
{
    zero<4>(a0);
    const Cam3 c = to_source_camera(F, px, py, pz);
    float feat[PE_KPT_PER_HALF][PE_FEATS];
    run_layer_b<LEVEL, 4, 180, false, layer_offset_b(L_MLP0, LEVEL)>(a0, ring0, W, la,
        [&](auto tc) -> float {
            constexpr int t = decltype(tc)::value;
            if constexpr (t < 147) return feat[t / 7][t % 7];
            else if constexpr (LEVEL >= 2 && t < 179) return lazy_act<1, ACT_RELU>(g64[(t - 147) / 16][(t - 147) % 16]);
            else return chain<32>(g64, std::integral_constant<int, t - 147>{}, one_h0);
        },
        [&](auto sc) {
            constexpr int s_ = decltype(sc)::value;
            constexpr int lo_k = s_ == 0 ? 0 : (8 * s_ - 1) / 7 + 1, hi_k = (8 * s_ + 7) / 7; // key points first needed by this step
            constexpr int last_k = hi_k < PE_KPT_PER_HALF ? hi_k : PE_KPT_PER_HALF - 1;
            static_for<(last_k - lo_k + 1 < 0 ? 0 : last_k - lo_k + 1)>([&](auto dc) {
                constexpr int i = lo_k + decltype(dc)::value;
                pe_features<1>(F, kp_lds, h, c, i, feat[i]);
            });
        });
}

// mlp1 .. mlp3.  a0: mlp0's output, then mlp2's; g8: the second scale; xv: the latent of mlp_geo.layers1
template <int MODE, int LEVEL>
__device__ __forceinline__ void mlp123(WRsrc W, const typename LaneSel<MODE>::type& la, int h, float one_h0, f32x16 (&a0)[4], const f32x16 (&g8)[1],
                                       f32x16 (&xv)[2])
{
    constexpr int T_MLP1 = kT_b(L_MLP1, LEVEL); // (lean: no bias k-pair, the accumulator starts from the bias table)
    auto r1 = ring_start_m<MODE, LEVEL, 4, T_MLP1, L_MLP1>(W, la);
    if constexpr (MODE == 0) softplus<4>(a0);
    f32x16 a1[4];
    if constexpr (LEVEL >= 2) load_bias<L_MLP1, 4>(h, a1);
    else zero<4>(a1);
    run_layer_m<MODE, LEVEL, 4, T_MLP1, L_MLP1>(a1, r1, W, la, [&](auto tc) -> float { return chain_sp<MODE, 64>(a0, tc, one_h0); });
    auto r2 = ring_start_m<MODE, LEVEL, 4, 69, L_MLP2>(W, la);
    if constexpr (MODE == 0) softplus<4>(a1);
    zero<4>(a0);
    run_layer_m<MODE, LEVEL, 4, 69, L_MLP2>(a0, r2, W, la, [&](auto tc) -> float {
        constexpr int t = decltype(tc)::value;
        if constexpr (t < 64) return lazy_act<MODE, ACT_SOFTPLUS>(a1[t / 16][t % 16]);
        else if constexpr (t < 68) return LEVEL >= 2 ? lazy_act<MODE, ACT_RELU>(g8[0][t - 64]) : g8[0][t - 64];
        else return one_h0;
    });
    auto r3 = ring_start_m<MODE, LEVEL, 2, 61, L_MLP3>(W, la);
    if constexpr (MODE == 0) softplus<4>(a0);
    zero<2>(xv);
    run_layer_m<MODE, LEVEL, 2, 61, L_MLP3>(xv, r3, W, la, [&](auto tc) -> float { return chain_sp<MODE, 60>(a0, tc, one_h0); });
}

// ---- PoolModule mean/var over V = 1 views (src/utils.py:744-779, 854-880): pool = [mean64 | var64] ----
template <int MODE> __device__ __forceinline__ void pool_mean_var(const typename LaneSel<MODE>::type& la, float pw, const f32x16 (&xv)[2], f32x16 (&pool)[4])
{
    if constexpr (MODE == 0)
        static_for<32>([&](auto rc) { constexpr int r = decltype(rc)::value; spill_aux<AUX_XV + r>(la, xv[r / 16][r % 16]); });
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float m = pw * xv[b][r];
            float d = xv[b][r] - m;
            pool[b][r] = m;
            pool[2 + b][r] = pw * (d * d);
        }
}

// ---- mlp_geo.layers2: 128 -> 64 -> 64 -> 2 (src/utils.py:709-719); rh0: the first layer's ring, started ahead of the pooling ----
template <int MODE, int LEVEL>
__device__ __forceinline__ void head_layers(WRsrc W, const typename LaneSel<MODE>::type& la, int h, float one_h0, typename RingSel<MODE, 2>::type& rh0,
                                            const f32x16 (&pool)[4], f32x16 (&head)[1])
{
    constexpr int T_HEAD0 = kT_b(L_HEAD0, LEVEL), T_HEAD1 = kT_b(L_HEAD1, LEVEL), T_HEAD2 = kT_b(L_HEAD2, LEVEL);
    f32x16 m0[2], m1[2];
    if constexpr (LEVEL >= 2) load_bias<L_HEAD0, 2>(h, m0);
    else zero<2>(m0);
    run_layer_m<MODE, LEVEL, 2, T_HEAD0, L_HEAD0>(m0, rh0, W, la, [&](auto tc) -> float { return chain<64>(pool, tc, one_h0); });
    static_assert(LDS_FIRST<LEVEL> == L_HEAD2 + 1 || LDS_FIRST<LEVEL> == L_HEAD0 + 1, "the ring is closed behind its last streamed layer");
    if constexpr (MODE == 1 && LDS_FIRST<LEVEL> == L_HEAD0 + 1) ring_close<LEVEL>(W, la);
    auto rh1 = ring_start_m<MODE, LEVEL, 2, T_HEAD1, L_HEAD1>(W, la);
    if constexpr (MODE == 0) softplus<2>(m0);
    if constexpr (LEVEL >= 2) load_bias<L_HEAD1, 2>(h, m1);
    else zero<2>(m1);
    run_layer_m<MODE, LEVEL, 2, T_HEAD1, L_HEAD1>(m1, rh1, W, la, [&](auto tc) -> float { return chain_sp<MODE, 32>(m0, tc, one_h0); });
    auto rh2 = ring_start_m<MODE, LEVEL, 1, T_HEAD2, L_HEAD2>(W, la);
    if constexpr (MODE == 0) softplus<2>(m1);
    if constexpr (LEVEL >= 2) load_bias<L_HEAD2, 1>(h, head);
    else zero<1>(head);
    run_layer_m<MODE, LEVEL, 1, T_HEAD2, L_HEAD2>(head, rh2, W, la, [&](auto tc) -> float { return chain_sp<MODE, 32>(m1, tc, one_h0); });
    if constexpr (MODE == 1 && LDS_FIRST<LEVEL> == L_HEAD2 + 1) ring_close<LEVEL>(W, la);
}

// ---- ibr_compress_gfeat 128 -> 24 (src/model.py:921); r_ta: the ring of the texture branch's first layer, started here ----
template <int MODE, int LEVEL>
__device__ __forceinline__ void ibr_compress(WRsrc W, const typename LaneSel<MODE>::type& la, int h, float one_h0, bool any_valid, const f32x16 (&pool)[4],
                                             f32x16 (&lat)[1], typename RingSel<MODE, 3>::type& r_ta)
{
    constexpr int T_IBR = kT_b(L_IBR, LEVEL), T_TEX_AT = kT_b(L_TEX_AT_A, LEVEL);
    if (MODE == 1 && !any_valid) {
        // all-invalid group: the pooled latent is exactly zero, the layer returns its bias -- the block's constant (same chain, same bits)
        r_ta = ring_start_m<MODE, LEVEL, 3, T_TEX_AT, L_TEX_AT_A>(W, la);
        if constexpr (MODE == 1)
            static_for<16>([&](auto rc) { constexpr int r = decltype(rc)::value; lat[0][r] = __uint_as_float(reinterpret_cast<const lds_u32_t*>((size_t)LDS_LAT0)[h * 16 + r]); });
    } else {
        auto r_ibr = ring_start_m<MODE, LEVEL, 1, T_IBR, L_IBR>(W, la);
        r_ta = ring_start_m<MODE, LEVEL, 3, T_TEX_AT, L_TEX_AT_A>(W, la);
        if constexpr (LEVEL >= 2) load_bias<L_IBR, 1>(h, lat);
        else zero<1>(lat);
        run_layer_m<MODE, LEVEL, 1, T_IBR, L_IBR>(lat, r_ibr, W, la, [&](auto tc) -> float { return chain<64>(pool, tc, one_h0); });
    }
}

// ---- TexVisFusion per-sample part (src/networks.py:281-293): both gated layers and the six gates ----
// vp: hoisted kernels, the ungated first layer starts from P[i], the two vertex rows' share of it, and runs [query6 | latent12 | 2 visibility pairs]
template <int MODE, int LEVEL>
__device__ __forceinline__ void tex_vis_fusion(WRsrc W, const typename LaneSel<MODE>::type& la, const float* vp, int h, int nn_idx, float q_vis, float vis_nn,
                                               float vis_tw, float (&row)[32], const float (&qi)[4], const float (&qt)[8], const f32x16 (&lat)[1],
                                               typename RingSel<MODE, 3>::type& r_ta, f32x16 (&rgb)[1])
{
    constexpr bool HOIST = LEVEL >= 1, LEAN = LEVEL >= 2;
    constexpr int T_TEX_AT = kT_b(L_TEX_AT_A, LEVEL), T_TEX = kT_b(L_TEX_A, LEVEL);
    float q[6];
    q[0] = h ? qt[3] : qi[0]; q[1] = h ? qt[4] : qi[1]; q[2] = h ? qt[5] : qi[2];
    q[3] = h ? qt[6] : qt[0]; q[4] = h ? qt[7] : qt[1]; q[5] = h ? (LEAN ? vis_tw : 0.0f) : qt[2]; // (lean: k-pair (qt[2] | vis_twin))
    const float t0 = h ? vis_nn : q_vis; // k-pair (qvis | vis_nn)
    [[maybe_unused]] const float t1 = h ? 0.0f : vis_tw;  // k-pair (vis_twin | -) (not in the lean stream)
    f32x16 latg = lat[0];
    auto tex_in = [&](auto tc) -> float {
        constexpr int t = decltype(tc)::value;
        if constexpr (t < 29) return row[t];
        else if constexpr (t < 35) return q[t - 29];
        else if constexpr (t < 47) return latg[t - 35];
        else if constexpr (t == 47) return t0;
        else { static_assert(!LEAN || t < 48, "the lean stream has no (vis_twin | -) pair"); return t1; }
    };
    auto from_ta = [&](auto& ta_) { return [&](auto tc) -> float { constexpr int t = decltype(tc)::value; return lazy_act<MODE, ACT_RELU>(ta_[t / 16][t % 16]); }; };
    auto tex_at_in = [&](auto tc) -> float {
        constexpr int t = decltype(tc)::value;
        if constexpr (!HOIST) return tex_in(tc);
        else if constexpr (t < 6) return q[t];
        else if constexpr (t < 18) return latg[t - 6];
        else if constexpr (t == 18) return t0;
        else { static_assert(!LEAN || t < 19, "the lean stream has no (vis_twin | -) pair"); return t1; }
    };
    f32x16 ta[3];
    if constexpr (HOIST) load_acc<3>(vp + VP_P, (unsigned)(nn_idx * (int)VP_P_ROW + 48 * h), ta);
    else zero<3>(ta);
    run_layer_m<MODE, LEVEL, 3, T_TEX_AT, L_TEX_AT_A>(ta, r_ta, W, la, tex_at_in);
    auto r_tg = ring_start_m<MODE, LEVEL, 1, 48, L_TEX_AT_B>(W, la);
    if constexpr (MODE == 0) relu<3>(ta);
    f32x16 tg[1];
    zero<1>(tg);
    run_layer_m<MODE, LEVEL, 1, 48, L_TEX_AT_B>(tg, r_tg, W, la, from_ta(ta));
    auto r_tb = ring_start_m<MODE, LEVEL, 3, T_TEX, L_TEX_A>(W, la);
    // six gates: rows 0..3 -> h = 0 lanes regs 0..3, rows 4,5 -> h = 1 lanes regs 0,1
    float m0 = sigmoid_f(tg[0][0]), m1 = sigmoid_f(tg[0][1]), m2 = sigmoid_f(tg[0][2]), m3 = sigmoid_f(tg[0][3]);
    float o0 = __shfl_xor(m0, 32), o1 = __shfl_xor(m1, 32), o2 = __shfl_xor(m2, 32);
    const float gq = h ? o0 : m0;     // gate 0: query feature
    const float g11 = h ? o2 : m1;    // gate 1 (nearest) / gate 2 (twin): [img3|tex8]
    const float ggf = h ? m0 : m3;    // gate 3 (nearest) / gate 4 (twin): global feature
    const float glat = h ? m1 : o1;   // gate 5: compressed latent
    if constexpr (MODE == 0) {
        spill_aux<AUX_TEX>(la, gq); spill_aux<AUX_TEX + 1>(la, g11); spill_aux<AUX_TEX + 2>(la, ggf); spill_aux<AUX_TEX + 3>(la, glat);
        static_for<12>([&](auto rc) { constexpr int r = decltype(rc)::value; spill_aux<AUX_LAT + r>(la, lat[0][r]); });
    }
#pragma unroll
    for (int t = 0; t < 11; ++t) row[t] *= g11;
#pragma unroll
    for (int t = 11; t < 29; ++t) row[t] *= ggf;
#pragma unroll
    for (int t = 0; t < (LEAN ? 5 : 6); ++t) q[t] *= gq;
    if constexpr (LEAN) q[5] = h ? q[5] : q[5] * gq; // the h = 1 half of the merged pair is vis_twin: not gated
#pragma unroll
    for (int r = 0; r < 12; ++r) latg[r] = lat[0][r] * glat;
    zero<3>(ta);
    run_layer_m<MODE, LEVEL, 3, T_TEX, L_TEX_A>(ta, r_tb, W, la, tex_in);
    auto r_rgb = ring_start_m<MODE, LEVEL, 1, 48, L_TEX_B>(W, la);
    if constexpr (MODE == 0) relu<3>(ta);
    zero<1>(rgb);
    run_layer_m<MODE, LEVEL, 1, 48, L_TEX_B>(rgb, r_rgb, W, la, from_ta(ta));
}

// ---- eval_func (src/model.py:1140-1160): rows 0,1 of the head / 0..2 of the colour live in the h = 0 lanes ----
__device__ __forceinline__ void store_sample(const QueryParams& P, bool live, int h, long long s, float mask, const f32x16 (&head)[1], const f32x16 (&rgb)[1])
{
    if (live && h == 0) {
        float rad = head[0][1];
        if (P.noise) rad += P.noise[s];
        float* o = P.out + 5 * s;
        o[0] = P.raw ? head[0][0] : mask * fmaxf(rad, 0.0f);
        o[1] = P.raw ? head[0][1] : mask * head[0][0] + (1.0f - mask) * P.f.invalid_sdf;
        o[2] = rgb[0][0];
        o[3] = rgb[0][1];
        o[4] = rgb[0][2];
        if (P.valid) P.valid[s] = mask > 0.0f;
    }
}

// The kernel: the round's protocol and the stages above in sequence.
// Work distribution.  A block claims one 32-sample group per wave and round from a device-scope counter (wave w takes group
// base + w) and its waves meet at one barrier per round: they walk the weight stream together -- in the fp32 kernel three of the four
// fetches of every fragment hit the CU's L1 instead of L2 (launch 7.6 -> 6.8 ms; with per-wave claims the waves drift apart and every wave
// streams the 660 KB from L2 on its own), in the split-bf16 kernel the eight waves share one copy in the LDS ring.  The claim for round r + 2
// is issued at the start of round r (thread 0) and published through LDS at the start of round r + 1: no wave waits for the atomic.  The same
// barrier makes the "no valid sample" decision block-uniform, which is what allows barriers inside the layer stack.  Every block leaves the
// loop once the counter passes ngroups: the grid always drains.
// The short path.  A sample whose projection misses the source view / foreground mask has pixel weight 0: its pooled latent is exactly
// zero (0 * x), the density head is masked out by eval_func and only the colour branch (fed by the bias of
// ibr_compress) survives.  When ALL 32 samples of the wave are such samples, GeoVisFusion, mlp_geo.layers1 and the head
// (82 % of the MFMAs) are skipped -- same bits, wave-uniform branch.  With real foreground masks most samples are.
// The hand-over (HANDOVER: the launch has a validity partition and query_short_kernel stands behind it on the stream).  The partition puts the
// all-invalid groups behind the others, so behind the first all-invalid round of ANY block every round is all-invalid.  A block that meets such
// a round records its base in the second word of the launch's queue -- atomicMax of the complement: the word ends as ~(smallest base) and stays 0
// when no block met one -- and leaves; all of its waves leave together (the decision is block-uniform), so the barriers stay matched.  Every
// round in front of the smallest recorded base was claimed by a block that ran it in full; query_short_kernel runs every group from that base on.
template <int MODE, bool SPILL = false, int LEVEL = 0, bool HANDOVER = false>
__global__ __launch_bounds__(64 * WPB<MODE>, SPILL ? WAVES_PER_SIMD_SPILL : WAVES_PER_SIMD) void query_kernel(const QueryParams P)
{
    static_assert(!SPILL || MODE == 0, "the training spill runs on the fp32 kernel");
    static_assert(!HANDOVER || LEVEL >= 2, "the short-only kernel exists at the lean level (it serves the texel level as it stands)");
    static_assert(LEVEL >= 0 && LEVEL <= 3 && (LEVEL == 0 || MODE == 1), "only the split-bf16 kernel has a hoisted, a lean and a texel variant");
    constexpr bool HOIST = LEVEL >= 1;
    constexpr int WAVES_PER_BLOCK = WPB<MODE>;
    const int lane_k = threadIdx.x & 63;
    [[maybe_unused]] const int lane = lane_k, j = lane & 31; // (shadowed inside the sample loop)
    [[maybe_unused]] const long long wave = (long long)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6); // STAMPS builds
    const long long ngroups = (P.n + 31) / 32;
    const VanerfFrame& F = P.f;
    const WRsrc W = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P.w), 0, P.wbytes, 0x00020000); // kernarg-derived: wave-uniform
    [[maybe_unused]] WRsrc xs_rs = W, aux_rs = W; // spill mode: the two spills as buffers of their exact sizes (the host checks they stay below 4 GB)
    if constexpr (SPILL) {
        xs_rs = __builtin_amdgcn_make_buffer_rsrc(P.xs, 0, (unsigned)(X_ROWS * 4ll * P.npad), 0x00020000);
        aux_rs = __builtin_amdgcn_make_buffer_rsrc(P.aux, 0, (unsigned)(AUX_ROWS * 4ll * P.npad), 0x00020000);
    }
#ifdef VANERF_STAMPS
    unsigned long long phase_cycles[N_PHASES] = {};
    unsigned long long t_prev, rt0;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt0)::"memory");
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_prev)::"memory");
#endif
    if constexpr (MODE == 1) key_points_to_lds(F);
    unsigned short_groups = 0;
    // control words in LDS: fp32 kernel static, split-bf16 kernel inside its dynamic region (see the LDS map in bf16x3_ring.h)
    __shared__ unsigned s_ctrl0[MODE == 0 ? 2 + 2 * WAVES_PER_BLOCK : 1];
    auto s_base = [&](unsigned i) -> auto& { if constexpr (MODE == 0) return s_ctrl0[i]; else return lds_ctrl()[i]; };
    auto s_valid = [&](unsigned pp, unsigned k) -> auto& { if constexpr (MODE == 0) return s_ctrl0[2 + pp * WAVES_PER_BLOCK + k]; else return lds_ctrl()[2 + pp * WAVES_PER_BLOCK + k]; };
    const unsigned wv = threadIdx.x >> 6;
    [[maybe_unused]] const unsigned wv_u = (unsigned)__builtin_amdgcn_readfirstlane((int)wv); // the same in a scalar register
    unsigned pending = 0, par = 1;
    if (threadIdx.x == 0) s_base(0) = atomicAdd(P.queue, (unsigned)WAVES_PER_BLOCK);
    if constexpr (MODE == 1) fill_lds<LEVEL>(P, W, lane, wv_u);
    __syncthreads();
    if constexpr (MODE == 1) {
        short_path_latent<LEVEL>(W, lane, wv_u);
        __syncthreads();
    }
    unsigned base_cur = s_base(0);
    if (threadIdx.x == 0) pending = atomicAdd(P.queue, (unsigned)WAVES_PER_BLOCK);
    SampleIn in_next = fetch_sample(P, base_cur + wv, j);
    while (base_cur < (unsigned)ngroups) {
        const long long g = (long long)base_cur + wv; // a wave whose group lies beyond the last one runs with live == false: the block's barriers stay matched
        const SampleIn in = in_next;
        // split-bf16 kernel: the lane id and what follows from it are re-derived in every round (v_mbcnt, volatile), so that none of it is carried
        // around the loop in registers the 256-register budget does not have
        const int lane = MODE == 1 ? lane_id_fresh() : lane_k, j = lane & 31, h = lane >> 5;
        const float one_h0 = h ? 0.0f : 1.0f; // B operand of the bias k-step
        // the lane's fragment offsets, opaque per round (nothing derived from them is hoisted out of the loop and parked in registers)
        typename LaneSel<MODE>::type la;
        [[maybe_unused]] unsigned kp_lds = 0;
        if constexpr (MODE == 1) { la = make_laddr(lane, wv_u); kp_lds = LDS_KPT + ((la.w[0] >> 9) & 1u) * (PE_KPT_PER_HALF * 16u); }
        else la = make_llane<SPILL>(lane, xs_rs, aux_rs, P.npad, g, ngroups);
        const long long s_raw = g * 32 + j;
        const bool live = s_raw < P.n;
        long long s = live ? s_raw : P.n - 1;
        if (P.order) s = P.order[s];
        const float px = in.px, py = in.py, pz = in.pz;
        const float q_sdf = in.sdf;
        const float q_vis = in.vis ? 1.0f : 0.0f;
        // ---- projection into the source view, validity mask, boundary weight (src/model.py:780-821) ----
        const Projected pr = project_and_mask(F, P.wm1[0], P.hm1[0], px, py, pz);
        const float x = pr.x, y = pr.y, mask = pr.mask;
        const bool wave_valid = __builtin_amdgcn_ballot_w64(mask > 0.0f) != 0ull;
        if (lane == 0) s_valid(par, wv) = wave_valid ? 1u : 0u;
        if (threadIdx.x == 0) s_base(par) = pending;
        block_barrier_lds();
        const unsigned base_next = (unsigned)__builtin_amdgcn_readfirstlane((int)s_base(par));
        unsigned anyv = 0;
#pragma unroll
        for (int k = 0; k < WAVES_PER_BLOCK; ++k) anyv |= s_valid(par, k);
        const bool any_valid = SPILL || __builtin_amdgcn_readfirstlane((int)anyv) != 0; // (spill mode: every group writes every row)
        if constexpr (HANDOVER) {
            if (!any_valid) { // this round and every round behind it belong to query_short_kernel
                if (threadIdx.x == 0) atomicMax(P.queue + 1, ~base_cur);
                break;
            }
        }
        par ^= 1u;
        if (threadIdx.x == 0) pending = atomicAdd(P.queue, (unsigned)WAVES_PER_BLOCK);
        in_next = fetch_sample(P, base_next + wv, j);
        base_cur = base_next;
        __builtin_amdgcn_sched_barrier(0x000F); // keep these loads here (the scheduler sinks loads to their first use)
        const Bilin bi = bilin_setup(x, y, F.hi, F.wi, P.wm1[0], P.hm1[0]); // source-image taps (the same the mask used)
        const float pw = boundary_weight(pr);
        if constexpr (MODE == 0) spill_aux<AUX_PW>(la, pw);
        STAMP(0); // front end
        // ---- 1-NN vertex (src/networks.py:27-33): found by vanerf_mesh_query_accel (same pass as the SDF) ----------
        const int nn_idx = in.knn;
        const int tw_idx = nn_idx >= VANERF_NV_HAND ? nn_idx - VANERF_NV_HAND : nn_idx + VANERF_NV_HAND;
        const float vis_nn = ld_off<float>(F.vert_vis, 4u * nn_idx), vis_tw = ld_off<float>(F.vert_vis, 4u * tw_idx);
        const float sc0 = h ? q_vis : q_sdf;   // k-pair (sdf | qvis)
        const float sc1 = h ? vis_tw : vis_nn; // k-pair (vis_nn | vis_twin)
        STAMP(1); // 1-NN
        // ---- GeoVisFusion (src/networks.py:75-106) ---------------------------------------------------------
        // Every layer's fragment ring is started ahead of the previous layer's epilogue (see ring_start).  The fp32 kernel issues the gathers
        // of the second scale and of the texture branch early, so that their L2 latency hides behind the layers in front of them; the
        // split-bf16 kernel has no registers to park them in and issues them where they are consumed (the partner wave hides the latency).
        float row[32], qi[4], qt[8]; // the texture branch's inputs (tex_gathers)
        f32x16 pool[4], head[1];
        if (any_valid) {
            auto r_at0 = ring_start_m<MODE, LEVEL, 1, kT_b(L_GEO_AT0_A, LEVEL), L_GEO_AT0_A>(W, la);
            f32x16 g64[2], g8[1]; // the outputs of the two GeoVisFusion scales (lean kernel: their hidden layers `mid` before the ReLU)
            float pix8[4], nn8[4], tw8[4];
            {
                float pix[32], nn[32], tw[32];
                [[maybe_unused]] float a0s[8];
                geo0_gathers<HOIST, LEVEL == 3>(P, x, y, h, nn_idx, tw_idx, pix, nn, tw, a0s);
                if constexpr (MODE == 0) geo1_gathers(P, x, y, h, nn_idx, tw_idx, pix8, nn8, tw8);
                STAMP(2); // geo gathers
                if constexpr (HOIST) geo_scale0_vp<MODE, LEVEL>(W, lane, la, r_at0, pix, a0s, nn, tw, sc0, sc1, g64);
                else geo_scale<MODE, LEVEL, 32, 2, 16, L_GEO_AT0_A>(W, lane, la, r_at0, pix, nn, tw, sc0, sc1, g64);
                if constexpr (MODE == 1) geo1_gathers(P, x, y, h, nn_idx, tw_idx, pix8, nn8, tw8);
                STAMP(3); // geo0 layers
            }
            Mlp0Ring<MODE> ring0;
            geo_scale1<MODE, LEVEL>(W, lane, la, pix8, nn8, tw8, sc0, sc1, g8, ring0);
            STAMP(4); // geo1
            f32x16 xv[2];
            {
                f32x16 a0[4];
                if constexpr (MODE == 0) mlp0_f32(F, W, la, h, one_h0, px, py, pz, ring0, g64, a0);
                else mlp0_b<LEVEL>(F, W, la, kp_lds, h, one_h0, px, py, pz, ring0, g64, a0);
                STAMP(5); // mlp0 (PE + geo64)
                mlp123<MODE, LEVEL>(W, la, h, one_h0, a0, g8, xv);
            }
            STAMP(6); // softplus x3 + mlp1..3
            if constexpr (MODE == 0) tex_gathers(P, x, y, bi, h, nn_idx, tw_idx, row, qi, qt); // ~2 layers before the texture branch needs them
            auto rh0 = ring_start_m<MODE, LEVEL, 2, kT_b(L_HEAD0, LEVEL), L_HEAD0>(W, la);
            pool_mean_var<MODE>(la, pw, xv, pool);
            head_layers<MODE, LEVEL>(W, la, h, one_h0, rh0, pool, head);
        } else {
            if constexpr (MODE == 0) tex_gathers(P, x, y, bi, h, nn_idx, tw_idx, row, qi, qt);
            zero<4>(pool);
            zero<1>(head);
        }
        if (!wave_valid && lane == 0 && g < ngroups) ++short_groups; // counted by the wave's own samples (what bench.py prices), not by the block's path
        if constexpr (MODE == 1) tex_gathers(P, x, y, bi, h, nn_idx, tw_idx, row, qi, qt);
        STAMP(7); // pool + head
        f32x16 lat[1];
        typename RingSel<MODE, 3>::type r_ta;
        ibr_compress<MODE, LEVEL>(W, la, h, one_h0, any_valid, pool, lat, r_ta);
        STAMP(8); // ibr
        f32x16 rgb[1];
        tex_vis_fusion<MODE, LEVEL>(W, la, P.vp, h, nn_idx, q_vis, vis_nn, vis_tw, row, qi, qt, lat, r_ta, rgb);
        STAMP(9); // tex
        // split-bf16 kernel: the DMA this wave issued in the round's last phase (phase 0 of the next full round) has landed before the wave reaches
        // the next top-of-round barrier -- waited for here, ahead of the stores, where nothing younger is in flight
        if constexpr (MODE == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        store_sample(P, live, h, s, mask, head, rgb);
        STAMP(10); // store
    }
    if (P.short_groups && (MODE == 1 ? lane_id_fresh() : lane) == 0 && short_groups) atomicAdd(P.short_groups, (unsigned long long)short_groups);
#ifdef VANERF_STAMPS
    unsigned long long rt1;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt1)::"memory");
    phase_cycles[N_PHASES - 1] = rt1 - rt0; // 100 MHz reference clock over the same span: clock = sum(phases) / this * 100 MHz
    if (P.stamps && lane == 0)
        for (int k = 0; k < N_PHASES; ++k) P.stamps[wave * N_PHASES + k] = phase_cycles[k];
#endif
}

// The short-only kernel: the all-invalid groups a HANDOVER launch of query_kernel<1, false, LEVEL> left behind, from group ~queue[1] on.  It is
// the round of query_kernel with any_valid == false as a constant -- the same stages with the same arguments in the same order, so the same bits
// -- in a shape of its own: nothing of the full path is compiled in, so the stages fit 168 registers and TWELVE waves share the block's one
// LDS copy (the SHORT map, bf16x3_ring.h) -- three waves per SIMD to hide the gathers and the dependent ds_read_b128s of a latency-bound path,
// where the full kernel's shape has two, which run the same gathers at the same moment.  (Sixteen waves at 128 registers put 46 of them in
// scratch: TexVisFusion's second layer holds 48 accumulators, 32 row values and its fragments at once.)  No ring, no phase barriers, no queue:
// the range is known at launch and its groups cost the same, so they are dealt statically -- wave w of block b takes groups
// start + 12 (b + k gridDim) + w.
// Every group it executes is a short group (the counter bench.py prices FLOPs with): with the full kernel's count, the parent's number.
template <int LEVEL>
__global__ __launch_bounds__(64 * SHORT_WAVES) void query_short_kernel(const QueryParams P)
{
    static_assert(LEVEL == 2, "the lean level (the hoisted level's stages need 5 registers more than three waves per SIMD have: it keeps the in-kernel short path)");
    const unsigned word = P.queue[1];
    if (word == 0u) return; // no block of the full kernel met an all-invalid round
    const long long ngroups = (P.n + 31) / 32;
    const long long first = (long long)(~word) + (long long)SHORT_WAVES * blockIdx.x; // the block's first group
    if (first >= ngroups) return; // no work: before the LDS fill
    const VanerfFrame& F = P.f;
    const WRsrc W = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P.w), 0, P.wbytes, 0x00020000);
    const unsigned wv_u = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    resident_to_lds<LEVEL, SHORT_BASE_DW<LEVEL>, SHORT_RES_DW<LEVEL>, SHORT_LDS_RES<LEVEL>, 64 * SHORT_WAVES>(P);
    __syncthreads();
    short_path_latent<LEVEL>(W, (int)(threadIdx.x & 63), wv_u);
    __syncthreads();
    unsigned short_groups = 0;
    long long g = first + wv_u;
    // the slot's sample (a hand-over launch has a partition): fetched one group ahead -- the index only, one register; the full kernel's six
    // inputs ahead do not fit the register budget here, and the waves of a SIMD hide the one level of latency that is left
    auto slot_sample = [&](long long grp, int j) -> int {
        const long long sr = (grp < ngroups ? grp : ngroups - 1) * 32 + j;
        return P.order[sr < P.n ? sr : P.n - 1];
    };
    int s_next = slot_sample(g, (int)(threadIdx.x & 31));
    for (; g < ngroups; g += (long long)SHORT_WAVES * gridDim.x) {
        const int lane = lane_id_fresh(), j = lane & 31, h = lane >> 5;
        const float one_h0 = h ? 0.0f : 1.0f;
        const LAddr la = make_laddr(lane, wv_u);
        const bool live = g * 32 + j < P.n;
        const int s = s_next; // (a lane beyond n: the last slot's sample, not stored)
        const SampleIn in = fetch_at(P, s);
        s_next = slot_sample(g + (long long)SHORT_WAVES * gridDim.x, j);
        __builtin_amdgcn_sched_barrier(0x000F);
        const float px = in.px, py = in.py, pz = in.pz;
        const float q_vis = in.vis ? 1.0f : 0.0f;
        const Projected pr = project_and_mask(F, P.wm1[0], P.hm1[0], px, py, pz);
        const float x = pr.x, y = pr.y, mask = pr.mask;
        const Bilin bi = bilin_setup(x, y, F.hi, F.wi, P.wm1[0], P.hm1[0]);
        const int nn_idx = in.knn;
        const int tw_idx = nn_idx >= VANERF_NV_HAND ? nn_idx - VANERF_NV_HAND : nn_idx + VANERF_NV_HAND;
        const float vis_nn = ld_off<float>(F.vert_vis, 4u * nn_idx), vis_tw = ld_off<float>(F.vert_vis, 4u * tw_idx);
        float row[32], qi[4], qt[8];
        f32x16 pool[4], head[1];
        zero<4>(pool);
        zero<1>(head);
        if (lane == 0) ++short_groups;
        tex_gathers(P, x, y, bi, h, nn_idx, tw_idx, row, qi, qt);
        f32x16 lat[1];
        RingB<3> r_ta;
        ibr_compress<1, LEVEL>(W, la, h, one_h0, false, pool, lat, r_ta);
        f32x16 rgb[1];
        tex_vis_fusion<1, LEVEL>(W, la, P.vp, h, nn_idx, q_vis, vis_nn, vis_tw, row, qi, qt, lat, r_ta, rgb);
        store_sample(P, live, h, s, mask, head, rgb);
    }
    if (P.short_groups && lane_id_fresh() == 0 && short_groups) atomicAdd(P.short_groups, (unsigned long long)short_groups);
}

// ---- what the launch entries share: argument checks, the QueryParams of a launch, grid sizing, the launch itself ----
void check_queue_word(const char* who, const void* queue_word)
{
    if (!queue_word || (reinterpret_cast<uintptr_t>(queue_word) & 7u)) throw_error("%s: queue_word must be 8 bytes of device memory, 8-byte aligned", who);
}
void check_frame_pointers(const char* who, const VanerfFrame& f)
{
    if (!f.geo0 || !f.geo1 || !f.tex || !f.img || !f.mask || !f.verts || !f.vfeat0 || !f.vfeat1 || !f.vfeat_tex || !f.vert_vis || !f.kpt_cam)
        throw_error("%s: frame has a null pointer", who);
}

// The parameters every launch has; what only some have (noise, order, valid, stamps, short_groups, vp, the spills) starts out absent.
// The kernel runs on stream `s` of the handle; the lean kernel reads the bias table, which sits directly behind its stream, through the same buffer.
QueryParams query_params(const VanerfFrame& f, const VanerfWeights& w, Stream s, const float* pts, const float* query_sdf,
                         const uint8_t* query_vis, const int32_t* knn_idx, int raw, int64_t n, float* out)
{
    QueryParams P = {};
    P.f = f; P.w = w.stream[s]; P.wbytes = (unsigned)((w.words[s] + (s == STREAM_LEAN ? w.words[STREAM_LEAN_BIAS] : s == STREAM_TEXEL ? w.words[STREAM_TEXEL_BIAS] : 0)) * sizeof(float));
    P.pts = pts; P.qsdf = query_sdf; P.qvis = query_vis; P.knn_in = knn_idx; P.raw = raw; P.n = n; P.out = out;
    const int ws[4] = {f.wi, f.wt, f.w0, f.w1}, hs[4] = {f.hi, f.ht, f.h0, f.h1};
    for (int i = 0; i < 4; ++i) { P.wm1[i] = (float)(ws[i] - 1); P.hm1[i] = (float)(hs[i] - 1); }
    return P;
}

// One instantiation of query_kernel and the shape of its launch.  Blocks per CU follow from the kernel's waves per SIMD (four SIMDs per CU):
// fp32 two 4-wave blocks -- fp32 MFMA and fp32 VALU do not overlap on gfx950 (tools/probe_mfma_valu.hip: every VALU instruction adds its issue
// cycles to the MFMA time), so the second wave does not hide VALU work behind MFMAs; what it hides is load latency and the in-order issue gaps
// of its partner --, split-bf16 ONE 8-wave block (it owns the CU's LDS), spill build one 4-wave block (it takes the whole register file).
struct QueryLaunch { void (*kernel)(QueryParams); int wpb, blocks_per_cu; unsigned lds_bytes; };
template <int MODE, bool SPILL = false, int LEVEL = 0, bool HANDOVER = false> QueryLaunch query_launch()
{
    return {query_kernel<MODE, SPILL, LEVEL, HANDOVER>, WPB<MODE>, (SPILL ? WAVES_PER_SIMD_SPILL : WAVES_PER_SIMD) * 4 / WPB<MODE>, MODE == 1 ? DYN_LDS_BYTES<LEVEL> : 0u};
}

// persistent grid: one block per WPB groups, at most what the device holds at once (the blocks claim their groups from the queue word)
long long query_blocks(const QueryLaunch& L, int64_t n)
{
    const long long ngroups = (n + 31) / 32;
    int dev = 0, cus = 256;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    return std::min<long long>((ngroups + L.wpb - 1) / L.wpb, (long long)cus * L.blocks_per_cu);
}

void launch_kernel(const QueryLaunch& L, long long blocks, const QueryParams& P, void* stream)
{
    // the opt-in above 64 KB of dynamic LDS is per device: set on every call (cheap), as vanerf_mesh_query_accel does
    if (L.lds_bytes) HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(L.kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds_bytes));
    hipLaunchKernelGGL(L.kernel, dim3((unsigned)blocks), dim3(64 * L.wpb), L.lds_bytes, (hipStream_t)stream, P);
    HIP_CHECK(hipGetLastError());
}

// The launch's queue word is 8 bytes, zeroed here: the first 32-bit word is the work-queue head, the second the hand-over word of a HANDOVER
// launch (no other kernel reads or writes it: without a hand-over it stays 0).
void launch_query(const QueryLaunch& L, long long blocks, QueryParams& P, void* queue_word, void* stream)
{
    P.queue = static_cast<unsigned*>(queue_word); // the caller's word: no launch shares a queue head with another (any number in flight, any streams)
    HIP_CHECK(hipMemsetAsync(P.queue, 0, 8, (hipStream_t)stream));
    launch_kernel(L, blocks, P, stream);
}

// The short-only kernel behind a HANDOVER launch, same stream, same parameters: launched without knowing whether, or from where, there is work
// for it (no host synchronisation) -- it reads the hand-over word; 0 ends it at once.  One 12-wave block per CU, at most one per 12 groups.
template <int LEVEL> void launch_short(const QueryParams& P, void* stream)
{
    const QueryLaunch L = {query_short_kernel<LEVEL>, SHORT_WAVES, 1, DYN_LDS_BYTES<LEVEL>};
    launch_kernel(L, query_blocks(L, P.n), P, stream);
}

// VANERF_LEAN_STREAM (read at every launch, for tests and A/B runs): 0 = a bf16x3 handle with a table of vertex products runs the hoisted kernel
// instead of the lean one.  Unset or anything else: the lean kernel.
bool lean_stream_enabled()
{
    const char* e = std::getenv("VANERF_LEAN_STREAM");
    return !(e && e[0] == '0' && !e[1]);
}

// VANERF_SHORT_KERNEL (read at every launch, for tests and A/B runs): 0 = a launch with a validity partition stays ONE launch, its all-invalid
// groups on the short path inside the full kernel.  Unset or anything else: the hand-over to query_short_kernel.
bool short_kernel_enabled()
{
    const char* e = std::getenv("VANERF_SHORT_KERNEL");
    return !(e && e[0] == '0' && !e[1]);
}

// VANERF_TEXEL_PRODUCTS (read at every launch, for tests and A/B runs): 0 = the lean level even where the table holds the per-texel products.
bool texel_products_enabled()
{
    const char* e = std::getenv("VANERF_TEXEL_PRODUCTS");
    return !(e && e[0] == '0' && !e[1]);
}

} // namespace

// vertex_products: the frame's table from vanerf_vertex_products (built with the same handle, after its last update), or NULL.  With the
// table a bf16x3 handle runs the lean kernel on its lean stream (the hoisted kernel on the hoisted stream under VANERF_LEAN_STREAM=0); without
// it every handle runs the un-hoisted kernel of its mode.
extern "C" int vanerf_query_samples(const VanerfWeights* w, const VanerfFrame* frame, const float* pts, const float* query_sdf,
                                    const uint8_t* query_vis, const int32_t* knn_idx, const float* noise, const int32_t* order, int raw, int64_t n,
                                    float* out, uint8_t* valid, void* queue_word, const float* vertex_products, void* stream)
{
    return guarded([&] {
        if (n < 0) throw_error("vanerf_query_samples: n = %lld < 0", (long long)n);
        if (n == 0) return; // an empty batch is valid (and has null data pointers)
        if (!w || !w->block[BLOCK_MAIN] || !frame || !pts || !query_sdf || !query_vis || !knn_idx || !out) throw_error("vanerf_query_samples: null argument");
        check_queue_word("vanerf_query_samples", queue_word);
        if ((n + 31) / 32 >= 0xffffff00LL) throw_error("vanerf_query_samples: n = %lld too large for one launch", (long long)n);
        const VanerfFrame& f = *frame;
        check_frame_pointers("vanerf_query_samples", f);
        if (f.h0 < 1 || f.w0 < 1 || f.h1 < 1 || f.w1 < 1 || f.ht < 1 || f.wt < 1 || f.hi < 1 || f.wi < 1)
            throw_error("vanerf_query_samples: feature-map sizes must be positive");
        const bool hoist = vertex_products != nullptr;
        if (hoist && !w->stream[STREAM_HOISTED]) throw_error("vanerf_query_samples: a table of vertex products needs a bf16x3 weight handle");
        if (hoist && (reinterpret_cast<uintptr_t>(vertex_products) & 15u)) throw_error("vanerf_query_samples: the table must be 16-byte aligned");
        // the texel level: the table's per-texel part is filled for this frame (vanerf_vertex_products asked the same question of the same fields)
        const bool texel = hoist && w->stream[STREAM_TEXEL] && texel_products_fit(f.h0, f.w0) && lean_stream_enabled() && texel_products_enabled();
        const Stream s = !hoist ? forward_stream(w->mode) : texel ? STREAM_TEXEL : w->stream[STREAM_LEAN] && lean_stream_enabled() ? STREAM_LEAN : STREAM_HOISTED;
        QueryParams P = query_params(f, *w, s, pts, query_sdf, query_vis, knn_idx, raw, n, out);
        P.noise = noise; P.order = order; P.valid = valid; P.short_groups = w->stats; P.vp = vertex_products;
        // with a partition (`order`: vanerf_query_order's, the all-invalid groups last) the lean kernel hands those groups over
        const bool handover = order && (s == STREAM_LEAN || s == STREAM_TEXEL) && short_kernel_enabled();
        const QueryLaunch L = s == STREAM_TEXEL     ? (handover ? query_launch<1, false, 3, true>() : query_launch<1, false, 3>())
                              : s == STREAM_LEAN    ? (handover ? query_launch<1, false, 2, true>() : query_launch<1, false, 2>())
                              : s == STREAM_HOISTED ? query_launch<1, false, 1>()
                              : s == STREAM_BF16X3  ? query_launch<1>()
                                                    : query_launch<0>();
        launch_query(L, query_blocks(L, n), P, queue_word, stream);
        if (handover) { // the short path touches neither of the two shortened layers: the short-only kernel runs on the lean stream at either level
            if (s == STREAM_TEXEL) { const QueryParams lean = query_params(f, *w, STREAM_LEAN, pts, query_sdf, query_vis, knn_idx, raw, n, out); P.w = lean.w; P.wbytes = lean.wbytes; }
            launch_short<2>(P, stream);
        }
    });
}

// Training: the fp32 kernel in spill mode -- the same forward pass of N samples (raw outputs [sdf_pred, rad, r, g, b]),
// which also writes every layer's operands and a few auxiliary values for the fused backward chain (query_backward.hip); layouts in layer_spec.h.
extern "C" int vanerf_query_forward_spill(const VanerfWeights* w, const VanerfFrame* frame, const float* pts, const float* query_sdf,
                                          const uint8_t* query_vis, const int32_t* knn_idx, int64_t n, int64_t npad, float* out_raw, uint8_t* valid,
                                          float* xs, float* aux, void* queue_word, void* stream)
{
    return guarded([&] {
        if (n <= 0) throw_error("vanerf_query_forward_spill: n = %lld", (long long)n);
        if (!w || !w->stream[STREAM_FP32]) throw_error("vanerf_query_forward_spill: needs an fp32 weight handle (vanerf_weights_pack mode 0)");
        if (!frame || !pts || !query_sdf || !query_vis || !knn_idx || !out_raw || !xs || !aux) throw_error("vanerf_query_forward_spill: null argument");
        check_queue_word("vanerf_query_forward_spill", queue_word);
        if (npad < n || npad % 32 != 0) throw_error("vanerf_query_forward_spill: npad = %lld must be a multiple of 32 and >= n = %lld", (long long)npad, (long long)n);
        if ((long long)X_ROWS * 4 * npad >= (long long)SPILL_OFF)
            throw_error("vanerf_query_forward_spill: a block of %lld samples spills more than 4 GB (the kernels address the spills with 32-bit offsets): at most %lld",
                        (long long)npad, (long long)SPILL_OFF / (4 * X_ROWS) / 32 * 32);
        const VanerfFrame& f = *frame;
        check_frame_pointers("vanerf_query_forward_spill", f);
        QueryParams P = query_params(f, *w, STREAM_FP32, pts, query_sdf, query_vis, knn_idx, 1, n, out_raw);
        P.valid = valid; P.xs = xs; P.aux = aux; P.npad = npad;
        const QueryLaunch L = query_launch<0, true>();
        launch_query(L, query_blocks(L, n), P, queue_word, stream);
    });
}

#ifdef VANERF_STAMPS
// Diagnostic build: same launch with a per-wave phase-cycle table [waves][12] (device pointer, zero-initialised by the caller).
extern "C" int vanerf_debug_query_stamps(const VanerfWeights* w, const VanerfFrame* frame, const float* pts, const float* query_sdf,
                                         const uint8_t* query_vis, const int32_t* knn_idx, int64_t n, float* out, unsigned long long* stamps, int* n_waves, void* queue_word, void* stream)
{
    return guarded([&] {
        QueryParams P = query_params(*frame, *w, forward_stream(w->mode), pts, query_sdf, query_vis, knn_idx, 0, n, out);
        P.stamps = stamps;
        const QueryLaunch L = w->mode == 1 ? query_launch<1>() : query_launch<0>();
        const long long blocks = query_blocks(L, n);
        *n_waves = (int)blocks * L.wpb;
        if (stamps) launch_query(L, blocks, P, queue_word, stream); // (without a table: the caller asks how many waves there will be)
    });
}
#endif
