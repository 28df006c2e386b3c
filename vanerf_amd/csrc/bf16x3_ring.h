// bf16x3_ring.h -- what only the split-bf16 ("bf16x3") kernels of query_kernel.hip use: the LDS map of the block that owns its CU's LDS, the
// fragment ring the block's eight waves share the streamed layers through, and the layer runner with its pinned software pipeline.
#pragma once
#include "common.h"
#include "mfma_chain.h"

namespace vanerf {
namespace {

using namespace vanerf_chain;

// ---------------------------------------------------------------------------------------------
// split-bf16 ("bf16x3") variant of the layer runner: W = W_hi + W_lo, X = X_hi + X_lo (bf16 each),
// acc += W_hi X_hi + W_hi X_lo + W_lo X_hi on v_mfma_f32_32x32x16_bf16 (fp32 accumulate).  One bf16 k-step covers 8 consecutive
// k-pairs of the fp32 ordering, so the accumulator -> operand chaining of layer_spec.h is unchanged.  Measured against the fp32
// oracle the dropped W_lo X_lo term and the 16-bit operands cost 1.2e-5 absolute on the outputs (the fp32-MFMA path: 9e-6).
// ---------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct FragB { u32x4 hi, lo; }; // A fragments (hi and lo parts) of one 32-row output block of one bf16 k-step

constexpr int RING_WAVES = 8; // the waves of the kernel's one block per CU, which share the ring

// Fragments of the LAST layers of the stream stay resident in LDS for the whole launch (split-bf16 kernel: one block per CU, persistent):
// every group needs them -- the all-invalid groups need nothing else -- and the CU's vector-memory path (L1: 64 B per clock) is what the
// fragment stream loads most (profiles/r02_a_*): ds_read_b128 has four times that width and a fifth of the latency.
// Layers LDS_FIRST .. NUM_LAYERS-1 are copied once per block: ibr_compress and the four TexVisFusion layers (126 KB: what the all-invalid
// groups need).  The layers in front of them are SHARED by the block's waves through an LDS ring of 32 KB (below).
// The lean stream is short enough for L_HEAD1 and L_HEAD2 to stay as well (24 KB more): four ring phases and their barriers less per round.
// (LEVEL: the stream of layer_spec.h the kernel walks, 0 plain, 1 hoisted, 2 lean, 3 texel -- layers differ in length, so every offset, the ring's phases
// and the resident size differ)
template <int LEVEL> constexpr int LDS_FIRST = lean_level(LEVEL) ? L_HEAD1 : L_IBR;
template <int LEVEL> constexpr unsigned RES_BASE_DW = layer_offset_b(LDS_FIRST<LEVEL>, LEVEL);
template <int LEVEL> constexpr unsigned RES_DW = layer_offset_b(NUM_LAYERS, LEVEL) - layer_offset_b(LDS_FIRST<LEVEL>, LEVEL);
// (The key points live in LDS because 256 registers per wave hold nothing long-lived: one ds_read_b128 per key point and group.)
// LDS map of the split-bf16 kernel (all of it in the dynamic region, which then starts at LDS address 0: no static __shared__ in this kernel):
//   [0, 672)      the 42 key points as float4                              [672, 768)  control words: s_base[2], s_valid[2][waves per block]
//   [1024, 1024 + 32 KB)     fragment ring                                 [LDS_RES, LDS_RES + RES_DW * 4)  resident fragments
//   lean kernel: [LDS_RES + RES_DW * 4, + 1280)  the bias table (layer_spec.h)
constexpr unsigned RING_PHASE_PIECES = 16u, RING_BYTES = 2u * RING_PHASE_PIECES * 1024u; // two halves of one 16 KB phase each
constexpr unsigned LDS_KPT = 0u, LDS_CTRL = 2u * PE_KPT_PER_HALF * 16u, LDS_LAT0 = 768u, LDS_RING = 1024u, LDS_RES = LDS_RING + RING_BYTES;
// [768, 896): ibr_compress of an all-zero pooled latent (its bias through the same MFMA chain), [lane half][16 registers]: what every sample of an
// all-invalid group gets from that layer -- computed once per block, read by the short path instead of 27 MFMAs per group
template <int LEVEL> constexpr unsigned LDS_BIAS = LDS_RES + RES_DW<LEVEL> * 4u;
template <int LEVEL> constexpr unsigned DYN_LDS_BYTES = LDS_BIAS<LEVEL> + (lean_level(LEVEL) ? BIAS_TABLE_FLOATS * 4u : 0u);
// The streamed part of the fragment stream (layers 0 .. LDS_FIRST-1) as 1 KB pieces (one (k-step, output block, hi | lo) fragment each = one
// LDS-DMA wave instruction), in the order the layers consume them; a PHASE is 16 consecutive pieces.
template <int LEVEL> constexpr unsigned RING_PIECES = RES_BASE_DW<LEVEL> / 256u;
// RING_PHASES is even (phase P lives in half P % 2, and phase 0 of the next round must not land on the half the last phase is read from).  When the
// stream has an odd number of phases (the hoisted stream: 31) nobody reads the last, padding phase, so no read begins it: the kernel begins it by
// hand behind the last streamed layer (ring_close), which is what issues phase 0 of the next round.
template <int LEVEL> constexpr unsigned RING_STREAM_PHASES = (RING_PIECES<LEVEL> + RING_PHASE_PIECES - 1u) / RING_PHASE_PIECES;
template <int LEVEL> constexpr unsigned RING_PHASES = (RING_STREAM_PHASES<LEVEL> + 1u) / 2u * 2u;
static_assert(RING_WAVES == 8 && 2u * RING_WAVES == RING_PHASE_PIECES, "the ring's DMA schedule deals 2 pieces of a phase to each of 8 waves");
static_assert(RING_PHASES<0> * RING_PHASE_PIECES * 256u <= layer_offset_b(NUM_LAYERS), "the last phase's DMA must stay inside the stream");
static_assert(RING_PHASES<1> * RING_PHASE_PIECES * 256u <= layer_offset_b(NUM_LAYERS, 1), "the last phase's DMA must stay inside the hoisted stream");
static_assert(RING_PHASES<2> * RING_PHASE_PIECES * 256u <= layer_offset_b(NUM_LAYERS, 2), "the last phase's DMA must stay inside the lean stream");
static_assert(RING_PHASES<3> * RING_PHASE_PIECES * 256u <= layer_offset_b(NUM_LAYERS, 3), "the last phase's DMA must stay inside the texel stream");
static_assert(RING_STREAM_PHASES<1> == 31u && RING_STREAM_PHASES<2> == 27u && RING_STREAM_PHASES<3> == 26u, "the streamed parts: 486 KB hoisted, 426 KB lean, 402 KB texel");
static_assert(LDS_BIAS<3> == LDS_BIAS<2> && DYN_LDS_BYTES<3> == DYN_LDS_BYTES<2>, "the texel level's resident part and bias table are the lean level's");
static_assert(LDS_CTRL + 8u + 2u * 4u * RING_WAVES <= LDS_LAT0 && LDS_LAT0 + 128u <= LDS_RING, "control words / constant latent overlap their neighbours");
static_assert(DYN_LDS_BYTES<0> <= 160u * 1024u && DYN_LDS_BYTES<1> <= DYN_LDS_BYTES<0> && DYN_LDS_BYTES<2> <= 160u * 1024u,
              "key points + control words + ring + resident fragments (+ bias table) must fit the CU's 160 KB");
static_assert(LDS_BIAS<2> % 16u == 0, "the bias table is read 16 bytes at a time");
// The SHORT map, of the short-only kernel (query_short_kernel: all-invalid groups only, twelve waves on one copy).  It is the LEVEL map with
// holes: every region the short path reads keeps the address it has in the full kernel's map, so the stages instantiate unchanged (same
// functions, same LDS offsets, same bits), and what the short path never reads is never filled --
//   [672, 768)  control words: unused           [768, 896)  the constant latent            [0, 672), [1024, 1024 + 32 KB)  key points, ring: not filled
//   [SHORT_LDS_RES, + SHORT_RES_DW * 4)  resident fragments of L_IBR and the four TexVisFusion layers (lean: 16 + 78 KB; the head layers in
//   front of them are not filled)                [LDS_BIAS, + 1280)  lean kernel: the bias table (L_IBR's row starts the constant latent)
// The block's allocation stays DYN_LDS_BYTES<LEVEL>: one block per CU either way, the holes cost nothing.
constexpr int SHORT_WAVES = 12; // waves of the short-only kernel's one block per CU: three per SIMD (168 registers; four would need 128)
template <int LEVEL> constexpr unsigned SHORT_BASE_DW = layer_offset_b(L_IBR, LEVEL);
template <int LEVEL> constexpr unsigned SHORT_RES_DW = layer_offset_b(NUM_LAYERS, LEVEL) - SHORT_BASE_DW<LEVEL>;
template <int LEVEL> constexpr unsigned SHORT_LDS_RES = LDS_RES + (SHORT_BASE_DW<LEVEL> - RES_BASE_DW<LEVEL>) * 4u;
static_assert(L_IBR >= LDS_FIRST<2> && SHORT_RES_DW<2> == (16u + 78u) * 256u, "the short path's layers are resident in the full map");
extern __shared__ __attribute__((aligned(16))) u32x4 s_dyn[];
typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
typedef __attribute__((address_space(3))) unsigned lds_u32_t;
// A ds instruction addresses base VGPR + 16-bit immediate.  Left to itself the compiler forms one base register (lane * 16 + constant) per
// access beyond the first 64 KB, hoists all of them out of the sample loop and spills them; so the three 64 KB windows get one base each,
// re-made opaque at the top of every round (LAddr), and every access names its window and its offset inside it.
struct LAddr {
    unsigned w[3];
    unsigned dma_lds, dma_src;  // the wave's LDS-DMA destination / stream offset inside a phase, wave-uniform
};
__device__ __forceinline__ LAddr make_laddr(int lane, unsigned wv_uniform = 0u)
{
    LAddr a;
    a.dma_lds = LDS_RING + wv_uniform * 2048u; a.dma_src = wv_uniform * 2048u;
    a.w[0] = (unsigned)lane * 16u;
    asm volatile("" : "+v"(a.w[0]));
    a.w[1] = a.w[0] + 0x10000u; a.w[2] = a.w[0] + 0x20000u;
    asm volatile("" : "+v"(a.w[1]), "+v"(a.w[2]));
    return a;
}
template <unsigned BYTE> __device__ __forceinline__ u32x4 lds_frag(const LAddr& a) // 16 bytes at LDS address BYTE + lane * 16
{
    return *reinterpret_cast<const lds_u32x4_t*>((size_t)(a.w[BYTE >> 16] + (BYTE & 0xffffu)));
}
__device__ __forceinline__ lds_u32_t* lds_ctrl() { return reinterpret_cast<lds_u32_t*>((size_t)LDS_CTRL); }
// ring depth in BLOCK fragments (one (hi, lo) pair = 8 registers, 2 KB of stream): two blocks ahead, one for the one-block layers -- 4 / 3 / 2 / 2
// blocks (for layers with 4 / 3 / 2 / 1 output blocks) measured the same 5.42 ms with 15 more registers, 6 / 4 spill
template <int NB> struct RingDepthB { static constexpr int value = NB == 1 ? 1 : 2; };
template <int NB> struct RingB { FragB b[RingDepthB<NB>::value]; };

// ---- the fragment ring ---------------------------------------------------------------------------------------------------------------
// The eight waves of the block walk the same fragment stream one round at a time.  Fetched by every wave for itself, the stream is 8 x 516 KB
// per round through the CU's 64 B / clock vector-memory path: 65 % busy, the largest share of what the waves wait for (profiles/r03_a_*).
// Instead phase P (16 KB) is brought into one half of a 32 KB LDS ring ONCE -- every wave issues two `buffer_load_dwordx4 ... lds` (LDS-DMA:
// 1 KB of memory to M0 + 16 * lane, no registers) -- while the waves read phase P - 1 from the other half with ds_read_b128.  Protocol, per
// wave, at the first read of phase P (phase_begin<P>; everything is unrolled, so P is a compile-time constant at every read):
//     s_waitcnt vmcnt(0) lgkmcnt(0)   my two pieces of phase P have landed (they were issued a phase ago); my reads of phase P - 1 are back
//     s_barrier                        ... and so have / are everybody's: phase P may be read, the half of phase P - 1 may be overwritten
//     issue the DMA of phase P + 1     into the half phase P - 1 occupied
// The last phase issues phase 0 of the NEXT full round, the top-of-round barrier (every wave has passed a vmcnt(0) before its stores) stands in
// for phase_begin<0>, and rounds that take the all-invalid path touch neither half: half 0 holds phase 0 whenever a round starts.
// vmcnt(0) is exact here: gathers are issued where they are consumed, nothing else is in flight inside the layer stack.
template <unsigned P> __device__ __forceinline__ void ring_dma(WRsrc rs, const LAddr& la) // this wave's two pieces of phase P -> half P % 2
{
    constexpr unsigned lds_off = (P % 2u) * RING_PHASE_PIECES * 1024u, src_off = P * RING_PHASE_PIECES * 1024u;
    unsigned keep, soff;
    // M0 = LDS destination (written and used in ONE statement: hipcc owns M0 everywhere else); one wait state between its write and the DMA
    asm volatile("s_mov_b32 %0, m0\n\ts_add_u32 m0, %2, %4\n\ts_add_u32 %1, %3, %5\n\ts_nop 0\n\t"
                 "buffer_load_dwordx4 %6, %7, %1 offen lds\n\tbuffer_load_dwordx4 %6, %7, %1 offen offset:1024 lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep), "=&s"(soff)
                 : "s"(la.dma_lds), "s"(la.dma_src), "i"(lds_off), "i"(src_off), "v"(la.w[0]), "s"(rs)
                 : "memory");
}
template <int LEVEL, unsigned P> __device__ __forceinline__ void phase_begin(WRsrc rs, const LAddr& la)
{
    if constexpr (P > 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    ring_dma<(P + 1u) % RING_PHASES<LEVEL>>(rs, la);
}

// behind the last streamed layer of a full round: begins the padding phase of a stream with an odd number of phases (see RING_PHASES)
template <int LEVEL> __device__ __forceinline__ void ring_close(WRsrc rs, const LAddr& la)
{
    if constexpr (RING_STREAM_PHASES<LEVEL> % 2u == 1u) phase_begin<LEVEL, RING_PHASES<LEVEL> - 1u>(rs, la);
}

// DW: dword offset of the block's hi part in the stream (the lo part follows 1 KB later); the lane's 16 bytes sit at lane * 16
template <int LEVEL, bool RES, unsigned DW> __device__ __forceinline__ FragB wload_blk(WRsrc rs, const LAddr& la)
{
    constexpr unsigned PHASES = RING_PHASES<LEVEL>, BASE_DW = RES_BASE_DW<LEVEL>;
    static_assert(RES == (DW >= BASE_DW), "a layer's fragments are either resident or streamed through the ring: nothing is fetched per wave");
    FragB r;
    if constexpr (RES) { // resident layer
        r.hi = lds_frag<LDS_RES + (DW - BASE_DW) * 4u>(la);
        r.lo = lds_frag<LDS_RES + (DW - BASE_DW + 256u) * 4u>(la);
    } else { // streamed layer, through the ring
        constexpr unsigned q = DW / 256u; // piece index of the hi part
        static_assert(q % 2u == 0 && q + 1u < PHASES * RING_PHASE_PIECES, "block fragments are two consecutive pieces inside the streamed part");
        if constexpr (q % RING_PHASE_PIECES == 0) phase_begin<LEVEL, q / RING_PHASE_PIECES>(rs, la);
        r.hi = lds_frag<LDS_RING + (q % (2u * RING_PHASE_PIECES)) * 1024u>(la);
        r.lo = lds_frag<LDS_RING + ((q + 1u) % (2u * RING_PHASE_PIECES)) * 1024u>(la);
    }
    return r;
}

// Block fragment i of a layer = (k-step i / NB, output block i % NB) lies i * 512 dwords into the layer's stream.
template <int LEVEL, int NB, int T, bool RES, unsigned SBASE_DW> __device__ __forceinline__ RingB<NB> ring_start_b(WRsrc rs, const LAddr& la)
{
    constexpr int D = RingDepthB<NB>::value, S = (T + 7) / 8;
    RingB<NB> r;
    static_for<D>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if constexpr (i < S * NB) r.b[i] = wload_blk<LEVEL, RES, SBASE_DW + i * 512u>(rs, la);
    });
    __builtin_amdgcn_sched_barrier(0x000F); // keep the ring fill where it is written: ahead of the previous layer's epilogue
    return r;
}

__device__ __forceinline__ unsigned pack_bf16(float a, float b)
{
    const bf16x2 v = {(__bf16)a, (__bf16)b}; // v_cvt_pk_bf16_f32 (round to nearest even)
    return __builtin_bit_cast(unsigned, v);
}

struct NoPre { template <class C> __device__ __forceinline__ void operator()(C) const {} };

// pre(integral_constant<int, s>) runs before the operands of bf16 step s are gathered (lazy producers, e.g. the positional encoding).
//
// Software pipeline, written out and pinned.  A wave issues in order: a bf16 32x32x16 MFMA costs the wave ~16 issue cycles
// and then runs 34 cycles beside whatever the wave issues next, so up to ~4 VALU instructions per MFMA are free -- IF they stand
// between the MFMAs (tools/probe_bf16_valu.hip).  Left to itself the machine scheduler emits the 3*NB MFMAs of a k-step back to
// back (the wave sits in MFMA issue) and then the operand split of the next step (the matrix pipe idles), and it sinks every ring
// re-load to just above its use (no prefetch).  An ablation priced that at 5 ms of MFMA time added to 4.4 ms of everything else.
// So: step s's MFMAs are cut into four chunks, after each chunk comes one pair-split of step s+1's operands (5 VALU), the re-load of
// the consumed ring slot is issued before the first chunk, and a sched_barrier(0) after every chunk keeps that order.
// (sched_group_barrier could request the same interleave, but its solver did not finish on this 10 k-instruction block in 15 min.)
template <int LEVEL, int NB, int T, bool RES, unsigned SBASE_DW, class Op, class Pre = NoPre>
__device__ __forceinline__ void run_layer_b(f32x16 (&acc)[NB], RingB<NB>& ring, WRsrc rs, const LAddr& la, Op&& operand,
                                            Pre&& pre = Pre{})
{
    constexpr int D = RingDepthB<NB>::value, S = (T + 7) / 8;
    constexpr int NCH = 4; // chunks a step's MFMAs are cut into (one of the four operand pairs of the next step is split after each)
    // hi = bf16(x) (round to nearest even), lo = bf16(x - hi) for operand pair i of step s: 6 VALU -- v_cvt_pk, v_lshlrev, v_and, two
    // v_sub_f32, v_cvt_pk (no packed f32 math: a v_pk_add_f32 beside MFMAs costs more than the two scalar ops it replaces, and the file
    // is built with -fno-slp-vectorize for the same reason).  The empty asm keeps the packed hi opaque: without it the compiler
    // re-converts each element on its own to feed the subtraction (7 per pair).
    auto split_pair = [&](auto sc, auto ic, u32x4& bh, u32x4& bl) {
        constexpr int s = decltype(sc)::value, i = decltype(ic)::value, t0 = 8 * s + 2 * i;
        float x0 = 0.0f, x1 = 0.0f;
        if constexpr (t0 < T) x0 = operand(std::integral_constant<int, t0>{});
        if constexpr (t0 + 1 < T) x1 = operand(std::integral_constant<int, t0 + 1>{});
        unsigned hpk = pack_bf16(x0, x1);
        asm("" : "+v"(hpk));
        bh[i] = hpk;
        bl[i] = pack_bf16(x0 - __uint_as_float(hpk << 16), x1 - __uint_as_float(hpk & 0xffff0000u));
    };
    u32x4 bh, bl;
    pre(std::integral_constant<int, 0>{});
    static_for<4>([&](auto ic) { split_pair(std::integral_constant<int, 0>{}, ic, bh, bl); });
    __builtin_amdgcn_sched_barrier(0);
    static_for<S>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        FragB a[NB];
        const bf16x8 xh = __builtin_bit_cast(bf16x8, bh), xl = __builtin_bit_cast(bf16x8, bl);
        u32x4 nh = {}, nl = {};
        // MFMA m of the step (m = 3*ob + product) belongs to chunk m * 4 / (3*NB); products of one block stay in order hh, hl, lh.
        // A block's fragment leaves the ring at its first product and its slot is re-loaded at once with the fragment D blocks ahead.
        static_for<NCH>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            static_for<3 * NB>([&](auto mc) {
                constexpr int m = decltype(mc)::value, ob = m / 3, pr = m % 3, idx = s * NB + ob;
                if constexpr (m * NCH / (3 * NB) == c) {
                    if constexpr (pr == 0) {
                        a[ob] = ring.b[idx % D];
                        if constexpr (idx + D < S * NB) ring.b[idx % D] = wload_blk<LEVEL, RES, SBASE_DW + (idx + D) * 512u>(rs, la);
                    }
                    const bf16x8 wh = __builtin_bit_cast(bf16x8, a[ob].hi), wl = __builtin_bit_cast(bf16x8, a[ob].lo);
                    acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pr == 2 ? wl : wh, pr == 1 ? xl : xh, acc[ob], 0, 0, 0);
                }
            });
            if constexpr (s + 1 < S) {
                if constexpr (c == 0) pre(std::integral_constant<int, s + 1>{});
                split_pair(std::integral_constant<int, s + 1>{}, cc, nh, nl);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        bh = nh; bl = nl;
    });
}

// Lean kernel: the accumulators of layer L start from its rows of the bias table in LDS ([lane half][block][register], layer_spec.h): 4 NB
// ds_read_b128.  The address is formed here, opaque, so that it is neither hoisted out of the sample loop nor kept across layers.
template <int L, int NB> __device__ __forceinline__ void load_bias(int h, f32x16 (&acc)[NB])
{
    static_assert(bias_table_floats(L) == 2u * NB * 16u, "the layer has a row in the bias table");
    unsigned a = (unsigned)h * (NB * 64u) + (LDS_BIAS<2> + bias_table_offset(L) * 4u);
    asm volatile("" : "+v"(a));
#pragma unroll
    for (int ob = 0; ob < NB; ++ob)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u32x4 v = *reinterpret_cast<const lds_u32x4_t*>((size_t)(a + 64u * ob + 16u * i));
            acc[ob][4 * i] = __uint_as_float(v.x); acc[ob][4 * i + 1] = __uint_as_float(v.y);
            acc[ob][4 * i + 2] = __uint_as_float(v.z); acc[ob][4 * i + 3] = __uint_as_float(v.w);
        }
}

// lane id from v_mbcnt, not from a register that would have to stay live (or be spilled) across the whole sample loop
__device__ __forceinline__ int lane_id_fresh()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// Barrier of the block's waves: LDS writes before it are visible after it (s_waitcnt lgkmcnt(0) + s_barrier; NOT __syncthreads(), whose
// workgroup-scope release also drains vmcnt -- the fragment prefetch and the stores of the previous group are in flight here).
__device__ __forceinline__ void block_barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// (More barriers inside a round were measured and lost: four rendezvous points in the layer stack cost 3.4 % -- 6.62 -> 6.84 ms.)

} // namespace
} // namespace vanerf
