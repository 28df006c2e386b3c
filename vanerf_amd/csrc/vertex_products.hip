// vertex_products.hip -- the per-vertex half of three first layers, once per source frame (layer_spec.h: the hoisted bf16x3 stream).
//
// geo_vis_fusion.fconv_at.0 (196 -> 10), geo_vis_fusion.fconv_ated.0 (196 -> 64) and tex_vis_fusion.fconv_at.0 (96 -> 96)
// (reference src/networks.py:86-93, 285-288) have no bias and nothing in front of their matrix product, and 128 / 128 / 58 of their input
// channels are rows of the per-frame vertex tables selected by the sample's 1-NN vertex i and its twin tw(i) = (i + 779) mod 1558.  Their
// share of the product is therefore one fixed vector per vertex and frame; query_kernel<1, hoisted> starts its accumulators from these rows
// instead of spending 64 / 64 / 29 k-pairs per sample on them.  The second layer's rows are gated per sample (a1 nn, a2 twin):
// W (a1 x) = a1 (W x), so its two halves are kept apart (N0, T0) and scaled in the kernel.
//
// Behind the per-vertex parts stand the per-texel products of the 64-channel geometry map (layer_spec.h, level 3): the pixel feature of the two
// geo layers is the bilinear sample of geo0, which is linear in the tap values, so the kernel samples GA = Wat[:, 0:64] geo0 and
// GM = Wated[:, 0:64] geo0 instead (the gate a0 is a scalar: W (a0 pix) = a0 (W pix)).  The part has room for VP_TEXELS_MAX texels; a larger
// map leaves it unwritten (the launch then runs the lean level), rows of texels beyond h0 * w0 hold 0.
//
// Arithmetic: fp32, one thread per table element, one fmaf chain in ascending input-channel order (nearest vertex's columns, then the
// twin's): the same bits on every build.  One launch, no allocation, no host synchronisation.
#include "common.h"

using namespace vanerf;

namespace {

static_assert(VP_NV == VANERF_NV, "the table is laid out for the two-hand mesh");
constexpr unsigned VP_PER_VERTEX = VP_A0_ROW + 2u * VP_N0_ROW + VP_P_ROW;
constexpr unsigned VP_PER_TEXEL = VP_A0_ROW + VP_N0_ROW;
static_assert(VP_GA % 4u == 0 && VP_GM % 4u == 0, "texel rows are read 16 bytes at a time");

__device__ __forceinline__ float dot_chain(float acc, const float* __restrict__ w, const float* __restrict__ x, int n)
{
    for (int k = 0; k < n; ++k) acc = fmaf(w[k], x[k], acc);
    return acc;
}

// wat [10][196], wated [64][196], wtex [96][96]: the layers' effective (= plain) weights
__global__ __launch_bounds__(256) void vertex_products_kernel(const float* __restrict__ wat, const float* __restrict__ wated, const float* __restrict__ wtex,
                                                              const float* __restrict__ vfeat0, const float* __restrict__ vfeat_tex, float* __restrict__ table)
{
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= VP_NV * VP_PER_VERTEX) return;
    const unsigned i = idx / VP_PER_VERTEX, e = idx % VP_PER_VERTEX;
    const unsigned tw = i >= VANERF_NV_HAND ? i - VANERF_NV_HAND : i + VANERF_NV_HAND;
    // output row of element q of a row laid out [h][nb][nr registers]
    auto out_row = [](unsigned q, unsigned nb, unsigned nr) {
        const unsigned h = q / (nb * nr), ob = (q % (nb * nr)) / nr, r = q % nr;
        return 32u * ob + (r & 3u) + 8u * (r >> 2) + 4u * h;
    };
    const float* x_nn = vfeat0 + 64u * i;
    const float* x_tw = vfeat0 + 64u * tw;
    if (e < VP_A0_ROW) {
        const unsigned o = out_row(e, 1u, 8u);
        float v = 0.0f;
        if (o < 10u) v = dot_chain(dot_chain(0.0f, wat + 196u * o + 64u, x_nn, 64), wat + 196u * o + 128u, x_tw, 64);
        table[VP_A0 + VP_A0_ROW * i + e] = v;
    } else if (e < VP_A0_ROW + VP_N0_ROW) {
        const unsigned q = e - VP_A0_ROW, o = out_row(q, 2u, 16u);
        table[VP_N0 + VP_N0_ROW * i + q] = dot_chain(0.0f, wated + 196u * o + 64u, x_nn, 64);
    } else if (e < VP_A0_ROW + 2u * VP_N0_ROW) {
        const unsigned q = e - VP_A0_ROW - VP_N0_ROW, o = out_row(q, 2u, 16u);
        table[VP_T0 + VP_N0_ROW * i + q] = dot_chain(0.0f, wated + 196u * o + 128u, x_tw, 64);
    } else {
        // TexVisFusion input [q11 | nn11 | tw11 | nn_gf18 | tw_gf18 | ...]; a vertex row is [img3 | tex8 | gf18 | 3 unused]
        const unsigned q = e - VP_A0_ROW - 2u * VP_N0_ROW, o = out_row(q, 3u, 16u);
        const float* w = wtex + 96u * o;
        const float* t_nn = vfeat_tex + 32u * i;
        const float* t_tw = vfeat_tex + 32u * tw;
        float v = dot_chain(dot_chain(0.0f, w + 11, t_nn, 11), w + 33, t_nn + 11, 18);
        v = dot_chain(dot_chain(v, w + 22, t_tw, 11), w + 51, t_tw + 11, 18);
        table[VP_P + VP_P_ROW * i + q] = v;
    }
}

// geo0 [texels][64]: the source frame's geometry map, channel-last
__global__ __launch_bounds__(256) void texel_products_kernel(const float* __restrict__ wat, const float* __restrict__ wated, const float* __restrict__ geo0,
                                                             unsigned texels, float* __restrict__ table)
{
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= VP_TEXELS_MAX * VP_PER_TEXEL) return;
    const unsigned i = idx / VP_PER_TEXEL, e = idx % VP_PER_TEXEL;
    const float* x = geo0 + 64u * i;
    if (e < VP_A0_ROW) {
        const unsigned h = e / 8u, r = e % 8u, o = (r & 3u) + 8u * (r >> 2) + 4u * h;
        table[VP_GA + VP_A0_ROW * i + e] = (i < texels && o < 10u) ? dot_chain(0.0f, wat + 196u * o, x, 64) : 0.0f;
    } else {
        const unsigned q = e - VP_A0_ROW, h = q / 32u, ob = (q % 32u) / 16u, r = q % 16u, o = 32u * ob + (r & 3u) + 8u * (r >> 2) + 4u * h;
        table[VP_GM + VP_N0_ROW * i + q] = i < texels ? dot_chain(0.0f, wated + 196u * o, x, 64) : 0.0f;
    }
}

} // namespace

// Returns the number of floats the table takes when `table` is NULL, 0 after a launch, < 0 on error.
extern "C" int vanerf_vertex_products(const VanerfWeights* w, const VanerfFrame* frame, float* table, int64_t cap_floats, void* stream)
{
    int size = 0;
    const int rc = guarded([&] {
        if (!table) { size = (int)VP_FLOATS; return; }
        if (!w || !frame) throw_error("vanerf_vertex_products: null argument");
        const float* eff = w->block[BLOCK_EFF]; // the effective weights themselves: a bf16x3 handle holds them from the pack on
        if (w->mode != 1 || !eff) throw_error("vanerf_vertex_products: needs a bf16x3 weight handle (vanerf_weights_pack mode 1)");
        if (!frame->vfeat0 || !frame->vfeat_tex || !frame->geo0) throw_error("vanerf_vertex_products: frame has a null pointer");
        if (cap_floats < (int64_t)VP_FLOATS) throw_error("vanerf_vertex_products: room for %lld floats, %u needed", (long long)cap_floats, VP_FLOATS);
        if (reinterpret_cast<uintptr_t>(table) & 15u) throw_error("vanerf_vertex_products: the table must be 16-byte aligned");
        const unsigned n = VP_NV * VP_PER_VERTEX;
        hipLaunchKernelGGL(vertex_products_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, eff + eff_layer_offset(L_GEO_AT0_A),
                           eff + eff_layer_offset(L_GEO_ATED0_A), eff + eff_layer_offset(L_TEX_AT_A), frame->vfeat0, frame->vfeat_tex, table);
        HIP_CHECK(hipGetLastError());
        if (texel_products_fit(frame->h0, frame->w0)) { // else the part stays unwritten: vanerf_query_samples takes the same decision
            const unsigned nt = VP_TEXELS_MAX * VP_PER_TEXEL;
            hipLaunchKernelGGL(texel_products_kernel, dim3((nt + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, eff + eff_layer_offset(L_GEO_AT0_A),
                               eff + eff_layer_offset(L_GEO_ATED0_A), frame->geo0, (unsigned)(frame->h0 * frame->w0), table);
            HIP_CHECK(hipGetLastError());
        }
    });
    return rc != VANERF_OK ? rc : size;
}
