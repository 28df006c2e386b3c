// common.h -- error plumbing shared by the translation units of libvanerf_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vanerf_hip.h"
#include "layer_spec.h"
#include "pack_math.h"
#include "streams.h"

namespace vanerf {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

[[noreturn]] inline void throw_error(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    throw Error(VANERF_EINVAL, buf);
}

inline void hip_check(hipError_t e, const char* what)
{
    if (e != hipSuccess) {
        char buf[512];
        snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        throw Error(VANERF_EHIP, buf);
    }
}
#define HIP_CHECK(x) ::vanerf::hip_check((x), #x)

void set_last_error(const char* msg);

// Runs `fn`, converts C++ exceptions into the C ABI's negative return codes (never throws across the ABI).
template <class F>
int guarded(F&& fn) noexcept
{
    try {
        fn();
        return VANERF_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("out of host memory");
        return VANERF_ENOMEM;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return VANERF_EINVAL;
    } catch (...) {
        set_last_error("unknown error");
        return VANERF_EINVAL;
    }
}

// The packer's two stages (weights_pack.cpp).  Stage 1: where a layer's parameters are and where its effective weights go in the flat array
// `eff` (every layer's [out][in] matrix with weight-norm folded, then its bias; the folded matrices of the lean stream behind the last layer).
unsigned eff_layer_offset(int l); // where layer l's [nout][kin] matrix starts in eff
struct LayerSrc {
    const float* w; // [nout][kin] (weight-normed layers: weight_v)
    const float* g; // weight_g or null
    const float* b; // bias or null
    int nout, kin;
    unsigned eff;   // offset of the layer in eff: [nout][kin], then the bias
};
void layer_sources(const VanerfWeightTable& w, LayerSrc out[NUM_LAYERS]);
void fold_products(FoldProduct out[2]);                   // the two folded matrices, F0 then F1, back to back at eff_slice_offset()
std::vector<float> fold_host(const VanerfWeightTable& w); // eff from host pointers
// Stage 2: the placement of eff in the streams (streams.h), weight independent and built once per process.
struct PackTables {
    std::vector<int> place[NUM_STREAMS]; // the gathers' ids (empty: EFF_SLICE)
    LayerOffsets offs{};                 // of the fp32 forward stream
    unsigned n_eff = 0;
    size_t words(int s) const { return kStreams[s].kind == EFF_SLICE ? FOLD_FLOATS : place[s].size() / (kStreams[s].kind == GATHER_BF16X3 ? 2 : 1); }
};
const PackTables& pack_tables();
unsigned eff_slice_offset();                                           // where the EFF_SLICE stream starts in eff
std::vector<float> stream_host(const std::vector<float>& eff, int which); // any stream of streams.h from eff (bf16x3 words as raw floats)
LayerOffsets layer_offsets(int mode);                                  // of the forward stream of a handle of `mode`
int layer_slots(int layer, int* k_of_slot, int cap);

// A pass marches n_views * nx * ny * S samples in one launch; the validity partition (vanerf_query_order) indexes them with 32 bits, so
// vanerf_render_pass and the table form of vanerf_ray_setup refuse a launch that reaches this many (the bound vanerf_query_order itself applies).
constexpr long long VIEWS_MAX_ITEMS = 0x7fffffffLL;
void check_camera_source(const char* who, const VanerfPassDesc& d); // render_kernels.hip: n_views and cams agree, and the table form has the plain grid

} // namespace vanerf

struct VanerfWeights {
    float* block[vanerf::NUM_BLOCKS] = {};   // the device allocations (streams.h); fp32 handles get BLOCK_EFF at their first vanerf_weights_update
    float* stream[vanerf::NUM_STREAMS] = {}; // where each stream starts in its block (null: the handle does not carry it) ...
    size_t words[vanerf::NUM_STREAMS] = {};  // ... and its 32-bit words; both set once, at the pack
    vanerf::LayerOffsets offs{};
    int mode = 0;
    float beta = 0.1f;      // sigmoid_beta as packed from the host (clamped); stale once vanerf_weights_update took it from the device ...
    float* dev_beta = nullptr; // ... so the passes' composites read this device copy (one float, clamped)
    int device = 0;
    unsigned long long* stats = nullptr; // [0]: running count of 32-sample groups that took query_kernel's all-invalid short path
};
