// api.cpp -- ABI bookkeeping: version, thread-local last error, packed-weight handle.
#include <algorithm>
#include <cstddef>

#include <cstring>

#include "common.h"

namespace vanerf {
static thread_local std::string g_last_error;
void set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }
} // namespace vanerf

using namespace vanerf;

extern "C" int vanerf_abi_version(void) { return VANERF_ABI_VERSION; }

extern "C" const char* vanerf_last_error(void) { return g_last_error.c_str(); }

namespace {
// frees everything a handle holds and the handle; the first error, if any
hipError_t release(VanerfWeights* h)
{
    hipError_t first = hipSuccess;
    for (void* p : {(void*)h->block[BLOCK_MAIN], (void*)h->block[BLOCK_BACKWARD], (void*)h->block[BLOCK_EFF], (void*)h->stats, (void*)h->dev_beta}) {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        if (first == hipSuccess) first = e;
    }
    delete h;
    return first;
}

void copy_out(const char* who, const std::vector<float>& src, float* out, int64_t cap, int64_t* n_out)
{
    *n_out = (int64_t)src.size();
    if (!out) return;
    if (cap < (int64_t)src.size()) throw_error("%s: buffer too small", who);
    std::memcpy(out, src.data(), src.size() * sizeof(float)); // raw copy: the bf16x3 words are not numbers
}
} // namespace

extern "C" int vanerf_weights_pack(const VanerfWeightTable* w, int mode, VanerfWeights** out)
{
    return guarded([&] {
        if (!w || !out) throw_error("vanerf_weights_pack: null argument");
        if (mode != 0 && mode != 1) throw_error("vanerf_weights_pack: mode %d not supported (0 = fp32 MFMA, 1 = split-bf16 x3)", mode);
        const float* const* ptrs = reinterpret_cast<const float* const*>(w);
        constexpr size_t n_ptrs = offsetof(VanerfWeightTable, sigmoid_beta) / sizeof(const float*);
        for (size_t i = 0; i < n_ptrs; ++i)
            if (!ptrs[i]) throw_error("vanerf_weights_pack: weight pointer #%d is null", (int)i);
        // every block's host image: the streams the mode carries back to back in the table's order (BLOCK_EFF: eff itself)
        const std::vector<float> eff = fold_host(*w);
        std::vector<float> host[NUM_BLOCKS];
        size_t at[NUM_STREAMS] = {};
        for (int s = 0; s < NUM_STREAMS; ++s) {
            if (!carries(mode, s)) continue;
            std::vector<float>& image = host[kStreams[s].block];
            if (kStreams[s].kind == EFF_SLICE) {
                image = eff;
                at[s] = eff_slice_offset();
            } else {
                const std::vector<float> v = stream_host(eff, s);
                at[s] = image.size();
                image.insert(image.end(), v.begin(), v.end());
            }
        }
        auto* h = new VanerfWeights();
        h->offs = layer_offsets(mode);
        h->mode = mode;
        h->beta = w->sigmoid_beta < 2e-3f ? 2e-3f : w->sigmoid_beta; // sdf_activation clamp (src/model.py:880)
        try {
            HIP_CHECK(hipGetDevice(&h->device));
            for (int b = 0; b < NUM_BLOCKS; ++b) { // one allocation and one copy per block
                if (host[b].empty()) continue;
                HIP_CHECK(hipMalloc(&h->block[b], host[b].size() * sizeof(float)));
                HIP_CHECK(hipMemcpy(h->block[b], host[b].data(), host[b].size() * sizeof(float), hipMemcpyHostToDevice));
            }
            for (int s = 0; s < NUM_STREAMS; ++s) {
                if (!carries(mode, s)) continue;
                h->stream[s] = h->block[kStreams[s].block] + at[s];
                h->words[s] = pack_tables().words(s);
            }
            HIP_CHECK(hipMalloc(&h->stats, sizeof(unsigned long long)));
            HIP_CHECK(hipMemset(h->stats, 0, sizeof(unsigned long long)));
            HIP_CHECK(hipMalloc(&h->dev_beta, sizeof(float)));
            HIP_CHECK(hipMemcpy(h->dev_beta, &h->beta, sizeof(float), hipMemcpyHostToDevice));
        } catch (...) {
            (void)release(h);
            throw;
        }
        *out = h;
    });
}

extern "C" int vanerf_weights_free(VanerfWeights* w)
{
    return guarded([&] {
        if (w) hip_check(release(w), "vanerf_weights_free");
    });
}

// Host-only view of the fp32 forward stream, used by the CPU tests of the packer (no GPU needed).
extern "C" int vanerf_weights_pack_host(const VanerfWeightTable* w, float* out, int64_t cap, int64_t* n_out, unsigned* offsets)
{
    return guarded([&] {
        if (!w || !n_out) throw_error("vanerf_weights_pack_host: null argument");
        if (offsets) std::copy_n(layer_offsets(0).off, (size_t)NUM_LAYERS, offsets);
        copy_out("vanerf_weights_pack_host", stream_host(fold_host(*w), STREAM_FP32), out, cap, n_out);
    });
}

// Host-only view of any of the streams a handle can carry (streams.h; the bf16x3 words returned as raw floats).
extern "C" int vanerf_weights_stream_host(const VanerfWeightTable* w, int which, float* out, int64_t cap, int64_t* n_out)
{
    return guarded([&] {
        if (!w || !n_out) throw_error("vanerf_weights_stream_host: null argument");
        if (which < 0 || which >= NUM_STREAMS || which == STREAM_NONE)
            throw_error("vanerf_weights_stream_host: which = %d (0 fp32, 1 bf16x3, 2 backward, 3 hoisted bf16x3, 4 lean bf16x3, 5 its bias table, 6 its folded matrices, "
                        "8 texel bf16x3, 9 its copy of the bias table)", which);
        copy_out("vanerf_weights_stream_host", stream_host(fold_host(*w), which), out, cap, n_out);
    });
}

// The streams a handle holds on the device, copied back (blocking; tests of vanerf_weights_update): which = 0 the forward stream of the handle's
// mode, otherwise a stream of streams.h.
extern "C" int vanerf_weights_download(const VanerfWeights* w, int which, float* out, int64_t cap, int64_t* n_out)
{
    return guarded([&] {
        if (!w || !n_out) throw_error("vanerf_weights_download: null argument");
        if (which != 0 && (which < 2 || which >= NUM_STREAMS || which == STREAM_NONE))
            throw_error("vanerf_weights_download: which = %d (0 forward, 2 backward, 3 hoisted bf16x3, 4 lean bf16x3, 5 its bias table, 6 its folded matrices, "
                        "8 texel bf16x3, 9 its copy of the bias table)", which);
        if (which == STREAM_FP32) which = forward_stream(w->mode); // 0 asks for the forward stream of whichever mode
        if (!w->stream[which]) throw_error("vanerf_weights_download: the handle carries no such stream");
        *n_out = (int64_t)w->words[which];
        if (out) {
            if (cap < *n_out) throw_error("vanerf_weights_download: buffer too small");
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(out, w->stream[which], w->words[which] * sizeof(float), hipMemcpyDeviceToHost));
        }
    });
}

// Running count (since the handle was packed) of 32-sample groups for which vanerf_query_samples skipped GeoVisFusion / mlp_geo
// because every sample of the group was invalid.  Synchronises the device; meant for benchmarks and tests, not for the render loop.
extern "C" int vanerf_weights_short_groups(const VanerfWeights* w, uint64_t* count)
{
    return guarded([&] {
        if (!w || !count) throw_error("vanerf_weights_short_groups: null argument");
        unsigned long long v = 0;
        HIP_CHECK(hipMemcpy(&v, w->stats, sizeof v, hipMemcpyDeviceToHost));
        *count = v;
    });
}
