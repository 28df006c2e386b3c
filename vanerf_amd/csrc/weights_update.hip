// weights_update.hip -- re-packs a weight handle IN PLACE from parameters that live on the device: the training step's path.
// vanerf_weights_pack copies every parameter to the host, folds and permutes there and uploads (~100 blocking copies, two hipMalloc / hipFree
// pairs: 4.8 ms of host time per training step for the two handles of the step, and a drained GPU at the start of every step).  Here the
// packer's two stages (weights_pack.cpp) run as launches on the caller's stream, nothing blocks and no address changes:
//   fold_kernel    eff = [every layer's [out][in] matrix with weight-norm folded | its bias]
//   fold_products_kernel   the two folded matrices of the lean bf16x3 stream behind them in eff (layer_spec.h; bf16x3 handles)
//   place_*_kernel one per gathered stream the handle carries (streams.h), through the placement tables (uploaded once per device)
// The arithmetic is pack_math.h's, the host packer's: bit-identical to a fresh vanerf_weights_pack of the same parameters
// (tests/test_hip_parity.py, tests/test_weight_streams.py).
#include <hip/hip_runtime.h>

#include <mutex>

#include "common.h"

using namespace vanerf;

namespace {

struct FoldArgs {
    LayerSrc l[NUM_LAYERS];
};

// one block per (row, layer); the weight-norm scale of the row by one lane
__global__ __launch_bounds__(64) void fold_kernel(FoldArgs a, float* __restrict__ eff, const float* __restrict__ beta_src, float* __restrict__ beta_dst)
{
    const LayerSrc L = a.l[blockIdx.y];
    const int o = blockIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && beta_src) beta_dst[0] = fmaxf(beta_src[0], 2e-3f); // sdf_activation clamp (src/model.py:880)
    if (o >= L.nout) return;
    const float* v = L.w + (size_t)o * L.kin;
    float* e = eff + L.eff + (size_t)o * L.kin;
    __shared__ float s_scale;
    if (L.g) {
        if (threadIdx.x == 0) s_scale = weight_norm_scale(v, L.kin, L.g[o]);
        __syncthreads();
        const float scale = s_scale;
        for (int k = threadIdx.x; k < L.kin; k += 64) e[k] = v[k] * scale;
    } else {
        for (int k = threadIdx.x; k < L.kin; k += 64) e[k] = v[k];
    }
    if (L.b && threadIdx.x == 0) eff[L.eff + (size_t)L.nout * L.kin + o] = L.b[o];
}

// one thread per element of the two folded matrices
__global__ __launch_bounds__(256) void fold_products_kernel(FoldProduct p0, FoldProduct p1, float* __restrict__ eff)
{
    unsigned idx = blockIdx.x * 256u + threadIdx.x;
    const unsigned n0 = (unsigned)(p0.nout * p0.nc);
    const FoldProduct p = idx < n0 ? p0 : p1;
    if (idx >= n0) idx -= n0;
    if (idx < (unsigned)(p.nout * p.nc)) eff[p.dst + idx] = folded_element(eff, p, idx);
}

__global__ void place_f32_kernel(const int* __restrict__ tab, const float* __restrict__ eff, float* __restrict__ out, unsigned n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = placed_f32(eff, tab[i]);
}

__global__ void place_b_kernel(const int2* __restrict__ tab, const float* __restrict__ eff, unsigned* __restrict__ out, unsigned n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = placed_bf16x3(eff, tab[i].x, tab[i].y);
}

// the placement tables on each device, uploaded at the first update there (blocking, once)
struct DeviceTables {
    int* place[NUM_STREAMS] = {};
    bool ready = false;
};
const DeviceTables& device_tables(int device)
{
    static std::mutex mu;
    static DeviceTables per_device[64];
    if (device < 0 || device >= 64) throw_error("vanerf_weights_update: device %d", device);
    std::lock_guard<std::mutex> lock(mu);
    DeviceTables& t = per_device[device];
    for (int s = 0; s < NUM_STREAMS && !t.ready; ++s) {
        const std::vector<int>& v = pack_tables().place[s];
        if (v.empty() || t.place[s]) continue;
        int* d = nullptr;
        HIP_CHECK(hipMalloc(&d, v.size() * sizeof(int)));
        HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
        t.place[s] = d;
    }
    t.ready = true;
    return t;
}

} // namespace

extern "C" int vanerf_weights_update(VanerfWeights* h, const VanerfWeightTable* dev, const float* sigmoid_beta_dev, void* stream)
{
    return guarded([&] {
        if (!h || !dev) throw_error("vanerf_weights_update: null argument");
        int device = -1;
        HIP_CHECK(hipGetDevice(&device));
        if (device != h->device) throw_error("vanerf_weights_update: handle packed on device %d, current device %d", h->device, device);
        const PackTables& p = pack_tables();
        for (int s = 0; s < NUM_STREAMS; ++s)
            if ((h->stream[s] != nullptr) != carries(h->mode, s) || h->words[s] != (h->stream[s] ? p.words(s) : 0))
                throw_error("internal: handle and placement tables disagree on the stream sizes");
        FoldArgs a;
        layer_sources(*dev, a.l); // checks the pointers the layers need
        const DeviceTables& t = device_tables(device);
        float*& eff = h->block[BLOCK_EFF];
        if (!eff) HIP_CHECK(hipMalloc(&eff, (size_t)p.n_eff * sizeof(float)));
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(fold_kernel, dim3(128, NUM_LAYERS), dim3(64), 0, st, a, eff, sigmoid_beta_dev, h->dev_beta);
        if (h->stream[STREAM_LEAN_FOLDED]) { // into eff before the placements that gather them
            FoldProduct f[2];
            fold_products(f);
            hipLaunchKernelGGL(fold_products_kernel, dim3((FOLD_FLOATS + 255u) / 256u), dim3(256), 0, st, f[0], f[1], eff);
        }
        for (int s = 0; s < NUM_STREAMS; ++s) {
            const unsigned n = (unsigned)h->words[s];
            if (!h->stream[s] || kStreams[s].kind == EFF_SLICE) continue;
            if (kStreams[s].kind == GATHER_BF16X3)
                hipLaunchKernelGGL(place_b_kernel, dim3((n + 255) / 256), dim3(256), 0, st, reinterpret_cast<const int2*>(t.place[s]), eff,
                                   reinterpret_cast<unsigned*>(h->stream[s]), n);
            else
                hipLaunchKernelGGL(place_f32_kernel, dim3((n + 255) / 256), dim3(256), 0, st, t.place[s], eff, h->stream[s], n);
        }
        HIP_CHECK(hipGetLastError());
        if (!sigmoid_beta_dev) { // the table's own value (host float), as vanerf_weights_pack takes it
            h->beta = dev->sigmoid_beta < 2e-3f ? 2e-3f : dev->sigmoid_beta;
            HIP_CHECK(hipMemcpyAsync(h->dev_beta, &h->beta, sizeof(float), hipMemcpyHostToDevice, st));
        }
    });
}
