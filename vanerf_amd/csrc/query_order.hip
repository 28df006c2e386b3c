// query_order.hip -- the validity partition in front of query_kernel (query_kernel.hip); shares project_and_mask (sample_math.h) with it.
//
// Built with -ffp-contract=off, as query_kernel.hip: both must take the same decision for every sample.
#include "common.h"
#include "sample_math.h"

using namespace vanerf;

// ---------------------------------------------------------------------------------------------
// Validity partition.  A 32-sample group whose samples ALL miss the source view takes the short path of query_kernel; groups are
// consecutive samples of a ray, and on the benchmark view 12.5 % of them are mixed: their invalid samples (7 % of all samples) ride
// through the long path.  vanerf_query_order computes the validity of every sample with the kernel's own project_and_mask and writes the
// stable partition [valid samples in order | invalid samples in order]; query_kernel then works on slot k = sample order[k], so only one
// group per launch is mixed.  Results are the same bits (the networks are per-sample functions; outputs are stored at the sample's place).
// Three small kernels: flags + per-block counts, scan of the block counts, scatter.
// ---------------------------------------------------------------------------------------------
constexpr int CP_BLOCK = 1024;

__global__ __launch_bounds__(CP_BLOCK) void order_count_kernel(const VanerfFrame F, float wm1, float hm1, const float* __restrict__ pts, long long n,
                                                               uint8_t* __restrict__ flags, unsigned* __restrict__ block_valid)
{
    const long long s = (long long)blockIdx.x * CP_BLOCK + threadIdx.x;
    int valid = 0;
    if (s < n) {
        valid = project_and_mask(F, wm1, hm1, pts[3 * s], pts[3 * s + 1], pts[3 * s + 2]).mask > 0.0f;
        flags[s] = (uint8_t)valid;
    }
    const int cnt = __syncthreads_count(valid);
    if (threadIdx.x == 0) block_valid[blockIdx.x] = (unsigned)cnt;
}

// exclusive scan of block_valid[nblocks] in place; total -> block_valid[nblocks]
__global__ __launch_bounds__(CP_BLOCK) void order_scan_kernel(unsigned* __restrict__ block_valid, int nblocks)
{
    __shared__ unsigned s_sum[CP_BLOCK];
    const int per = (nblocks + CP_BLOCK - 1) / CP_BLOCK;
    const int b0 = threadIdx.x * per, b1 = min(b0 + per, nblocks);
    unsigned loc = 0;
    for (int b = b0; b < b1; ++b) loc += block_valid[b];
    s_sum[threadIdx.x] = loc;
    __syncthreads();
    for (int d = 1; d < CP_BLOCK; d <<= 1) { // Hillis-Steele inclusive scan
        const unsigned v = threadIdx.x >= (unsigned)d ? s_sum[threadIdx.x - d] : 0u;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned run = s_sum[threadIdx.x] - loc; // exclusive prefix of this thread's chunk
    for (int b = b0; b < b1; ++b) { const unsigned c = block_valid[b]; block_valid[b] = run; run += c; }
    if (threadIdx.x == CP_BLOCK - 1) block_valid[nblocks] = s_sum[CP_BLOCK - 1];
}

__global__ __launch_bounds__(CP_BLOCK) void order_scatter_kernel(const uint8_t* __restrict__ flags, long long n, const unsigned* __restrict__ block_off,
                                                                 int nblocks, int32_t* __restrict__ order)
{
    __shared__ unsigned s_wave[CP_BLOCK / 64];
    const long long s = (long long)blockIdx.x * CP_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool live = s < n;
    const bool valid = live && flags[s] != 0;
    const unsigned long long m = __ballot(valid);
    const unsigned below = (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wv] = (unsigned)__builtin_popcountll(m);
    __syncthreads();
    unsigned wbase = 0;
    for (int k = 0; k < wv; ++k) wbase += s_wave[k];
    if (!live) return;
    const unsigned rank_valid = wbase + below;                       // valid samples of this block before this one
    const unsigned off_valid = block_off[blockIdx.x], total_valid = block_off[nblocks];
    const unsigned long long before = (unsigned long long)blockIdx.x * CP_BLOCK; // samples before this block
    const unsigned long long pos = valid ? (unsigned long long)off_valid + rank_valid
                                         : (unsigned long long)total_valid + (before - off_valid) + (threadIdx.x - rank_valid);
    order[pos] = (int32_t)s;
}

extern "C" int vanerf_query_order(const VanerfFrame* frame, const float* pts, int64_t n, int32_t* order, void* scratch, int64_t scratch_bytes,
                                  void* stream)
{
    return guarded([&] {
        if (n < 0) throw_error("vanerf_query_order: n = %lld < 0", (long long)n);
        if (n == 0) return;
        if (!frame || !pts || !order || !scratch) throw_error("vanerf_query_order: null argument");
        if (n >= 0x7fffffffLL) throw_error("vanerf_query_order: n = %lld does not fit a 32-bit index", (long long)n);
        const VanerfFrame& f = *frame;
        if (!f.mask || f.hi < 1 || f.wi < 1) throw_error("vanerf_query_order: frame has no mask");
        const int nblocks = (int)((n + CP_BLOCK - 1) / CP_BLOCK);
        const int64_t need = n + 4 * ((int64_t)nblocks + 1) + 16;
        if (scratch_bytes < need) throw_error("vanerf_query_order: scratch of %lld bytes, %lld needed (vanerf_query_order_scratch)", (long long)scratch_bytes, (long long)need);
        uint8_t* flags = static_cast<uint8_t*>(scratch);
        unsigned* block_off = reinterpret_cast<unsigned*>(flags + ((n + 15) / 16) * 16);
        const hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(order_count_kernel, dim3(nblocks), dim3(CP_BLOCK), 0, st, f, (float)(f.wi - 1), (float)(f.hi - 1), pts, (long long)n, flags, block_off);
        hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(CP_BLOCK), 0, st, block_off, nblocks);
        hipLaunchKernelGGL(order_scatter_kernel, dim3(nblocks), dim3(CP_BLOCK), 0, st, flags, (long long)n, block_off, nblocks, order);
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int64_t vanerf_query_order_scratch(int64_t n) { return n + 4 * ((n + CP_BLOCK - 1) / CP_BLOCK + 1) + 32; }
