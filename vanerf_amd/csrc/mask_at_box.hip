// mask_at_box.hip -- the dataset's mask_at_box and near / far range of V target views, on the device: Dataset.get_mask_at_box -> get_rays /
// get_near_far (src/dataset.py:122-129, 609-658) restated with a fully specified definition (the comment of
// vanerf_mask_at_box in the header).  The restatement the tests hold these kernels to is the fp64 numpy code of tests/test_mask_at_box.py.
//
// Two launches: the six plane intersections per pixel with one block per (tile, view) and seven partials per block (min near, max far, the
// count, the extent in x and y), then one block per view that folds the tiles' partials.  No atomics, no device globals, and only minima,
// maxima and integer sums: the same bits every call, per view whatever V is.
//
// A tile is MB_TILE consecutive pixels of the row-major image (not a rectangle): lane l of a wave takes pixel base + l, so a wave stores 64
// consecutive bytes of mask and 256 consecutive bytes of near / far whatever W is, and the view's base offset v H W needs no alignment.
//
// Precision: the ray is formed in fp64 from the fp32 table and rounded to fp32 once (the reference's .astype(np.float32)); everything behind
// it is fp64 and the library is built without contraction, so each operation rounds as numpy's does.  Results are rounded to fp32 once.
#include "common.h"

#include <cmath>

using namespace vanerf;

namespace {

constexpr int MB_BLOCK = 256;              // four waves
constexpr int MB_PER_THREAD = 4;           // pixels of a thread, MB_BLOCK apart
constexpr int MB_TILE = MB_BLOCK * MB_PER_THREAD;
constexpr int MB_MAX_EDGE = 4096;          // H W <= 2^24: n_mask and the rectangle are exact in the fp32 table
constexpr int MB_CAM = 24;                 // floats per camera: invK_T[9], RT[12], znear, zfar, pad

struct MbPart {                            // a block's partials: 48 bytes, written whole on every call
    double near_min, far_max;
    int32_t n, x0, x1, y0, y1, pad[3];
};
static_assert(sizeof(MbPart) == 48, "MbPart is three 16-byte words");

struct MbBounds { float b[6]; };

__device__ __forceinline__ double wave_min(double a)
{
    for (int m = 32; m >= 1; m >>= 1) { const double b = __shfl_xor(a, m); a = b < a ? b : a; }
    return a;
}
__device__ __forceinline__ double wave_max(double a)
{
    for (int m = 32; m >= 1; m >>= 1) { const double b = __shfl_xor(a, m); a = b > a ? b : a; }
    return a;
}
__device__ __forceinline__ int wave_min(int a)
{
    for (int m = 32; m >= 1; m >>= 1) a = min(a, __shfl_xor(a, m));
    return a;
}
__device__ __forceinline__ int wave_max(int a)
{
    for (int m = 32; m >= 1; m >>= 1) a = max(a, __shfl_xor(a, m));
    return a;
}
__device__ __forceinline__ int wave_sum(int a)
{
    for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m);
    return a;
}

struct MbAcc {
    double near_min, far_max;
    int n, x0, x1, y0, y1;
};

// Folds the block's accumulators (wave butterflies, then the four waves in order) into thread 0's copy.
__device__ __forceinline__ void block_fold(MbAcc& a)
{
    __shared__ double s_d[MB_BLOCK / 64][2];
    __shared__ int s_i[MB_BLOCK / 64][5];
    a.near_min = wave_min(a.near_min); a.far_max = wave_max(a.far_max);
    a.n = wave_sum(a.n); a.x0 = wave_min(a.x0); a.x1 = wave_max(a.x1); a.y0 = wave_min(a.y0); a.y1 = wave_max(a.y1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_d[wave][0] = a.near_min; s_d[wave][1] = a.far_max;
        s_i[wave][0] = a.n; s_i[wave][1] = a.x0; s_i[wave][2] = a.x1; s_i[wave][3] = a.y0; s_i[wave][4] = a.y1;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < MB_BLOCK / 64; ++w) {
        a.near_min = s_d[w][0] < a.near_min ? s_d[w][0] : a.near_min;
        a.far_max = s_d[w][1] > a.far_max ? s_d[w][1] : a.far_max;
        a.n += s_i[w][0];
        a.x0 = min(a.x0, s_i[w][1]); a.x1 = max(a.x1, s_i[w][2]); a.y0 = min(a.y0, s_i[w][3]); a.y1 = max(a.y1, s_i[w][4]);
    }
}

// Launch 1, one block per (tile, view).
__global__ __launch_bounds__(MB_BLOCK) void mb_tile_kernel(const float* __restrict__ cams, int H, int W, MbBounds B, uint8_t* __restrict__ mask,
                                                           float* __restrict__ near, float* __restrict__ far, MbPart* __restrict__ part)
{
    const int tile = blockIdx.x, v = blockIdx.y;
    const int npix = H * W;
    const float* cam = cams + (size_t)v * MB_CAM;
    double K[9], R[9], T[3];
    for (int k = 0; k < 9; ++k) K[k] = (double)cam[k];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (double)cam[9 + 4 * i + j];
        T[i] = (double)cam[9 + 4 * i + 3];
    }
    // o = -R^T T, kept in fp64 for the direction and rounded to fp32 for everything behind it
    double o64[3], o[3];
    for (int j = 0; j < 3; ++j) {
        o64[j] = -((R[j] * T[0] + R[3 + j] * T[1]) + R[6 + j] * T[2]);
        o[j] = (double)(float)o64[j];
    }
    // the box, widened by a centimetre, and the hit test's interval around it
    double b[6], lo[3], hi[3];
    for (int j = 0; j < 3; ++j) {
        b[j] = (double)B.b[j] + -0.01;
        b[3 + j] = (double)B.b[3 + j] + 0.01;
        lo[j] = b[j] - 1e-6;
        hi[j] = b[3 + j] + 1e-6;
    }
    const double nan = __longlong_as_double(0x7ff8000000000000LL), inf = __longlong_as_double(0x7ff0000000000000LL);
    MbAcc a = {inf, -inf, 0, W, -1, H, -1};
    const size_t base = (size_t)v * npix;
#pragma unroll 1 // one pixel's plane tests at a time: the fp64 work leaves nothing to overlap, and four unrolled copies cost registers
    for (int k = 0; k < MB_PER_THREAD; ++k) {
        const int i = tile * MB_TILE + k * MB_BLOCK + threadIdx.x;
        if (i >= npix) break;
        const int r = i / W, c = i - r * W;
        const double gx = (double)c, gy = (double)r;
        double pc[3], d[3];
        for (int j = 0; j < 3; ++j) pc[j] = ((gx * K[j] + gy * K[3 + j]) + K[6 + j]) - T[j];
        for (int j = 0; j < 3; ++j) {
            const float f = (float)(((pc[0] * R[j] + pc[1] * R[3 + j]) + pc[2] * R[6 + j]) - o64[j]);
            d[j] = (double)(fabsf(f) < 1e-5f ? 1e-5f : f);
        }
        int cnt = 0;
        double q0 = 0.0, q1 = 0.0; // squared distances of the first two hits from the origin
#pragma unroll
        for (int pl = 0; pl < 6; ++pl) {
            const int ax = pl % 3;
            const double t = (b[pl] - o[ax]) / d[ax];
            const double p0 = t * d[0] + o[0], p1 = t * d[1] + o[1], p2 = t * d[2] + o[2];
            const bool in = p0 >= lo[0] && p0 <= hi[0] && p1 >= lo[1] && p1 <= hi[1] && p2 >= lo[2] && p2 <= hi[2];
            const double e0 = p0 - o[0], e1 = p1 - o[1], e2 = p2 - o[2];
            const double q = (e0 * e0 + e1 * e1) + e2 * e2;
            q0 = (in && cnt == 0) ? q : q0;
            q1 = (in && cnt == 1) ? q : q1;
            cnt += in ? 1 : 0;
        }
        const bool hit = cnt == 2;
        double zn = nan, zf = nan;
        if (hit) {
            const double nd = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            const double d0 = sqrt(q0) / nd, d1 = sqrt(q1) / nd;
            zn = d0 < d1 ? d0 : d1;
            zf = d0 < d1 ? d1 : d0;
            a.near_min = zn < a.near_min ? zn : a.near_min;
            a.far_max = zf > a.far_max ? zf : a.far_max;
            ++a.n;
            a.x0 = min(a.x0, c); a.x1 = max(a.x1, c); a.y0 = min(a.y0, r); a.y1 = max(a.y1, r);
        }
        mask[base + i] = hit ? 1 : 0;
        if (near) near[base + i] = (float)zn;
        if (far) far[base + i] = (float)zf;
    }
    block_fold(a);
    if (threadIdx.x != 0) return;
    MbPart p; // ordinary stores: every slot of the block is written on every call
    p.near_min = a.near_min; p.far_max = a.far_max;
    p.n = a.n; p.x0 = a.x0; p.x1 = a.x1; p.y0 = a.y0; p.y1 = a.y1;
    p.pad[0] = p.pad[1] = p.pad[2] = 0;
    part[(size_t)v * gridDim.x + tile] = p;
}

// Launch 2, one block per view: thread t folds tiles t, t + 256, ..., then the block.
__global__ __launch_bounds__(MB_BLOCK) void mb_finish_kernel(const MbPart* __restrict__ part, int tiles, int H, int W, float* __restrict__ out)
{
    const int v = blockIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL), inf = __longlong_as_double(0x7ff0000000000000LL);
    MbAcc a = {inf, -inf, 0, W, -1, H, -1};
    for (int t = threadIdx.x; t < tiles; t += MB_BLOCK) {
        const MbPart& p = part[(size_t)v * tiles + t];
        a.near_min = p.near_min < a.near_min ? p.near_min : a.near_min;
        a.far_max = p.far_max > a.far_max ? p.far_max : a.far_max;
        a.n += p.n;
        a.x0 = min(a.x0, p.x0); a.x1 = max(a.x1, p.x1); a.y0 = min(a.y0, p.y0); a.y1 = max(a.y1, p.y1);
    }
    block_fold(a);
    if (threadIdx.x != 0) return;
    const bool empty = a.n == 0;
    float* o = out + (size_t)v * 8;
    o[0] = (float)(empty ? nan : a.near_min);
    o[1] = (float)(empty ? nan : a.far_max);
    o[2] = (float)a.n;
    o[3] = (float)(empty ? 0 : a.x0);
    o[4] = (float)(empty ? 0 : a.y0);
    o[5] = (float)(empty ? 0 : a.x1 - a.x0 + 1);
    o[6] = (float)(empty ? 0 : a.y1 - a.y0 + 1);
    o[7] = 0.0f;
}

bool shape_ok(int V, int H, int W) { return V > 0 && V <= 65535 && H >= 1 && W >= 1 && H <= MB_MAX_EDGE && W <= MB_MAX_EDGE; }

int64_t tiles_of(int H, int W) { return ((int64_t)H * W + MB_TILE - 1) / MB_TILE; }

} // namespace

extern "C" int64_t vanerf_mask_at_box_scratch(int V, int H, int W)
{
    if (!shape_ok(V, H, W)) return 0;
    return (int64_t)V * tiles_of(H, W) * (int64_t)sizeof(MbPart);
}

extern "C" int vanerf_mask_at_box(const float* cams, int V, int H, int W, const float* bounds, uint8_t* mask, float* near, float* far, void* scratch,
                                  int64_t scratch_bytes, float* out, void* stream)
{
    return guarded([&] {
        if (!cams || !bounds || !mask || !scratch || !out) throw_error("vanerf_mask_at_box: null argument");
        if (!shape_ok(V, H, W)) throw_error("vanerf_mask_at_box: V=%d H=%d W=%d (1 <= V <= 65535; 1 <= H, W <= %d)", V, H, W, MB_MAX_EDGE);
        if (reinterpret_cast<uintptr_t>(cams) % 4 != 0 || reinterpret_cast<uintptr_t>(near) % 4 != 0 || reinterpret_cast<uintptr_t>(far) % 4 != 0
            || reinterpret_cast<uintptr_t>(out) % 4 != 0)
            throw_error("vanerf_mask_at_box: cams, near, far and out must be 4-byte aligned");
        if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0) throw_error("vanerf_mask_at_box: scratch must be 16-byte aligned");
        const int64_t need = vanerf_mask_at_box_scratch(V, H, W);
        if (scratch_bytes < need) throw_error("vanerf_mask_at_box: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
        MbBounds B;
        for (int k = 0; k < 6; ++k) B.b[k] = bounds[k];
        const int tiles = (int)tiles_of(H, W);
        MbPart* part = static_cast<MbPart*>(scratch);
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(mb_tile_kernel, dim3((unsigned)tiles, (unsigned)V), dim3(MB_BLOCK), 0, st, cams, H, W, B, mask, near, far, part);
        hipLaunchKernelGGL(mb_finish_kernel, dim3((unsigned)V), dim3(MB_BLOCK), 0, st, (const MbPart*)part, tiles, H, W, out);
        HIP_CHECK(hipGetLastError());
    });
}
