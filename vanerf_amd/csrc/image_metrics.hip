// image_metrics.hip -- the scores of the reference's validation / test steps for V rendered views, on the device: MSE, PSNR and scikit-image's
// SSIM on the crop to the bounding rectangle of mask_at_box (Evaluator.compute_score, src/evaluator.py:84-114), and kornia's masked PSNR and
// Gaussian SSIM (compute_test_metric, src/model.py:210-235).  Neither library is a dependency: the arithmetic is restated with a fully specified
// definition (the comment of vanerf_image_metrics in the header), parity against kornia 0.7.1 / scikit-image 0.16.2 is
// unpinned.  The restatement the tests hold these kernels to is the fp64 numpy code of tests/test_image_metrics.py.
//
// Three launches: the bounding rectangle and mask count per view (integers only), the window moments and S per pixel with one block per
// 32 x 32 tile, the sum of the tiles' partials in a fixed order.  No atomics, no device globals: the same bits every call.
//
// Precision: the window moments, S and the sums are fp64.  The products of two fp32 values are exact in fp64, so sigma = E[x^2] - mu^2 loses
// nothing to cancellation (in fp32 it loses ~1e-7 / (sigma + C2), 1e-4 of S on a flat patch), and the sum of 3 H W squares holds the 1e-7 the
// tests ask of mse; what is left is the one rounding of each result to fp32.
#include "common.h"

#include <cmath>

using namespace vanerf;

namespace {

constexpr int IM_T = 32;                  // pixel tile edge
constexpr int IM_R = 3;                   // window radius: 7 x 7 windows
constexpr int IM_S = IM_T + 2 * IM_R;     // staged tile edge (38)
constexpr int IM_BLOCK = 256;             // four waves; a thread takes IM_T * IM_T / IM_BLOCK = 4 pixels
constexpr int IM_HDR = 8;                 // int32 per view at the head of the scratch block: x, y, w, h of the rectangle, n_mask
constexpr int IM_PART = 4;                // doubles per (view, tile): sum d^2, sum d^2 [mask], sum S_gauss [mask], sum S_uniform [valid windows]
constexpr int IM_MAX_EDGE = 4096;         // n_mask <= 2^24 is exact in the fp32 table

struct ImWindow {
    double g[2 * IM_R + 1]; // the normalised 1-D Gaussian, sigma 1.5
};

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
__device__ __forceinline__ double wave_sum(double a)
{
    for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m); // a fixed butterfly: every lane ends with the same bits
    return a;
}

// Launch 1, one block per view: cv2.boundingRect of the nonzero pixels of mask_at_box (the whole image without one; w = h = 0 for an empty
// mask) and the number of nonzero pixels of mask (H W without one).
__global__ __launch_bounds__(IM_BLOCK) void im_box_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ box, int H, int W,
                                                          int32_t* __restrict__ hdr)
{
    __shared__ int s_red[IM_BLOCK / 64][5];
    const int v = blockIdx.x, npix = H * W;
    int x0 = W, y0 = H, x1 = -1, y1 = -1, n = 0;
    if (mask || box) {
        const uint8_t* m = mask ? mask + (size_t)v * npix : nullptr;
        const uint8_t* b = box ? box + (size_t)v * npix : nullptr;
        for (int i = threadIdx.x; i < npix; i += IM_BLOCK) {
            if (m && m[i]) ++n;
            if (b && b[i]) {
                const int r = i / W, c = i - r * W;
                x0 = min(x0, c); x1 = max(x1, c);
                y0 = min(y0, r); y1 = max(y1, r);
            }
        }
    }
    x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1); n = wave_sum(n);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = x0; s_red[wave][1] = y0; s_red[wave][2] = x1; s_red[wave][3] = y1; s_red[wave][4] = n;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < IM_BLOCK / 64; ++w) {
        x0 = min(x0, s_red[w][0]); y0 = min(y0, s_red[w][1]); x1 = max(x1, s_red[w][2]); y1 = max(y1, s_red[w][3]); n += s_red[w][4];
    }
    int32_t* h = hdr + (size_t)v * IM_HDR;
    if (!box) { x0 = 0; y0 = 0; x1 = W - 1; y1 = H - 1; }
    const bool empty = x1 < x0;
    h[0] = empty ? 0 : x0;
    h[1] = empty ? 0 : y0;
    h[2] = empty ? 0 : x1 - x0 + 1;
    h[3] = empty ? 0 : y1 - y0 + 1;
    h[4] = mask ? n : npix;
    h[5] = h[6] = h[7] = 0;
}

// torch's `reflect` about the border without repeating the edge pixel.  One reflection is exact for -3 <= i <= n + 2 with n >= 4, the range the
// windows of in-image pixels reach; the rest of a staged tile that hangs over the image is never read by them and is clamped into the image.
__device__ __forceinline__ int reflect_index(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// Launch 2, one block per (tile, view).  The tile and its 3-pixel halo of pred and gt are staged in LDS channel by channel (38 x 38 floats
// each).  A wave's two 32-lane halves each read 32 consecutive dwords of one staged row per tap, so the 38-dword row stride costs no bank
// conflict (ds_read_b32 banks are address / 4 mod 32 within a half).  Per pixel and channel the five moments of both windows are summed
// over the 49 taps row by row (the Gaussian is the outer product of g with itself: a row's sums weighted by g[dx], the rows by g[dy]).
__global__ __launch_bounds__(IM_BLOCK) void im_tile_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           const uint8_t* __restrict__ mask, int H, int W, int clamp_pred, double C1g,
                                                           double C2g, ImWindow win, const int32_t* __restrict__ hdr,
                                                           double* __restrict__ part)
{
    __shared__ float s_x[IM_S * IM_S], s_y[IM_S * IM_S];
    __shared__ double s_red[IM_BLOCK / 64][IM_PART];
    __shared__ double s_g[2 * IM_R + 1]; // the row weights, indexed by the rolled row loop (the column weights stay in SGPRs)
    if (threadIdx.x < 2 * IM_R + 1) s_g[threadIdx.x] = win.g[threadIdx.x];
    const int tiles_x = (W + IM_T - 1) / IM_T;
    const int tile = blockIdx.x, v = blockIdx.y;
    const int c0 = (tile % tiles_x) * IM_T, r0 = (tile / tiles_x) * IM_T;
    const size_t npix = (size_t)H * W;
    const int32_t* h = hdr + (size_t)v * IM_HDR;
    const int bx = h[0], by = h[1], bw = h[2], bh = h[3];
    const bool box_ok = bw >= 2 * IM_R + 1 && bh >= 2 * IM_R + 1;
    constexpr double C1u = (0.01 * 2.0) * (0.01 * 2.0), C2u = (0.03 * 2.0) * (0.03 * 2.0); // data_range 2
    constexpr double NW = (2 * IM_R + 1) * (2 * IM_R + 1), COV = NW / (NW - 1.0);
    double a_sse = 0.0, a_ssem = 0.0, a_sg = 0.0, a_su = 0.0;
#pragma unroll 1
    for (int ch = 0; ch < 3; ++ch) {
        const float* px = pred + ((size_t)v * 3 + ch) * npix;
        const float* py = gt + ((size_t)v * 3 + ch) * npix;
        __syncthreads(); // the previous channel's readers are done
        for (int i = threadIdx.x; i < IM_S * IM_S; i += IM_BLOCK) {
            const int rr = i / IM_S, cc = i - rr * IM_S;
            const size_t at = (size_t)reflect_index(r0 - IM_R + rr, H) * W + reflect_index(c0 - IM_R + cc, W);
            float x = px[at];
            if (clamp_pred) x = fminf(fmaxf(x, 0.0f), 1.0f);
            s_x[i] = x;
            s_y[i] = py[at];
        }
        __syncthreads();
#pragma unroll 1 // one pixel's 20 fp64 accumulators at a time
        for (int k = 0; k < IM_T * IM_T / IM_BLOCK; ++k) {
            const int p = k * IM_BLOCK + threadIdx.x;
            const int lr = p / IM_T, lc = p % IM_T;
            const int r = r0 + lr, c = c0 + lc;
            if (r >= H || c >= W) continue;
            double gx = 0.0, gy = 0.0, gxx = 0.0, gyy = 0.0, gxy = 0.0; // Gaussian moments
            double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0; // sums of the uniform window
#pragma unroll 1 // a row of taps at a time: unrolled, the 98 staged values of a window are all loaded and widened up front (256 VGPRs and scratch)
            for (int dy = 0; dy < 2 * IM_R + 1; ++dy) {
                double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
                double tx = 0.0, ty = 0.0, txx = 0.0, tyy = 0.0, txy = 0.0;
#pragma unroll
                for (int dx = 0; dx < 2 * IM_R + 1; ++dx) {
                    const double x = (double)s_x[(lr + dy) * IM_S + lc + dx], y = (double)s_y[(lr + dy) * IM_S + lc + dx];
                    const double xx = x * x, yy = y * y, xy = x * y; // exact: 24-bit factors
                    const double w = win.g[dx];
                    hx = fma(w, x, hx); hy = fma(w, y, hy); hxx = fma(w, xx, hxx); hyy = fma(w, yy, hyy); hxy = fma(w, xy, hxy);
                    tx += x; ty += y; txx += xx; tyy += yy; txy += xy;
                }
                const double w = s_g[dy];
                gx = fma(w, hx, gx); gy = fma(w, hy, gy); gxx = fma(w, hxx, gxx); gyy = fma(w, hyy, gyy); gxy = fma(w, hxy, gxy);
                ux += tx; uy += ty; uxx += txx; uyy += tyy; uxy += txy;
            }
            const double x = (double)s_x[(lr + IM_R) * IM_S + lc + IM_R], y = (double)s_y[(lr + IM_R) * IM_S + lc + IM_R];
            const double d2 = (x - y) * (x - y);
            a_sse += d2;
            if (!mask || mask[(size_t)v * npix + (size_t)r * W + c]) {
                const double s1 = gxx - gx * gx, s2 = gyy - gy * gy, s12 = gxy - gx * gy; // no sample correction
                const double num = (2.0 * gx * gy + C1g) * (2.0 * s12 + C2g);
                const double den = (gx * gx + gy * gy + C1g) * (s1 + s2 + C2g);
                a_ssem += d2;
                a_sg += num / (den + 1e-12);
            }
            if (box_ok && r - IM_R >= by && r + IM_R < by + bh && c - IM_R >= bx && c + IM_R < bx + bw) {
                const double mx = ux / NW, my = uy / NW;
                const double vx = COV * (uxx / NW - mx * mx), vy = COV * (uyy / NW - my * my), vxy = COV * (uxy / NW - mx * my);
                a_su += ((2.0 * mx * my + C1u) * (2.0 * vxy + C2u)) / ((mx * mx + my * my + C1u) * (vx + vy + C2u));
            }
        }
    }
    a_sse = wave_sum(a_sse); a_ssem = wave_sum(a_ssem); a_sg = wave_sum(a_sg); a_su = wave_sum(a_su);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = a_sse; s_red[wave][1] = a_ssem; s_red[wave][2] = a_sg; s_red[wave][3] = a_su;
    }
    __syncthreads();
    if (threadIdx.x < IM_PART) { // ordinary stores: every slot of the block is written on every call
        double s = s_red[0][threadIdx.x];
        for (int w = 1; w < IM_BLOCK / 64; ++w) s += s_red[w][threadIdx.x];
        part[((size_t)v * gridDim.x + tile) * IM_PART + threadIdx.x] = s;
    }
}

// Launch 3, one block per view: thread t adds tiles t, t + 256, ... in ascending order, then the fixed butterfly and the waves in order.
__global__ __launch_bounds__(IM_BLOCK) void im_finish_kernel(const int32_t* __restrict__ hdr, const double* __restrict__ part, int tiles, int H,
                                                             int W, double max_val, float* __restrict__ out)
{
    __shared__ double s_red[IM_BLOCK / 64][IM_PART];
    const int v = blockIdx.x;
    double a[IM_PART] = {0.0, 0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < tiles; t += IM_BLOCK) {
        const double* p = part + ((size_t)v * tiles + t) * IM_PART;
        for (int k = 0; k < IM_PART; ++k) a[k] += p[k];
    }
    for (int k = 0; k < IM_PART; ++k) a[k] = wave_sum(a[k]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < IM_PART; ++k) s_red[wave][k] = a[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < IM_BLOCK / 64; ++w)
        for (int k = 0; k < IM_PART; ++k) a[k] += s_red[w][k];
    const int32_t* h = hdr + (size_t)v * IM_HDR;
    const int bw = h[2], bh = h[3], nm = h[4];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double mse = a[0] / (3.0 * (double)H * (double)W);
    float* o = out + (size_t)v * 8;
    o[0] = (float)mse;
    o[1] = (float)(-10.0 * log10(mse));
    const bool box_ok = bw >= 2 * IM_R + 1 && bh >= 2 * IM_R + 1;
    o[2] = (float)(box_ok ? a[3] / (3.0 * (double)(bw - 2 * IM_R) * (double)(bh - 2 * IM_R)) : nan);
    o[3] = (float)(nm > 0 ? 10.0 * log10(max_val * max_val / (a[1] / (3.0 * (double)nm))) : nan);
    o[4] = (float)(nm > 0 ? a[2] / (3.0 * (double)nm) : nan);
    o[5] = (float)nm;
    o[6] = (float)bw;
    o[7] = (float)bh;
}

bool shape_ok(int V, int H, int W)
{
    return V > 0 && V <= 65535 && H >= 4 && W >= 4 && H <= IM_MAX_EDGE && W <= IM_MAX_EDGE;
}

int64_t tiles_of(int H, int W) { return (int64_t)((W + IM_T - 1) / IM_T) * ((H + IM_T - 1) / IM_T); }

} // namespace

extern "C" int64_t vanerf_image_metrics_scratch(int V, int H, int W)
{
    if (!shape_ok(V, H, W)) return 0;
    return (int64_t)V * IM_HDR * (int64_t)sizeof(int32_t) + (int64_t)V * tiles_of(H, W) * IM_PART * (int64_t)sizeof(double);
}

extern "C" int vanerf_image_metrics(const float* pred, const float* gt, const uint8_t* mask, const uint8_t* mask_at_box, int V, int H, int W,
                                    double max_val, int clamp_pred, void* scratch, int64_t scratch_bytes, float* out, void* stream)
{
    return guarded([&] {
        if (!pred || !gt || !scratch || !out) throw_error("vanerf_image_metrics: null argument");
        if (!shape_ok(V, H, W))
            throw_error("vanerf_image_metrics: V=%d H=%d W=%d (1 <= V <= 65535; 4 <= H, W <= %d: reflect padding by 3 needs 4 pixels)", V, H, W,
                        IM_MAX_EDGE);
        if (!(max_val > 0.0) || !std::isfinite(max_val)) throw_error("vanerf_image_metrics: max_val=%g (positive and finite)", max_val);
        if (reinterpret_cast<uintptr_t>(pred) % 4 != 0 || reinterpret_cast<uintptr_t>(gt) % 4 != 0 || reinterpret_cast<uintptr_t>(out) % 4 != 0)
            throw_error("vanerf_image_metrics: pred, gt and out must be 4-byte aligned");
        if (reinterpret_cast<uintptr_t>(scratch) % 16 != 0) throw_error("vanerf_image_metrics: scratch must be 16-byte aligned");
        const int64_t need = vanerf_image_metrics_scratch(V, H, W);
        if (scratch_bytes < need)
            throw_error("vanerf_image_metrics: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
        ImWindow win;
        double sum = 0.0;
        for (int k = 0; k < 2 * IM_R + 1; ++k) {
            const double d = (double)(k - IM_R);
            win.g[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
            sum += win.g[k];
        }
        for (int k = 0; k < 2 * IM_R + 1; ++k) win.g[k] /= sum;
        const double C1g = (0.01 * max_val) * (0.01 * max_val), C2g = (0.03 * max_val) * (0.03 * max_val);
        int32_t* hdr = static_cast<int32_t*>(scratch);
        double* part = reinterpret_cast<double*>(hdr + (size_t)V * IM_HDR); // V * 32 bytes in: 16-byte aligned
        const int tiles = (int)tiles_of(H, W);
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(im_box_kernel, dim3((unsigned)V), dim3(IM_BLOCK), 0, st, mask, mask_at_box, H, W, hdr);
        hipLaunchKernelGGL(im_tile_kernel, dim3((unsigned)tiles, (unsigned)V), dim3(IM_BLOCK), 0, st, pred, gt, mask, H, W, clamp_pred, C1g, C2g, win,
                           (const int32_t*)hdr, part);
        hipLaunchKernelGGL(im_finish_kernel, dim3((unsigned)V), dim3(IM_BLOCK), 0, st, (const int32_t*)hdr, (const double*)part, tiles, H, W, max_val,
                           out);
        HIP_CHECK(hipGetLastError());
    });
}
