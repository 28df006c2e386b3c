// What does one packed f32 VALU instruction (v_pk_mul_f32 / v_pk_add_f32: two IEEE f32 operations per lane) cost on gfx950 against one
// scalar v_mul_f32 / v_add_f32, in a VALU-only stream (no MFMA anywhere)?  Each loop iteration issues 16 instructions of one kind, on 8
// independent registers (pairs) or on one dependent chain, at 1, 2 and 4 waves per SIMD (256-thread blocks: one wave per SIMD per block).
// Reports core cycles per instruction per wave (s_memtime) and SIMD throughput (instructions per SIMD per ns, from the kernel time).
// mesh_query_accel_kernel is VALU-issue bound: packing its two depths pays if a packed op costs well under two scalar ones.
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int OP, bool DEP> __global__ __launch_bounds__(256) void k(float* out, long long* cyc, int iters)
{
    const float y = 1.0f + threadIdx.x * 1e-9f;
    const f32x2 y2 = {y, y};
    float v[8];
    f32x2 w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { v[i] = threadIdx.x * 1e-3f + i; w[i] = f32x2{v[i], v[i] + 0.5f}; }
    const long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = DEP ? 0 : j % 8;
            if constexpr (OP == 0) asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(w[i]) : "v"(y2));
            else if constexpr (OP == 1) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(w[i]) : "v"(y2));
            else if constexpr (OP == 2) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(v[i]) : "v"(y));
            else asm volatile("v_add_f32 %0, %0, %1" : "+v"(v[i]) : "v"(y));
        }
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i] + w[i].x + w[i].y;
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

template <int OP, bool DEP> void run(int waves_per_simd)
{
    int ncu = 0;
    hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0);
    const int nb = ncu * waves_per_simd, iters = 20000;
    float* out;
    long long* cyc;
    hipMalloc(&out, (size_t)nb * 256 * 4);
    hipMalloc(&cyc, (size_t)nb * 8);
    hipLaunchKernelGGL((k<OP, DEP>), dim3(nb), dim3(256), 0, 0, out, cyc, 100); // warm-up (code object load)
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipEventRecord(e0);
    hipLaunchKernelGGL((k<OP, DEP>), dim3(nb), dim3(256), 0, 0, out, cyc, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0.0f;
    hipEventElapsedTime(&ms, e0, e1);
    static long long h[65536];
    hipMemcpy(h, cyc, (size_t)nb * 8, hipMemcpyDeviceToHost);
    double m = 0.0;
    for (int i = 0; i < nb; ++i) m += h[i];
    m /= nb;
    const double n_inst = (double)iters * 16;
    const char* ops[] = {"v_pk_mul_f32", "v_pk_add_f32", "v_mul_f32", "v_add_f32"};
    printf("%-13s %-11s %d wave(s)/SIMD: %6.2f cycles per instruction per wave, %6.3f instructions per SIMD per ns, %7.1f f32 ops per SIMD per ns\n", ops[OP],
           DEP ? "dependent" : "independent", waves_per_simd, m / n_inst, n_inst * waves_per_simd / (ms * 1e6),
           n_inst * waves_per_simd * (OP < 2 ? 2 : 1) * 64 / (ms * 1e6));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipFree(out);
    hipFree(cyc);
}

int main()
{
    for (int wps : {1, 2, 4}) {
        run<0, false>(wps); run<2, false>(wps); run<1, false>(wps); run<3, false>(wps);
        run<0, true>(wps); run<2, true>(wps); run<1, true>(wps); run<3, true>(wps);
    }
    return 0;
}
