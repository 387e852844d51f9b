// valu_rate_f64.hip - float64 VALU issue-rate probe for gfx950 (design input for the location search, which is
// v_add_f64 / v_mul_f64 without contraction).  Measures cycles per wave-instruction per SIMD and the chip-wide
// rate of v_add_f64, v_mul_f64 and v_fma_f64 at 1/2/4/8 waves per SIMD, 8 independent chains per lane.
#include <hip/hip_runtime.h>
#include <cstdio>

#define REP8(X) X X X X X X X X
template <int OP>
__global__ void __launch_bounds__(256) probe(double *out, int iters, unsigned long long *cyc)
{
    double a0 = threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
    double b = 1.0000001, c = 1e-9;
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < iters; i++) {
        if (OP == 0) { REP8(asm volatile("v_add_f64 %0, %0, %8\n v_add_f64 %1, %1, %8\n v_add_f64 %2, %2, %8\n v_add_f64 %3, %3, %8\n v_add_f64 %4, %4, %8\n v_add_f64 %5, %5, %8\n v_add_f64 %6, %6, %8\n v_add_f64 %7, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(c));) }
        if (OP == 1) { REP8(asm volatile("v_mul_f64 %0, %0, %8\n v_mul_f64 %1, %1, %8\n v_mul_f64 %2, %2, %8\n v_mul_f64 %3, %3, %8\n v_mul_f64 %4, %4, %8\n v_mul_f64 %5, %5, %8\n v_mul_f64 %6, %6, %8\n v_mul_f64 %7, %7, %8" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b));) }
        if (OP == 2) { REP8(asm volatile("v_fma_f64 %0, %0, %8, %9\n v_fma_f64 %1, %1, %8, %9\n v_fma_f64 %2, %2, %8, %9\n v_fma_f64 %3, %3, %8, %9\n v_fma_f64 %4, %4, %8, %9\n v_fma_f64 %5, %5, %8, %9\n v_fma_f64 %6, %6, %8, %9\n v_fma_f64 %7, %7, %8, %9" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c));) }
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * 256 + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
    if (threadIdx.x == 0 && blockIdx.x == 0) *cyc = t1 - t0;
}

template <int OP>
void run(const char *name)
{
    double *out; unsigned long long *cyc, hc;
    hipMalloc(&out, 256 * 8 * 256 * sizeof(double)); hipMalloc(&cyc, 8);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int iters = 2000;
    for (int wps : {1, 2, 4, 8}) {      // waves per SIMD = blocks of 256 threads per CU
        int blocks = 256 * wps;
        probe<OP><<<blocks, 256>>>(out, 10, cyc);
        hipDeviceSynchronize();
        hipEventRecord(e0);
        probe<OP><<<blocks, 256>>>(out, iters, cyc);
        hipEventRecord(e1); hipDeviceSynchronize();
        float ms; hipEventElapsedTime(&ms, e0, e1);
        hipMemcpy(&hc, cyc, 8, hipMemcpyDeviceToHost);
        double instr_per_wave = (double)iters * 64;
        double cyc_per_instr_per_simd = (double)hc / (instr_per_wave * wps);
        double tops = (double)blocks * 4 * instr_per_wave * 64 / (ms * 1e-3) / 1e12;
        printf("%-10s waves/SIMD %d: %.2f cycles per wave-instr per SIMD (memtime), %.3f ms, %.2f T lane-ops/s, eff clock %.2f GHz\n",
               name, wps, cyc_per_instr_per_simd, ms, tops, (double)hc / (ms * 1e-3) / 1e9);
    }
}

int main()
{
    run<0>("v_add_f64");
    run<1>("v_mul_f64");
    run<2>("v_fma_f64");
    return 0;
}
