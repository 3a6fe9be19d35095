// Micro-benchmark (diagnostics): SIMD cycles of the depthwise 3x3 stencil body of the DS-CNN unit (kws_dscnn_stages.h) in its two
// forms -- eleven instructions with the ten weights in ten registers, twelve with every weight taken through row_newbcast from
// one register that a row of lanes shares -- with one and two wavefronts per SIMD, alone and beside one
// v_mfma_f32_32x32x16_f16 per about 30 issue slots (three per eight bodies).  Eight independent accumulator sets per wavefront.
//   hipcc --offload-arch=gfx950 -O2 tools/dw_stencil_rate.hip -o tools/bin/dw_stencil_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float body_regs(const float* w, float up, float mid, float dn, float ml, float mr) {
    float c, tr, tl;
    asm volatile("v_mul_f32 %1, %3, %13\n\t"
                 "v_mul_f32 %2, %5, %13\n\t"
                 "v_fma_f32 %0, %4, %13, %12\n\t"
                 "v_fmac_f32 %1, %6, %14\n\t"
                 "v_fmac_f32 %2, %8, %14\n\t"
                 "v_fmac_f32 %0, %7, %14\n\t"
                 "v_fmac_f32 %1, %9, %15\n\t"
                 "v_fmac_f32 %2, %11, %15\n\t"
                 "v_fmac_f32 %0, %10, %15\n\t"
                 "v_fmac_f32_dpp %0, %1, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %0, %2, %17 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                 : "=&v"(c), "=&v"(tr), "=&v"(tl)
                 : "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]), "v"(w[7]), "v"(w[8]), "v"(w[9]), "v"(up),
                   "v"(mid), "v"(dn), "v"(ml), "v"(mr));
    return c;
}
__device__ __forceinline__ float body_row(float w, float up, float mid, float dn, float ml, float mr) {
    float c, tr, tl;
    asm volatile("v_mov_b32_dpp %0, %3 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %1, %3, %4 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mul_f32_dpp %2, %3, %4 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f32_dpp %0, %3, %4 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f32_dpp %1, %3, %5 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f32_dpp %2, %3, %5 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f32_dpp %0, %3, %5 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f32_dpp %1, %3, %6 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f32_dpp %2, %3, %6 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f32_dpp %0, %3, %6 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f32_dpp %0, %1, %7 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                 "v_fmac_f32_dpp %0, %2, %8 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                 : "=&v"(c), "=&v"(tr), "=&v"(tl)
                 : "v"(w), "v"(up), "v"(mid), "v"(dn), "v"(ml), "v"(mr));
    return c;
}

template <bool ROW, bool MFMA>
__global__ void k_stencil(float* out, unsigned long long* cyc, int iters) {
    const int lane = threadIdx.x & 63;
    float w[10];
    for (int i = 0; i < 10; ++i) w[i] = 0.05f + 0.01f * (ROW ? (lane & 15) : i);  // (tap i: the same value either way)
    const float mid = 0.5f + lane * 1e-3f, dn = 0.25f - lane * 1e-3f, ml = lane ? 1.f : 0.f, mr = lane < 63 ? 1.f : 0.f;
    float f[8];
    for (int i = 0; i < 8; ++i) f[i] = threadIdx.x * 1e-3f + i;
    floatx16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    halfx8 a, b;
    for (int i = 0; i < 8; ++i) a[i] = (_Float16)(0.01f * (lane + i)), b[i] = (_Float16)(0.02f * i);
    __syncthreads();
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                f[i] = ROW ? body_row(w[0], f[i], mid, dn, ml, mr) : body_regs(w, f[i], mid, dn, ml, mr);
                __builtin_amdgcn_sched_barrier(0);
                if (MFMA && (i == 2 || i == 5 || i == 7)) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0;
    for (int i = 0; i < 8; ++i) s += f[i];
    for (int i = 0; i < 16; ++i) s += acc[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (lane == 0) cyc[blockIdx.x * 16 + (threadIdx.x >> 6)] = t1 - t0;
}

template <typename K>
double run(K kern, int threads, float* check) {
    const int grid = 256, iters = 64;
    float* out; unsigned long long* cyc;
    (void)hipMalloc(&out, sizeof(float) * grid * threads);
    (void)hipMalloc(&cyc, sizeof(unsigned long long) * grid * 16);
    for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), 0, 0, out, cyc, iters);
    (void)hipDeviceSynchronize();
    std::vector<unsigned long long> h(grid * 16);
    (void)hipMemcpy(h.data(), cyc, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost);
    (void)hipMemcpy(check, out + 37, sizeof(float), hipMemcpyDeviceToHost);
    double m = 0; int n = 0;
    for (int g = 0; g < grid; ++g) for (int w = 0; w < threads / 64; ++w) { m += h[g * 16 + w]; ++n; }
    (void)hipFree(out); (void)hipFree(cyc);
    return m / n / (iters * 32.0);  // s_memtime ticks per body and wavefront
}
int main() {
    printf("s_memtime ticks (the unit of profiles/r03_valu_rates.txt) per stencil body and wavefront; x waves/SIMD = the SIMD's cost of a body in the same unit\n");
    printf("%-34s %10s %10s %12s\n", "body", "1 wave", "2 waves", "2 waves SIMD");
    float c0, c1;
    auto row = [&](const char* name, auto k) {
        const double a1 = run(k, 256, &c0), a2 = run(k, 512, &c1);
        printf("%-34s %10.4f %10.4f %12.4f   (value %.6g)\n", name, a1, a2, a2 / 2, c0);
    };
    row("11 instr, weights in registers", k_stencil<false, false>);
    row("12 instr, row_newbcast", k_stencil<true, false>);
    row("11 instr + 3 MFMA per 8 bodies", k_stencil<false, true>);
    row("12 instr + 3 MFMA per 8 bodies", k_stencil<true, true>);
    return 0;
}
