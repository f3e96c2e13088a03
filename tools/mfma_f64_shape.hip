// Micro-benchmark: float64 matrix against vector arithmetic on gfx950 at one output tile per wave,
// for the choice of the float64 window gridder's form.  The tile is 16 x 16 doubles
// (a 16 x 8 complex128 block of the window):
//   mfma: v_mfma_f64_16x16x4_f64, 4 independent accumulators of 4 doubles per lane, 2048 FLOP per
//         instruction (K = 4 carries (Re a, Im a) of two visibilities, as the float32 pair form);
//   valu: v_fma_f64 on the same 4 accumulators x 4 doubles per lane, 128 FLOP per instruction.
// Bare loops, operands in registers, 1 .. 4 waves per SIMD; reports TFLOP/s per form.
//   hipcc -O3 --offload-arch=gfx950 tools/mfma_f64_shape.hip -o mfma_f64_shape && ./mfma_f64_shape
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <bool MFMA>
__global__ __launch_bounds__(256) void k(double *out, int iters, double seed)
{
    const double a = seed + threadIdx.x * 1e-3, b = seed - threadIdx.x * 1e-3;
    f64x4 c[4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) c[i][j] = 0.0;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (MFMA) {
                c[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a + i, b, c[i], 0, 0, 0);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    c[i][j] = fma(a + i, b, c[i][j]);
            }
        }
    }
    double s = 0.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) s += c[i][j];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <bool MFMA>
double run(int waves_per_simd, double *out)
{
    int cus = 0;
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
    const int iters = 20000;
    const int blocks = cus * waves_per_simd;          // 4 waves (256 threads) per block: one per SIMD
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    k<MFMA><<<blocks, 256>>>(out, 100, 1.0);
    hipEventRecord(e0);
    k<MFMA><<<blocks, 256>>>(out, iters, 1.0);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    // per wave per iteration: mfma 4 x 2048 FLOP; valu 16 x 128 FLOP
    const double flop_per_wave_iter = MFMA ? 4.0 * 2048 : 16.0 * 128;
    return flop_per_wave_iter * iters * blocks * 4 / (ms * 1e-3) / 1e12;
}

int main()
{
    double *out = nullptr;
    hipMalloc(&out, 256 * 4 * 1024 * sizeof(double));
    for (int w = 1; w <= 4; w++)
        printf("waves/SIMD %d: v_mfma_f64_16x16x4_f64 %6.1f TFLOP/s   v_fma_f64 %6.1f TFLOP/s\n", w,
               run<true>(w, out), run<false>(w, out));
    hipFree(out);
    return 0;
}
