// Micro-benchmark: the clock the chip holds on the two f32-input MFMA shapes of gfx950 at the same
// output tile per wave -- a 32 x 64-float window, the gridder's float32 accumulators:
//   32x32: 2 tiles of v_mfma_f32_32x32x2_f32 (16 regs each), 2 instructions per visibility;
//   16x16: 8 tiles of v_mfma_f32_16x16x4_f32 (4 regs each), 8 instructions per PAIR of visibilities.
// Both are 128 SIMD cycles per visibility.  Bare loops, operands in registers with random bits,
// 3 waves per SIMD (12-wave blocks, one per CU), with and without 4 VALU instructions per visibility
// feeding the operands (v_mul_f32 + v_fmac_f32 for A, v_pk_mul_f32 for B, v_lshl_add_u64 -- the
// gridder's hot loop).  Reports the wall time per launch and, from s_memtime / s_memrealtime stamps
// around each wave's loop (lane 0, a buffer of their own), the wave's cycles and the in-kernel clock.
//   hipcc -O3 --offload-arch=gfx950 tools/mfma_f32_shape.hip -o mfma_f32_shape && ./mfma_f32_shape
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <stdio.h>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

__device__ inline unsigned hash(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ inline float rnd(unsigned x)       // uniform in [-1, 1)
{
    return (float) (int) hash(x) * (1.0f / 2147483648.0f);
}

// one visibility's operands: A from (c, kv) by two VALU, B from b times a sign by one v_pk_mul_f32;
// the 64-bit add stands for the LDS address.  (c0 - a keeps the values bounded and random.)
#define OPERANDS(a, b, c0, c1, kv0, kv1, bs, adr, inc)                                               \
    if (VALU) {                                                                                    \
        asm volatile("v_mul_f32 %0, %2, %3\n v_fmac_f32 %0, %4, %5\n v_pk_mul_f32 %1, %1, %6\n"      \
                     "v_lshl_add_u64 %7, %7, 0, %8"                                                \
                     : "=&v"(a), "+v"(b), "+v"(c0), "+v"(kv0), "+v"(c1), "+v"(kv1), "+v"(bs), "+v"(adr) \
                     : "v"(inc));                                                                   \
    }

template <bool PAIRS, bool VALU>
__global__ __launch_bounds__(768) void k(float *out, long long *stamps, int iters, unsigned seed)
{
    const unsigned id = (blockIdx.x * blockDim.x + threadIdx.x) * 64u + seed;
    float a[4], c0[4], c1[4], kv0[4], kv1[4];
    v2f b[4], bs;
    for (int i = 0; i < 4; i++) {
        a[i] = rnd(id + i); c0[i] = rnd(id + 8 + i); c1[i] = rnd(id + 16 + i);
        kv0[i] = rnd(id + 24 + i); kv1[i] = rnd(id + 32 + i);
        b[i] = v2f{rnd(id + 40 + i), rnd(id + 48 + i)};
    }
    bs = v2f{-1.0f, -1.0f};
    unsigned long long adr = id, inc = seed | 1u;
    f32x16 t0, t1;
    f32x4 q[8];
    for (int j = 0; j < 16; j++) t0[j] = t1[j] = 0.0f;
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) q[i][j] = 0.0f;
    const long long m0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; it++) {
        // 4 visibilities per iteration: 8 x 32x32x2 or 2 pairs x 8 x 16x16x4 (512 SIMD cycles)
#pragma unroll
        for (int v = 0; v < 4; v++)
            OPERANDS(a[v], b[v], c0[v], c1[v], kv0[v], kv1[v], bs, adr, inc);
        __builtin_amdgcn_sched_barrier(0);
        if (!PAIRS) {
#pragma unroll
            for (int v = 0; v < 4; v++) {
                t0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[v], b[v].x, t0, 0, 0, 0);
                t1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[v], b[v].y, t1, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int p = 0; p < 2; p++)
#pragma unroll
                for (int t = 0; t < 8; t++)     // (2 row blocks, each A; 4 column blocks, each B)
                    q[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2 * p + (t >> 2)],
                                                               (t & 1) ? b[2 * p + (t >> 2)].y : b[2 * p + (t >> 2)].x,
                                                               q[t], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    const long long m1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float s = (float) (adr & 1) + bs.x;
    for (int i = 0; i < 4; i++) s += a[i] + b[i].x + b[i].y;
    for (int j = 0; j < 16; j++) s += t0[j] + t1[j];
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) s += q[i][j];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) {
        const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        stamps[2 * w] = m1 - m0;
        stamps[2 * w + 1] = r1 - r0;
    }
}

template <bool PAIRS, bool VALU>
void run(float *out, long long *stamps, int cus, const char *name)
{
    const int iters = 16384, waves = cus * 12;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    // >= 2 s of back-to-back launches before the timed ones (the clock settles under load)
    const auto t0 = std::chrono::steady_clock::now();
    int warm = 0;
    while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 2.0) {
        for (int i = 0; i < 20; i++)
            k<PAIRS, VALU><<<cus, 768>>>(out, stamps, iters, 1234u + warm++);
        hipDeviceSynchronize();
    }
    std::vector<float> ms(7);
    std::vector<double> clk;
    std::vector<double> cyc;
    std::vector<long long> h(2 * waves);
    for (int r = 0; r < 7; r++) {
        hipEventRecord(e0);
        k<PAIRS, VALU><<<cus, 768>>>(out, stamps, iters, 77u + r);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        hipEventElapsedTime(&ms[r], e0, e1);
        if (r == 6) {
            hipMemcpy(h.data(), stamps, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
            for (int w = 0; w < waves; w++) {
                clk.push_back(h[2 * w + 1] > 0 ? (double) h[2 * w] / h[2 * w + 1] * 100.0 : 0.0);
                cyc.push_back((double) h[2 * w] / iters / 4);   // wave cycles per visibility
            }
        }
    }
    std::sort(ms.begin(), ms.end());
    std::sort(clk.begin(), clk.end());
    std::sort(cyc.begin(), cyc.end());
    // 4 visibilities x 3 waves per SIMD x 128 MFMA cycles per visibility
    const double mfma_cycles = (double) iters * 4 * 3 * 128;
    const double med = ms[3];
    printf("%-22s wall %.3f ms (min %.3f max %.3f)  in-kernel clock %.0f MHz (p10 %.0f p90 %.0f)  "
           "wave cycles/vis %.1f  matrix-pipe share at that clock %.3f  warm launches %d\n",
           name, med, ms[0], ms[6], clk[clk.size() / 2], clk[clk.size() / 10], clk[clk.size() * 9 / 10],
           cyc[cyc.size() / 2], mfma_cycles / (med * 1e-3 * clk[clk.size() / 2] * 1e6), warm);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
}

int main()
{
    hipDeviceProp_t prop;
    hipGetDeviceProperties(&prop, 0);
    const int cus = prop.multiProcessorCount;
    float *out;
    long long *stamps;
    hipMalloc(&out, (size_t) cus * 768 * sizeof(float));
    hipMalloc(&stamps, (size_t) cus * 12 * 2 * sizeof(long long));
    printf("%d CUs, 12 waves per CU (3 per SIMD), 16384 x 4 visibilities per wave\n", cus);
    // interleaved so that a drift of the device's clock shows as a spread, not as a shape difference
    for (int rep = 0; rep < 2; rep++) {
        run<false, false>(out, stamps, cus, "32x32x2 bare");
        run<true, false>(out, stamps, cus, "16x16x4 bare");
        run<false, true>(out, stamps, cus, "32x32x2 + 4 VALU/vis");
        run<true, true>(out, stamps, cus, "16x16x4 + 4 VALU/vis");
    }
    hipFree(out);
    hipFree(stamps);
    return 0;
}
