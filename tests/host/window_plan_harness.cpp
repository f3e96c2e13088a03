// Host test of the window kernels' launch plan (csrc/kimg_window_plan.h, kimg_window_launch.h): the
// scramble multiplier is coprime to the chunk count it is chosen for, and what the gridder's kernel
// recomputes on the device for a shorter (folded) stream covers that stream with the host's
// workgroups.  Built for the host only:
//     hipcc -x hip --offload-host-only -no-hip-rt -I katsdpimager_amd/csrc tests/host/window_plan_harness.cpp
#include "kimg_window_launch.h"
#include <stdio.h>
#include <vector>

static int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// what grid_mfma_kernel's prologue computes from the device's record count
struct device_plan { int64_t vis_per_block, chunk, scramble, chunks; };
static device_plan plan_on_device(int64_t num_vis, int blocks, int NW, int64_t min_chunk, int64_t max_parts)
{
    device_plan d;
    d.vis_per_block = window_vis_per_block_of(num_vis, blocks, NW);
    d.chunk = window_chunk_of(num_vis, (int64_t) blocks * NW, min_chunk, max_parts);
    d.chunks = d.chunk > 0 ? (num_vis + d.chunk - 1) / d.chunk : 0;
    d.scramble = d.chunk > 0 ? window_scramble_of(d.chunks) : 1;
    return d;
}

int main()
{
    // every chunk count 1 .. 100 000: the first candidate that does not divide it, coprime to it
    for (int64_t chunks = 1; chunks <= 100000; chunks++) {
        const int64_t m = window_scramble_of(chunks);
        EXPECT(m > 1 && gcd64(m, chunks) == 1, "chunks %lld multiplier %lld", (long long) chunks, (long long) m);
        for (int i = 0; i < KIMG_SCRAMBLE_CANDIDATES && window_scramble_candidate(i) != m; i++)
            EXPECT(chunks % window_scramble_candidate(i) == 0, "chunks %lld skips candidate %d", (long long) chunks, i);
    }
    // every multiple of every candidate up to 10^7 (where the first choice is the wrong one)
    for (int i = 0; i < KIMG_SCRAMBLE_CANDIDATES; i++) {
        const int64_t c = window_scramble_candidate(i);
        for (int j = 0; j < i; j++)
            EXPECT(gcd64(c, window_scramble_candidate(j)) == 1, "candidates %d %d", i, j);
        for (int64_t chunks = c; chunks <= 10000000; chunks += c) {
            const int64_t m = window_scramble_of(chunks);
            EXPECT(m != c && gcd64(m, chunks) == 1, "chunks %lld multiplier %lld", (long long) chunks, (long long) m);
        }
    }
    // a coprime multiplier visits every chunk once; the host's multiplier on the device's count need not
    {
        const int64_t chunks = 7919 * 3;
        std::vector<int> seen(chunks, 0);
        const int64_t m = window_scramble_of(chunks);
        for (int64_t t = 0; t < chunks; t++)
            seen[(size_t) ((unsigned long long) t * m % chunks)]++;
        for (int64_t c = 0; c < chunks; c++)
            EXPECT(seen[(size_t) c] == 1, "chunk %lld taken %d times", (long long) c, seen[(size_t) c]);
    }
    // host plan against the helpers, and the device's plan for a folded stream of the same launch
    const int64_t min_chunk = 384, max_parts = 16;
    for (int NW : {8, 12})
        for (int blocks_max : {1, 2, 256, 512})
            for (int64_t n = 1; n < 60000000; n += 1 + n / 3) {
                const window_partition p = window_partition_of(n, NW, blocks_max, min_chunk, max_parts, true);
                const device_plan same = plan_on_device(n, p.blocks, NW, min_chunk, max_parts);
                EXPECT(p.blocks >= 1 && p.blocks <= blocks_max, "n %lld blocks %d", (long long) n, p.blocks);
                EXPECT((int64_t) p.blocks * p.vis_per_block >= n, "n %lld", (long long) n);
                // the unfolded length gives the device the host's own plan
                EXPECT(same.chunk == p.chunk && same.scramble == p.scramble, "n %lld NW %d", (long long) n, NW);
                EXPECT(p.chunk > 0 || same.vis_per_block == p.vis_per_block, "n %lld NW %d", (long long) n, NW);
                for (int64_t h : {n / 2, n / 3, n / 7, n / 50, (int64_t) 1}) {
                    if (h < 1)
                        continue;
                    const device_plan d = plan_on_device(h, p.blocks, NW, min_chunk, max_parts);
                    EXPECT(d.vis_per_block % 64 == 0 && d.vis_per_block >= 64 * NW
                           && (int64_t) p.blocks * d.vis_per_block >= h, "h %lld", (long long) h);
                    EXPECT(d.chunk % 64 == 0, "h %lld", (long long) h);
                    if (d.chunk > 0) {
                        EXPECT(d.chunk >= min_chunk && d.chunks * d.chunk >= h && (d.chunks - 1) * d.chunk < h,
                               "h %lld chunk %lld", (long long) h, (long long) d.chunk);
                        EXPECT(gcd64(d.scramble, d.chunks) == 1, "h %lld", (long long) h);
                    }
                }
            }
    if (failures)
        printf("%d failures\n", failures);
    else
        printf("ok\n");
    return failures ? 1 : 0;
}
