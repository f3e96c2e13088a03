// RFI flagging (include/kimg.h, "RFI flagging"): SumThreshold over the time-frequency plane of every
// group of up to 64 consecutive rows of one baseline, per polarization, on a [channel][row][pol] block
// of raw visibilities; the weights of the flagged samples are set to +0.  katsdpimager_amd/rfiflag.py
// holds the same contract as numpy (rfiflag_host), and the order of every sum below is that
// contract's: the device has the twin's bits.
//
// The thread layout, the channel mask, the load round and the group tables are kimg_channel_block.h's.
// All launches are plain, there is no LDS and no atomic but the three counters'.
//
// Between the launches the workspace holds, per sample,
//   zs     float64: z = w (re^2 + im^2) of a usable sample of a mask channel, -1 for every other
//          sample (unusable, or in a protected channel): what a window adds is decided by one sign
//          test, and the passes read 8 bytes per sample where (vis, weight) are 12;
//   stamp  one byte: 0 while the sample is unflagged, else the number of the step that flagged it:
//          1 + k for the window pass of length 2^k, then STAMP_FREQ and STAMP_TIME for the first two
//          extensions.  A step reads "flagged on entry" as 0 < stamp < its own number, so ONE plane
//          serves as the state that enters a pass and as the state that leaves it: a pass only ever
//          turns a 0 into its own number, whoever reads that byte during the pass takes either value
//          for "not flagged on entry", and nothing depends on the order in which windows are
//          evaluated.  (Two planes to ping-pong would need a copy of the whole state per pass.)
// and per plane element two sets of the level's per-row partial sums (Z, M), read and written in turn
// by the level iterations.
//
// Launches: prepare (zs, stamp = 0, partials of L0); one per level iteration; level (L per group and
// polarization, the skipped count); per window length one along frequency and one along time;
// extension over a row; extension over a group's channel; finish (extension over polarizations, the
// flags, the weights, the two sample counters).
//   frequency: the thread walks its own channels with the window's m values in registers (the kernel
//     is a template of m, every index static: no scratch), one direct ascending sum per window, and
//     a "flag through channel e" counter instead of a second look at the hits.
//   time: the thread of row s evaluates the window that STARTS at s, the m - 1 later rows of the same
//     channel read through the caches (P elements apart, never past the group's end); on a hit it
//     stamps the window's rows itself.
#include "kimg_channel_block.h"

namespace {

constexpr int RF_MAX_PASSES = 6;                // window lengths 1 .. KIMG_RFIFLAG_MAX_WINDOW
constexpr uint8_t STAMP_FREQ = RF_MAX_PASSES + 1;
constexpr uint8_t STAMP_TIME = RF_MAX_PASSES + 2;

// The workspace: zs and stamp [C][plane], the partials [plane]
struct rf_state {
    double *zs;
    uint8_t *stamp;
    double *Z[2];
    int *M[2];
    int64_t plane;
};

// (Z, M) of the group from the rows' partials in ascending row order; the level, and whether it is one
__device__ inline bool rf_group_level(const rf_state &st, int set, const cb_groups &t, const cb_place &at,
                                      double &L)
{
    double Z = 0.0;
    int M = 0;
    for (int rr = at.r0; rr < at.r1; rr++) {
        const int64_t k = (int64_t) rr * t.P + at.p;
        Z += st.Z[set][k];
        M += st.M[set][k];
    }
    L = Z / (double) M;
    return M > 0 && isfinite(L) && L > 0.0;
}

__global__ __launch_bounds__(CB_THREADS)
void rfi_prepare_kernel(const float2 *__restrict__ vis, int64_t vis_pitch,
                        const float *__restrict__ weights, int64_t weights_pitch, int C,
                        const cb_mask mask, rf_state st)
{
    const int64_t j = cb_element();
    if (j >= st.plane)
        return;
    const float2 *v_ptr = vis + j;
    const float *w_ptr = weights + j;
    double Z = 0.0;
    int M = 0;
    for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
        float2 v[CB_UNROLL];
        float w[CB_UNROLL];
        bool fit[CB_UNROLL];
        cb_load_round(v_ptr, vis_pitch, w_ptr, weights_pitch, C, mask, c0, v, w, fit);
#pragma unroll
        for (int u = 0; u < CB_UNROLL; u++) {
            const int c = c0 + u;
            if (c >= C)
                continue;
            double z = -1.0;
            if (fit[u] && cb_usable_finite_weight(w[u], v[u])) {
                double t = (double) v[u].x * (double) v[u].x;
                t = t + (double) v[u].y * (double) v[u].y;
                z = (double) w[u] * t;
                Z += z;
                M++;
            }
            st.zs[(int64_t) c * st.plane + j] = z;
            st.stamp[(int64_t) c * st.plane + j] = 0;
        }
    }
    st.Z[0][j] = Z;
    st.M[0][j] = M;
}

// One level iteration: the mean of the samples not above clip times the level of partials `set`, as
// partials `set ^ 1`.  A group without a level leaves partials of nothing, and so stays without one.
__global__ __launch_bounds__(CB_THREADS)
void rfi_level_kernel(int C, cb_groups groups, rf_state st, int set, double clip)
{
    const int64_t j = cb_element();
    if (j >= st.plane)
        return;
    const cb_place at = cb_place_of(groups, j);
    double L;
    const bool ok = rf_group_level(st, set, groups, at, L);
    const double limit = clip * L;
    const double *z_ptr = st.zs + j;
    double Z = 0.0;
    int M = 0;
    if (ok) {
        for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
            double z[CB_UNROLL];
#pragma unroll
            for (int u = 0; u < CB_UNROLL; u++)
                z[u] = c0 + u < C ? z_ptr[(int64_t) (c0 + u) * st.plane] : -1.0;
#pragma unroll
            for (int u = 0; u < CB_UNROLL; u++) {
                if (z[u] >= 0.0 && z[u] <= limit) {
                    Z += z[u];
                    M++;
                }
            }
        }
    }
    st.Z[set ^ 1][j] = Z;
    st.M[set ^ 1][j] = M;
}

// The level of every (group, polarization), NaN where there is none, written by the group's first row
__global__ __launch_bounds__(CB_THREADS)
void rfi_level_out_kernel(cb_groups groups, rf_state st, int set, double *__restrict__ level,
                          unsigned long long *__restrict__ counts)
{
    const cb_lane t = cb_lane_of(st.plane);
    const bool live = t.live;
    const cb_place at = cb_place_of(groups, t.jj);
    double L;
    const bool ok = rf_group_level(st, set, groups, at, L);
    const bool first = live && at.r == at.r0;
    if (first)
        level[(int64_t) at.g * groups.P + at.p] = ok ? L : __longlong_as_double(0x7ff8000000000000LL);
    const unsigned long long skipped = __popcll(__ballot(first && !ok));
    if ((threadIdx.x & (WAVE - 1)) == 0 && skipped)
        atomicAdd(&counts[2], skipped);
}

// A window pass along frequency, windows of M channels, stamp `mine` (1 + log2 M).  a[i] is what
// channel c + i adds to a window (z - L, or chi), good bit i whether that is its own z, open bit i whether the sample
// may be stamped (a usable sample of a mask channel that nothing has flagged).
template <int M>
__global__ __launch_bounds__(CB_THREADS)
void rfi_freq_kernel(int C, cb_groups groups, rf_state st, const double *__restrict__ level,
                     double factor, uint8_t mine)
{
    const int64_t j = cb_element();
    if (j >= st.plane)
        return;
    const cb_place at = cb_place_of(groups, j);
    const double L = level[(int64_t) at.g * groups.P + at.p];
    if (!(L == L))
        return;
    const double chi = factor * L;
    const double limit = (double) M * chi;
    const double *z_ptr = st.zs + j;
    uint8_t *s_ptr = st.stamp + j;

    double a[M];
    uint32_t good = 0, open = 0;
    auto take = [&](double z, uint8_t s) {          // the sample that enters at the window's far end
        const bool usable = z >= 0.0;
        const bool entered = s != 0 && s < mine;
        a[M - 1] = usable && !entered ? z - L : chi;
        good |= (uint32_t) (usable && !entered) << (M - 1);
        open |= (uint32_t) (usable && s == 0) << (M - 1);
    };
    auto shift = [&]() {
#pragma unroll
        for (int i = 0; i + 1 < M; i++)
            a[i] = a[i + 1];
        a[M - 1] = 0.0;
        good >>= 1;
        open >>= 1;
    };
#pragma unroll
    for (int i = 0; i < M; i++)
        a[i] = 0.0;
    // channels 0 .. M - 2 into a[1 .. M - 1]
#pragma unroll
    for (int i = 0; i + 1 < M; i++) {
        shift();
        if (i < C)
            take(z_ptr[(int64_t) i * st.plane], s_ptr[(int64_t) i * st.plane]);
    }
    int through = -1;                               // flag through this channel
    for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
        double z[CB_UNROLL];
        uint8_t s[CB_UNROLL];
#pragma unroll
        for (int u = 0; u < CB_UNROLL; u++) {
            const int c = c0 + u + M - 1;
            z[u] = -1.0;
            s[u] = 0;
            if (c < C) {
                z[u] = z_ptr[(int64_t) c * st.plane];
                s[u] = s_ptr[(int64_t) c * st.plane];
            }
        }
#pragma unroll
        for (int u = 0; u < CB_UNROLL; u++) {
            const int c = c0 + u;
            shift();
            if (c + M - 1 < C)
                take(z[u], s[u]);
            if (c + M <= C) {
                double sum = 0.0;
#pragma unroll
                for (int i = 0; i < M; i++)
                    sum = sum + a[i];
                if (good != 0 && sum > limit)
                    through = c + M - 1;
            }
            if (c < C && c <= through && (open & 1u))
                s_ptr[(int64_t) c * st.plane] = mine;
        }
    }
}

// A window pass along time, windows of m rows of one group in one mask channel.  The thread of row s
// has the window s .. s + m - 1.
__global__ __launch_bounds__(CB_THREADS)
void rfi_time_kernel(int C, const cb_mask mask, cb_groups groups, rf_state st,
                     const double *__restrict__ level, double factor, int m, uint8_t mine)
{
    const int64_t j = cb_element();
    if (j >= st.plane)
        return;
    const cb_place at = cb_place_of(groups, j);
    if (at.r + m > at.r1)
        return;
    const double L = level[(int64_t) at.g * groups.P + at.p];
    if (!(L == L))
        return;
    const double chi = factor * L;
    const double limit = (double) m * chi;
    const int64_t step = groups.P;
    for (int c = 0; c < C; c++) {
        if (!mask[c])
            continue;
        const double *z_ptr = st.zs + (int64_t) c * st.plane + j;
        uint8_t *s_ptr = st.stamp + (int64_t) c * st.plane + j;
        double sum = 0.0;
        uint32_t good = 0, open = 0;
#pragma unroll 4
        for (int i = 0; i < m; i++) {
            const double z = z_ptr[i * step];
            const uint8_t s = s_ptr[i * step];
            const bool own = z >= 0.0 && !(s != 0 && s < mine);
            sum = sum + (own ? z - L : chi);
            good |= (uint32_t) own << i;
            open |= (uint32_t) (z >= 0.0 && s == 0) << i;
        }
        if (good != 0 && sum > limit)
            for (int i = 0; i < m; i++)
                if ((open >> i) & 1u)
                    s_ptr[i * step] = mine;
    }
}

// Extension over a row: with more than `share` of its usable samples of mask channels flagged, all its
// usable samples are, those of protected channels (which zs knows nothing of) included
__global__ __launch_bounds__(CB_THREADS)
void rfi_extend_freq_kernel(const float2 *__restrict__ vis, int64_t vis_pitch,
                            const float *__restrict__ weights, int64_t weights_pitch, int C,
                            const cb_mask mask, cb_groups groups, rf_state st,
                            const double *__restrict__ level, double share)
{
    const int64_t j = cb_element();
    if (j >= st.plane)
        return;
    const cb_place at = cb_place_of(groups, j);
    const double L = level[(int64_t) at.g * groups.P + at.p];
    if (!(L == L))
        return;
    int have = 0, hit = 0;
    for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
        double z[CB_UNROLL];
        uint8_t s[CB_UNROLL];
#pragma unroll
        for (int u = 0; u < CB_UNROLL; u++) {
            const int c = c0 + u;
            z[u] = -1.0;
            s[u] = 0;
            if (c < C && mask[c]) {
                z[u] = st.zs[(int64_t) c * st.plane + j];
                s[u] = st.stamp[(int64_t) c * st.plane + j];
            }
        }
#pragma unroll
        for (int u = 0; u < CB_UNROLL; u++) {
            have += z[u] >= 0.0;
            hit += z[u] >= 0.0 && s[u] != 0;
        }
    }
    if (!((double) hit > share * (double) have))
        return;
    for (int c = 0; c < C; c++) {
        uint8_t *s_ptr = st.stamp + (int64_t) c * st.plane + j;
        bool open;
        if (mask[c])
            open = st.zs[(int64_t) c * st.plane + j] >= 0.0 && *s_ptr == 0;
        else
            open = cb_usable_finite_weight(weights[(int64_t) c * weights_pitch + j], vis[(int64_t) c * vis_pitch + j]);
        if (open)
            *s_ptr = STAMP_FREQ;
    }
}

// Extension over a channel of a group: with more than `share` of its usable rows flagged (by anything
// before this step), all its usable rows are.  Every row of the group counts for itself, reads the
// others through the caches, and stamps its own sample only.
__global__ __launch_bounds__(CB_THREADS)
void rfi_extend_time_kernel(int C, const cb_mask mask, cb_groups groups, rf_state st, double share)
{
    const int64_t j = cb_element();
    if (j >= st.plane)
        return;
    const cb_place at = cb_place_of(groups, j);
    const int64_t first = (int64_t) at.r0 * groups.P + at.p;
    const int rows = at.r1 - at.r0;
    for (int c = 0; c < C; c++) {
        if (!mask[c])
            continue;
        const double *z_ptr = st.zs + (int64_t) c * st.plane;
        uint8_t *s_ptr = st.stamp + (int64_t) c * st.plane;
        int have = 0, hit = 0;
#pragma unroll 4
        for (int i = 0; i < rows; i++) {
            const double z = z_ptr[first + (int64_t) i * groups.P];
            const uint8_t s = s_ptr[first + (int64_t) i * groups.P];
            have += z >= 0.0;
            hit += z >= 0.0 && s != 0 && s != STAMP_TIME;
        }
        if ((double) hit > share * (double) have && z_ptr[j] >= 0.0 && s_ptr[j] == 0)
            s_ptr[j] = STAMP_TIME;
    }
}

// Extension over polarizations; the flags, the weights, the counts of usable samples kept and flagged
__global__ __launch_bounds__(CB_THREADS)
void rfi_finish_kernel(const float2 *__restrict__ vis, int64_t vis_pitch, float *__restrict__ weights,
                       int64_t weights_pitch, int C, cb_groups groups, rf_state st,
                       const double *__restrict__ level, int extend_pols,
                       uint8_t *__restrict__ flags, unsigned long long *__restrict__ counts)
{
    const cb_lane t = cb_lane_of(st.plane);
    const int64_t j = t.j;
    const bool live = t.live;
    int kept = 0, flagged = 0;
    if (live) {
        const cb_place at = cb_place_of(groups, j);
        const double L = level[(int64_t) at.g * groups.P + at.p];
        const bool spread = extend_pols && L == L;
        const int64_t row = j - at.p;
        for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
            float2 v[CB_UNROLL];
            float w[CB_UNROLL];
            bool own[CB_UNROLL], any[CB_UNROLL];
#pragma unroll
            for (int u = 0; u < CB_UNROLL; u++) {
                const int c = c0 + u;
                v[u] = make_float2(0.0f, 0.0f);
                w[u] = 0.0f;
                own[u] = any[u] = false;
                if (c < C) {
                    v[u] = vis[(int64_t) c * vis_pitch + j];
                    w[u] = weights[(int64_t) c * weights_pitch + j];
                    own[u] = st.stamp[(int64_t) c * st.plane + j] != 0;
                    if (spread)
                        for (int q = 0; q < groups.P; q++)
                            any[u] |= st.stamp[(int64_t) c * st.plane + row + q] != 0;
                }
            }
#pragma unroll
            for (int u = 0; u < CB_UNROLL; u++) {
                const int c = c0 + u;
                if (c >= C)
                    continue;
                const bool usable = cb_usable_finite_weight(w[u], v[u]);
                const bool flag = own[u] || (any[u] && usable);
                flags[(int64_t) c * st.plane + j] = flag;
                if (flag)
                    weights[(int64_t) c * weights_pitch + j] = 0.0f;
                kept += usable && !flag;
                flagged += flag;
            }
        }
    }
    cb_count_sums(kept, flagged, counts);
}

}  // namespace

extern "C" int kimg_rfi_flag(const void *vis, int64_t vis_channel_pitch, float *weights,
                             int64_t weights_channel_pitch, int num_channels, int64_t num_rows,
                             int num_pols, const uint8_t *mask_host, const int32_t *group_offsets,
                             int64_t num_groups, const int32_t *row_group, int time_bin,
                             const double *factors_host, int max_window, int directions,
                             int level_iterations, double level_clip, double extend_freq,
                             double extend_time, int extend_pols, uint8_t *flags, double *level,
                             void *workspace, size_t workspace_bytes, uint64_t *counts, void *stream)
{
    KIMG_CHECK_ARG(factors_host && flags && level);
    KIMG_CHECK_ARG(max_window >= 1 && max_window <= KIMG_RFIFLAG_MAX_WINDOW
                   && (max_window & (max_window - 1)) == 0);
    KIMG_CHECK_ARG(directions >= 1 && directions <= (KIMG_RFIFLAG_TIME | KIMG_RFIFLAG_FREQ));
    KIMG_CHECK_ARG(level_iterations >= 0 && level_iterations <= KIMG_RFIFLAG_MAX_LEVEL_ITERATIONS);
    KIMG_CHECK_ARG(level_clip > 0.0);                                       // (false for a NaN)
    KIMG_CHECK_ARG(extend_freq >= 0.0 && extend_freq <= 1.0 && extend_time >= 0.0 && extend_time <= 1.0);
    int passes = 0;
    while ((1 << passes) <= max_window)
        passes++;
    for (int k = 0; k < passes; k++)
        KIMG_CHECK_ARG(factors_host[k] > 0.0);
    int64_t plane;
    const int rc = cb_check_block(vis, vis_channel_pitch, weights, weights_channel_pitch, num_channels,
                                  num_rows, num_pols, mask_host, group_offsets, num_groups, row_group,
                                  time_bin, workspace, workspace_bytes, KIMG_RFIFLAG_WORKSPACE_PER_ROW,
                                  KIMG_RFIFLAG_WORKSPACE_PER_ELEMENT, counts, plane);
    if (rc != 0 || plane == 0)
        return rc;
    const size_t samples = (size_t) plane * num_channels;

    cb_mask mask;
    cb_pack_mask(mask_host, num_channels, mask);
    rf_state st;
    st.plane = plane;
    st.zs = (double *) workspace;
    st.Z[0] = st.zs + samples;
    st.Z[1] = st.Z[0] + plane;
    st.M[0] = (int *) (st.Z[1] + plane);
    st.M[1] = st.M[0] + plane;
    st.stamp = (uint8_t *) (st.M[1] + plane);
    const cb_groups groups = {group_offsets, row_group, (int) num_groups, (int) num_rows, num_pols};
    const float2 *v = (const float2 *) vis;
    hipStream_t s = (hipStream_t) stream;
    const unsigned blocks = cb_blocks(plane);
    unsigned long long *n = (unsigned long long *) counts;

    rfi_prepare_kernel<<<blocks, CB_THREADS, 0, s>>>(
        v, vis_channel_pitch, weights, weights_channel_pitch, num_channels, mask, st);
    int set = 0;
    for (int i = 0; i < level_iterations; i++, set ^= 1)
        rfi_level_kernel<<<blocks, CB_THREADS, 0, s>>>(num_channels, groups, st, set, level_clip);
    rfi_level_out_kernel<<<blocks, CB_THREADS, 0, s>>>(groups, st, set, level, n);
    for (int k = 0; k < passes; k++) {
        const int m = 1 << k;
        const uint8_t mine = (uint8_t) (1 + k);
        const double factor = factors_host[k];
        if ((directions & KIMG_RFIFLAG_FREQ) && m <= num_channels) {
            auto launch = [&](auto length) {
                rfi_freq_kernel<decltype(length)::value><<<blocks, CB_THREADS, 0, s>>>(
                    num_channels, groups, st, level, factor, mine);
            };
            switch (m) {
            case 1: launch(std::integral_constant<int, 1>{}); break;
            case 2: launch(std::integral_constant<int, 2>{}); break;
            case 4: launch(std::integral_constant<int, 4>{}); break;
            case 8: launch(std::integral_constant<int, 8>{}); break;
            case 16: launch(std::integral_constant<int, 16>{}); break;
            default: launch(std::integral_constant<int, 32>{}); break;
            }
            // (a window of one sample is the same window in either direction)
            if (m == 1)
                continue;
        }
        if ((directions & KIMG_RFIFLAG_TIME) && m <= time_bin)
            rfi_time_kernel<<<blocks, CB_THREADS, 0, s>>>(num_channels, mask, groups, st, level, factor,
                                                         m, mine);
    }
    if (extend_freq > 0.0)
        rfi_extend_freq_kernel<<<blocks, CB_THREADS, 0, s>>>(
            v, vis_channel_pitch, weights, weights_channel_pitch, num_channels, mask, groups, st, level,
            extend_freq);
    if (extend_time > 0.0)
        rfi_extend_time_kernel<<<blocks, CB_THREADS, 0, s>>>(num_channels, mask, groups, st, extend_time);
    rfi_finish_kernel<<<blocks, CB_THREADS, 0, s>>>(
        v, vis_channel_pitch, weights, weights_channel_pitch, num_channels, groups, st, level,
        extend_pols, flags, n);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(rfi_prepare_kernel)
