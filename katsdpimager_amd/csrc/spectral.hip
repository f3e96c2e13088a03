// Spectral smoothing and channel averaging (include/kimg.h, "Spectral filter"): a short non-negative
// FIR along the channel axis of a [channel][row][pol] block of raw visibilities, followed by an
// integer decimation, weighted and aware of flags; new dense vis and weights arrays come out.
// katsdpimager_amd/spectral.py holds the same contract as numpy (filter_host).
//
// The thread layout is kimg_channel_block.h's.  The combined coefficients g (taps convolved with the box of the bin, at most 72 doubles) are a kernel
// argument: the same for every lane, they come through the scalar cache.  The channel axis is split
// over blockIdx.y in chunks of SF_CHUNK output channels, so that a block of few rows and thousands of
// channels still fills the device; a chunk starts its window afresh and re-reads its halo.
//
// Three forms, one arithmetic (sf_sample / sf_add / sf_finish, float64, ascending tap order):
//   sliding  (step == 1, L = 3, 5, 7, 9: Hanning and its kin): the L most recent inputs live in
//            registers as (w, w vr, w vi), in a ring whose slots are compile-time constants because
//            the loop over outputs is unrolled by a multiple of L.  Every input is loaded once.
//   disjoint (one tap: pure binning): the windows of successive outputs do not overlap and lie inside
//            the band, so every input is loaded once and no channel bound is tested.
//   window   (everything else): each output walks its own L inputs; the overlap of neighbouring
//            windows (K - 1 of K + n - 1 channels) is re-read, through the cache.
// No LDS, no atomics on data; the two counters take one atomic add per wave each.
#include "kimg_channel_block.h"

namespace {

constexpr int SF_UNROLL = 4;                    // inputs of a window whose loads are in flight together
constexpr int SF_CHUNK = 64;                    // output channels per blockIdx.y
constexpr int SF_MAX_LENGTH = KIMG_SPECTRAL_MAX_TAPS + KIMG_SPECTRAL_MAX_BIN - 1;

struct sf_coeff {
    double g[SF_MAX_LENGTH];
};

// One input, as the sums want it: w = 0 marks an input that is not usable.  (w * v is exact in
// float64: two 24-bit significands.)
struct sf_sample {
    double w, wr, wi;
};

struct sf_sums {
    double cov, s1, s2, nr, ni;
};

__device__ inline sf_sample sf_make(float2 v, float w)
{
    const bool usable = cb_usable(w, v);
    sf_sample s;
    s.w = usable ? (double) w : 0.0;
    s.wr = usable ? (double) w * (double) v.x : 0.0;
    s.wi = usable ? (double) w * (double) v.y : 0.0;
    return s;
}

// (an unusable input adds +0.0 to sums that start at +0.0 and never become -0.0: the same bits as
// leaving it out)
__device__ inline void sf_add(sf_sums &a, double g, const sf_sample &s)
{
    const double gw = g * s.w;
    a.cov += s.w > 0.0 ? g : 0.0;
    a.s1 += gw;
    a.s2 += g * gw;
    a.nr += g * s.wr;
    a.ni += g * s.wi;
}

// The output sample of finished sums, stored by live lanes; returns how many live lanes kept theirs.
__device__ inline unsigned sf_finish(const sf_sums &a, double min_sum, bool live, float2 *vis_out,
                                     float *weight_out)
{
    const bool keep = a.cov >= min_sum;
    float2 v = make_float2(0.0f, 0.0f);
    float w = 0.0f;
    if (keep) {
        // 1 / S1 once instead of two divisions (a third of the arithmetic of a Hanning output went
        // into the three): N * (1 / S1) lies within 2^-52 |N / S1| of the quotient, far inside the
        // float32 rounding that follows.  The weight is the contract's expression as it stands.
        const double r = 1.0 / a.s1;
        v = make_float2((float) (a.nr * r), (float) (a.ni * r));
        w = (float) (a.s1 * a.s1 / a.s2);
    }
    if (live) {
        *vis_out = v;
        *weight_out = w;
    }
    return (unsigned) __popcll(__ballot(live && keep));
}

// The addressing every form shares.  Lanes past the plane run along (cb_lane_of): sf_finish ballots.
struct sf_lane {
    const float2 *v_in;
    const float *w_in;
    float2 *v_out;
    float *w_out;
    bool live;
    int o_begin, o_end;             // this workgroup's output channels
};

struct sf_arrays {
    const float2 *vis_in;
    int64_t vis_in_pitch;
    const float *weights_in;
    int64_t weights_in_pitch;
    int C_in;
    float2 *vis_out;
    int64_t vis_out_pitch;
    float *weights_out;
    int64_t weights_out_pitch;
    int C_out;
    int64_t plane;
};

__device__ inline sf_lane sf_lane_of(const sf_arrays &a)
{
    const cb_lane at = cb_lane_of(a.plane);
    sf_lane t;
    t.live = at.live;
    t.v_in = a.vis_in + at.jj;
    t.w_in = a.weights_in + at.jj;
    t.v_out = a.vis_out + at.jj;
    t.w_out = a.weights_out + at.jj;
    t.o_begin = (int) blockIdx.y * SF_CHUNK;
    t.o_end = min(a.C_out, t.o_begin + SF_CHUNK);
    return t;
}

__device__ inline void sf_count(const sf_lane &t, unsigned long long kept, int64_t plane,
                                unsigned long long *__restrict__ counts)
{
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        // (the wave's live lanes: its first lane's element up to the end of the plane)
        const int64_t first = cb_element();
        const int64_t lanes = max((int64_t) 0, min((int64_t) WAVE, plane - first));
        cb_add_nonzero(counts, kept, (unsigned long long) lanes * (t.o_end - t.o_begin) - kept);
    }
}

// One input channel of a lane as it lies in memory.  The address is always a valid one -- the channel
// clamped into the band -- so that the loads of a round stand in straight-line code, without a branch
// each, and the wave waits for every one only where it is used; sf_make then takes a channel that was
// not wanted as unusable.
struct sf_raw {
    float2 v;
    float w;
};

__device__ inline sf_raw sf_load(const sf_lane &t, const sf_arrays &a, int c)
{
    const int cc = min(max(c, 0), a.C_in - 1);
    sf_raw r;
    r.v = t.v_in[(int64_t) cc * a.vis_in_pitch];
    r.w = t.w_in[(int64_t) cc * a.weights_in_pitch];
    return r;
}

__device__ inline sf_sample sf_make(const sf_raw &r, bool wanted)
{
    return sf_make(r.v, wanted ? r.w : 0.0f);
}

// step == 1, `L` coefficients: output o takes the inputs o - offset + i, i = 0 .. L - 1.  Input c of
// the chunk sits in slot (c - (o_begin - offset)) % L; the loop over outputs advances by L * M, so
// that the slot of tap i of the u-th output of a round is (u + i) % L, a constant.  The loads of the
// next round are issued before the arithmetic and the stores of this one: in the wave's memory
// counter they are then older than the stores, and waiting for them never waits for a store.
template <int L, int M>
__global__ __launch_bounds__(CB_THREADS)
void spectral_sliding_kernel(const sf_arrays a, const sf_coeff coeff, int offset, double min_sum,
                             unsigned long long *__restrict__ counts)
{
    const sf_lane t = sf_lane_of(a);
    constexpr int R = L * M;                    // outputs, and new inputs, per round
    sf_sample win[L];
    {
        sf_raw first[L - 1];
#pragma unroll
        for (int i = 0; i < L - 1; i++)
            first[i] = sf_load(t, a, t.o_begin - offset + i);
#pragma unroll
        for (int i = 0; i < L - 1; i++) {
            const int c = t.o_begin - offset + i;
            win[i] = sf_make(first[i], c >= 0 && c < a.C_in);
        }
    }
    // (the newest input of output o is o - offset + L - 1)
    sf_raw next[R];
#pragma unroll
    for (int u = 0; u < R; u++)
        next[u] = sf_load(t, a, t.o_begin + u - offset + (L - 1));
    unsigned long long kept = 0;
    for (int o0 = t.o_begin; o0 < t.o_end; o0 += R) {
        sf_raw cur[R];
#pragma unroll
        for (int u = 0; u < R; u++)
            cur[u] = next[u];
        if (o0 + R < t.o_end) {
#pragma unroll
            for (int u = 0; u < R; u++)
                next[u] = sf_load(t, a, o0 + R + u - offset + (L - 1));
        }
#pragma unroll
        for (int u = 0; u < R; u++) {
            const int o = o0 + u;
            if (o < t.o_end) {
                const int c = o - offset + (L - 1);
                win[(u + L - 1) % L] = sf_make(cur[u], c >= 0 && c < a.C_in);
                sf_sums s = {};
#pragma unroll
                for (int i = 0; i < L; i++)
                    sf_add(s, coeff.g[i], win[(u + i) % L]);
                kept += sf_finish(s, min_sum, t.live, t.v_out + (int64_t) o * a.vis_out_pitch,
                                  t.w_out + (int64_t) o * a.weights_out_pitch);
            }
        }
    }
    sf_count(t, kept, a.plane, counts);
}

// Output o takes the inputs o * step - offset + i, i = 0 .. length - 1, SF_UNROLL of them in flight.
// DISJOINT: offset == 0 and length == step, so that all of them lie inside the band.
template <bool DISJOINT>
__global__ __launch_bounds__(CB_THREADS)
void spectral_window_kernel(const sf_arrays a, const sf_coeff coeff, int length, int offset, int step,
                            double min_sum, unsigned long long *__restrict__ counts)
{
    const sf_lane t = sf_lane_of(a);
    unsigned long long kept = 0;
    for (int o = t.o_begin; o < t.o_end; o++) {
        const int c_first = o * step - (DISJOINT ? 0 : offset);
        sf_sums s = {};
        for (int i0 = 0; i0 < length; i0 += SF_UNROLL) {
            sf_raw in[SF_UNROLL];
#pragma unroll
            for (int u = 0; u < SF_UNROLL; u++)
                in[u] = sf_load(t, a, c_first + i0 + u);
#pragma unroll
            for (int u = 0; u < SF_UNROLL; u++) {
                const int c = c_first + i0 + u;
                if (i0 + u < length)
                    sf_add(s, coeff.g[i0 + u], sf_make(in[u], DISJOINT || (c >= 0 && c < a.C_in)));
            }
        }
        kept += sf_finish(s, min_sum, t.live, t.v_out + (int64_t) o * a.vis_out_pitch,
                          t.w_out + (int64_t) o * a.weights_out_pitch);
    }
    sf_count(t, kept, a.plane, counts);
}

// Whether an array that starts at `p` starts inside the `bytes` bytes from `base`.
bool sf_starts_inside(const void *p, const void *base, uint64_t bytes)
{
    const uintptr_t x = (uintptr_t) p, b = (uintptr_t) base;
    return x >= b && x - b < bytes;
}

}  // namespace

extern "C" int kimg_spectral_filter(const void *vis_in, int64_t vis_in_channel_pitch,
                                    const float *weights_in, int64_t weights_in_channel_pitch,
                                    int num_channels_in, void *vis_out,
                                    int64_t vis_out_channel_pitch, float *weights_out,
                                    int64_t weights_out_channel_pitch, int num_channels_out,
                                    int64_t plane_elements, const double *coeff_host, int length,
                                    int offset, int step, double min_sum, uint64_t *counts,
                                    void *stream)
{
    KIMG_CHECK_ARG(vis_in && weights_in && vis_out && weights_out && coeff_host && counts);
    KIMG_CHECK_ARG(length >= 1 && step >= 1 && offset >= 0 && offset < length);
    if (length > SF_MAX_LENGTH || step > KIMG_SPECTRAL_MAX_BIN)
        return KIMG_EUNSUPPORTED;
    sf_coeff coeff = {};
    for (int i = 0; i < length; i++) {
        KIMG_CHECK_ARG(coeff_host[i] >= 0.0 && coeff_host[i] <= 1.7976931348623157e308);   // (NaN fails)
        coeff.g[i] = coeff_host[i];
    }
    KIMG_CHECK_ARG(min_sum > 0.0 && min_sum <= 1.7976931348623157e308);
    KIMG_CHECK_ARG(num_channels_out >= 1 && (int64_t) num_channels_out * step <= num_channels_in);
    KIMG_CHECK_ARG(plane_elements >= 0);
    KIMG_CHECK_ARG(vis_in_channel_pitch >= plane_elements && weights_in_channel_pitch >= plane_elements
                   && vis_out_channel_pitch >= plane_elements
                   && weights_out_channel_pitch >= plane_elements);
    const int chunks = kimg_divup(num_channels_out, SF_CHUNK);
    if (!cb_plane_fits(plane_elements) || chunks > 65535)
        return KIMG_EUNSUPPORTED;
    // out of place: an output that starts inside an input would be written while still being read
    const uint64_t vis_in_bytes =
        ((uint64_t) (num_channels_in - 1) * vis_in_channel_pitch + plane_elements) * sizeof(float2);
    const uint64_t weights_in_bytes =
        ((uint64_t) (num_channels_in - 1) * weights_in_channel_pitch + plane_elements) * sizeof(float);
    for (const void *out : {(const void *) vis_out, (const void *) weights_out})
        KIMG_CHECK_ARG(!sf_starts_inside(out, vis_in, vis_in_bytes)
                       && !sf_starts_inside(out, weights_in, weights_in_bytes));
    if (plane_elements == 0)
        return 0;

    const sf_arrays a = {(const float2 *) vis_in, vis_in_channel_pitch, weights_in,
                         weights_in_channel_pitch, num_channels_in, (float2 *) vis_out,
                         vis_out_channel_pitch, weights_out, weights_out_channel_pitch,
                         num_channels_out, plane_elements};
    hipStream_t s = (hipStream_t) stream;
    const dim3 blocks(cb_blocks(plane_elements), (unsigned) chunks);
    unsigned long long *c = (unsigned long long *) counts;
    auto sliding = [&](auto l, auto m) {
        spectral_sliding_kernel<decltype(l)::value, decltype(m)::value><<<blocks, CB_THREADS, 0, s>>>(
            a, coeff, offset, min_sum, c);
    };
    using std::integral_constant;
    if (step == 1 && length == 3)
        sliding(integral_constant<int, 3>{}, integral_constant<int, 2>{});
    else if (step == 1 && length == 5)
        sliding(integral_constant<int, 5>{}, integral_constant<int, 1>{});
    else if (step == 1 && length == 7)
        sliding(integral_constant<int, 7>{}, integral_constant<int, 1>{});
    else if (step == 1 && length == 9)
        sliding(integral_constant<int, 9>{}, integral_constant<int, 1>{});
    else if (offset == 0 && length == step)
        spectral_window_kernel<true><<<blocks, CB_THREADS, 0, s>>>(a, coeff, length, offset, step,
                                                                   min_sum, c);
    else
        spectral_window_kernel<false><<<blocks, CB_THREADS, 0, s>>>(a, coeff, length, offset, step,
                                                                    min_sum, c);
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(spectral_window_kernel<false>)
