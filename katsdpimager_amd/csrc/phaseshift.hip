// Phase-centre shift (include/kimg.h, "Phase-centre shift"): the raw visibilities of a
// [channel][row][pol] block re-phased to another direction, and the block's baseline coordinates
// rotated into that direction's frame.  katsdpimager_amd/phaseshift.py holds the same contract as
// numpy (phase_shift_host).
//
// The thread layout is kimg_channel_block.h's.  The thread reads its row's three coordinates once and
// forms d = delay . uvw in float64; per channel the turn count d / lambda_c is formed and reduced to
// [-0.5, 0.5] in float64 (it runs to thousands of turns; float32 has lost the phase long before), and
// only the reduced angle goes to float32: sincospif of its float32 value, corrected to first order by
// the float32 remainder of the rounding.  1 / lambda_c is the same for every lane and comes through
// the scalar cache.  The channels are walked CB_UNROLL at a time, the loads of all of them issued
// before the first is used.  The thread of a row's first polarization writes the rotated
// coordinates; other waves may still be reading that row, which is why uvw_out may not overlap uvw_in.
// No LDS, no atomics.  Traffic: 16 bytes per element and channel, 12 (+ 12) per row.
#include "kimg_channel_block.h"

namespace {

struct ps_params {
    double rotation[9];                         // row-major: uvw' = rotation . uvw
    double delay[3];
};

// Q_T: the number of polarizations, or 0 for "use the runtime value"
template <int Q_T>
__global__ __launch_bounds__(CB_THREADS)
void phase_shift_kernel(float2 *__restrict__ vis, int64_t vis_pitch, int C, int64_t plane, int Q,
                        const float *__restrict__ uvw_in, float *__restrict__ uvw_out,
                        const double *__restrict__ inv_wavelength, const ps_params p)
{
    const int64_t j = cb_element();
    if (j >= plane)
        return;
    const int64_t n = Q_T ? j / Q_T : j / Q;
    const double u = (double) uvw_in[3 * n], v = (double) uvw_in[3 * n + 1], w = (double) uvw_in[3 * n + 2];
    if (uvw_out != nullptr && j == n * (Q_T ? Q_T : Q)) {
#pragma unroll
        for (int i = 0; i < 3; i++)
            uvw_out[3 * n + i] =
                (float) ((p.rotation[3 * i] * u + p.rotation[3 * i + 1] * v) + p.rotation[3 * i + 2] * w);
    }
    const double d = (p.delay[0] * u + p.delay[1] * v) + p.delay[2] * w;
    float2 *v_ptr = vis + j;

    for (int c0 = 0; c0 < C; c0 += CB_UNROLL) {
        float2 x[CB_UNROLL];
#pragma unroll
        for (int k = 0; k < CB_UNROLL; k++)
            if (c0 + k < C)
                x[k] = v_ptr[(int64_t) (c0 + k) * vis_pitch];
#pragma unroll
        for (int k = 0; k < CB_UNROLL; k++) {
            const int c = c0 + k;
            if (c >= C)
                continue;
            const double turns = d * inv_wavelength[c];
            const double r = turns - rint(turns);       // exact; [-0.5, 0.5]
            const double half_turns = r + r;            // sincospif takes units of pi
            const float a = (float) half_turns;
            const float rest = (float) (half_turns - (double) a);
            float s, co;
            sincospif(a, &s, &co);
            const float delta = 3.14159265358979323846f * rest;
            const float s1 = fmaf(co, delta, s);
            const float c1 = fmaf(-s, delta, co);
            v_ptr[(int64_t) c * vis_pitch] =
                make_float2(x[k].x * c1 - x[k].y * s1, x[k].x * s1 + x[k].y * c1);
        }
    }
}

}  // namespace

extern "C" int kimg_phase_shift(void *vis, int64_t vis_channel_pitch, int num_channels,
                                int64_t num_rows, int num_polarizations, const float *uvw_in,
                                float *uvw_out, const double *inv_wavelength,
                                const double *params12_host, void *stream)
{
    KIMG_CHECK_ARG(vis && uvw_in && inv_wavelength && params12_host);
    KIMG_CHECK_ARG(num_channels >= 1 && num_polarizations >= 1 && num_rows >= 0);
    KIMG_CHECK_ARG(num_rows <= INT64_MAX / 4 / num_polarizations);
    const int64_t plane = num_rows * num_polarizations;
    KIMG_CHECK_ARG(vis_channel_pitch >= plane);
    if (uvw_out) {
        // (as integers: the two arrays need not belong to one object)
        const uintptr_t in = (uintptr_t) uvw_in, out = (uintptr_t) uvw_out;
        const uintptr_t bytes = (uintptr_t) num_rows * 3 * sizeof(float);
        KIMG_CHECK_ARG(in + bytes <= out || out + bytes <= in);
    }
    if (!cb_plane_fits(plane))
        return KIMG_EUNSUPPORTED;
    if (num_rows == 0)
        return 0;
    ps_params p;
    for (int i = 0; i < 9; i++)
        p.rotation[i] = params12_host[i];
    for (int i = 0; i < 3; i++)
        p.delay[i] = params12_host[9 + i];
    hipStream_t s = (hipStream_t) stream;
    const unsigned blocks = cb_blocks(plane);
    auto launch = [&](auto q) {
        phase_shift_kernel<decltype(q)::value><<<blocks, CB_THREADS, 0, s>>>(
            (float2 *) vis, vis_channel_pitch, num_channels, plane, num_polarizations, uvw_in, uvw_out,
            inv_wavelength, p);
    };
    if (num_polarizations <= 4)
        kimg_for_pols(num_polarizations, launch);
    else
        launch(std::integral_constant<int, 0>{});
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT(phase_shift_kernel<1>)
