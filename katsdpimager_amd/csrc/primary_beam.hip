// Primary-beam correction (include/kimg.h, "Primary-beam correction"): a radially symmetric beam
// model sampled on the pixel grid, and the model and residual images divided by its power, in one
// pass.  katsdpimager_amd/primary_beam.py holds the same contract as numpy (sample_host,
// correct_host); this file is built with -ffp-contract=off and the results agree bit for bit.
//
// A workgroup is 4 waves; a wave owns 256 consecutive pixels of one image row (4 per lane, 16-byte
// loads and stores where the pointers and pitches are 16-byte aligned), and the workgroup walks
// down the image 4 rows at a time.  The table -- the row's samples next to their first differences,
// one float2 per interval -- is staged in LDS once per workgroup, so a pixel costs one ds_read_b64.
// The beam value is computed once per pixel and used by every polarization; the loads of all
// polarizations are issued before the first quotient is stored.  No float64, no atomics.
// Traffic: 4 bytes per pixel written for the beam, 16 per pixel and polarization for the images.
#include "kimg_common.h"
#include "kimg_layer_math.h"

namespace {

constexpr int PB_LANES = 64;            // threadIdx.x: 4 pixels each
constexpr int PB_ROWS = 4;              // threadIdx.y: image rows in flight per workgroup
constexpr int PB_MAX_BLOCKS = 2048;     // the rest of the image is walked

// (sample, sample of the next radius - sample) of the interval `pos`, pos < num_samples - 1
__device__ inline float pb_power(const float2 *table, float limit, float ll, float mm, float inv_step)
{
    const float s = sqrtf(ll + mm) * inv_step;
    if (!(s < limit))           // beyond the last sample, or NaN
        return __builtin_nanf("");
    const int pos = (int) s;    // 0 <= s < num_samples - 1
    const float frac = s - (float) pos;
    const float2 t = table[pos];
    const float v = t.x + t.y * frac;
    return v * v;
}

__device__ inline float pb_model(float value, float power, float threshold)
{
    return power >= threshold ? value / power : 0.0f;
}

__device__ inline float pb_dirty(float value, float power, float threshold)
{
    return power >= threshold ? value / power : __builtin_nanf("");
}

// P: the number of polarizations, 0 = no images (sample only).  VEC: every row of every array starts
// on a 16-byte boundary.
template <int P, bool VEC>
__global__ __launch_bounds__(PB_LANES * PB_ROWS) void primary_beam_kernel(
    float *__restrict__ beam_power, int64_t beam_row_pitch, float *__restrict__ model,
    float *__restrict__ dirty, int64_t row_pitch, int64_t pol_pitch, int width, int height,
    const float *__restrict__ row, int num_samples, float inv_step, float lm_scale, float lm_bias,
    float threshold)
{
    extern __shared__ float2 pb_table[];
    for (int i = threadIdx.y * PB_LANES + threadIdx.x; i < num_samples - 1; i += PB_LANES * PB_ROWS) {
        const float a = row[i], b = row[i + 1];
        pb_table[i] = make_float2(a, b - a);
    }
    __syncthreads();
    const int64_t x = ((int64_t) blockIdx.x * PB_LANES + threadIdx.x) * 4;
    if (x >= width)
        return;
    const float limit = (float) (num_samples - 1);
    const int count = width - x < 4 ? (int) (width - x) : 4;
    float ll[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float l = lm_coord((int) (x + (k < count ? k : 0)), lm_scale, lm_bias);
        ll[k] = l * l;
    }
    for (int64_t y = (int64_t) blockIdx.y * PB_ROWS + threadIdx.y; y < height;
         y += (int64_t) gridDim.y * PB_ROWS) {
        const float m = lm_coord((int) y, lm_scale, lm_bias);
        const float mm = m * m;
        float power[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            power[k] = pb_power(pb_table, limit, ll[k], mm, inv_step);
        const int64_t beam_at = y * beam_row_pitch + x;
        const int64_t image_at = y * row_pitch + x;
        if (VEC && count == 4) {
            if (beam_power)
                *reinterpret_cast<float4 *>(beam_power + beam_at) =
                    make_float4(power[0], power[1], power[2], power[3]);
            if constexpr (P > 0) {
                float4 mv[P], dv[P];
#pragma unroll
                for (int p = 0; p < P; p++) {
                    mv[p] = *reinterpret_cast<const float4 *>(model + image_at + p * pol_pitch);
                    dv[p] = *reinterpret_cast<const float4 *>(dirty + image_at + p * pol_pitch);
                }
#pragma unroll
                for (int p = 0; p < P; p++) {
                    *reinterpret_cast<float4 *>(model + image_at + p * pol_pitch) = make_float4(
                        pb_model(mv[p].x, power[0], threshold), pb_model(mv[p].y, power[1], threshold),
                        pb_model(mv[p].z, power[2], threshold), pb_model(mv[p].w, power[3], threshold));
                    *reinterpret_cast<float4 *>(dirty + image_at + p * pol_pitch) = make_float4(
                        pb_dirty(dv[p].x, power[0], threshold), pb_dirty(dv[p].y, power[1], threshold),
                        pb_dirty(dv[p].z, power[2], threshold), pb_dirty(dv[p].w, power[3], threshold));
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (k >= count)
                    break;
                if (beam_power)
                    beam_power[beam_at + k] = power[k];
                if constexpr (P > 0) {
#pragma unroll
                    for (int p = 0; p < P; p++) {
                        const int64_t at = image_at + k + p * pol_pitch;
                        model[at] = pb_model(model[at], power[k], threshold);
                        dirty[at] = pb_dirty(dirty[at], power[k], threshold);
                    }
                }
            }
        }
    }
}

bool pb_aligned(const void *ptr, int64_t pitch)
{
    return ptr == nullptr || ((uintptr_t) ptr % 16 == 0 && pitch % 4 == 0);
}

}  // namespace

extern "C" int kimg_primary_beam(float *beam_power, int64_t beam_row_pitch, float *model,
                                 float *dirty, int64_t row_pitch, int64_t pol_pitch, int width,
                                 int height, int num_polarizations, const float *row,
                                 int num_samples, float inv_step, float lm_scale, float lm_bias,
                                 float threshold, void *stream)
{
    KIMG_CHECK_ARG(row && width > 0 && height > 0);
    KIMG_CHECK_ARG(num_polarizations >= 1 && num_polarizations <= 4);
    KIMG_CHECK_ARG(num_samples >= 2 && num_samples <= KIMG_PRIMARY_BEAM_MAX_SAMPLES);
    KIMG_CHECK_ARG(inv_step > 0.0f);                    // (a NaN is refused too)
    KIMG_CHECK_ARG((model != nullptr) == (dirty != nullptr));
    KIMG_CHECK_ARG(model || beam_power);
    KIMG_CHECK_ARG(!beam_power || beam_row_pitch >= width);
    if (model) {
        KIMG_CHECK_ARG(model != dirty && row_pitch >= width);
        KIMG_CHECK_ARG(row_pitch <= (INT64_MAX / 8) / height);
        // the planes of the polarizations do not run into each other
        KIMG_CHECK_ARG(num_polarizations == 1 || pol_pitch >= (int64_t) (height - 1) * row_pitch + width);
    }
    KIMG_CHECK_ARG(!beam_power || beam_row_pitch <= (INT64_MAX / 8) / height);
    const bool vec = pb_aligned(beam_power, beam_row_pitch) && pb_aligned(model, row_pitch)
                     && pb_aligned(dirty, row_pitch) && (model == nullptr || pol_pitch % 4 == 0);
    const int gx = kimg_divup(kimg_divup(width, 4), PB_LANES);
    int gy = kimg_divup(height, PB_ROWS);
    const int most = PB_MAX_BLOCKS / gx > 0 ? PB_MAX_BLOCKS / gx : 1;
    if (gy > most)
        gy = most;
    const dim3 grid(gx, gy), block(PB_LANES, PB_ROWS);
    const size_t lds = (size_t) (num_samples - 1) * sizeof(float2);
    hipStream_t s = (hipStream_t) stream;
    auto launch = [&](auto p, auto v) {
        primary_beam_kernel<decltype(p)::value, decltype(v)::value><<<grid, block, lds, s>>>(
            beam_power, beam_row_pitch, model, dirty, row_pitch, pol_pitch, width, height, row,
            num_samples, inv_step, lm_scale, lm_bias, threshold);
    };
    auto launch_pols = [&](auto v) {
        if (model)
            kimg_for_pols(num_polarizations, [&](auto p) { launch(p, v); });
        else
            launch(std::integral_constant<int, 0>{}, v);
    };
    if (vec)
        launch_pols(std::true_type{});
    else
        launch_pols(std::false_type{});
    return kimg_launch_status();
}

KIMG_PRELOAD_THIS_UNIT((primary_beam_kernel<1, true>))
