// Body of cycle_subtract_update_kernel and cycle_subtract_update_masked_kernel (clean.hip), which
// include it with KIMG_LOAD_ALLOWED(y, x) / KIMG_AND_ALLOWED(y, x) defined as nothing and as the load
// of the pixel's mask byte (issued ahead of the pixel loads, so that it travels with them) / "&& it".
// (One text for both, and the unmasked kernel's text what it was: as a function shared by two
// kernels, or as one template with optional trailing arguments, the same body compiled to a
// different schedule of the unmasked kernel.)
    // one round trip for all the state words (they share a cache line)
    const int4 st = *reinterpret_cast<const int4 *>(state);    // count, done, limit, threshold
    const int2 pos = *reinterpret_cast<const int2 *>(&state->pos_y);
    const int done = st.y, py = pos.x, px = pos.y;
    const float4 sc = *reinterpret_cast<const float4 *>(state->scale);
    const float scale[4] = {sc.x, sc.y, sc.z, sc.w};
    if (done)
        return;
    const int x0 = px - patch_w / 2, y0 = py - patch_h / 2;      // clean.py:1024-1027
    // floor division: the lattice extends into the border with negative indices
    const int bx0 = (x0 - border) >= 0 ? (x0 - border) / TILE : -((border - x0 + TILE - 1) / TILE);
    const int by0 = (y0 - border) >= 0 ? (y0 - border) / TILE : -((border - y0 + TILE - 1) / TILE);
    const int tx = bx0 + (int) blockIdx.x, ty = by0 + (int) blockIdx.y;
    const int ox = tx * TILE + border, oy = ty * TILE + border;
    const int psf_dx = psf_w / 2 - px, psf_dy = psf_h / 2 - py;  // psf index = image index + d
    const bool is_tile = tx >= 0 && tx < tiles_x && ty >= 0 && ty < tiles_y;

    float best = 0.0f;
    int best_idx = INT_MAX;             // row-major index within the tile; INT_MAX = none yet
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int idx = threadIdx.x + k * 256;
        const int x = ox + (idx & 31), y = oy + (idx >> 5);
        if (x < 0 || x >= width || y < 0 || y >= height)
            continue;
        const int64_t ia = (int64_t) y * row_stride + x;
        KIMG_LOAD_ALLOWED(y, x)
        const bool in_patch = x >= x0 && x < x0 + patch_w && y >= y0 && y < y0 + patch_h;
        const bool in_tile = is_tile && x < width - border && y < height - border KIMG_AND_ALLOWED(y, x);
        float metric = 0.0f;
        if (MODE == KIMG_CLEAN_I) {
            float d = dirty[ia];
            if (in_patch) {
                const float t = scale[0] * psf[(int64_t) (y + psf_dy) * psf_row_stride + (x + psf_dx)];
                d -= t;
                dirty[ia] = d;
                for (int p = 1; p < P; p++) {
                    const float tp = scale[p] * psf[p * psf_pol_stride
                                                    + (int64_t) (y + psf_dy) * psf_row_stride + (x + psf_dx)];
                    dirty[p * pol_stride + ia] -= tp;
                }
            }
            metric = fabsf(d);
        } else {
            for (int p = 0; p < P; p++) {
                float d = dirty[p * pol_stride + ia];
                if (in_patch) {
                    const float t = scale[p] * psf[p * psf_pol_stride
                                                   + (int64_t) (y + psf_dy) * psf_row_stride + (x + psf_dx)];
                    d -= t;
                    dirty[p * pol_stride + ia] = d;
                }
                metric += d * d;
            }
        }
        if (in_tile && metric > best) {
            best = metric;
            best_idx = idx;
        }
    }
    if (!is_tile)
        return;
    __shared__ key_t s_keys[16];
    const key_t kb = block_max_key(best_idx == INT_MAX ? 0 : make_key(best, best_idx), s_keys);
    if (threadIdx.x == 0) {
        const int t = ty * tiles_x + tx;
        store_tile_record(kb, ox, oy, tile_max, tile_pos, t);
    }
