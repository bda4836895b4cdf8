// Training-ray generation for gfx950: pixel selection (uniform and error-buffer importance sampling) and the
// pixel -> ray gather, all on device-resident dataset tensors.  SURVEY.md section 8f row N2: the step immediately before
// the hot path (datasets/base/pixel_source.py:39-76 get_rays, :564-731 sample_important_rays / sample_uniform_rays /
// get_train_rays).
//
//   * emer_gen_rays: ONE kernel does everything get_train_rays does after the (img, y, x) selection: pinhole ray through
//     pixel (x + 0.5, y + 0.5), rotation by the camera-to-world matrix, normalisation, and the gathers of colour, sky
//     mask, timestamp and camera id.  The reference issues ~25 indexing / elementwise launches for this.
//   * emer_sample_uniform: torch.randint x3 + an index gather -> one launch on a counter-based generator
//     (splitmix64 of (seed, counter): every sample is a pure function of its index, so a captured hipGraph replays
//     different rays by bumping the seed word in device memory).
//   * emer_sample_importance: torch.multinomial(error_map, n, replacement=False) over several million weights.  Sampling
//     WITHOUT replacement with probabilities proportional to w is the Efraimidis-Spirakis race: key_i = -log(u_i) / w_i,
//     take the n smallest keys.  The n-th smallest key is found by a 3-pass radix select (11 + 11 + 10 bits, LDS
//     histograms, state in device memory: no host round trip), then one compaction pass emits the winners.  Keys are
//     recomputed from the generator in every pass instead of being stored (the weights are read 4 times = 4 x 31 MB for
//     200 images at 160 x 240: ~25 us at HBM speed).
//   * emer_render_rays_lowres: get_render_rays at a downscale factor (:733-846) -- antialiased bicubic colours, nearest
//     masks, rays of the scaled camera, features -- one launch per image.
//   * emer_pixel_error_image / emer_pixel_error_normalise: update_pixel_error_maps (:491-517) on the device, in place.
#include "common.h"

namespace emer {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t rnd32(uint64_t seed, uint64_t ctr) { return (uint32_t)(mix64(seed + ctr * 0x9E3779B97F4A7C15ull) >> 32); }
__device__ __forceinline__ uint32_t rnd_below(uint64_t seed, uint64_t ctr, uint32_t n) { return (uint32_t)(((uint64_t)rnd32(seed, ctr) * n) >> 32); }

// ------------------------------------------------------------------------------------------------- ray gather
struct GenRaysArgs {
    const int64_t *img_idx, *y, *x;          // [n]
    const float *c2w;                        // [n_imgs][4][4]
    const float *intrinsics;                 // [n_imgs][3][3]
    const float *images;                     // [n_imgs][H][W][3] or null
    const float *sky_masks;                  // [n_imgs][H][W] or null
    const float *timestamps;                 // [n_imgs] or null
    const int64_t *cam_ids;                  // [n_imgs] or null
    int64_t n; int32_t H, W;
    float *origins, *viewdirs, *direction_norms, *pixel_coords, *pixels, *sky, *ray_t;
    int64_t *ray_cam;
};

__global__ __launch_bounds__(256) void gen_rays_kernel(const GenRaysArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int64_t im = a.img_idx[i], yy = a.y[i], xx = a.x[i];
    const float *K = a.intrinsics + im * 9, *M = a.c2w + im * 16;
    // pixel_source.py:57-66: camera_dirs = ((x - cx + 0.5) / fx, (y - cy + 0.5) / fy, 1)
    const float cd[3] = {((float)xx - K[2] + 0.5f) / K[0], ((float)yy - K[5] + 0.5f) / K[4], 1.0f};
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = (cd[0] * M[r * 4 + 0] + cd[1] * M[r * 4 + 1]) + cd[2] * M[r * 4 + 2];  // (camera_dirs * R).sum(-1)
    const float nrm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        a.origins[i * 3 + r] = M[r * 4 + 3];
        a.viewdirs[i * 3 + r] = d[r] / (nrm + 1e-8f);
    }
    a.direction_norms[i] = nrm;
    if (a.pixel_coords) { a.pixel_coords[i * 2 + 0] = (float)yy / (float)a.H; a.pixel_coords[i * 2 + 1] = (float)xx / (float)a.W; }
    const int64_t pix = (im * a.H + yy) * a.W + xx;
    if (a.images) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.pixels[i * 3 + c] = a.images[pix * 3 + c];
    }
    if (a.sky_masks) a.sky[i] = a.sky_masks[pix];
    if (a.timestamps) a.ray_t[i] = a.timestamps[im];
    if (a.cam_ids) a.ray_cam[i] = a.cam_ids[im];
}

// ---------------------------------------------------------------------------------------------- uniform pixels
__global__ __launch_bounds__(256) void sample_uniform_kernel(const uint64_t *__restrict__ seed_word, uint64_t salt, int64_t n,
                                                             const int64_t *__restrict__ cand, int32_t n_cand, int32_t H, int32_t W,
                                                             int64_t *__restrict__ img_idx, int64_t *__restrict__ y, int64_t *__restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t seed = seed_word[0] ^ salt;
    const uint32_t c = rnd_below(seed, 3ull * (uint64_t)i + 0, (uint32_t)n_cand);
    img_idx[i] = cand ? cand[c] : (int64_t)c;
    x[i] = (int64_t)rnd_below(seed, 3ull * (uint64_t)i + 1, (uint32_t)W);
    y[i] = (int64_t)rnd_below(seed, 3ull * (uint64_t)i + 2, (uint32_t)H);
}

// ------------------------------------------------------------------------------------------------ lidar rays
// datasets/base/lidar_source.py:223-308: sample_uniform_rays draws torch.randint(0, len(cached), n) and get_train_rays gathers origins,
// directions, ranges and normalised timestamps of the cached scans with it (five launches); one launch here.  idx_in != null: gather only
// (the draw was made elsewhere, e.g. a recording).
__global__ __launch_bounds__(256) void lidar_sample_kernel(const uint64_t *__restrict__ seed_word, uint64_t salt, int64_t n, int64_t n_points,
                                                           const int64_t *__restrict__ idx_in, const float *__restrict__ origins,
                                                           const float *__restrict__ dirs, const float *__restrict__ ranges,
                                                           const float *__restrict__ ts, int64_t *__restrict__ idx_out, float *__restrict__ o,
                                                           float *__restrict__ d, float *__restrict__ r, float *__restrict__ t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t p;
    if (idx_in) {
        p = idx_in[i];
    } else {   // 64-bit product: scans of a whole log may hold more than 2^32 / 2 points
        const uint64_t seed = seed_word[0] ^ salt;
        const uint64_t u = mix64(seed + (uint64_t)i * 0x9E3779B97F4A7C15ull);
        p = (int64_t)__umul64hi(u, (uint64_t)n_points);
    }
    if (idx_out) idx_out[i] = p;
#pragma unroll
    for (int c = 0; c < 3; ++c) { o[i * 3 + c] = origins[p * 3 + c]; d[i * 3 + c] = dirs[p * 3 + c]; }
    r[i] = ranges[p];
    if (ts) t[i] = ts[p];
}

// ------------------------------------------------------------------------------- importance sampling (race)
// race key of element i as an order-preserving u32 (positive floats compare like their bit patterns); w <= 0 -> +inf
__device__ __forceinline__ uint32_t race_key(uint64_t seed, int64_t i, float w) {
    if (!(w > 0.0f)) return 0x7F800000u;
    const float u = ((float)(rnd32(seed, (uint64_t)i) >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
    const float key = -logf(u) / w;
    return __float_as_uint(key) & 0x7FFFFFFFu;  // u = 1 gives -log(1) / w = -0.0: the sign bit must not reach the radix digits
}

// state (device): [0] prefix value of the bits fixed so far, [1] winners still to be found inside the prefix bucket,
// [2] compaction cursor for keys below the threshold, [3] cursor for keys equal to it
constexpr int kSelBins = 2048;

__global__ __launch_bounds__(256) void race_hist_kernel(const float *__restrict__ w, int64_t n, const uint64_t *__restrict__ seed_word,
                                                        uint64_t salt, const uint32_t *__restrict__ state, uint32_t prefix_mask,
                                                        int shift, uint32_t bin_mask, uint32_t *__restrict__ hist) {
    __shared__ uint32_t lh[kSelBins];
    for (int b = threadIdx.x; b < kSelBins; b += 256) lh[b] = 0;
    __syncthreads();
    const uint64_t seed = seed_word[0] ^ salt;
    const uint32_t prefix = state[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t k = race_key(seed, i, w[i]);
        if ((k & prefix_mask) == prefix) atomicAdd(lh + ((k >> shift) & bin_mask), 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kSelBins; b += 256)
        if (lh[b]) atomicAdd(hist + b, lh[b]);
}

// one workgroup: find the bin holding the state[1]-th smallest key of the bucket, extend the prefix, clear the histogram
__global__ __launch_bounds__(1024) void race_select_kernel(uint32_t *__restrict__ hist, int n_bins, int shift, uint32_t *__restrict__ state) {
    __shared__ uint32_t cum[kSelBins];
    for (int b = threadIdx.x; b < kSelBins; b += 1024) cum[b] = b < n_bins ? hist[b] : 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t need = state[1], acc = 0;
        int b = 0;
        for (; b < n_bins - 1; ++b) {
            if (acc + cum[b] >= need) break;
            acc += cum[b];
        }
        state[0] |= (uint32_t)b << shift;
        state[1] = need - acc;  // winners to take from bin b (>= 1)
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_bins; b += 1024) hist[b] = 0u;
}

__global__ __launch_bounds__(256) void race_emit_kernel(const float *__restrict__ w, int64_t n, const uint64_t *__restrict__ seed_word,
                                                        uint64_t salt, uint32_t *__restrict__ state, uint32_t k_total,
                                                        int64_t *__restrict__ out) {
    const uint64_t seed = seed_word[0] ^ salt;
    const uint32_t thr = state[0], n_eq = state[1], n_lt = k_total - n_eq;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t k = race_key(seed, i, w[i]);
        if (k < thr) {
            const uint32_t p = atomicAdd(state + 2, 1u);
            if (p < n_lt) out[p] = i;  // (always true when the histograms are consistent; never write out of bounds)
        } else if (k == thr) {
            const uint32_t p = atomicAdd(state + 3, 1u);
            if (p < n_eq) out[n_lt + p] = i;
        }
    }
}

__global__ void race_init_kernel(uint32_t *__restrict__ state, uint32_t k, uint32_t *__restrict__ hist) {
    if (threadIdx.x == 0) { state[0] = 0; state[1] = k; state[2] = 0; state[3] = 0; }
    for (int b = threadIdx.x; b < kSelBins; b += blockDim.x) hist[b] = 0u;
}

// flat index into [n_cand][Hb][Wb] -> (image, y, x) at full resolution with a random sub-cell offset (:600-620)
__global__ __launch_bounds__(256) void buffer_to_pixels_kernel(const int64_t *__restrict__ flat, int64_t n, int32_t Hb, int32_t Wb,
                                                               int32_t downscale, const int64_t *__restrict__ cand, int32_t H,
                                                               int32_t W, const uint64_t *__restrict__ seed_word, uint64_t salt,
                                                               int64_t *__restrict__ img_idx, int64_t *__restrict__ y, int64_t *__restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t seed = seed_word[0] ^ salt;
    const int64_t f = flat[i], plane = (int64_t)Hb * Wb;
    const int64_t c = f / plane, rem = f - c * plane;
    int64_t yy = (rem / Wb) * downscale + (int64_t)rnd_below(seed, 2ull * (uint64_t)i, (uint32_t)downscale);
    int64_t xx = (rem % Wb) * downscale + (int64_t)rnd_below(seed, 2ull * (uint64_t)i + 1, (uint32_t)downscale);
    yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
    xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
    img_idx[i] = cand ? cand[c] : c;
    y[i] = yy; x[i] = xx;
}

// dynamic mask and DINO-feature gathers of get_train_rays / get_render_rays (pixel_source.py:439-468,704-708,786-811): one
// work item per (ray, 16-byte chunk of its feature row) -- consecutive lanes copy consecutive chunks of a row; the item of
// chunk 0 also gathers the mask.  Feature coordinates are torch's float32 product truncated toward zero:
// (y * downscale[0]).long() with y an int64 tensor and downscale a Python float.
__global__ __launch_bounds__(256) void pixel_extras_kernel(const int64_t *__restrict__ img_idx, const int64_t *__restrict__ y,
                                                           const int64_t *__restrict__ x, int64_t n, int32_t H, int32_t W,
                                                           const float *__restrict__ dynamic_masks, const float *__restrict__ features,
                                                           int32_t Hf, int32_t Wf, int32_t E, float scale_y, float scale_x,
                                                           int32_t chunks, float *__restrict__ out_masks, float *__restrict__ out_features) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * chunks) return;
    const int64_t ray = i / chunks;
    const int32_t k = (int32_t)(i - ray * chunks);
    const int64_t img = img_idx[ray], yy = y[ray], xx = x[ray];
    if (k == 0 && dynamic_masks) out_masks[ray] = dynamic_masks[(img * H + yy) * W + xx];
    if (!features) return;
    int64_t fy = (int64_t)((float)yy * scale_y), fx = (int64_t)((float)xx * scale_x);
    fy = fy < 0 ? 0 : (fy > Hf - 1 ? Hf - 1 : fy);   // (in range for every pixel of the image; kept inside the map regardless)
    fx = fx < 0 ? 0 : (fx > Wf - 1 ? Wf - 1 : fx);
    const int64_t src = ((img * Hf + fy) * Wf + fx) * E;
    if ((E & 3) == 0) {
        reinterpret_cast<float4 *>(out_features + ray * E)[k] = reinterpret_cast<const float4 *>(features + src)[k];
    } else {
        for (int32_t e = k; e < E; e += chunks) out_features[ray * E + e] = features[src + e];
    }
}

// ------------------------------------------------------------------------------- low-resolution render rays
// get_render_rays at a downscale factor s != 1 (pixel_source.py:733-846): ONE launch per image, one workgroup per output
// row.  Colours are torch's interpolate(mode="bicubic", antialias=True): a separable filter whose per-axis windows and
// normalised weights come as tables (built once per factor by the host in double precision and rounded to fp32 once, so a
// weight carries one rounding).  The workgroup first applies the row's vertical weights to the source rows it covers --
// work items stride over x * 3 + c, so every source row is read coalesced -- and leaves the W * 3 partial sums in LDS; then
// one work item per output (x, c) applies that column's horizontal weights to them.  Each sum is one serial fma chain
// in registers: no atomics.  Masks are torch's mode="nearest" (source index floor(float(i) * float(1 / s))), the rays are
// gen_rays_kernel's arithmetic on the w x h grid with the intrinsics scaled by float(s), features are get_features' lookup
// with the map's scale divided by s.
struct LowresArgs {
    const float *images, *sky_masks, *dynamic_masks, *features;   // [n_imgs][H][W][3] | [n_imgs][H][W] x2 | [n_imgs][Hf][Wf][E]; each may be null
    const float *c2w, *intrinsics, *timestamps;                   // timestamps may be null
    const int64_t *cam_ids;                                       // may be null
    const int32_t *ymin, *ysize; const float *wy;                 // [h], [h], [h][ky]
    const int32_t *xmin, *xsize; const float *wx;                 // [w], [w], [w][kx]
    int64_t img;
    int32_t H, W, h, w, ky, kx, Hf, Wf, E;
    float s, inv_s, feat_scale_y, feat_scale_x;
    float *origins, *viewdirs, *direction_norm, *pixel_coords, *pixels, *sky, *dyn, *feat, *ray_t;
    int64_t *ray_img, *ray_cam;
};

__global__ __launch_bounds__(256) void render_rays_lowres_kernel(const LowresArgs a) {
    extern __shared__ float col[];   // [W * 3]: this output row's vertically filtered source row
    const int32_t oy = blockIdx.x, tid = threadIdx.x;
    if (a.images) {
        const int32_t row_len = a.W * 3;
        int32_t y0 = a.ymin[oy], ny = a.ysize[oy];
        y0 = y0 < 0 ? 0 : (y0 > a.H ? a.H : y0);                     // (tables are validated by the host; never read outside the image regardless)
        ny = ny < 0 ? 0 : (ny > a.ky ? a.ky : ny);
        if (ny > a.H - y0) ny = a.H - y0;
        const float *src = a.images + ((int64_t)a.img * a.H + y0) * row_len;
        const float *wy = a.wy + (int64_t)oy * a.ky;
        for (int32_t e = tid; e < row_len; e += 256) {
            float acc = 0.0f;
            for (int32_t j = 0; j < ny; ++j) acc = fmaf(wy[j], src[(int64_t)j * row_len + e], acc);
            col[e] = acc;
        }
        __syncthreads();
        for (int32_t o = tid; o < a.w * 3; o += 256) {
            const int32_t ox = o / 3, c = o - ox * 3;
            int32_t x0 = a.xmin[ox], nx = a.xsize[ox];
            x0 = x0 < 0 ? 0 : (x0 > a.W ? a.W : x0);
            nx = nx < 0 ? 0 : (nx > a.kx ? a.kx : nx);
            if (nx > a.W - x0) nx = a.W - x0;
            const float *wx = a.wx + (int64_t)ox * a.kx;
            float acc = 0.0f;
            for (int32_t j = 0; j < nx; ++j) acc = fmaf(wx[j], col[(x0 + j) * 3 + c], acc);
            a.pixels[((int64_t)oy * a.w + ox) * 3 + c] = acc;
        }
    }
    const float *K = a.intrinsics + a.img * 9, *M = a.c2w + a.img * 16;
    // intrinsics * s with [2][2] reset to 1 (:827-828); the products are rounded on their own, as torch rounds them
    const float fx = __fmul_rn(K[0], a.s), cx = __fmul_rn(K[2], a.s), fy = __fmul_rn(K[4], a.s), cy = __fmul_rn(K[5], a.s);
    int32_t sy = (int32_t)floorf((float)oy * a.inv_s);
    sy = sy > a.H - 1 ? a.H - 1 : sy;
    for (int32_t ox = tid; ox < a.w; ox += 256) {
        const int64_t i = (int64_t)oy * a.w + ox;
        const float cd[3] = {((float)ox - cx + 0.5f) / fx, ((float)oy - cy + 0.5f) / fy, 1.0f};
        float d[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = (cd[0] * M[r * 4 + 0] + cd[1] * M[r * 4 + 1]) + cd[2] * M[r * 4 + 2];
        const float nrm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a.origins[i * 3 + r] = M[r * 4 + 3];
            a.viewdirs[i * 3 + r] = d[r] / (nrm + 1e-8f);
        }
        a.direction_norm[i] = nrm;
        a.pixel_coords[i * 2 + 0] = (float)oy / (float)a.h;
        a.pixel_coords[i * 2 + 1] = (float)ox / (float)a.w;
        int32_t sx = (int32_t)floorf((float)ox * a.inv_s);
        sx = sx > a.W - 1 ? a.W - 1 : sx;
        const int64_t pix = ((int64_t)a.img * a.H + sy) * a.W + sx;
        if (a.sky_masks) a.sky[i] = a.sky_masks[pix];
        if (a.dynamic_masks) a.dyn[i] = a.dynamic_masks[pix];
        if (a.timestamps) a.ray_t[i] = a.timestamps[a.img];
        if (a.cam_ids) a.ray_cam[i] = a.cam_ids[a.img];
        a.ray_img[i] = a.img;
    }
    if (a.features) {
        int64_t fr = (int64_t)((float)oy * a.feat_scale_y);
        fr = fr < 0 ? 0 : (fr > a.Hf - 1 ? a.Hf - 1 : fr);
        for (int32_t o = tid; o < a.w * a.E; o += 256) {
            const int32_t ox = o / a.E, e = o - ox * a.E;
            int64_t fc = (int64_t)((float)ox * a.feat_scale_x);
            fc = fc < 0 ? 0 : (fc > a.Wf - 1 ? a.Wf - 1 : fc);
            a.feat[((int64_t)oy * a.w + ox) * a.E + e] = a.features[((a.img * a.Hf + fr) * a.Wf + fc) * a.E + e];
        }
    }
}

// ------------------------------------------------------------------------------------ error-buffer refresh
// update_pixel_error_maps (:491-517) on the device, in place.  pixel_error_image_kernel: ONE workgroup writes an image's
// row of the buffer, err = mean_c |gt - pred| (x 5 where the dynamic opacity exceeds 0.1), and leaves the row's (min, max)
// in extrema[2 * img ..]: wave shuffles, then LDS across the 16 waves -- no atomics.  pixel_error_normalise_kernel: every
// workgroup reduces the per-image extrema itself (a few hundred pairs) and normalises its share of the buffer.
__device__ __forceinline__ void block_min_max(float &lo, float &hi, float *red /* [32] */) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, kWave));
        hi = fmaxf(hi, __shfl_xor(hi, off, kWave));
    }
    const int wave = threadIdx.x / kWave, n_waves = blockDim.x / kWave;
    if (threadIdx.x % kWave == 0) { red[wave] = lo; red[16 + wave] = hi; }
    __syncthreads();
    lo = red[0]; hi = red[16];
    for (int k = 1; k < n_waves; ++k) { lo = fminf(lo, red[k]); hi = fmaxf(hi, red[16 + k]); }
}

__global__ __launch_bounds__(1024) void pixel_error_image_kernel(const float *__restrict__ pred, const float *__restrict__ gt,
                                                                 const float *__restrict__ dyn_opacity, int64_t n_cells,
                                                                 float *__restrict__ err, float *__restrict__ extrema) {
    __shared__ float red[32];
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = threadIdx.x; i < n_cells; i += 1024) {
        float e = ((fabsf(gt[i * 3 + 0] - pred[i * 3 + 0]) + fabsf(gt[i * 3 + 1] - pred[i * 3 + 1])) + fabsf(gt[i * 3 + 2] - pred[i * 3 + 2])) / 3.0f;
        if (dyn_opacity && dyn_opacity[i] > 0.1f) e *= 5.0f;
        err[i] = e;
        lo = fminf(lo, e); hi = fmaxf(hi, e);
    }
    block_min_max(lo, hi, red);
    if (threadIdx.x == 0) { extrema[0] = lo; extrema[1] = hi; }
}

__global__ __launch_bounds__(256) void pixel_error_normalise_kernel(float *__restrict__ maps, int64_t n, const float *__restrict__ extrema,
                                                                    int32_t n_imgs) {
    __shared__ float red[32];
    float lo = INFINITY, hi = -INFINITY;
    for (int32_t k = threadIdx.x; k < n_imgs; k += 256) { lo = fminf(lo, extrema[2 * k]); hi = fmaxf(hi, extrema[2 * k + 1]); }
    block_min_max(lo, hi, red);
    const float range = hi - lo;   // 0 when every cell is equal: 0 / 0 = NaN, as the reference's division gives
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) maps[i] = (maps[i] - lo) / range;
}

}  // namespace emer

using namespace emer;

extern "C" int emer_gen_rays(const int64_t *img_idx, const int64_t *y, const int64_t *x, const float *cam_to_worlds, const float *intrinsics,
                             const float *images, const float *sky_masks, const float *timestamps, const int64_t *cam_ids, int64_t n,
                             int32_t height, int32_t width, float *origins, float *viewdirs, float *direction_norms, float *pixel_coords,
                             float *pixels, float *sky, float *ray_timestamps, int64_t *ray_cam_ids, void *stream) {
    EMER_REQUIRE(n >= 0 && height >= 1 && width >= 1, "gen_rays: bad sizes");
    if (n == 0) return EMER_OK;
    EMER_REQUIRE(img_idx && y && x && cam_to_worlds && intrinsics && origins && viewdirs && direction_norms, "gen_rays: null pointer");
    EMER_REQUIRE((!images || pixels) && (!sky_masks || sky) && (!timestamps || ray_timestamps) && (!cam_ids || ray_cam_ids),
                 "gen_rays: a dataset tensor was given without its output buffer");
    GenRaysArgs a{img_idx, y, x, cam_to_worlds, intrinsics, images, sky_masks, timestamps, cam_ids, n, height, width,
                  origins, viewdirs, direction_norms, pixel_coords, pixels, sky, ray_timestamps, ray_cam_ids};
    hipLaunchKernelGGL(gen_rays_kernel, dim3((uint32_t)ceil_div(n, 256)), dim3(256), 0, as_stream(stream), a);
    return check_launch("gen_rays");
}

extern "C" int emer_gather_pixel_extras(const int64_t *img_idx, const int64_t *y, const int64_t *x, int64_t n, int32_t height, int32_t width,
                                        const float *dynamic_masks, const float *features, int32_t feat_height, int32_t feat_width,
                                        int32_t feat_dim, float scale_y, float scale_x, float *out_masks, float *out_features,
                                        void *stream) {
    EMER_REQUIRE(n >= 0 && height >= 1 && width >= 1, "gather_pixel_extras: bad sizes");
    EMER_REQUIRE(!features || (feat_height >= 1 && feat_width >= 1 && feat_dim >= 1), "gather_pixel_extras: bad feature-map sizes");
    if (n == 0 || (!dynamic_masks && !features)) return EMER_OK;
    EMER_REQUIRE(img_idx && y && x && (!dynamic_masks || out_masks) && (!features || out_features), "gather_pixel_extras: null pointer");
    EMER_REQUIRE(!features || (feat_dim & 3) != 0 || ((((uintptr_t)features | (uintptr_t)out_features) & 15) == 0),
                 "gather_pixel_extras: feature buffers must be 16-byte aligned");
    // chunks per ray: 16-byte chunks of the feature row (scalar copies when feat_dim % 4 != 0, 64 lanes' worth at most)
    const int32_t chunks = !features ? 1 : ((feat_dim & 3) == 0 ? feat_dim / 4 : (feat_dim < 64 ? feat_dim : 64));
    hipLaunchKernelGGL(pixel_extras_kernel, dim3((uint32_t)ceil_div(n * chunks, 256)), dim3(256), 0, as_stream(stream), img_idx, y, x, n, height,
                       width, dynamic_masks, features, feat_height, feat_width, feat_dim, scale_y, scale_x, chunks, out_masks, out_features);
    return check_launch("gather_pixel_extras");
}

extern "C" int emer_sample_uniform(const uint64_t *seed_word, uint64_t salt, int64_t n, const int64_t *candidates, int32_t n_candidates,
                                   int32_t height, int32_t width, int64_t *img_idx, int64_t *y, int64_t *x, void *stream) {
    EMER_REQUIRE(n >= 0 && n_candidates >= 1 && height >= 1 && width >= 1, "sample_uniform: bad sizes");
    if (n == 0) return EMER_OK;
    EMER_REQUIRE(seed_word && img_idx && y && x, "sample_uniform: null pointer");
    hipLaunchKernelGGL(sample_uniform_kernel, dim3((uint32_t)ceil_div(n, 256)), dim3(256), 0, as_stream(stream), seed_word, salt, n,
                       candidates, n_candidates, height, width, img_idx, y, x);
    return check_launch("sample_uniform");
}

extern "C" int emer_lidar_sample_rays(const uint64_t *seed_word, uint64_t salt, int64_t n, int64_t n_points, const int64_t *idx_in,
                                      const float *origins, const float *directions, const float *ranges, const float *timestamps,
                                      int64_t *idx_out, float *out_origins, float *out_directions, float *out_ranges, float *out_timestamps,
                                      void *stream) {
    EMER_REQUIRE(n >= 0 && n_points >= 1, "lidar_sample_rays: need n >= 0 and at least one cached point");
    if (n == 0) return EMER_OK;
    EMER_REQUIRE((seed_word || idx_in) && origins && directions && ranges && out_origins && out_directions && out_ranges,
                 "lidar_sample_rays: null pointer");
    EMER_REQUIRE((timestamps == nullptr) == (out_timestamps == nullptr), "lidar_sample_rays: timestamps and their output go together");
    hipLaunchKernelGGL(lidar_sample_kernel, dim3((uint32_t)ceil_div(n, 256)), dim3(256), 0, as_stream(stream), seed_word, salt, n, n_points, idx_in,
                       origins, directions, ranges, timestamps, idx_out, out_origins, out_directions, out_ranges, out_timestamps);
    return check_launch("lidar_sample_rays");
}

// workspace: 4 + 2048 u32 words (reset by the first launch: it may hold anything).  flat_out receives the k winners in the order
// the emit pass's atomic cursors hand out, not sorted.  k beyond the number of finite keys fills up with entries of key +inf.
// Key +inf is shared by the weights that are not positive (zero, negative, NaN) and by positive weights so small that
// -logf(u) / w overflows: w < 24 ln 2 / FLT_MAX = 4.9e-38, subnormals and the two lowest binades of the normal range.  Such a
// weight counts as support in PixelSource.sample_important_rays but is drawn like a zero weight.  The normalised error map
// (e - lo) / (hi - lo) with hi - lo <= 5 holds one only where a cell's mean |gt - pred| lies within 2.4e-37 of the minimum
// without being equal to it, i.e. a rendered colour that agrees with an 8-bit ground truth to 37 decimals in all three
// channels yet not exactly; the arithmetic does not exclude it (a sigmoid output below 1e-37 against a black pixel), nothing
// rendered has produced it, and it only matters when k reaches the size of the support.
extern "C" int emer_sample_importance(const float *weights, int64_t n_weights, const uint64_t *seed_word, uint64_t salt, int64_t k,
                                      uint32_t *workspace, int64_t *flat_out, void *stream) {
    EMER_REQUIRE(n_weights >= 1 && k >= 0 && k <= n_weights && k < (1ll << 31), "sample_importance: need 0 <= k <= n_weights");
    if (k == 0) return EMER_OK;
    EMER_REQUIRE(weights && seed_word && workspace && flat_out, "sample_importance: null pointer");
    hipStream_t st = as_stream(stream);
    uint32_t *state = workspace, *hist = workspace + 4;
    hipLaunchKernelGGL(race_init_kernel, dim3(1), dim3(1024), 0, st, state, (uint32_t)k, hist);
    int64_t blocks = ceil_div(n_weights, 256 * 8);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    // keys are non-negative floats: bit 31 is 0, so the three digits are bits 30..21 | 20..10 | 9..0 -> 10 + 11 + 10 bits
    const int shifts[3] = {21, 10, 0};
    const int bins[3] = {1024, 2048, 1024};
    uint32_t prefix_mask = 0;
    for (int p = 0; p < 3; ++p) {
        hipLaunchKernelGGL(race_hist_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, weights, n_weights, seed_word, salt, state, prefix_mask,
                           shifts[p], (uint32_t)(bins[p] - 1), hist);
        hipLaunchKernelGGL(race_select_kernel, dim3(1), dim3(1024), 0, st, hist, bins[p], shifts[p], state);
        prefix_mask |= (uint32_t)(bins[p] - 1) << shifts[p];
    }
    hipLaunchKernelGGL(race_emit_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, weights, n_weights, seed_word, salt, state, (uint32_t)k, flat_out);
    return check_launch("sample_importance");
}

extern "C" int emer_buffer_to_pixels(const int64_t *flat, int64_t n, int32_t buffer_height, int32_t buffer_width, int32_t downscale,
                                     const int64_t *candidates, int32_t height, int32_t width, const uint64_t *seed_word, uint64_t salt,
                                     int64_t *img_idx, int64_t *y, int64_t *x, void *stream) {
    EMER_REQUIRE(n >= 0 && buffer_height >= 1 && buffer_width >= 1 && downscale >= 1, "buffer_to_pixels: bad sizes");
    if (n == 0) return EMER_OK;
    EMER_REQUIRE(flat && seed_word && img_idx && y && x, "buffer_to_pixels: null pointer");
    hipLaunchKernelGGL(buffer_to_pixels_kernel, dim3((uint32_t)ceil_div(n, 256)), dim3(256), 0, as_stream(stream), flat, n, buffer_height,
                       buffer_width, downscale, candidates, height, width, seed_word, salt, img_idx, y, x);
    return check_launch("buffer_to_pixels");
}

extern "C" int emer_render_rays_lowres(int64_t img_idx, const float *cam_to_worlds, const float *intrinsics, const float *images,
                                       const float *sky_masks, const float *dynamic_masks, const float *features,
                                       const float *timestamps, const int64_t *cam_ids, int32_t height, int32_t width,
                                       int32_t out_height, int32_t out_width, float scale, float inv_scale, const int32_t *ymin,
                                       const int32_t *ysize, const float *wy, int32_t ky, const int32_t *xmin, const int32_t *xsize,
                                       const float *wx, int32_t kx, int32_t feat_height, int32_t feat_width, int32_t feat_dim,
                                       float feat_scale_y, float feat_scale_x, float *origins, float *viewdirs, float *direction_norm,
                                       float *pixel_coords, float *pixels, float *sky, float *dyn, float *out_features,
                                       float *ray_timestamps, int64_t *ray_img_idx, int64_t *ray_cam_ids, void *stream) {
    EMER_REQUIRE(img_idx >= 0 && height >= 1 && width >= 1 && out_height >= 1 && out_width >= 1 && out_height <= height && out_width <= width,
                 "render_rays_lowres: need 1 <= out size <= size");
    EMER_REQUIRE(scale > 0.0f && inv_scale > 0.0f, "render_rays_lowres: need a positive scale");
    EMER_REQUIRE(cam_to_worlds && intrinsics && origins && viewdirs && direction_norm && pixel_coords && ray_img_idx,
                 "render_rays_lowres: null pointer");
    EMER_REQUIRE((!images || (pixels && ymin && ysize && wy && xmin && xsize && wx && ky >= 1 && kx >= 1)) && (!sky_masks || sky) &&
                 (!dynamic_masks || dyn) && (!timestamps || ray_timestamps) && (!cam_ids || ray_cam_ids) && (!features || out_features),
                 "render_rays_lowres: a dataset tensor was given without its output buffer or filter tables");
    EMER_REQUIRE(!features || (feat_height >= 1 && feat_width >= 1 && feat_dim >= 1), "render_rays_lowres: bad feature-map sizes");
    const size_t lds = images ? (size_t)width * 3 * sizeof(float) : 0;
    EMER_REQUIRE(lds <= 48 * 1024, "render_rays_lowres: images wider than 4096 pixels are not supported (row buffer in LDS)");
    LowresArgs a{images, sky_masks, dynamic_masks, features, cam_to_worlds, intrinsics, timestamps, cam_ids, ymin, ysize, wy, xmin, xsize, wx,
                 img_idx, height, width, out_height, out_width, ky, kx, feat_height, feat_width, feat_dim, scale, inv_scale, feat_scale_y,
                 feat_scale_x, origins, viewdirs, direction_norm, pixel_coords, pixels, sky, dyn, out_features, ray_timestamps, ray_img_idx,
                 ray_cam_ids};
    hipLaunchKernelGGL(render_rays_lowres_kernel, dim3((uint32_t)out_height), dim3(256), lds, as_stream(stream), a);
    return check_launch("render_rays_lowres");
}

extern "C" int emer_pixel_error_image(const float *pred_rgb, const float *gt_rgb, const float *dynamic_opacity, int64_t n_cells,
                                      float *error_row, float *extrema, void *stream) {
    EMER_REQUIRE(n_cells >= 1, "pixel_error_image: need at least one cell");
    EMER_REQUIRE(pred_rgb && gt_rgb && error_row && extrema, "pixel_error_image: null pointer");
    hipLaunchKernelGGL(pixel_error_image_kernel, dim3(1), dim3(1024), 0, as_stream(stream), pred_rgb, gt_rgb, dynamic_opacity, n_cells,
                       error_row, extrema);
    return check_launch("pixel_error_image");
}

extern "C" int emer_pixel_error_normalise(float *error_maps, int64_t n_cells, const float *extrema, int32_t n_imgs, void *stream) {
    EMER_REQUIRE(n_cells >= 1 && n_imgs >= 1, "pixel_error_normalise: need at least one cell and one image");
    EMER_REQUIRE(error_maps && extrema, "pixel_error_normalise: null pointer");
    int64_t blocks = ceil_div(n_cells, 256 * 4);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(pixel_error_normalise_kernel, dim3((uint32_t)blocks), dim3(256), 0, as_stream(stream), error_maps, n_cells, extrema, n_imgs);
    return check_launch("pixel_error_normalise");
}
