// Video frames of the eval loop for gfx950: what the reference's save_videos builds per timestep on the host with numpy
// (radiance_fields/video_utils.py:471-627, utils/visualization_tools.py:30-33,79-156) -- every key's images side by side, the
// keys stacked, depth coloured with the turbo table, everything cut to 8 bits -- as ONE launch that reads the fp32 images where
// the render loop left them and writes the merged uint8 [rows * H, cams * W, 3] frame.  Only 3 bytes per pixel leave the GPU.
//
//   * A frame is a list of TILES (emer_frame_tile): a source image, its kind and its (row, column) cell in the frame.
//       colour3          [H, W, 3]: the three channels as they are
//       grey1            [H, W]:    the value on all three channels                      (gt_sky_masks)
//       one-minus-grey1  [H, W]:    1 - value, one fp32 subtraction, on three channels   (sky_masks, from the opacity)
//       depth            [H, W] + opacity [H, W]: t = -logf(x + 1e-6f) in fp32; then in fp64 v = clip((t - dmin) / dabs, 0, 1),
//                        NaN -> 0, p = v * opacity; the colour is row min(trunc(256 p), 255) of the 256-row 8-bit turbo table,
//                        row 0 for p < 0, black for a NaN p.  Three fp64 operations per pixel; logf is the library's, not a
//                        fast intrinsic.
//     8 bits: uint8(255 * clip(x, 0, 1)) truncating, the product in fp32 or -- `fp64_scale`, the reference's frames that hold a
//     depth row -- in fp64 (they differ at rounding ties only); NaN is written as 0.
//   * Bandwidth-bound (4 to 12 bytes read, 3 written per pixel).  A lane takes FOUR horizontally adjacent pixels of one tile
//     row: consecutive lanes read consecutive 16-byte quads (one per lane for one-channel tiles, three for colour tiles) with
//     non-temporal loads -- every source byte is read once -- and write 12 consecutive bytes as three dword stores.  All loads
//     of a lane are issued before the first use and none sits behind a branch: an index past the row's end is clamped into the
//     row and its result dropped, a tile without an opacity reads its source twice.
//   * Paths, chosen on the host, same bytes on each: 16-byte loads need W % 4 == 0 and 16-byte aligned bases (per tile), scalar
//     loads otherwise; dword stores need a 4-byte aligned frame, cams * W % 4 == 0 and col * W % 4 == 0 for every tile (so
//     that every group of four pixels starts on a dword), byte stores otherwise.
//   * The 768-byte table comes from the host and is staged in LDS once per workgroup, one packed dword per row and a black
//     row behind them.
//
// No atomics, no inter-workgroup traffic: a pixel's bytes depend on its own inputs, the tile's kind and the flag alone -- not on
// the tile's cell, the other tiles, the frame's size or the grid.
#include "common.h"
#include <string.h>

// every operation is rounded on its own, as numpy evaluates the chain
#pragma clang fp contract(off)

namespace emer {

constexpr int kFrameThreads = 256;
constexpr int kFrameMaxBlocks = 2048;    // 256 CUs x 8 workgroups; the rest of the frame is grid-strided
constexpr int kTurboRows = 256;

struct FrameTiles { emer_frame_tile t[EMER_FRAME_TILES_MAX]; };
static_assert(sizeof(FrameTiles) <= 2048, "the by-value tile list stays well under the 4 KiB kernel-argument limit");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Four consecutive floats from `row + 4 q`: one 16-byte streamed load, or the same elements one by one with the index clamped
// to `last` (what lies past it is never stored).
template <bool kVec>
__device__ __forceinline__ float4 load4(const float *__restrict__ row, int32_t q, int32_t last) {
    if (kVec) {
        const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(row) + q);
        return make_float4(x.x, x.y, x.z, x.w);
    }
    const int32_t e = 4 * q;
    return make_float4(row[min(e, last)], row[min(e + 1, last)], row[min(e + 2, last)], row[min(e + 3, last)]);
}

// uint8(255 * clip(x, 0, 1)): np.clip leaves NaN, whose cast numpy does not define -- written as 0
__device__ __forceinline__ uint32_t to8(float x, bool fp64_scale) {
    const float c = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    if (c != c) return 0u;
    return fp64_scale ? (uint32_t)(int32_t)(255.0 * (double)c) : (uint32_t)(int32_t)__fmul_rn(255.0f, c);
}

__device__ __forceinline__ uint32_t grey8(float x, bool fp64_scale) { return to8(x, fp64_scale) * 0x010101u; }

// the table row of one depth pixel (row kTurboRows is black)
__device__ __forceinline__ int32_t depth_row(float x, float opacity, double dmin, double dabs) {
    const float t = -logf(__fadd_rn(x, 1e-6f));
    double v = __ddiv_rn(__dsub_rn((double)t, dmin), dabs);
    v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    v = v != v ? 0.0 : v;                                   // nan_to_num after the clip
    const double p = __dmul_rn(v, (double)opacity);
    const int32_t row = p >= 1.0 ? kTurboRows - 1 : (p < 0.0 ? 0 : (int32_t)(p * 256.0));   // 256 p is exact
    return p != p ? kTurboRows : row;
}

__device__ __forceinline__ uint32_t depth8(float x, float opacity, double dmin, double dabs, const uint32_t *__restrict__ lut) {
    return lut[depth_row(x, opacity, dmin, dabs)];
}

// The four pixels `4 g .. 4 g + 3` of row `y` of one tile as four packed colours (r | g << 8 | b << 16).
template <bool kVec>
__device__ __forceinline__ void tile_quad(const emer_frame_tile &T, int32_t y, int32_t g, int32_t W, bool fp64_scale, double dmin,
                                          double dabs, const uint32_t *__restrict__ lut, uint32_t (&px)[4]) {
    const float *__restrict__ src = T.src;
    if (T.kind == EMER_TILE_COLOUR3) {
        const float *__restrict__ row = src + (int64_t)y * W * 3;
        const int32_t last = 3 * W - 1;
        const float4 a = load4<kVec>(row, 3 * g, last), b = load4<kVec>(row, 3 * g + 1, last), c = load4<kVec>(row, 3 * g + 2, last);
        px[0] = to8(a.x, fp64_scale) | to8(a.y, fp64_scale) << 8 | to8(a.z, fp64_scale) << 16;
        px[1] = to8(a.w, fp64_scale) | to8(b.x, fp64_scale) << 8 | to8(b.y, fp64_scale) << 16;
        px[2] = to8(b.z, fp64_scale) | to8(b.w, fp64_scale) << 8 | to8(c.x, fp64_scale) << 16;
        px[3] = to8(c.y, fp64_scale) | to8(c.z, fp64_scale) << 8 | to8(c.w, fp64_scale) << 16;
        return;
    }
    const float *__restrict__ opa = T.opacity != nullptr ? T.opacity : src;   // no branch around the second load
    const int64_t off = (int64_t)y * W;
    const float4 x = load4<kVec>(src + off, g, W - 1), o = load4<kVec>(opa + off, g, W - 1);
    const float xs[4] = {x.x, x.y, x.z, x.w}, os[4] = {o.x, o.y, o.z, o.w};
    if (T.kind == EMER_TILE_DEPTH) {
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = depth8(xs[k], os[k], dmin, dabs, lut);
    } else {
        const bool inv = T.kind == EMER_TILE_ONE_MINUS_GREY1;
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = grey8(inv ? __fsub_rn(1.0f, xs[k]) : xs[k], fp64_scale);
    }
}

// One work item: four pixels of one tile row.  Items are numbered tile-major, then row, then quad, so consecutive lanes take
// consecutive quads of a row.
template <bool kDword>
__global__ __launch_bounds__(kFrameThreads) void compose_frame_kernel(FrameTiles F, uint32_t n_items, int32_t H, int32_t W, int32_t cams,
                                                                     uint64_t vec_mask, int32_t fp64_scale, double dmin, double dabs,
                                                                     const uint8_t *__restrict__ table, uint8_t *__restrict__ out) {
    __shared__ uint32_t lut[kTurboRows + 1];
    for (int32_t i = threadIdx.x; i < kTurboRows + 1; i += kFrameThreads)
        lut[i] = i < kTurboRows ? ((uint32_t)table[3 * i] | (uint32_t)table[3 * i + 1] << 8 | (uint32_t)table[3 * i + 2] << 16) : 0u;
    __syncthreads();
    const uint32_t quads = (uint32_t)(W + 3) / 4, per_tile = quads * (uint32_t)H;
    const int64_t pitch = (int64_t)cams * W * 3;
    const uint32_t step = gridDim.x * kFrameThreads;
    for (uint32_t i = blockIdx.x * kFrameThreads + threadIdx.x; i < n_items; i += step) {
        const uint32_t tile = i / per_tile, r = i - tile * per_tile;
        const int32_t y = (int32_t)(r / quads), g = (int32_t)(r - (uint32_t)y * quads);
        const emer_frame_tile &T = F.t[tile];
        uint32_t px[4];
        if ((vec_mask >> tile) & 1) tile_quad<true>(T, y, g, W, fp64_scale != 0, dmin, dabs, lut, px);
        else tile_quad<false>(T, y, g, W, fp64_scale != 0, dmin, dabs, lut, px);
        uint8_t *__restrict__ dst = out + ((int64_t)T.row * H + y) * pitch + ((int64_t)T.col * W + 4 * g) * 3;
        const int32_t n = min(4, W - 4 * g);
        if (kDword && n == 4) {        // 12 bytes on a dword boundary
            uint32_t *__restrict__ d = reinterpret_cast<uint32_t *>(dst);
            d[0] = px[0] | px[1] << 24;
            d[1] = px[1] >> 8 | px[2] << 16;
            d[2] = px[2] >> 16 | px[3] << 8;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < n) {
                    dst[3 * k] = (uint8_t)px[k];
                    dst[3 * k + 1] = (uint8_t)(px[k] >> 8);
                    dst[3 * k + 2] = (uint8_t)(px[k] >> 16);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the five-view resize
// The reference shrinks the two outer views of a group of five (resize_five_views, utils/visualization_tools.py:36-49): the view
// becomes black with scipy.ndimage.zoom(img, [h / H, 1, 1]) -- a cubic spline -- in its bottom h rows.  Along x and the channels
// that zoom is the identity, so the work is one recursive prefilter and one 4-tap resampling down every column of every
// channel, in fp64, and ONE launch does it for all resized tiles of a frame and writes their cells of the 8-bit frame, black
// rows included.  No fp64 coefficient image exists in global memory.
//
//   * The rule on one column s[0 .. H-1], pole z = sqrt(3) - 2, gain g = (1 - z)(1 - 1/z) = 6: with s continued by mirroring
//     (s[-i] = s[i], s[H-1+i] = s[H-1-i], period 2 (H - 1)) the coefficients are
//         up[i] = g s[i] + z up[i-1],        c[i] = z (c[i+1] - up[i])   =>   c[i] = -sum_{k >= 0} z^(k+1) up[i+k]
//     over the whole line; scipy's whole-line start values are these sums in closed form, and the mirrored c is what its
//     resampling reads for a row outside the image.  Output row y samples at cc = fl(zoom * y), zoom = fl((H - 1) / (h - 1))
//     (formed on the host, the same two roundings as scipy's), with the four B-spline weights of cc - floor(cc) on the rows
//     floor(cc) - 1 .. floor(cc) + 2.
//   * Blocks of kZoomRows input rows.  The block of rows [r0, r1) emits the output rows whose floor(cc) lies in it and so needs
//     c[r0 - 1 .. r1 + 1].  It runs `up` from kZoomWarm rows below r0 - 1 (started at 0), keeps up[r0 - 1 .. r1] in LDS -- one
//     column of doubles per lane, which no other lane touches: no barrier -- runs on for kZoomWarm rows past r1 + 1 while it
//     sums c[r1 + 1] from the formula above, then descends: each step makes one c[i] from LDS into a 4-row register window, and
//     the window emits an output row whenever one falls on it.  Every row index goes through the mirror map, so the two image
//     ends, and an image shorter than the warm-up, need no case of their own.
//   * kZoomWarm: |up| <= g max|s| / (1 - |z|) < 8.2 max|s|, so the dropped start of `up` is below 8.2 |z|^K max|s| at the first
//     kept row, and less once it has gone through the downward pass; the dropped tail of the sum for c[r1 + 1] is below
//     8.2 |z|^(K+2) / (1 - |z|) max|s|.  Together under 9 |z|^K max|s|; against the unit 3 max|s| 2^-53 of the tests' bound, K = 36
//     gives 3 * 2^-68.4: a 2^-13 of one rounding (K = 33 is the first below 2^-60 altogether; three rows more cost 3 % and
//     leave the truncation out of every error budget).
//   * One lane per column and channel: consecutive lanes read consecutive floats of a row (4-byte loads, 256 bytes per wave
//     and row: coalesced for any W and any alignment, so there is one load path) and write consecutive bytes.  The mask kinds
//     are computed once per pixel and written three times.  A depth lane forms its pixel's table row as depth8 does and reads
//     its channel of the 256 x 3 fp64 table, staged in LDS (a NaN position is black).  A lane past the row's end is clamped
//     into it and its results dropped; every loop bound is the same for all lanes.
//   * A source row is read by every block within kZoomWarm rows of it (about 3.3 times, from L2).  The row indices do not
//     depend on data, so the loads of kZoomBatch rows are issued together and each is waited for where it is used (with one
//     load and one full wait per step the launch took 1.9 times as long); the downward pass reads its LDS rows the same way.
//     The tile's kind is decided once per workgroup (zoom_column<kind>), not per step.
//   * Per block and lane: 70 upward steps of 3 fp64 operations, 37 tail steps of 5, 34 downward steps of 2 and some 22 output
//     rows of 7 plus the weights -- about 33 fp64 operations per source value, under a third of them warm-up -- every step
//     waiting for the one before it.  A depth lane also forms its table position at every step (logf, an fp64 division), three
//     lanes per pixel and 3.3 blocks per row: that, not the recurrence, is the longest chain of a frame.  34 816 + 6 144 bytes
//     of LDS are a quarter of a CU's 160 KiB: 4 workgroups, 8 waves per CU.  The dependent chains set the time, not the
//     bandwidth (tools/five_view_timing.py).
constexpr int kZoomThreads = 128;
constexpr int kZoomRows = 32;
constexpr int kZoomWarm = 36;
constexpr int kZoomStore = kZoomRows + 2;       // up[r0 - 1 .. r1]
constexpr int kZoomBatch = 16;                  // rows whose loads are in flight together

__device__ __forceinline__ int32_t mirror_row(int32_t i, int32_t H) {
    const int32_t period = 2 * (H - 1);
    int32_t m = i % period;
    m = m < 0 ? m + period : m;
    return m < H ? m : period - m;
}

// What the zoom reads at one image row, in two halves so that the loads of a whole batch of rows are in flight before the
// first is used: the raw floats of the lane's pixel (a depth lane reads two), and the fp64 value made of them.
template <int kKind>
__device__ __forceinline__ float2 zoom_fetch(const float *__restrict__ src, const float *__restrict__ opacity, int32_t row, int32_t W, int32_t j,
                                             int32_t x) {
    if (kKind == EMER_TILE_COLOUR3) return make_float2(src[(int64_t)row * W * 3 + j], 0.0f);
    const int64_t at = (int64_t)row * W + x;
    return make_float2(src[at], kKind == EMER_TILE_DEPTH ? opacity[at] : 0.0f);
}

template <int kKind>
__device__ __forceinline__ double zoom_value(float2 a, int32_t ch, double dmin, double dabs, const double *__restrict__ lut) {
    if (kKind == EMER_TILE_DEPTH) {
        const int32_t row = depth_row(a.x, a.y, dmin, dabs);
        const double c = lut[3 * min(row, kTurboRows - 1) + ch];
        return row == kTurboRows ? 0.0 : c;         // a NaN position is black
    }
    return (double)(kKind == EMER_TILE_ONE_MINUS_GREY1 ? __fsub_rn(1.0f, a.x) : a.x);
}

struct ZoomArgs {
    int32_t H, W, h, cams, fp64_scale, n_rblocks;
    double dmin, dabs, zoom, z, g;
};

// One lane's column of one row block (the scheme above).  `up`: the lane's LDS column, kZoomThreads doubles from row to row.
template <int kKind>
__device__ __forceinline__ void zoom_column(const emer_frame_tile &T, const ZoomArgs &A, int32_t rb, int32_t j, int32_t width,
                                            double *__restrict__ up, const double *__restrict__ lut, uint8_t *__restrict__ cell,
                                            double *__restrict__ vals) {
    constexpr bool grey = kKind == EMER_TILE_GREY1 || kKind == EMER_TILE_ONE_MINUS_GREY1;
    const int32_t H = A.H, W = A.W, h = A.h;
    const double z = A.z, g = A.g, zoom = A.zoom;
    const bool live = j < width;
    const int32_t jc = min(j, width - 1), x = grey ? jc : jc / 3, ch = grey ? 0 : jc - 3 * x;
    const float *__restrict__ src = T.src, *__restrict__ opacity = T.opacity;
    const int32_t r0 = rb * kZoomRows, r1 = min(r0 + kZoomRows, H), lo = r0 - 1, hi = r1 + 1;

    // upwards over the rows lo - K .. hi + K: warm-up, the kept rows, the tail that sums c[hi] = -sum_k z^(k+1) up[hi + k]
    const int32_t first = lo - kZoomWarm, n_up = hi + kZoomWarm - first + 1;
    double cp = 0.0, tail = 0.0, zp = z;
    for (int32_t b = 0; b < n_up; b += kZoomBatch) {
        float2 a[kZoomBatch];
#pragma unroll
        for (int k = 0; k < kZoomBatch; ++k)        // past the last row of the pass: that row again, dropped below
            a[k] = zoom_fetch<kKind>(src, opacity, mirror_row(first + min(b + k, n_up - 1), H), W, jc, x);
#pragma unroll
        for (int k = 0; k < kZoomBatch; ++k) {
            const int32_t i = first + b + k;
            if (b + k < n_up) {
                cp = g * zoom_value<kKind>(a[k], ch, A.dmin, A.dabs, lut) + z * cp;
                if (i >= lo && i < hi) up[(i - lo) * kZoomThreads] = cp;
                if (i >= hi) {
                    tail = tail + zp * cp;
                    zp = zp * z;
                }
            }
        }
    }

    // the last output row of this block: the largest y with fl(zoom y) < r1
    int32_t y = min(h - 1, (int32_t)((double)r1 / zoom));
    while (y + 1 < h && zoom * (double)(y + 1) < (double)r1) ++y;
    while (y >= 0 && zoom * (double)y >= (double)r1) --y;

    const int64_t pitch = (int64_t)A.cams * W * 3;
    double c0 = -tail, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    for (int32_t ib = hi - 1; ib >= lo; ib -= kZoomBatch) {
        double u[kZoomBatch];
#pragma unroll
        for (int k = 0; k < kZoomBatch; ++k) u[k] = up[(max(ib - k, lo) - lo) * kZoomThreads];
#pragma unroll
        for (int k = 0; k < kZoomBatch; ++k) {
            const int32_t i = ib - k;
            if (i < lo) break;
            c3 = c2;
            c2 = c1;
            c1 = c0;
            c0 = z * (c1 - u[k]);                   // c0 .. c3 = c[i .. i + 3]
            while (i <= hi - 3 && y >= 0 && (int32_t)floor(zoom * (double)y) == i + 1) {
                const double cc = zoom * (double)y, t = cc - floor(cc), w = 1.0 - t;
                const double w1 = __ddiv_rn(t * t * (t - 2.0) * 3.0 + 4.0, 6.0), w2 = __ddiv_rn(w * w * (w - 2.0) * 3.0 + 4.0, 6.0);
                const double w0 = __ddiv_rn(w * w * w, 6.0), w3 = 1.0 - w0 - w1 - w2;
                const double v = c0 * w0 + c1 * w1 + c2 * w2 + c3 * w3;
                uint32_t b8;
                if (kKind == EMER_TILE_DEPTH) {     // an fp64 image in the reference: no rounding to fp32, 255 x in fp64
                    const double c = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
                    b8 = c != c ? 0u : (uint32_t)(int32_t)(255.0 * c);
                } else {
                    b8 = to8((float)v, A.fp64_scale != 0);   // scipy returns the fp32 image's type
                }
                if (live) {
                    uint8_t *__restrict__ dst = cell + (int64_t)(H - h + y) * pitch;
                    double *__restrict__ vd = vals + (vals != nullptr ? (int64_t)y * W * 3 : 0);
                    if (grey) {
                        dst[3 * x] = (uint8_t)b8;
                        dst[3 * x + 1] = (uint8_t)b8;
                        dst[3 * x + 2] = (uint8_t)b8;
                        if (vals != nullptr) {
                            vd[3 * x] = v;
                            vd[3 * x + 1] = v;
                            vd[3 * x + 2] = v;
                        }
                    } else {
                        dst[jc] = (uint8_t)b8;
                        if (vals != nullptr) vd[jc] = v;
                    }
                }
                --y;
            }
        }
    }
    // the black rows above, shared out among the row blocks
    if (live) {
        for (int32_t yb = rb; yb < H - h; yb += A.n_rblocks) {
            uint8_t *__restrict__ dst = cell + (int64_t)yb * pitch;
            if (grey) {
                dst[3 * x] = 0;
                dst[3 * x + 1] = 0;
                dst[3 * x + 2] = 0;
            } else {
                dst[jc] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(kZoomThreads) void zoom_tiles_kernel(FrameTiles F, ZoomArgs A, int32_t n_groups, const double *__restrict__ table64,
                                                                 uint8_t *__restrict__ out, double *__restrict__ values) {
    __shared__ double up[kZoomStore * kZoomThreads];
    __shared__ double lut[3 * kTurboRows];
    const int32_t tid = threadIdx.x;
    const int32_t group = (int32_t)(blockIdx.x % (uint32_t)n_groups), rb = (int32_t)(blockIdx.x / (uint32_t)n_groups % (uint32_t)A.n_rblocks);
    const int32_t tile = (int32_t)(blockIdx.x / ((uint32_t)n_groups * (uint32_t)A.n_rblocks));
    const emer_frame_tile &T = F.t[tile];
    const int32_t kind = T.kind;
    const int32_t width = kind == EMER_TILE_GREY1 || kind == EMER_TILE_ONE_MINUS_GREY1 ? A.W : 3 * A.W;
    if (group * kZoomThreads >= width) return;      // the whole workgroup: a mask tile has a third of the lanes
    if (kind == EMER_TILE_DEPTH) {
        for (int32_t i = tid; i < 3 * kTurboRows; i += kZoomThreads) lut[i] = table64[i];
        __syncthreads();
    }
    const int32_t j = group * kZoomThreads + tid;
    uint8_t *__restrict__ cell = out + (int64_t)T.row * A.H * ((int64_t)A.cams * A.W * 3) + (int64_t)T.col * A.W * 3;
    double *__restrict__ vals = values != nullptr ? values + (int64_t)tile * A.h * A.W * 3 : nullptr;
    if (kind == EMER_TILE_COLOUR3) zoom_column<EMER_TILE_COLOUR3>(T, A, rb, j, width, up + tid, lut, cell, vals);
    else if (kind == EMER_TILE_GREY1) zoom_column<EMER_TILE_GREY1>(T, A, rb, j, width, up + tid, lut, cell, vals);
    else if (kind == EMER_TILE_ONE_MINUS_GREY1) zoom_column<EMER_TILE_ONE_MINUS_GREY1>(T, A, rb, j, width, up + tid, lut, cell, vals);
    else zoom_column<EMER_TILE_DEPTH>(T, A, rb, j, width, up + tid, lut, cell, vals);
}

}  // namespace emer

using namespace emer;

extern "C" int emer_compose_frame(const emer_frame_tile *tiles, int32_t n_tiles, int32_t H, int32_t W, int32_t rows, int32_t cams,
                                  int32_t fp64_scale, const double *depth_range, const uint8_t *table, uint8_t *out, void *stream) {
    EMER_REQUIRE(tiles && n_tiles >= 1 && n_tiles <= EMER_FRAME_TILES_MAX, "compose_frame: 1..%d tiles per launch", EMER_FRAME_TILES_MAX);
    EMER_REQUIRE(H >= 1 && W >= 1 && rows >= 1 && cams >= 1 && (int64_t)rows * H < (1ll << 31) && (int64_t)cams * W * 3 < (1ll << 31),
                 "compose_frame: need H, W, rows, cams >= 1 and a frame of fewer than 2^31 rows and bytes per row");
    EMER_REQUIRE(depth_range && table && out, "compose_frame: null depth range, table or frame");
    const double dmin = depth_range[0], dabs = depth_range[1];
    EMER_REQUIRE(dmin == dmin && dabs == dabs, "compose_frame: the depth range is NaN");
    const int64_t quads = ((int64_t)W + 3) / 4, n_items = quads * H * n_tiles;
    EMER_REQUIRE(n_items < (1ll << 31), "compose_frame: %d tiles of %d x %d are too many pixels for one launch", n_tiles, H, W);
    FrameTiles F;
    memset(&F, 0, sizeof(F));
    uint64_t vec_mask = 0;
    bool dword = ((uintptr_t)out & 3) == 0 && ((int64_t)cams * W) % 4 == 0;
    for (int32_t i = 0; i < n_tiles; ++i) {
        const emer_frame_tile &t = tiles[i];
        EMER_REQUIRE(t.src, "compose_frame: tile %d: null source", i);
        EMER_REQUIRE(t.kind >= EMER_TILE_COLOUR3 && t.kind <= EMER_TILE_DEPTH, "compose_frame: tile %d: unknown kind %d", i, t.kind);
        EMER_REQUIRE(t.kind != EMER_TILE_DEPTH || t.opacity, "compose_frame: tile %d: a depth tile needs its opacity", i);
        EMER_REQUIRE(t.row >= 0 && t.row < rows && t.col >= 0 && t.col < cams, "compose_frame: tile %d: cell (%d, %d) outside the %d x %d frame", i,
                     t.row, t.col, rows, cams);
        F.t[i] = t;
        if (t.kind != EMER_TILE_DEPTH) F.t[i].opacity = nullptr;
        if (W % 4 == 0 && ((uintptr_t)t.src & 15) == 0 && ((uintptr_t)F.t[i].opacity & 15) == 0) vec_mask |= 1ull << i;
        if (((int64_t)t.col * W) % 4 != 0) dword = false;
    }
    const int64_t blocks = ceil_div(n_items, kFrameThreads);
    const dim3 grid((uint32_t)(blocks < kFrameMaxBlocks ? blocks : kFrameMaxBlocks)), block(kFrameThreads);
    hipStream_t st = as_stream(stream);
    if (dword)
        hipLaunchKernelGGL(compose_frame_kernel<true>, grid, block, 0, st, F, (uint32_t)n_items, H, W, cams, vec_mask, fp64_scale, dmin, dabs, table, out);
    else
        hipLaunchKernelGGL(compose_frame_kernel<false>, grid, block, 0, st, F, (uint32_t)n_items, H, W, cams, vec_mask, fp64_scale, dmin, dabs, table, out);
    return check_launch("compose_frame");
}

extern "C" int emer_zoom_tiles(const emer_frame_tile *tiles, int32_t n_tiles, int32_t H, int32_t W, int32_t h_out, int32_t rows, int32_t cams,
                               int32_t fp64_scale, const double *depth_range, const double *table64, uint8_t *frame_out, double *values_out,
                               void *stream) {
    EMER_REQUIRE(tiles && n_tiles >= 1 && n_tiles <= EMER_FRAME_TILES_MAX, "zoom_tiles: 1..%d tiles per launch", EMER_FRAME_TILES_MAX);
    EMER_REQUIRE(H >= 1 && W >= 1 && rows >= 1 && cams >= 1 && (int64_t)rows * H < (1ll << 31) && (int64_t)cams * W * 3 < (1ll << 31),
                 "zoom_tiles: need H, W, rows, cams >= 1 and a frame of fewer than 2^31 rows and bytes per row");
    EMER_REQUIRE(h_out >= 2 && h_out <= H, "zoom_tiles: %d output rows from %d: need 2 <= h_out <= H", h_out, H);
    EMER_REQUIRE(depth_range && table64 && frame_out, "zoom_tiles: null depth range, table or frame");
    const double dmin = depth_range[0], dabs = depth_range[1];
    EMER_REQUIRE(dmin == dmin && dabs == dabs, "zoom_tiles: the depth range is NaN");
    FrameTiles F;
    memset(&F, 0, sizeof(F));
    for (int32_t i = 0; i < n_tiles; ++i) {
        const emer_frame_tile &t = tiles[i];
        EMER_REQUIRE(t.src, "zoom_tiles: tile %d: null source", i);
        EMER_REQUIRE(t.kind >= EMER_TILE_COLOUR3 && t.kind <= EMER_TILE_DEPTH, "zoom_tiles: tile %d: unknown kind %d", i, t.kind);
        EMER_REQUIRE(t.kind != EMER_TILE_DEPTH || t.opacity, "zoom_tiles: tile %d: a depth tile needs its opacity", i);
        EMER_REQUIRE(t.row >= 0 && t.row < rows && t.col >= 0 && t.col < cams, "zoom_tiles: tile %d: cell (%d, %d) outside the %d x %d frame", i,
                     t.row, t.col, rows, cams);
        F.t[i] = t;
        if (t.kind != EMER_TILE_DEPTH) F.t[i].opacity = nullptr;
    }
    const int64_t n_rblocks = ceil_div(H, kZoomRows), n_groups = ceil_div(3 * (int64_t)W, kZoomThreads), blocks = n_rblocks * n_groups * n_tiles;
    EMER_REQUIRE(blocks < (1ll << 31), "zoom_tiles: %d tiles of %d x %d are too many for one launch", n_tiles, H, W);
    ZoomArgs A;
    A.H = H, A.W = W, A.h = h_out, A.cams = cams, A.fp64_scale = fp64_scale, A.n_rblocks = (int32_t)n_rblocks;
    A.dmin = dmin, A.dabs = dabs, A.zoom = (double)(H - 1) / (double)(h_out - 1);
    A.z = sqrt(3.0) - 2.0, A.g = (1.0 - A.z) * (1.0 - 1.0 / A.z);
    hipLaunchKernelGGL(zoom_tiles_kernel, dim3((uint32_t)blocks), dim3(kZoomThreads), 0, as_stream(stream), F, A, (int32_t)n_groups, table64, frame_out,
                       values_out);
    return check_launch("zoom_tiles");
}
