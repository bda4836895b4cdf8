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

// the packed table row of one depth pixel (row kTurboRows is black)
__device__ __forceinline__ uint32_t depth8(float x, float opacity, double dmin, double dabs, const uint32_t *__restrict__ lut) {
    const float t = -logf(__fadd_rn(x, 1e-6f));
    double v = __ddiv_rn(__dsub_rn((double)t, dmin), dabs);
    v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    v = v != v ? 0.0 : v;                                   // nan_to_num after the clip
    const double p = __dmul_rn(v, (double)opacity);
    int32_t row = p >= 1.0 ? kTurboRows - 1 : (p < 0.0 ? 0 : (int32_t)(p * 256.0));   // 256 p is exact
    row = p != p ? kTurboRows : row;
    return lut[row];
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
