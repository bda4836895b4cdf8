// Voxel lift of the feature field for gfx950: what the reference's utils/visualization_tools.py:visualize_voxels does per image and
// per query chunk with a dense fp32 grid, an index_put, torch.nonzero and boolean gathers (:546-604, :610-638, :677-678), as
// streaming kernels over a BIT MASK -- one bit per voxel (or per candidate point), bit n in word n / 32 at position n % 32.
//
//   * emer_voxel_mark: ray end points -> voxel bits.  The grids of one image (static and dynamic) are the members of ONE launch.
//     o + d * depth, (p - aabb_min) / voxel_size and the truncation are the reference's fp32 operations in the reference's order,
//     each rounded on its own.  Bits are set with vector atomic ORs: idempotent, so the mask does not depend on the order.
//   * emer_mean_threshold_bits: bit n = mean over K density arrays > threshold (the selector of a query chunk), one ballot per wave.
//   * emer_bits_offsets + emer_bits_emit_voxels / emer_bits_emit_rows: ordered compaction.  A workgroup owns kBitsBlockWords
//     consecutive words; pass 1 counts their set bits, pass 2 (one workgroup) turns the counts into exclusive offsets and the
//     total, pass 3 gives every lane the position of its first set bit by a scan inside the workgroup and writes the rows in
//     ascending bit order.  No atomics, no order that depends on scheduling: the output is the same from run to run.
#include "common.h"
#include <string.h>

// Every product, sum and quotient below is one fp32 operation of the reference: nothing may be contracted.  __fmul_rn / __fadd_rn
// do not pin that: they are plain inline `x * y` / `x + y` of the HIP headers, parsed under the default contraction mode before
// this pragma is seen, and a product and a sum of theirs fuse into one v_fma after inlining.  The helpers below are parsed under
// contract(off).
#pragma clang fp contract(off)

namespace emer {

constexpr int kVoxThreads = 256;
constexpr int kVoxMaxBlocks = 2048;                       // 256 CUs x 8 workgroups
constexpr int kBitsWordsPerLane = 1;               // one coalesced word per lane: a dense mask keeps every CU busy and a lane's emit loop short
constexpr int kBitsBlockWords = kVoxThreads * kBitsWordsPerLane;   // 256 words = 8192 bits per compaction workgroup
static_assert(kBitsBlockWords * 32 == EMER_BITS_BLOCK_BITS, "the header's workspace size follows the compaction tile");

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }      // IEEE division: one rounding

__device__ __forceinline__ int64_t ceil_div_dev(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct MarkJobs { emer_voxel_mark_job j[EMER_VOXEL_JOBS_MAX]; };
struct DensityList { const float *d[EMER_MEAN_ARRAYS_MAX]; };

__global__ __launch_bounds__(kVoxThreads) void voxel_mark_kernel(MarkJobs J, int32_t blocks_per_job, int64_t n_rays) {
    const int32_t job = blockIdx.x / blocks_per_job, blk = blockIdx.x - job * blocks_per_job;
    const emer_voxel_mark_job &A = J.j[job];
    const float *__restrict__ org = A.origins, *__restrict__ dir = A.viewdirs, *__restrict__ depth = A.depth;
    uint32_t *__restrict__ bits = A.bits;
    const float max_depth = A.max_depth;
    const int32_t ry = A.res[1], rz = A.res[2];
    const int64_t step = (int64_t)blocks_per_job * kVoxThreads;
    const int64_t n_iter = ceil_div_dev(n_rays, step);
    int64_t r = (int64_t)blk * kVoxThreads + threadIdx.x;
    for (int64_t it = 0; it < n_iter; ++it, r += step) {
        // no branch around a load: rows past the end read the last ray and mark nothing
        const int64_t rc = r < n_rays ? r : n_rays - 1;
        const float t = depth[rc];
        bool keep = r < n_rays && t < max_depth;        // a NaN depth fails the comparison; max_depth = +inf keeps every finite depth
        int32_t idx[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p = add_rn(org[3 * rc + c], mul_rn(dir[3 * rc + c], t));
            const float v = div_rn(sub_rn(p, A.aabb_min[c]), A.voxel_size[c]);
            // .long() truncates toward zero: (-1, 0) lands in voxel 0.  The test is made on the float, so that a huge value never
            // reaches the conversion; NaN fails both comparisons.
            keep = keep && v > -1.0f && v < (float)A.res[c];
            idx[c] = keep ? (int32_t)v : 0;
        }
        if (keep) {
            const uint32_t n = ((uint32_t)idx[0] * (uint32_t)ry + (uint32_t)idx[1]) * (uint32_t)rz + (uint32_t)idx[2];
            atomicOr(bits + (n >> 5), 1u << (n & 31u));
        }
    }
}

__global__ __launch_bounds__(kVoxThreads) void mean_threshold_bits_kernel(DensityList L, int32_t K, int64_t n, float thr, uint32_t *__restrict__ bits) {
    const int64_t n_words = ceil_div_dev(n, 32);
    const int64_t n_padded = ceil_div_dev(n, kWave) * kWave;      // whole waves: every lane takes part in the ballot
    const int64_t step = (int64_t)gridDim.x * kVoxThreads;
    const float k_f = (float)K;
    for (int64_t i = (int64_t)blockIdx.x * kVoxThreads + threadIdx.x; i < n_padded; i += step) {
        const int64_t ic = i < n ? i : n - 1;
        float s = L.d[0][ic];
        for (int32_t k = 1; k < K; ++k) s = add_rn(s, L.d[k][ic]);    // ((d0 + d1) + d2) + ..., then one division
        const bool on = i < n && div_rn(s, k_f) > thr;
        const uint64_t m = __ballot(on);
        const int32_t lane = threadIdx.x & (kWave - 1);
        const int64_t w = (i - lane) >> 5;                     // first word of this wave's 64 elements
        if (lane == 0) bits[w] = (uint32_t)m;
        if (lane == 32 && w + 1 < n_words) bits[w + 1] = (uint32_t)(m >> 32);
    }
}

// ---- ordered compaction -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t wave_inclusive_sum_i32(int32_t v, int lane) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int32_t o = __shfl_up(v, off, kWave);
        if (lane >= off) v += o;
    }
    return v;
}

// (exclusive prefix of v over the workgroup's threads, the workgroup's total); lds: kVoxThreads / kWave ints
__device__ __forceinline__ int32_t block_exclusive_sum(int32_t v, int32_t *lds, int32_t &total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int32_t incl = wave_inclusive_sum_i32(v, lane);
    if (lane == kWave - 1) lds[wave] = incl;
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kVoxThreads / kWave; ++w) {
        const int32_t s = lds[w];
        before += w < wave ? s : 0;
        all += s;
    }
    __syncthreads();        // lds may be reused by the caller's next scan
    total = all;
    return before + incl - v;
}

// this lane's kBitsWordsPerLane consecutive words of workgroup `blk`; words past the mask read as 0, bits past n_bits are cut off
__device__ __forceinline__ void load_lane_words(const uint32_t *__restrict__ bits, int64_t n_bits, int64_t blk, uint32_t (&w)[kBitsWordsPerLane]) {
    const int64_t n_words = ceil_div_dev(n_bits, 32);
    const int64_t w0 = blk * kBitsBlockWords + (int64_t)threadIdx.x * kBitsWordsPerLane;
    const uint32_t tail = (uint32_t)(n_bits & 31);
#pragma unroll
    for (int k = 0; k < kBitsWordsPerLane; ++k) {
        const int64_t i = w0 + k;
        const uint32_t x = bits[i < n_words ? i : n_words - 1];
        uint32_t m = i < n_words ? 0xffffffffu : 0u;
        if (i == n_words - 1 && tail != 0) m = (1u << tail) - 1u;
        w[k] = x & m;
    }
}

__global__ __launch_bounds__(kVoxThreads) void bits_count_kernel(const uint32_t *__restrict__ bits, int64_t n_bits, int64_t *__restrict__ offsets) {
    __shared__ int32_t lds[kVoxThreads / kWave];
    uint32_t w[kBitsWordsPerLane];
    load_lane_words(bits, n_bits, blockIdx.x, w);
    int32_t c = 0;
#pragma unroll
    for (int k = 0; k < kBitsWordsPerLane; ++k) c += __popc(w[k]);
    int32_t total;
    block_exclusive_sum(c, lds, total);
    if (threadIdx.x == 0) offsets[blockIdx.x] = total;
}

// counts [n_blocks] -> exclusive offsets in place, offsets[n_blocks] = the total.  One workgroup, a fixed order.
__global__ __launch_bounds__(kVoxThreads) void bits_scan_kernel(int64_t *__restrict__ offsets, int64_t n_blocks) {
    __shared__ int32_t lds[kVoxThreads / kWave];
    int64_t carry = 0;
    for (int64_t base = 0; base < n_blocks; base += kVoxThreads) {
        const int64_t i = base + threadIdx.x;
        const int32_t c = (int32_t)offsets[i < n_blocks ? i : n_blocks - 1];      // a count is at most 8192
        int32_t total;
        const int32_t excl = block_exclusive_sum(i < n_blocks ? c : 0, lds, total);
        if (i < n_blocks) offsets[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) offsets[n_blocks] = carry;
}

// kVoxel: bit n -> (ix, iy, iz) of the row-major grid -> the voxel's world corner (and the indices); else: bit n -> row n of src
template <bool kVoxel>
__global__ __launch_bounds__(kVoxThreads) void bits_emit_kernel(const uint32_t *__restrict__ bits, int64_t n_bits, const int64_t *__restrict__ offsets,
                                                               int32_t ry, int32_t rz, float min_x, float min_y, float min_z, float vs_x, float vs_y,
                                                               float vs_z, float *__restrict__ coords, int32_t *__restrict__ indices,
                                                               const float *__restrict__ src, int32_t n_cols, float *__restrict__ out) {
    __shared__ int32_t lds[kVoxThreads / kWave];
    const int64_t first = offsets[blockIdx.x];
    if (offsets[blockIdx.x + 1] == first) return;      // nothing set in this workgroup's words (the same for every lane)
    uint32_t w[kBitsWordsPerLane];
    load_lane_words(bits, n_bits, blockIdx.x, w);
    int32_t c = 0;
#pragma unroll
    for (int k = 0; k < kBitsWordsPerLane; ++k) c += __popc(w[k]);
    int32_t total;
    int64_t m = first + block_exclusive_sum(c, lds, total);
    const int64_t bit0 = ((int64_t)blockIdx.x * kBitsBlockWords + (int64_t)threadIdx.x * kBitsWordsPerLane) * 32;
#pragma unroll
    for (int k = 0; k < kBitsWordsPerLane; ++k) {
        uint32_t x = w[k];
        while (x != 0) {
            const int64_t n = bit0 + 32 * k + (__ffs((int)x) - 1);
            x &= x - 1;
            if (kVoxel) {
                const uint32_t u = (uint32_t)n, xy = u / (uint32_t)rz;
                const int32_t iz = (int32_t)(u - xy * (uint32_t)rz), ix = (int32_t)(xy / (uint32_t)ry), iy = (int32_t)(xy - (uint32_t)ix * (uint32_t)ry);
                // voxel_coords_to_world_coords: aabb_min + float(i) * voxel_size, a product then a sum
                coords[3 * m] = add_rn(min_x, mul_rn((float)ix, vs_x));
                coords[3 * m + 1] = add_rn(min_y, mul_rn((float)iy, vs_y));
                coords[3 * m + 2] = add_rn(min_z, mul_rn((float)iz, vs_z));
                if (indices != nullptr) {
                    indices[3 * m] = ix;
                    indices[3 * m + 1] = iy;
                    indices[3 * m + 2] = iz;
                }
            } else {
                for (int32_t col = 0; col < n_cols; ++col) out[m * n_cols + col] = src[n * n_cols + col];
            }
            ++m;
        }
    }
}

static int64_t bits_blocks(int64_t n_bits) { return ceil_div(n_bits, (int64_t)EMER_BITS_BLOCK_BITS); }

}  // namespace emer

using namespace emer;

extern "C" int emer_voxel_mark(const emer_voxel_mark_job *jobs, int32_t n_jobs, int64_t n_rays, void *stream) {
    EMER_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= EMER_VOXEL_JOBS_MAX, "voxel_mark: 1..%d jobs", EMER_VOXEL_JOBS_MAX);
    EMER_REQUIRE(n_rays >= 0 && n_rays < (1ll << 40), "voxel_mark: bad ray count");
    MarkJobs J;
    memset(&J, 0, sizeof(J));
    for (int32_t i = 0; i < n_jobs; ++i) {
        const emer_voxel_mark_job &q = jobs[i];
        EMER_REQUIRE(q.bits && (n_rays == 0 || (q.origins && q.viewdirs && q.depth)), "voxel_mark: job %d: null pointer", i);
        EMER_REQUIRE(q.max_depth == q.max_depth, "voxel_mark: job %d: max_depth is NaN", i);
        int64_t voxels = 1;
        for (int c = 0; c < 3; ++c) {
            EMER_REQUIRE(q.res[c] >= 1 && q.res[c] < (1 << 24), "voxel_mark: job %d: resolution %d outside 1 .. 2^24 - 1", i, q.res[c]);
            EMER_REQUIRE(q.voxel_size[c] > 0.0f && q.voxel_size[c] <= 3.0e38f && q.aabb_min[c] - q.aabb_min[c] == 0.0f,
                         "voxel_mark: job %d: need a finite aabb_min and a finite voxel_size > 0", i);
            voxels *= q.res[c];
            EMER_REQUIRE(voxels <= EMER_VOXELS_MAX, "voxel_mark: job %d: more than 2^31 - 1 voxels", i);
        }
        J.j[i] = q;
    }
    if (n_rays == 0) return EMER_OK;
    int64_t b = ceil_div(n_rays, kVoxThreads);
    const int64_t cap = kVoxMaxBlocks / n_jobs;
    const int32_t bpj = (int32_t)(b > cap ? cap : b);
    hipLaunchKernelGGL(voxel_mark_kernel, dim3((uint32_t)(bpj * n_jobs)), dim3(kVoxThreads), 0, as_stream(stream), J, bpj, n_rays);
    return check_launch("voxel_mark");
}

extern "C" int emer_mean_threshold_bits(const float *const *densities, int32_t n_arrays, int64_t n, float threshold, uint32_t *bits, void *stream) {
    EMER_REQUIRE(densities && n_arrays >= 1 && n_arrays <= EMER_MEAN_ARRAYS_MAX, "mean_threshold_bits: 1..%d arrays", EMER_MEAN_ARRAYS_MAX);
    EMER_REQUIRE(n >= 0 && n < (1ll << 40), "mean_threshold_bits: bad element count");
    EMER_REQUIRE(threshold == threshold, "mean_threshold_bits: the threshold is NaN");
    if (n == 0) return EMER_OK;
    EMER_REQUIRE(bits, "mean_threshold_bits: no output");
    DensityList L;
    memset(&L, 0, sizeof(L));
    for (int32_t k = 0; k < n_arrays; ++k) {
        EMER_REQUIRE(densities[k], "mean_threshold_bits: array %d: null pointer", k);
        L.d[k] = densities[k];
    }
    int64_t b = ceil_div(n, kVoxThreads);
    if (b > kVoxMaxBlocks) b = kVoxMaxBlocks;
    hipLaunchKernelGGL(mean_threshold_bits_kernel, dim3((uint32_t)b), dim3(kVoxThreads), 0, as_stream(stream), L, n_arrays, n, threshold, bits);
    return check_launch("mean_threshold_bits");
}

extern "C" int64_t emer_bits_offsets_size(int64_t n_bits) { return n_bits < 0 ? 0 : bits_blocks(n_bits) + 1; }

extern "C" int emer_bits_offsets(const uint32_t *bits, int64_t n_bits, int64_t *offsets, void *stream) {
    EMER_REQUIRE(n_bits >= 1 && n_bits < (1ll << 40) && bits && offsets, "bits_offsets: need a mask of 1 .. 2^40 - 1 bits and the offsets");
    const int64_t blocks = bits_blocks(n_bits);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(bits_count_kernel, dim3((uint32_t)blocks), dim3(kVoxThreads), 0, st, bits, n_bits, offsets);
    int rc = check_launch("bits_offsets (count)");
    if (rc != EMER_OK) return rc;
    hipLaunchKernelGGL(bits_scan_kernel, dim3(1), dim3(kVoxThreads), 0, st, offsets, blocks);
    return check_launch("bits_offsets (scan)");
}

extern "C" int emer_bits_emit_voxels(const uint32_t *bits, const int64_t *offsets, int64_t total, const int32_t *res, const float *aabb_min,
                                     const float *voxel_size, float *coords, int32_t *indices, void *stream) {
    EMER_REQUIRE(bits && offsets && res && aabb_min && voxel_size, "bits_emit_voxels: null pointer");
    int64_t n_bits = 1;
    for (int c = 0; c < 3; ++c) {
        EMER_REQUIRE(res[c] >= 1 && res[c] < (1 << 24), "bits_emit_voxels: resolution %d outside 1 .. 2^24 - 1", res[c]);
        n_bits *= res[c];
        EMER_REQUIRE(n_bits <= EMER_VOXELS_MAX, "bits_emit_voxels: more than 2^31 - 1 voxels");
    }
    EMER_REQUIRE(total >= 0 && total <= n_bits, "bits_emit_voxels: the total is not a count of this mask");
    if (total == 0) return EMER_OK;      // no emit pass
    EMER_REQUIRE(coords, "bits_emit_voxels: no output");
    hipLaunchKernelGGL(bits_emit_kernel<true>, dim3((uint32_t)bits_blocks(n_bits)), dim3(kVoxThreads), 0, as_stream(stream), bits, n_bits, offsets,
                       res[1], res[2], aabb_min[0], aabb_min[1], aabb_min[2], voxel_size[0], voxel_size[1], voxel_size[2], coords, indices,
                       (const float *)nullptr, 0, (float *)nullptr);
    return check_launch("bits_emit_voxels");
}

extern "C" int emer_bits_emit_rows(const uint32_t *bits, int64_t n_bits, const int64_t *offsets, int64_t total, const float *src, int32_t n_cols,
                                   float *out, void *stream) {
    EMER_REQUIRE(bits && offsets && n_bits >= 1 && n_bits < (1ll << 40), "bits_emit_rows: need a mask of 1 .. 2^40 - 1 bits and its offsets");
    EMER_REQUIRE(n_cols >= 1 && n_cols <= EMER_BITS_ROW_COLS_MAX, "bits_emit_rows: 1..%d columns", EMER_BITS_ROW_COLS_MAX);
    EMER_REQUIRE(total >= 0 && total <= n_bits, "bits_emit_rows: the total is not a count of this mask");
    if (total == 0) return EMER_OK;      // no emit pass
    EMER_REQUIRE(src && out, "bits_emit_rows: null pointer");
    hipLaunchKernelGGL(bits_emit_kernel<false>, dim3((uint32_t)bits_blocks(n_bits)), dim3(kVoxThreads), 0, as_stream(stream), bits, n_bits, offsets, 1, 1,
                       0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, (float *)nullptr, (int32_t *)nullptr, src, n_cols, out);
    return check_launch("bits_emit_rows");
}
