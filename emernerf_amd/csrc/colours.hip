// Evaluation colours for gfx950: what the reference's eval loop computes per image with torch / numpy chains on E-wide feature
// images and flows (radiance_fields/video_utils.py:233-418, utils/visualization_tools.py:204-275), as three kernels whose
// members (several projections / blends / flow directions of one image) share ONE launch each.
//
//   * emer_feature_colours: out = clamp((feat @ M - lo) / (hi - lo), 0, 1) [* scale].  Bandwidth-bound (256 B per row at E = 64,
//     3 KB at E = 768 against 12 B written): a row is read by a GROUP of G lanes, G = the power of two >= ceil(E / 4) capped at
//     the wave, lane l of the group taking the 16-byte quads l, l + G, l + 2G, ... of the row, so a wave reads 64 consecutive
//     quads per load.  Every feature element is read once, with non-temporal 16-byte loads (a 640 x 960 x 768 image is 1.9 GB:
//     nothing of it is worth a cache line).  M, lo and hi are staged once per workgroup: M in LDS, and for E up to 3 quads per
//     lane (E <= 768) a lane's slice of M also in registers; there a lane works on 4 (E <= 256) or 2 rows at once, all their
//     loads issued back to back without a branch (a guarded load gets a full memory wait of its own) and one tile ahead of the
//     reduction.  The E-sum has a FIXED order that E alone decides: a lane accumulates its elements in ascending order with
//     fmaf, then the group's lanes combine in an xor butterfly.  The scalar path (E % 4 != 0 or an unaligned base) gives each
//     lane the same elements in the same order: same bits.
//   * emer_blend_over: clip(a o + b (1 - o), 0, 1) with every operation rounded on its own, as numpy evaluates it.
//   * emer_flow_colours: scene_flow_to_rgb for a fixed max radius; the 56 x 3 wheel comes from the host and is staged in LDS.
//
// No atomics, no inter-workgroup traffic: a row's result does not depend on the row count, the members or the grid.
#include "common.h"
#include <string.h>

// the reference rounds every product and sum on its own (torch / numpy elementwise chains): nothing here may be contracted
// into an fma except where the code says fmaf
#pragma clang fp contract(off)

namespace emer {

constexpr int kColThreads = 256;
constexpr int kColMaxBlocks = 2048;      // 256 CUs x 8 workgroups
constexpr int kColMaxFeat = 4080;        // M, lo and hi - lo stay below 48 KiB of LDS
constexpr int kColRegQuads = 3;          // quads of a row per lane held against a register copy of M (E <= 4 * 64 * 3 = 768)
static_assert(kColRegQuads == 3, "emer_feature_colours launches the instantiations 1, 2, 3 and 0");

struct FeatJobs { emer_feature_colour_job j[EMER_COLOUR_JOBS_MAX]; };
struct BlendJobs { emer_blend_over_job j[EMER_COLOUR_JOBS_MAX]; };
struct FlowJobs { emer_flow_colour_job j[EMER_COLOUR_JOBS_MAX]; };

// torch.clamp / np.clip: +-inf clamp, NaN stays NaN (both comparisons are false for it)
__device__ __forceinline__ float clamp01_nan(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

__device__ __forceinline__ int64_t ceil_div_dev(int64_t a, int64_t b) { return (a + b - 1) / b; }

// rows of a tile that a lane works on at once (all their loads are issued before the first use, one tile ahead): E alone decides
__host__ __device__ constexpr int rows_in_flight(int reg_quads) { return reg_quads == 0 ? 1 : (reg_quads == 1 ? 4 : 2); }

// One quad of a row: 16-byte load, or the same elements one by one (the tail of a row whose width is no multiple of 4 reads as 0).
// No branch around a load: a guarded load gets a full memory wait of its own and the loads of a tile would run one after another;
// addresses are clamped into the row instead and what lies outside is replaced by zero afterwards.
template <bool kVec>
__device__ __forceinline__ float4 load_quad(const float *__restrict__ row, int32_t q, int32_t E) {
    if (kVec) {   // read once: streamed past the caches
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        const f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(row) + q);
        return make_float4(x.x, x.y, x.z, x.w);
    }
    const int32_t e = 4 * q, last = E - 1;
    float4 v = make_float4(row[e], row[min(e + 1, last)], row[min(e + 2, last)], row[min(e + 3, last)]);
    v.y = e + 1 < E ? v.y : 0.0f;
    v.z = e + 2 < E ? v.z : 0.0f;
    v.w = e + 3 < E ? v.w : 0.0f;
    return v;
}

// The rows blk, blk + step, ... (in tiles) of one job.  A row's three sums: lane `lig` of the row's group adds the elements of
// the quads lig, lig + G, ... in ascending order with fmaf (kReg > 0: against its register copy of M, with exact zeros where the
// row or M has no element; kReg == 0: against M in LDS), then the group's lanes combine in an xor butterfly.
template <int kReg, bool kVec>
__device__ __forceinline__ void feature_colour_rows(const emer_feature_colour_job &A, int64_t n_rows, int32_t E, int32_t G, int32_t K,
                                                    int64_t first_tile, int64_t tile_step, const float *__restrict__ m_lds,
                                                    const float *__restrict__ lo_hi) {
    constexpr int KR = kReg > 0 ? kReg : 1, R = rows_in_flight(kReg);
    const int32_t n_quads = (E + 3) / 4;
    const int32_t lig = threadIdx.x & (G - 1);           // lane in its group (G is a power of two <= 64: groups never straddle a wave)
    const int32_t rows_per_block = kColThreads / G;
    const int32_t row_in_block = threadIdx.x / G;
    float m_reg[KR][12];
    if (kReg > 0) {
#pragma unroll
        for (int k = 0; k < kReg; ++k) {
            const int32_t e = 4 * (lig + k * G);
#pragma unroll
            for (int t = 0; t < 12; ++t) m_reg[k][t] = (e + t / 3) < E ? m_lds[3 * e + t] : 0.0f;
        }
    }
    const float *__restrict__ feat = A.feat;
    const float *__restrict__ scale = A.scale;
    float *__restrict__ out = A.out;
    const int64_t rows_per_tile = (int64_t)rows_per_block * R;
    const int64_t n_tiles = ceil_div_dev(n_rows, rows_per_tile);
    // kReg > 0: the quads of tile `t` for this lane -- every load back to back, rows past the end clamped to the last row (their
    // values are never stored); the loop below keeps the NEXT tile's loads in flight while it reduces the current one
    float4 v[R][KR];
    auto load_tile = [&](int64_t t, float4 (&dst)[R][KR]) {
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int64_t r = t * rows_per_tile + row_in_block + (int64_t)u * rows_per_block;
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                const int32_t q = lig + k * G;
                const bool keep = q < n_quads;
                const float4 x = load_quad<kVec>(feat + (r < n_rows ? r : n_rows - 1) * (int64_t)E, keep ? q : n_quads - 1, E);
                dst[u][k] = make_float4(keep ? x.x : 0.0f, keep ? x.y : 0.0f, keep ? x.z : 0.0f, keep ? x.w : 0.0f);
            }
        }
    };
    if (kReg > 0 && first_tile < n_tiles) load_tile(first_tile, v);
    for (int64_t tile = first_tile; tile < n_tiles; tile += tile_step) {
        const int64_t r0 = tile * rows_per_tile + row_in_block;      // this lane's rows: r0, r0 + rows_per_block, ...
        float acc[R][3];
        if (kReg > 0) {
            float4 w[R][KR];
            load_tile(tile + tile_step, w);     // (past the last tile: clamped, unused)
#pragma unroll
            for (int u = 0; u < R; ++u) {
                acc[u][0] = acc[u][1] = acc[u][2] = 0.0f;
#pragma unroll
                for (int k = 0; k < kReg; ++k) {
                    const float f[4] = {v[u][k].x, v[u][k].y, v[u][k].z, v[u][k].w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[u][c] = fmaf(f[t], m_reg[k][3 * t + c], acc[u][c]);
                    }
                }
#pragma unroll
                for (int k = 0; k < kReg; ++k) v[u][k] = w[u][k];
            }
        } else {
            acc[0][0] = acc[0][1] = acc[0][2] = 0.0f;
            if (r0 < n_rows) {
                const float *__restrict__ row = feat + r0 * (int64_t)E;
                for (int32_t k = 0; k < K; ++k) {
                    const int32_t q = lig + k * G;
                    if (q >= n_quads) break;
                    const float4 x = load_quad<kVec>(row, q, E);
                    const float f[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if (kVec || 4 * q + t < E) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) acc[0][c] = fmaf(f[t], m_lds[3 * (4 * q + t) + c], acc[0][c]);
                        }
                    }
                }
            }
        }
        for (int32_t off = G >> 1; off > 0; off >>= 1) {   // every lane of the wave takes part; the order depends on G alone
#pragma unroll
            for (int u = 0; u < R; ++u) {
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[u][c] += __shfl_xor(acc[u][c], off, kWave);
            }
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int64_t r = r0 + (int64_t)u * rows_per_block;
            if (r >= n_rows) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {   // channel c is finished by lane c of the group where it has three lanes, by lane 0 otherwise
                if (lig != (G >= 4 ? c : 0)) continue;
                const float lo = lo_hi[c], d = lo_hi[3 + c];
                float x = clamp01_nan(__fdiv_rn(__fsub_rn(acc[u][c], lo), d));
                if (scale != nullptr) x = __fmul_rn(x, scale[r]);
                out[3 * r + c] = x;
            }
        }
    }
}

// kReg: the quads of a row per lane (1 .. kColRegQuads) when the lane's slice of M lives in registers, 0 for any wider row.  Which
// copy of M the lanes read is a matter of speed only: E picks the instantiation, so a row's bits do not depend on anything else.
template <int kReg>
__global__ __launch_bounds__(kColThreads) void feature_colours_kernel(FeatJobs J, int32_t blocks_per_job, int64_t n_rows, int32_t E,
                                                                     int32_t G, int32_t K, int32_t vec_mask) {
    extern __shared__ __attribute__((aligned(16))) float col_lds[];   // M [E][3] | lo [3] | hi - lo [3]
    const int32_t job = blockIdx.x / blocks_per_job, blk = blockIdx.x - job * blocks_per_job;
    const emer_feature_colour_job &A = J.j[job];
    float *m_lds = col_lds, *lo_hi = col_lds + 3 * E;
    for (int32_t i = threadIdx.x; i < 3 * E; i += kColThreads) m_lds[i] = A.mat[i];
    if (threadIdx.x < 3) {
        const float lo = A.lo[threadIdx.x];
        lo_hi[threadIdx.x] = lo;
        lo_hi[3 + threadIdx.x] = __fsub_rn(A.hi[threadIdx.x], lo);
    }
    __syncthreads();
    if ((vec_mask >> job) & 1) feature_colour_rows<kReg, true>(A, n_rows, E, G, K, blk, blocks_per_job, m_lds, lo_hi);
    else feature_colour_rows<kReg, false>(A, n_rows, E, G, K, blk, blocks_per_job, m_lds, lo_hi);
}

__global__ __launch_bounds__(kColThreads) void blend_over_kernel(BlendJobs J, int32_t blocks_per_job, int64_t n_rows) {
    const int32_t job = blockIdx.x / blocks_per_job, blk = blockIdx.x - job * blocks_per_job;
    const emer_blend_over_job &A = J.j[job];
    const float *__restrict__ a = A.a, *__restrict__ o = A.o, *__restrict__ b = A.b;
    float *__restrict__ out = A.out;
    const int64_t total = 3 * n_rows, step = (int64_t)blocks_per_job * kColThreads;
    for (int64_t i = (int64_t)blk * kColThreads + threadIdx.x; i < total; i += step) {
        const float w = o[i / 3];
        const float y = __fadd_rn(__fmul_rn(a[i], w), __fmul_rn(b[i], __fsub_rn(1.0f, w)));
        out[i] = clamp01_nan(y);
    }
}

__global__ __launch_bounds__(kColThreads) void flow_colours_kernel(FlowJobs J, int32_t blocks_per_job, int64_t n_rows,
                                                                  const float *__restrict__ wheel, float max_radius, int32_t dark) {
    __shared__ float w_lds[EMER_WHEEL_ROWS * 3];
    for (int32_t i = threadIdx.x; i < EMER_WHEEL_ROWS * 3; i += kColThreads) w_lds[i] = wheel[i];
    __syncthreads();
    const int32_t job = blockIdx.x / blocks_per_job, blk = blockIdx.x - job * blocks_per_job;
    const float *__restrict__ flow = J.j[job].flow;
    float *__restrict__ out = J.j[job].out;
    const float two_pi = (float)(2.0 * 3.14159265358979323846);
    const float to_index = (float)((EMER_WHEEL_ROWS - 2) / (2.0 * 3.14159265358979323846));   // (N_COLS - 1) / 2 pi, N_COLS = 55
    const int64_t step = (int64_t)blocks_per_job * kColThreads;
    for (int64_t r = (int64_t)blk * kColThreads + threadIdx.x; r < n_rows; r += step) {
        const float x = flow[3 * r], y = flow[3 * r + 1];
        float radius = hypotf(x, y), angle = atan2f(y, x);
        if (max_radius > 0.0f) radius = __fdiv_rn(radius, max_radius);
        if (angle < 0.0f) angle = __fadd_rn(angle, two_pi);
        angle = __fmul_rn(angle, to_index);
        const float frac = fmodf(angle, 1.0f), one_m = __fsub_rn(1.0f, frac);
        // the indices stay inside the wheel whatever the flow holds (NaN and inf included)
        const int32_t i0 = (int32_t)fminf(fmaxf(truncf(angle), 0.0f), (float)(EMER_WHEEL_ROWS - 1));
        const int32_t i1 = (int32_t)fminf(fmaxf(ceilf(angle), 0.0f), (float)(EMER_WHEEL_ROWS - 1));
        const bool oversized = radius > 1.0f;
        const float factor = oversized ? __fdiv_rn(1.0f, radius) : radius;
        const bool s_axis = (dark != 0) == oversized;   // bright: S axis inside the radius, V axis beyond it; dark: the other way round
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float hue = __fadd_rn(__fmul_rn(w_lds[3 * i0 + c], one_m), __fmul_rn(w_lds[3 * i1 + c], frac));
            const float col = s_axis ? __fsub_rn(255.0f, __fmul_rn(factor, __fsub_rn(255.0f, hue))) : __fmul_rn(hue, factor);
            out[3 * r + c] = __fdiv_rn(col, 255.0f);
        }
    }
}

static int32_t colour_blocks(int64_t items, int32_t n_jobs) {
    int64_t b = ceil_div(items, kColThreads);
    const int64_t cap = kColMaxBlocks / n_jobs;
    return (int32_t)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace emer

using namespace emer;

extern "C" int emer_feature_colours(const emer_feature_colour_job *jobs, int32_t n_jobs, int64_t n_rows, int32_t n_feat, void *stream) {
    EMER_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= EMER_COLOUR_JOBS_MAX, "feature_colours: 1..%d jobs", EMER_COLOUR_JOBS_MAX);
    EMER_REQUIRE(n_rows >= 0 && n_rows < (1ll << 40) && n_feat >= 1 && n_feat <= kColMaxFeat, "feature_colours: need n_rows >= 0 and 1 <= n_feat <= %d",
                 kColMaxFeat);
    if (n_rows == 0) return EMER_OK;
    FeatJobs J;
    memset(&J, 0, sizeof(J));
    int32_t vec_mask = 0;
    for (int32_t i = 0; i < n_jobs; ++i) {
        const emer_feature_colour_job &q = jobs[i];
        EMER_REQUIRE(q.feat && q.mat && q.lo && q.hi && q.out, "feature_colours: job %d: null pointer", i);
        J.j[i] = q;
        if (n_feat % 4 == 0 && ((uintptr_t)q.feat & 15) == 0) vec_mask |= 1 << i;
    }
    // the group: the power of two >= the row's quads, at most a wave; K quads per lane
    const int32_t n_quads = (n_feat + 3) / 4;
    int32_t G = 1;
    while (G < n_quads && G < kWave) G <<= 1;
    const int32_t K = (int32_t)ceil_div(n_quads, G);
    // one workgroup per tile of 256 / G rows x rows_in_flight; a narrow M (cheap to stage) allows more workgroups, which evens out the tail
    const int64_t rows_per_tile = (int64_t)(kColThreads / G) * rows_in_flight(K <= kColRegQuads ? K : 0);
    const int64_t cap = (n_feat <= 128 ? 8 * kColMaxBlocks : kColMaxBlocks) / n_jobs, tiles = ceil_div(n_rows, rows_per_tile);
    const int32_t bpj = (int32_t)(tiles < cap ? tiles : cap);
    const size_t lds = (size_t)(3 * n_feat + 8) * sizeof(float);
    const dim3 grid((uint32_t)(bpj * n_jobs)), block(kColThreads);
    hipStream_t st = as_stream(stream);
#define EMER_COLOUR_LAUNCH(kReg) hipLaunchKernelGGL(feature_colours_kernel<kReg>, grid, block, lds, st, J, bpj, n_rows, n_feat, G, K, vec_mask)
    if (K == 1) EMER_COLOUR_LAUNCH(1);
    else if (K == 2) EMER_COLOUR_LAUNCH(2);
    else if (K == 3) EMER_COLOUR_LAUNCH(3);
    else EMER_COLOUR_LAUNCH(0);
#undef EMER_COLOUR_LAUNCH
    return check_launch("feature_colours");
}

extern "C" int emer_blend_over(const emer_blend_over_job *jobs, int32_t n_jobs, int64_t n_rows, void *stream) {
    EMER_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= EMER_COLOUR_JOBS_MAX, "blend_over: 1..%d jobs", EMER_COLOUR_JOBS_MAX);
    EMER_REQUIRE(n_rows >= 0 && n_rows < (1ll << 40), "blend_over: bad row count");
    if (n_rows == 0) return EMER_OK;
    BlendJobs J;
    memset(&J, 0, sizeof(J));
    for (int32_t i = 0; i < n_jobs; ++i) {
        EMER_REQUIRE(jobs[i].a && jobs[i].o && jobs[i].b && jobs[i].out, "blend_over: job %d: null pointer", i);
        J.j[i] = jobs[i];
    }
    const int32_t bpj = colour_blocks(3 * n_rows, n_jobs);
    hipLaunchKernelGGL(blend_over_kernel, dim3((uint32_t)(bpj * n_jobs)), dim3(kColThreads), 0, as_stream(stream), J, bpj, n_rows);
    return check_launch("blend_over");
}

extern "C" int emer_flow_colours(const emer_flow_colour_job *jobs, int32_t n_jobs, int64_t n_rows, const float *wheel, float max_radius,
                                 int32_t dark_background, void *stream) {
    EMER_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= EMER_COLOUR_JOBS_MAX, "flow_colours: 1..%d jobs", EMER_COLOUR_JOBS_MAX);
    EMER_REQUIRE(n_rows >= 0 && n_rows < (1ll << 40) && wheel, "flow_colours: bad row count or no wheel");
    EMER_REQUIRE(max_radius == max_radius, "flow_colours: max_radius is NaN");
    if (n_rows == 0) return EMER_OK;
    FlowJobs J;
    memset(&J, 0, sizeof(J));
    for (int32_t i = 0; i < n_jobs; ++i) {
        EMER_REQUIRE(jobs[i].flow && jobs[i].out, "flow_colours: job %d: null pointer", i);
        J.j[i] = jobs[i];
    }
    const int32_t bpj = colour_blocks(n_rows, n_jobs);
    hipLaunchKernelGGL(flow_colours_kernel, dim3((uint32_t)(bpj * n_jobs)), dim3(kColThreads), 0, as_stream(stream), J, bpj, n_rows, wheel,
                       max_radius, dark_background);
    return check_launch("flow_colours");
}
