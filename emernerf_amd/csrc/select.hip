// Order statistics for gfx950: the k-th smallest value of a large device array by an exact radix select, behind torch.quantile's
// linear rule (the lidar scene box of datasets/base/lidar_source.py:103-138, the flow radius of utils/visualization_tools.py:230-234)
// and the weighted percentile of visualization_tools.py:68-76 (the automatic depth range).  No sort, no size limit below 2^31 rows.
//
//   * keys: fp32 -> uint32 that orders as the values do (positive: sign bit set; negative: all bits inverted), -0 as +0, every NaN
//     as the largest key and an integer atomicOr on its source's flag.
//   * a SLOT is (source, target T): it finds K_hi, the smallest key whose cumulative weight cum(<= key) exceeds T, with cum(< K_hi)
//     and cum(<= K_hi); when no key does, the largest key of the source (found by an integer atomicMax in the first pass).  Weights
//     are integers (1 per row, or rint(clamp(w, 0, 1) * 2^32)), every sum is an integer sum, every atomic an integer atomic: the
//     results do not depend on the arrival order and are the same bits from run to run.
//   * four passes over an 8-bit digit, most significant first, one launch each.  A workgroup takes rows with a grid-stride loop; a
//     lane keeps, per slot, the digit of its last matching row and the weight summed since that digit began, and touches the LDS
//     histogram (256 x uint64 per slot, integer LDS atomics) only when the digit changes -- the rows of a real image share one or two
//     top bytes, and a wave's adds to one LDS address serialise.  Non-zero bins are then added to the slot's global histogram.
//   * the bin choice of pass p is made at the start of pass p + 1: every workgroup reads the slot's earlier histograms (2 KB each)
//     and derives prefix and remaining target on its own, one wave per slot.  The launch boundary is the only synchronisation
//     between workgroups: no tickets, no flags, no cooperative launch.
//   * the weighted percentile's lower neighbour (the largest key below K_hi whatever its weight) is one more pass with an integer
//     atomicMax; a last one-workgroup launch makes the final bin choice and writes the outputs.
//
// Loads: rows of a contiguous [n] or [n][3] array are read four per lane with 16-byte loads (a lane's three quads of an [n][3] array
// are its four rows: one read of the rows serves the jobs of all three columns); any other stride or an unaligned base takes one
// row per lane with scalar loads.  The histograms, hence the results, are the same either way.
#include "common.h"
#include <string.h>
#include <math.h>

// the outputs are stated operation by operation (include/emernerf_hip.h): nothing is contracted except where the code says fmaf
#pragma clang fp contract(off)

namespace emer {

constexpr int kSelThreads = 256;
constexpr int kSelMaxBlocks = 1024;                    // 256 CUs x 4 workgroups (32 KiB of LDS histograms each)
constexpr int kSelSrc = EMER_SELECT_SOURCES_MAX;
constexpr int kSelPer = EMER_SELECT_PER_SOURCE_MAX;
constexpr int kSelSlots = kSelSrc * kSelPer;           // slot = source * kSelPer + j
constexpr int kSelPasses = 4;
constexpr int kSelHdrBytes = 128;                      // nan [4] int32 | max key [4] uint32 | lower neighbour + 1 [16] uint32
constexpr int kSelRowsPerLane = 4;                     // vector path

struct SelArgs {
    const float *src, *weights;
    int64_t n;
    int32_t stride, radius;
    int32_t active, percent;            // bit per slot: in use | the target is param * (total / 100)
    int32_t col[kSelSrc];               // scalar path: the column of source s
    uint64_t target[kSelSlots];         // T, or the bits of the percentile
    uint64_t *hist;                     // [slot][pass][256]
    uint32_t *hdr;
};

struct SelOut { int32_t output, slot_a, slot_b, source; float w; void *out; };
struct SelOuts { SelOut j[EMER_SELECT_JOBS_MAX]; int32_t n_jobs; };

__device__ __forceinline__ uint32_t select_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    uint32_t b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float select_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ __forceinline__ uint64_t select_weight(float w) {
    w = fminf(fmaxf(w, 0.0f), 1.0f);                   // NaN -> 0
    return (uint64_t)rint((double)w * 4294967296.0);
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src, kWave), hi = __shfl((uint32_t)(v >> 32), src, kWave);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_inclusive_sum_u64(uint64_t v, int lane) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)v, off, kWave), hi = __shfl_up((uint32_t)(v >> 32), off, kWave);
        if (lane >= off) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

struct SelState { uint32_t prefix; int32_t found; uint64_t cum_lt, cum_le; double t; };

// One wave: the bin choices of the passes 0 .. n_pass - 1 of one slot, from its global histograms.  Every lane returns the same state.
__device__ SelState select_derive(const SelArgs &A, int slot, int n_pass, int lane) {
    SelState S;
    S.prefix = 0u; S.found = 1; S.cum_lt = 0; S.cum_le = 0; S.t = 0.0;
    uint64_t T = 0;
    for (int q = 0; q < n_pass; ++q) {
        const uint64_t *h = A.hist + ((size_t)slot * kSelPasses + q) * 256 + 4 * lane;
        const uint64_t b0 = h[0], b1 = h[1], b2 = h[2], b3 = h[3];
        const uint64_t s = b0 + b1 + b2 + b3;
        const uint64_t inc = wave_inclusive_sum_u64(s, lane);
        if (q == 0) {
            const uint64_t total = shfl_u64(inc, kWave - 1);
            if ((A.percent >> slot) & 1) {
                S.t = __longlong_as_double((long long)A.target[slot]) * ((double)total / 100.0);
                T = (uint64_t)floor(S.t);
            } else {
                T = A.target[slot];
                S.t = (double)T;
            }
            if (T >= total) { S.found = 0; return S; }
        }
        const uint64_t exc = inc - s;
        const bool mine = exc <= T && T < inc;          // one lane: the cumulative sums are monotonic and T < the pass's total
        int32_t d = 0;
        uint64_t e = exc, bd = 0;
        if (mine) {
            if (T < e + b0) { d = 0; bd = b0; }
            else if (T < e + b0 + b1) { d = 1; e += b0; bd = b1; }
            else if (T < e + b0 + b1 + b2) { d = 2; e += b0 + b1; bd = b2; }
            else { d = 3; e += b0 + b1 + b2; bd = b3; }
            d += 4 * lane;
        }
        const uint64_t owners = __ballot(mine);
        if (owners == 0) { S.found = 0; return S; }     // (cannot happen: a later pass's total is the chosen bin of the one before)
        const int owner = __ffsll((unsigned long long)owners) - 1;
        d = __shfl(d, owner, kWave);
        e = shfl_u64(e, owner);
        bd = shfl_u64(bd, owner);
        S.prefix |= (uint32_t)d << (24 - 8 * q);
        T -= e;
        S.cum_lt += e;
        S.cum_le = S.cum_lt + bd;
    }
    return S;
}

// kPass 0 .. 3: the histogram of digit kPass over the rows that match the prefix chosen so far; 4: the largest key below K_hi.
// kVec: rows of C (1 or 3) floats, four rows per lane with 16-byte loads (source s is column s, or the radius as source 0);
// else C == 0: one row per lane, source s is column col[s] of a row of `stride` floats.
template <int C, bool kVec>
__global__ __launch_bounds__(kSelThreads) void select_pass_kernel(SelArgs A, int32_t pass) {
    __shared__ uint64_t lds_hist[kSelSlots][256];
    __shared__ uint32_t lds_prefix[kSelSlots], lds_on[kSelSlots], lds_lo[kSelSlots], lds_nan[kSelSrc], lds_max[kSelSrc];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int i = tid; i < kSelSlots * 256; i += kSelThreads) (&lds_hist[0][0])[i] = 0;
    if (tid < kSelSlots) { lds_prefix[tid] = 0u; lds_on[tid] = (A.active >> tid) & 1; lds_lo[tid] = 0u; }
    if (tid < kSelSrc) { lds_nan[tid] = 0u; lds_max[tid] = 0u; }
    __syncthreads();
    if (pass > 0) {
        for (int slot = wave; slot < kSelSlots; slot += kSelThreads / kWave) {
            if (!((A.active >> slot) & 1)) continue;
            const SelState S = select_derive(A, slot, pass < kSelPasses ? pass : kSelPasses, lane);
            if (lane == 0) { lds_prefix[slot] = S.prefix; lds_on[slot] = (uint32_t)S.found; }
        }
        __syncthreads();
    }
    const bool pred = pass == kSelPasses;
    const uint32_t mask = pass == 0 ? 0u : (pred ? 0xFFFFFFFFu : 0xFFFFFFFFu << (32 - 8 * pass));
    const int shift = pred ? 0 : 24 - 8 * pass;
    uint32_t prefix[kSelSlots], cur_d[kSelSlots], lo[kSelSlots];
    bool on[kSelSlots], src_on[kSelSrc];
    uint64_t cur_sum[kSelSlots];
#pragma unroll
    for (int s = 0; s < kSelSrc; ++s) src_on[s] = false;
#pragma unroll
    for (int i = 0; i < kSelSlots; ++i) {
        prefix[i] = lds_prefix[i];
        on[i] = lds_on[i] != 0;
        cur_d[i] = 0u; cur_sum[i] = 0; lo[i] = 0u;
        src_on[i / kSelPer] = src_on[i / kSelPer] || on[i];
    }
    uint32_t nan_seen[kSelSrc], max_key[kSelSrc];
#pragma unroll
    for (int s = 0; s < kSelSrc; ++s) { nan_seen[s] = 0u; max_key[s] = 0u; }

    // one value of source s (a compile-time index after unrolling) with weight w
    auto feed = [&](int s, float x, uint64_t w) {
        const uint32_t k = select_key(x);
        if (pass == 0) {
            nan_seen[s] |= (x != x) ? 1u : 0u;
            max_key[s] = k > max_key[s] ? k : max_key[s];
        }
#pragma unroll
        for (int j = 0; j < kSelPer; ++j) {
            const int i = s * kSelPer + j;
            if (!on[i]) continue;
            if (pred) {
                if (k < prefix[i]) lo[i] = k + 1u > lo[i] ? k + 1u : lo[i];
                continue;
            }
            if (((k ^ prefix[i]) & mask) != 0u) continue;
            const uint32_t d = (k >> shift) & 255u;
            if (d != cur_d[i]) {
                if (cur_sum[i] != 0) atomicAdd((unsigned long long *)&lds_hist[i][cur_d[i]], (unsigned long long)cur_sum[i]);
                cur_d[i] = d;
                cur_sum[i] = 0;
            }
            cur_sum[i] += w;
        }
    };
    // one row given as C values (vector path) or by its index (scalar path)
    auto feed_row_scalar = [&](int64_t r) {
        const uint64_t w = A.weights ? select_weight(A.weights[r]) : 1ull;
        const float *row = A.src + r * (int64_t)A.stride;
        if (A.radius) {
            if (src_on[0]) feed(0, hypotf(row[0], row[1]), w);
            return;
        }
#pragma unroll
        for (int s = 0; s < kSelSrc; ++s) {
            if (src_on[s]) feed(s, row[A.col[s]], w);
        }
    };

    if (kVec) {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        constexpr int CC = C > 0 ? C : 1;
        const int64_t groups = A.n / kSelRowsPerLane, step = (int64_t)gridDim.x * kSelThreads;
        for (int64_t g = (int64_t)blockIdx.x * kSelThreads + tid; g < groups; g += step) {
            float v[kSelRowsPerLane * CC];
#pragma unroll
            for (int q = 0; q < CC; ++q) {
                const f32x4 x = *(reinterpret_cast<const f32x4 *>(A.src) + g * CC + q);
                v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
            }
            uint64_t w[kSelRowsPerLane];
            if (A.weights) {
                const f32x4 x = *(reinterpret_cast<const f32x4 *>(A.weights) + g);
                w[0] = select_weight(x.x); w[1] = select_weight(x.y); w[2] = select_weight(x.z); w[3] = select_weight(x.w);
            } else {
                w[0] = w[1] = w[2] = w[3] = 1ull;
            }
#pragma unroll
            for (int r = 0; r < kSelRowsPerLane; ++r) {
                if (A.radius) {
                    if (CC == 3 && src_on[0]) feed(0, hypotf(v[r * CC], v[r * CC + (CC > 1 ? 1 : 0)]), w[r]);
                } else {
#pragma unroll
                    for (int s = 0; s < CC && s < kSelSrc; ++s) {
                        if (src_on[s]) feed(s, v[r * CC + s], w[r]);
                    }
                }
            }
        }
        // the rows past the last full group of four: one each for the first lanes of workgroup 0
        const int64_t tail = groups * kSelRowsPerLane + tid;
        if (blockIdx.x == 0 && tail < A.n) feed_row_scalar(tail);
    } else {
        const int64_t step = (int64_t)gridDim.x * kSelThreads;
        for (int64_t r = (int64_t)blockIdx.x * kSelThreads + tid; r < A.n; r += step) feed_row_scalar(r);
    }

    // the lanes' open runs, then the workgroup's non-zero bins
#pragma unroll
    for (int i = 0; i < kSelSlots; ++i) {
        if (!on[i]) continue;
        if (pred) {
            if (lo[i] != 0u) atomicMax(&lds_lo[i], lo[i]);
        } else if (cur_sum[i] != 0) {
            atomicAdd((unsigned long long *)&lds_hist[i][cur_d[i]], (unsigned long long)cur_sum[i]);
        }
    }
    if (pass == 0) {
#pragma unroll
        for (int s = 0; s < kSelSrc; ++s) {
            if (!src_on[s]) continue;
            if (nan_seen[s]) atomicOr(&lds_nan[s], 1u);
            atomicMax(&lds_max[s], max_key[s]);
        }
    }
    __syncthreads();
    if (pred) {
        if (tid < kSelSlots && lds_lo[tid] != 0u) atomicMax(A.hdr + 2 * kSelSrc + tid, lds_lo[tid]);
        return;
    }
    for (int i = 0; i < kSelSlots; ++i) {
        if (!lds_on[i]) continue;
        const uint64_t v = lds_hist[i][tid];
        if (v != 0) atomicAdd((unsigned long long *)(A.hist + ((size_t)i * kSelPasses + pass) * 256 + tid), (unsigned long long)v);
    }
    if (pass == 0 && tid < kSelSrc) {
        if (lds_nan[tid]) atomicOr(A.hdr + tid, 1u);
        if (lds_max[tid]) atomicMax(A.hdr + kSelSrc + tid, lds_max[tid]);
    }
}

__global__ __launch_bounds__(kSelThreads) void select_finalise_kernel(SelArgs A, SelOuts J) {
    __shared__ SelState st[kSelSlots];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int slot = wave; slot < kSelSlots; slot += kSelThreads / kWave) {
        if (!((A.active >> slot) & 1)) continue;
        const SelState S = select_derive(A, slot, kSelPasses, lane);
        if (lane == 0) st[slot] = S;
    }
    __syncthreads();
    if (tid >= J.n_jobs) return;
    const SelOut &O = J.j[tid];
    const uint32_t top = A.hdr[kSelSrc + O.source];                 // the source's largest key
    const SelState a = st[O.slot_a];
    const uint32_t ka = a.found ? a.prefix : top;
    if (O.output == EMER_SELECT_ORDER) {
        *(float *)O.out = select_value(ka);
    } else if (O.output == EMER_SELECT_QUANTILE) {
        const SelState b = st[O.slot_b];
        const float va = select_value(ka), vb = select_value(b.found ? b.prefix : top);
        const float w = O.w, d = vb - va;
        const float r = w < 0.5f ? fmaf(w, d, va) : fmaf(-d, 1.0f - w, vb);
        *(float *)O.out = A.hdr[O.source] ? __uint_as_float(0x7FC00000u) : r;
    } else {
        const uint32_t below = A.hdr[2 * kSelSrc + O.slot_a];      // the lower neighbour's key + 1, 0 when there is none
        double r = (double)select_value(ka);
        if (a.found && below != 0u) {
            const double lo = (double)select_value(below - 1u), hi = r;
            const double frac = (a.t - (double)a.cum_lt) / (double)(a.cum_le - a.cum_lt);
            r = lo + frac * (hi - lo);
        }
        *(double *)O.out = r;
    }
}

}  // namespace emer

using namespace emer;

extern "C" int64_t emer_select_workspace_bytes(int32_t n_jobs) {
    (void)n_jobs;                                       // every call clears all slots' histograms: one size
    return (int64_t)kSelHdrBytes + (int64_t)kSelSlots * kSelPasses * 256 * (int64_t)sizeof(uint64_t);
}

extern "C" int emer_select(const float *src, int32_t source_kind, int32_t stride, const float *weights, const emer_select_job *jobs,
                           int32_t n_jobs, int64_t n, void *workspace, void *stream) {
    EMER_REQUIRE(src && jobs && workspace, "select: null pointer");
    EMER_REQUIRE(n_jobs >= 1 && n_jobs <= EMER_SELECT_JOBS_MAX, "select: 1..%d jobs, got %d", EMER_SELECT_JOBS_MAX, n_jobs);
    EMER_REQUIRE(n >= 1 && n <= EMER_SELECT_ROWS_MAX, "select: need 1 <= n < 2^31 rows");
    EMER_REQUIRE(source_kind == EMER_SELECT_COLUMNS || source_kind == EMER_SELECT_RADIUS, "select: unknown source kind %d", source_kind);
    EMER_REQUIRE(stride >= 1 && (source_kind != EMER_SELECT_RADIUS || stride == 3), "select: stride >= 1, and 3 for the radius source");
    EMER_REQUIRE(((uintptr_t)workspace & 15) == 0, "select: the workspace must be 16-byte aligned");
    const bool vec = (stride == 1 || stride == 3) && ((uintptr_t)src & 15) == 0 && ((uintptr_t)weights & 15) == 0;
    SelArgs A;
    memset(&A, 0, sizeof(A));
    SelOuts J;
    memset(&J, 0, sizeof(J));
    A.src = src; A.weights = weights; A.n = n; A.stride = stride; A.radius = source_kind == EMER_SELECT_RADIUS;
    A.hdr = reinterpret_cast<uint32_t *>(workspace);
    A.hist = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(workspace) + kSelHdrBytes);
    int32_t n_src = 0, src_col[kSelSrc], per_src[kSelSrc] = {0, 0, 0, 0};
    bool any_pred = false;
    for (int s = 0; s < kSelSrc; ++s) src_col[s] = -1;
    // a slot of source s with this target (shared by the jobs that ask for the same rank or percentile)
    auto slot_of = [&](int s, bool percent, uint64_t target) -> int {
        for (int j = 0; j < per_src[s]; ++j) {
            const int i = s * kSelPer + j;
            if ((((A.percent >> i) & 1) != 0) == percent && A.target[i] == target) return i;
        }
        if (per_src[s] == kSelPer) return -1;
        const int i = s * kSelPer + per_src[s]++;
        A.active |= 1 << i;
        if (percent) A.percent |= 1 << i;
        A.target[i] = target;
        return i;
    };
    for (int32_t q = 0; q < n_jobs; ++q) {
        const emer_select_job &job = jobs[q];
        EMER_REQUIRE(job.out, "select: job %d: null output", q);
        EMER_REQUIRE(job.output >= EMER_SELECT_ORDER && job.output <= EMER_SELECT_WPERCENT, "select: job %d: unknown output %d", q, job.output);
        EMER_REQUIRE((weights == nullptr) || job.output == EMER_SELECT_WPERCENT, "select: job %d: with weights every job is a weighted percentile", q);
        const int32_t col = A.radius ? 0 : job.column;
        EMER_REQUIRE(col >= 0 && col < stride, "select: job %d: column %d of %d", q, col, stride);
        int s = -1;
        if (vec) {              // the vector path reads whole rows: source s is column s
            s = col;
            if (src_col[s] < 0) { src_col[s] = col; ++n_src; }
        } else {
            for (int u = 0; u < n_src; ++u) if (src_col[u] == col) s = u;
            if (s < 0) {
                EMER_REQUIRE(n_src < kSelSrc, "select: more than %d columns in one call", kSelSrc);
                s = n_src++;
                src_col[s] = col;
            }
        }
        SelOut &O = J.j[q];
        O.output = job.output; O.source = s; O.out = job.out; O.w = 0.0f;
        int a = -1, b = -1;
        if (job.output == EMER_SELECT_ORDER) {
            EMER_REQUIRE(job.param >= 0 && job.param < (double)n && job.param == floor(job.param), "select: job %d: rank %g of %lld rows", q, job.param,
                         (long long)n);
            a = b = slot_of(s, false, (uint64_t)job.param);
        } else if (job.output == EMER_SELECT_QUANTILE) {
            EMER_REQUIRE(job.param >= 0 && job.param <= 1, "select: job %d: quantile %g outside [0, 1]", q, job.param);
            const float rank = (float)job.param * (float)(n - 1);          // torch.quantile: fp32 throughout
            const float lo = floorf(rank), hi = ceilf(rank);
            O.w = rank - lo;
            const uint64_t last = (uint64_t)(n - 1);                       // float(n - 1) may round up past n - 1 for n > 2^24
            const uint64_t ra = (uint64_t)lo < last ? (uint64_t)lo : last, rb = (uint64_t)hi < last ? (uint64_t)hi : last;
            a = slot_of(s, false, ra);
            b = a < 0 ? -1 : slot_of(s, false, rb);
        } else {
            EMER_REQUIRE(job.param >= 0 && job.param <= 100, "select: job %d: percentile %g outside [0, 100]", q, job.param);
            uint64_t bits;
            memcpy(&bits, &job.param, sizeof(bits));
            a = b = slot_of(s, true, bits);
            any_pred = true;
        }
        EMER_REQUIRE(a >= 0 && b >= 0, "select: job %d: more than %d ranks or percentiles of one column in one call", q, kSelPer);
        O.slot_a = a; O.slot_b = b;
    }
    J.n_jobs = n_jobs;
    for (int s = 0; s < kSelSrc; ++s) A.col[s] = src_col[s] < 0 ? 0 : src_col[s];
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(workspace, 0, (size_t)emer_select_workspace_bytes(n_jobs), st) != hipSuccess) {
        set_error("select: clearing the workspace failed: %s", hipGetErrorString(hipGetLastError()));
        return EMER_E_LAUNCH;
    }
    const int64_t rows_per_block = (int64_t)kSelThreads * (vec ? kSelRowsPerLane : 1);
    int64_t blocks = ceil_div(n, rows_per_block);
    blocks = blocks < 1 ? 1 : (blocks > kSelMaxBlocks ? kSelMaxBlocks : blocks);
    const dim3 grid((uint32_t)blocks), block(kSelThreads);
    for (int32_t pass = 0; pass < kSelPasses + (any_pred ? 1 : 0); ++pass) {
        if (vec && stride == 1) hipLaunchKernelGGL((select_pass_kernel<1, true>), grid, block, 0, st, A, pass);
        else if (vec) hipLaunchKernelGGL((select_pass_kernel<3, true>), grid, block, 0, st, A, pass);
        else hipLaunchKernelGGL((select_pass_kernel<0, false>), grid, block, 0, st, A, pass);
        const int rc = check_launch("select (pass)");
        if (rc != EMER_OK) return rc;
    }
    hipLaunchKernelGGL(select_finalise_kernel, dim3(1), block, 0, st, A, J);
    return check_launch("select (finalise)");
}
