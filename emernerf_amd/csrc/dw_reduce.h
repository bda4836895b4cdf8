// Sum of the per-workgroup partials of the weight-gradient kernels: the one copy of the reduction's body, its argument block and
// its grid rule.  csrc/mlp.hip launches it on its own (linear_dw_reduce_multi_kernel); csrc/rayinputs.hip runs it as one job of a
// multi-job launch (emer_ray_jobs).
//
// dw[i] += sum_b partials[b][off + i]  (i < n*k),  dbias[i - n*k] += ...  (i >= n*k), for up to EMER_DW_MAX_JOBS (dW | dbias) pairs of
// ONE partial buffer.  The partial blocks are cut into `ny` ranges so that the (small) n*k + n extent still fills the chip; each
// thread sums its range with four independent accumulators (loads in flight) and merges with one f32 atomic.
#pragma once
#include "common.h"

namespace emer {

struct DwDst {  // where column k of the (virtually concatenated) operand lands in dw: dw[n * ld + dst + (k - col)]
    int32_t col[EMER_CHAIN_MAX_SEGS], width[EMER_CHAIN_MAX_SEGS], dst[EMER_CHAIN_MAX_SEGS];
    int32_t n, K;
    int64_t ld;
};
struct DwJobs {
    int32_t n_jobs;
    int64_t off[EMER_DW_MAX_JOBS], nk[EMER_DW_MAX_JOBS], extent[EMER_DW_MAX_JOBS];   // start inside a partial, floats of dW, floats of dW + dbias
    float *dw[EMER_DW_MAX_JOBS], *dbias[EMER_DW_MAX_JOBS];
    DwDst dst[EMER_DW_MAX_JOBS];
};

// entry i of gradient j, range `by` of `ny` ranges of the partial blocks
__device__ __forceinline__ void dw_reduce_stage(const float *__restrict__ partials, int32_t n_blocks, int64_t stride, const DwJobs &jobs, int j,
                                                int64_t i, int32_t by, int32_t ny) {
    if (i >= jobs.extent[j]) return;
    const int32_t per = (n_blocks + ny - 1) / ny;
    const int32_t b0 = by * per;
    const int32_t b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    if (b0 >= b1) return;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    const float *__restrict__ p = partials + jobs.off[j] + i;
    int32_t b = b0;
    for (; b + 4 <= b1; b += 4) {
        a0 += p[(int64_t)b * stride];
        a1 += p[(int64_t)(b + 1) * stride];
        a2 += p[(int64_t)(b + 2) * stride];
        a3 += p[(int64_t)(b + 3) * stride];
    }
    for (; b < b1; ++b) a0 += p[(int64_t)b * stride];
    const float a = (a0 + a1) + (a2 + a3);
    const DwDst &dst = jobs.dst[j];
    if (i < jobs.nk[j]) {
        const int32_t n = (int32_t)(i / dst.K), k = (int32_t)(i - (int64_t)n * dst.K);
        int64_t o = -1;
#pragma unroll
        for (int sg = 0; sg < EMER_CHAIN_MAX_SEGS; ++sg)
            if (sg < dst.n && k >= dst.col[sg] && k < dst.col[sg] + dst.width[sg]) o = (int64_t)n * dst.ld + dst.dst[sg] + (k - dst.col[sg]);
        if (o >= 0) __hip_atomic_fetch_add(jobs.dw[j] + o, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (jobs.dbias[j]) __hip_atomic_fetch_add(jobs.dbias[j] + (i - jobs.nk[j]), a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static inline uint32_t dw_reduce_splits(int32_t n_blocks, int64_t stride) {
    // ~2048 workgroups in total, at least 8 partial blocks per range
    int64_t s = 2048 / ((stride + 255) / 256);
    if (s > n_blocks / 8) s = n_blocks / 8;
    return (uint32_t)(s < 1 ? 1 : s);
}

// The kernel's argument block for `n_jobs` gradients; returns the largest extent (floats of dW + dbias) among them.
static inline int64_t dw_reduce_pack(int n_jobs, const DwReduceJob *jb, DwJobs &jobs) {
    jobs.n_jobs = n_jobs;
    int64_t max_extent = 0;
    for (int j = 0; j < EMER_DW_MAX_JOBS; ++j) {
        const bool on = j < n_jobs;
        const DwReduceJob &q = jb[on ? j : 0];
        DwDst &d = jobs.dst[j];   // n_segs == 0: one block, column c of the partial at dw[row * ld_dw + c]
        for (int i = 0; i < EMER_CHAIN_MAX_SEGS; ++i) {
            const bool seg = i < q.n_segs;
            d.col[i] = seg ? q.col[i] : 0; d.width[i] = seg ? q.width[i] : (i == 0 && q.n_segs <= 0 ? q.k : 0); d.dst[i] = seg ? q.dst[i] : 0;
        }
        d.n = q.n_segs > 0 ? q.n_segs : 1; d.K = q.k; d.ld = q.ld_dw;
        jobs.off[j] = q.off; jobs.nk[j] = (int64_t)q.n * q.k; jobs.extent[j] = on ? (int64_t)q.n * q.k + (q.db ? q.n : 0) : 0;
        jobs.dw[j] = q.dw; jobs.dbias[j] = q.db;
        if (jobs.extent[j] > max_extent) max_extent = jobs.extent[j];
    }
    return max_extent;
}

}  // namespace emer
