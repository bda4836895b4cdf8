// Alpha-compositing volume renderer for gfx950.
//
// Replaces nerfacc's dense-tensor volrend as EmerNeRF calls it (render_transmittance_from_density,
// render_weight_from_density, accumulate_along_rays: radiance_fields/render_utils.py:35-43,73-77,
// 103-115,159-282; third_party/nerfacc_prop_net.py:165-168; loss/base.py:454-460).  Semantics:
// SURVEY.md Appendix A.2; CPU restatement: oracle/emer_oracle.c (orc_render_weights, orc_accumulate).
//
// Mapping: one 64-lane wavefront owns one ray; lane i holds sample 64*c + i of chunk c.  The
// exclusive cumsum of sigma*dt (and the reverse-mode suffix sums) are wave scans built from DPP
// shuffles -- no LDS traffic, no atomics, fully coalesced (R,S) loads/stores.  S is unbounded
// (chunks of 64 with a carried prefix); at the metric shape S=128 a ray is exactly two chunks.
//
// Tests: tests/test_composite_exact_gpu.py holds every kernel of this file entry by entry -- to the fp64 restatement
// exactly on probes whose fp32 operations are all exact (tests/_composite_probe.py: walls with sigma*dt in {0, 128},
// dyadic accumulate / blend inputs), and inside a derived first-order bound on realistic rays (tests/_bounds.py:
// render_bounds, dsigma_bound, epilogue_bounds, blend_c).  tests/_composite_model.py is a numpy model of the chunking,
// carries, tail masking, median latch, four-wave split and quads below; tests/test_composite_bounds_cpu.py runs it and its
// mutants against the same probes.  Each stage that two kernels share (scan chunk, ray statistics, chunk_base pre-pass, reverse
// chunk, blend ratios, the epilogue of ray_epilogue.h) is one function here, and the model follows those functions: a change to
// the summation structure of one of them needs the same change in that model.  tools/composite_digests.py: bitwise A/B of a refactor.
#include "common.h"
#include "ray_epilogue.h"

namespace emer {

constexpr int kRaysPerBlockC = 4;

// ---------------------------------------------------------------------------- stages shared by the scan kernels
// One 64-sample chunk of ray r at samples base .. base + 63, lane = sample, in two steps: load_chunk, the loads with the tail mask
// (a lane past S holds zeros), and scan_chunk, the wave scan of sigma*dt on top of `prefix` (the sum over the earlier chunks), T and
// e = exp(-sigma*dt).  A kernel with more to load per sample issues it between the two, ahead of the scan's waits.  The forward
// kernels carry `prefix` along, the backward kernels read it from chunk_base.
struct ScanChunk {
    int64_t i;  // flat (r, s)
    bool ok;    // s < S
    float sg, mid, dt, sdt, incl, T, e;
};
__device__ __forceinline__ ScanChunk load_chunk(const float *__restrict__ ts, const float *__restrict__ te,
                                                const float *__restrict__ sigma, int64_t r, int32_t S, int32_t base, int lane) {
    ScanChunk k;
    const int32_t s = base + lane;
    k.ok = s < S;
    k.i = r * S + s;
    const float a = k.ok ? ts[k.i] : 0.0f, b = k.ok ? te[k.i] : 0.0f;
    k.sg = k.ok ? sigma[k.i] : 0.0f;
    k.mid = (a + b) / 2.0f;
    k.dt = b - a;
    k.sdt = k.sg * k.dt;
    return k;
}
__device__ __forceinline__ float sub_unfused(float x, float y) {
#pragma clang fp contract(off)
    return x - y;
}
__device__ __forceinline__ void scan_chunk(ScanChunk &k, int lane, float prefix, bool fused_excl) {
    k.incl = wave_inclusive_sum(k.sdt, lane);
    // exclusive = inclusive - own.  The compiler's contraction has always made ONE fused multiply-add of `incl - sg * dt` in the two
    // forward kernels (the product unrounded) and left the rounded product and a subtraction in the two backward kernels; both are
    // written out here, so that no kernel's T depends on what gets contracted around it (making the two agree is a numerical change)
    const float own = fused_excl ? __fmaf_rn(-k.sg, k.dt, k.incl) : sub_unfused(k.incl, k.sdt);
    k.T = expf(-(prefix + own));
    k.e = expf(-k.sdt);
}

// (sum w, sum w*mid, median depth) of a ray, chunk by chunk.  Median depth: the midpoint of the first sample whose inclusive
// cumsum(w) reaches 0.5, else of the last sample (render_utils.py:107-115).
struct RayStats {
    float wsum = 0.0f, wmid = 0.0f, wcarry = 0.0f, median = 0.0f, last_mid = 0.0f;
    bool found = false;
    __device__ __forceinline__ void step(float w, float mid, bool ok, int32_t base, int32_t S, int lane) {
        const float cw = wcarry + wave_inclusive_sum(w, lane);
        const unsigned long long hit = __ballot(ok && cw >= 0.5f);
        if (!found && hit) {
            const int first = __ffsll((long long)hit) - 1;
            median = __shfl(mid, first, kWave);
            found = true;
        }
        const int last_lane = (S - 1 - base) < (kWave - 1) ? (S - 1 - base) : (kWave - 1);
        last_mid = __shfl(mid, last_lane, kWave);
        wcarry = __shfl(cw, kWave - 1, kWave);
        wsum += w;
        wmid += w * mid;
    }
    __device__ __forceinline__ float4 finish() { return make_float4(wave_sum(wsum), wave_sum(wmid), found ? median : last_mid, 0.0f); }
};

// Pre-pass of the backward kernels: row[c] = sum of sigma*dt over the chunks before c (S <= 4096: at most 64 chunks).
__device__ __forceinline__ void fill_chunk_base(const float *__restrict__ ts, const float *__restrict__ te,
                                                const float *__restrict__ sigma, int64_t r, int32_t S, int lane, float *row) {
    float carry = 0.0f;
    for (int32_t c = 0; c < (S + kWave - 1) / kWave; ++c) {
        const int32_t s = c * kWave + lane;
        const int64_t i = r * S + s;
        const float sdt = s < S ? sigma[i] * (te[i] - ts[i]) : 0.0f;
        if (lane == 0) row[c] = carry;
        carry += wave_sum(sdt);
    }
}

// Reverse mode.  With a_i = sigma_i*dt_i, T_i = exp(-sum_{j<i} a_j), w_i = T_i (1 - exp(-a_i)):
//   dL/da_i = gw_i * T_{i+1} - sum_{k>i} (gw_k w_k + gT_k T_k) + galpha_i * exp(-a_i),   T_{i+1} = T_i exp(-a_i)
// with gw_i = d_weights_i + g(sum w) + g(sum w*mid) * mid_i (alpha_i = 1 - exp(-a_i) is a differentiable output too:
// the reference's render_utils.py:73-77 forms weights = trans * alphas itself).
// One chunk of it: the first two terms of dL/da_i (the caller adds its alpha term and multiplies by dt); `suffix`, the sum over
// the later chunks of (gw w + gT T), moves on by this chunk.
__device__ __forceinline__ float reverse_chunk(const ScanChunk &k, float gw, float gT, int lane, float &suffix) {
    const float w = k.T * (1.0f - k.e);
    const float term = k.ok ? gw * w + gT * k.T : 0.0f;
    const float sfx_incl = wave_inclusive_suffix_sum(term, lane);
    const float later = suffix + (sfx_incl - term);  // strictly-later samples
    suffix += __shfl(sfx_incl, 0, kWave);
    return gw * k.T * k.e - later;
}

// ---------------------------------------------------------------------------- weights / transmittance scan
__global__ __launch_bounds__(256) void render_weights_fwd_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                                 const float *__restrict__ sigma, int64_t R, int32_t S,
                                                                 float *__restrict__ weights, float *__restrict__ trans,
                                                                 float *__restrict__ alphas, float *__restrict__ cdfs,
                                                                 float *__restrict__ ray_stats, float *__restrict__ t_mid,
                                                                 float *__restrict__ t_dist) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRaysPerBlockC + wave;
    if (r >= R) return;
    float carry = 0.0f;  // sum of sigma*dt over previous chunks
    RayStats stats;
    for (int32_t base = 0; base < S; base += kWave) {
        ScanChunk k = load_chunk(ts, te, sigma, r, S, base, lane);
        scan_chunk(k, lane, carry, true);
        const float al = 1.0f - k.e;
        const float w = k.ok ? k.T * al : 0.0f;
        if (k.ok) {
            if (weights) weights[k.i] = w;
            if (trans) trans[k.i] = k.T;
            if (alphas) alphas[k.i] = al;
            if (cdfs) cdfs[r * (int64_t)(S + 1) + base + lane] = 1.0f - k.T;
            if (t_mid) t_mid[k.i] = k.mid;  // extras["t_vals"], extras["t_dist"] of rendering (render_utils.py:84-85)
            if (t_dist) t_dist[k.i] = k.dt;
        }
        carry += __shfl(k.incl, kWave - 1, kWave);
        if (ray_stats) stats.step(w, k.mid, k.ok, base, S, lane);
    }
    if (cdfs && lane == 0) cdfs[r * (int64_t)(S + 1) + S] = 1.0f;  // 1 - [T, 0]
    if (ray_stats) {
        const float4 st = stats.finish();
        if (lane == 0) *reinterpret_cast<float4 *>(ray_stats + r * 4) = st;
    }
}

__global__ __launch_bounds__(256) void render_weights_bwd_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                                 const float *__restrict__ sigma,
                                                                 const float *__restrict__ d_weights,
                                                                 const float *__restrict__ d_trans,
                                                                 const float *__restrict__ d_alphas,
                                                                 const float *__restrict__ d_ray_stats, int64_t R, int32_t S,
                                                                 float *__restrict__ d_sigma) {
    __shared__ float chunk_base[kRaysPerBlockC][64];  // per-wave exclusive prefix of each 64-chunk (S <= 4096)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRaysPerBlockC + wave;
    const bool active = r < R;
    if (active) fill_chunk_base(ts, te, sigma, r, S, lane, chunk_base[wave]);
    __syncthreads();
    if (!active) return;
    const float g0 = d_ray_stats ? d_ray_stats[r * 4 + 0] : 0.0f;  // [R,4] like ray_stats (columns 2, 3 carry no gradient)
    const float g1 = d_ray_stats ? d_ray_stats[r * 4 + 1] : 0.0f;
    float suffix = 0.0f;
    for (int32_t c = (S + kWave - 1) / kWave - 1; c >= 0; --c) {
        ScanChunk k = load_chunk(ts, te, sigma, r, S, c * kWave, lane);
        scan_chunk(k, lane, chunk_base[wave][c], false);
        float gw = (k.ok && d_weights) ? d_weights[k.i] : 0.0f;
        gw += g0 + g1 * k.mid;
        const float gT = (k.ok && d_trans) ? d_trans[k.i] : 0.0f;
        const float gA = (k.ok && d_alphas) ? d_alphas[k.i] : 0.0f;
        const float da = reverse_chunk(k, gw, gT, lane, suffix);
        if (k.ok) d_sigma[k.i] = k.dt * (da + gA * k.e);
    }
}

// out[r,c] = sum_s w[r,s] * values[r,s,c].  Few channels (<= 8): lanes walk samples, one wave
// reduction per channel.  Many channels: lanes walk channels (coalesced rows), w broadcast.
template <int C>
__global__ __launch_bounds__(256) void accumulate_fwd_small_kernel(const float *__restrict__ w, const float *__restrict__ v,
                                                                   int64_t R, int32_t S, float *__restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRaysPerBlockC + wave;
    if (r >= R) return;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
    for (int32_t s = lane; s < S; s += kWave) {
        const float ws = w[r * S + s];
        if (v) {
            const float *vp = v + (r * S + s) * (int64_t)C;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += ws * vp[c];
        } else {
            acc[0] += ws;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) out[r * C + c] = acc[c];
    }
}

__global__ __launch_bounds__(256) void accumulate_fwd_wide_kernel(const float *__restrict__ w, const float *__restrict__ v,
                                                                  int64_t R, int32_t S, int32_t C, float *__restrict__ out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRaysPerBlockC + wave;
    if (r >= R) return;
    for (int32_t c0 = 0; c0 < C; c0 += kWave) {
        const int32_t c = c0 + lane;
        float acc = 0.0f;
        if (c < C)
            for (int32_t s = 0; s < S; ++s) acc += w[r * S + s] * v[(r * S + s) * (int64_t)C + c];
        if (c < C) out[r * (int64_t)C + c] = acc;
    }
}

template <int C>
__global__ __launch_bounds__(256) void accumulate_bwd_small_kernel(const float *__restrict__ w, const float *__restrict__ v,
                                                                   const float *__restrict__ d_out, int64_t R, int32_t S,
                                                                   float *__restrict__ d_w, float *__restrict__ d_v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // flat (r, s)
    if (i >= R * S) return;
    const int64_t r = i / S;
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = d_out[r * C + c];
    if (d_w) {
        float a = 0.0f;
        if (v) {
#pragma unroll
            for (int c = 0; c < C; ++c) a += g[c] * v[i * C + c];
        } else {
            a = g[0];
        }
        d_w[i] = a;
    }
    if (d_v) {
        const float ws = w[i];
#pragma unroll
        for (int c = 0; c < C; ++c) d_v[i * C + c] = ws * g[c];
    }
}

__global__ __launch_bounds__(256) void accumulate_bwd_wide_kernel(const float *__restrict__ w, const float *__restrict__ v,
                                                                  const float *__restrict__ d_out, int64_t R, int32_t S,
                                                                  int32_t C, float *__restrict__ d_w, float *__restrict__ d_v) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRaysPerBlockC + wave;
    if (r >= R) return;
    for (int32_t s = 0; s < S; ++s) {
        const float ws = w[r * S + s];
        float dot = 0.0f;
        for (int32_t c = lane; c < C; c += kWave) {
            const float g = d_out[r * (int64_t)C + c];
            const int64_t j = (r * S + s) * (int64_t)C + c;
            if (d_w) dot += g * v[j];
            if (d_v) d_v[j] = ws * g;
        }
        if (d_w) {
            dot = wave_sum(dot);
            if (lane == 0) d_w[r * S + s] = dot;
        }
    }
}


// ---------------------------------------------------------------------------- static / dynamic / shadow blend
// rendering's decomposed colour path (radiance_fields/render_utils.py:125-173) in one pass per direction:
//   a = sigma_s / (sigma + 1e-6), b = sigma_d / (sigma + 1e-6)                       (:131-136)
//   rgb = a * rgb_s * (1 - shadow) + b * rgb_d                                        (:169-173)
//   acc_rgb[r] = sum_s w * rgb,   acc_shadow[r] = sum_s w * shadow^2                  (:165-168,175)
// The reference materialises a, b and the blended [R,S,3] colour (plus their autograd graph: ~30 elementwise
// launches on 12 MB tensors); here one wave owns a ray, lanes walk its samples.
struct BlendRatios { float inv, a, b; };
__device__ __forceinline__ BlendRatios blend_ratios(float sig, float sig_s, float sig_d) {
    const float inv = 1.0f / (sig + 1e-6f);
    return {inv, sig_s * inv, sig_d * inv};
}

__global__ __launch_bounds__(256) void blend_accumulate_fwd_kernel(const float *__restrict__ w, const float *__restrict__ sig,
                                                                   const float *__restrict__ sig_s, const float *__restrict__ sig_d,
                                                                   const float *__restrict__ rgb_s, const float *__restrict__ rgb_d,
                                                                   const float *__restrict__ shadow, int64_t R, int32_t S,
                                                                   float *__restrict__ acc_rgb, float *__restrict__ acc_shadow) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRaysPerBlockC + wave;
    if (r >= R) return;
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, cs = 0.0f;
    for (int32_t s = lane; s < S; s += kWave) {
        const int64_t i = r * S + s;
        const float wi = w[i];
        const BlendRatios q = blend_ratios(sig[i], sig_s[i], sig_d[i]);
        const float sh = shadow ? shadow[i] : 0.0f;
        const float ka = q.a * (1.0f - sh);
        c0 += wi * (ka * rgb_s[i * 3 + 0] + q.b * rgb_d[i * 3 + 0]);
        c1 += wi * (ka * rgb_s[i * 3 + 1] + q.b * rgb_d[i * 3 + 1]);
        c2 += wi * (ka * rgb_s[i * 3 + 2] + q.b * rgb_d[i * 3 + 2]);
        cs += wi * sh * sh;
    }
    c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2); cs = wave_sum(cs);
    if (lane == 0) {
        acc_rgb[r * 3 + 0] = c0; acc_rgb[r * 3 + 1] = c1; acc_rgb[r * 3 + 2] = c2;
        if (acc_shadow) acc_shadow[r] = cs;
    }
}

__global__ __launch_bounds__(256) void blend_accumulate_bwd_kernel(const float *__restrict__ w, const float *__restrict__ sig,
                                                                   const float *__restrict__ sig_s, const float *__restrict__ sig_d,
                                                                   const float *__restrict__ rgb_s, const float *__restrict__ rgb_d,
                                                                   const float *__restrict__ shadow, const float *__restrict__ g_rgb,
                                                                   const float *__restrict__ g_shadow, int64_t R, int32_t S,
                                                                   float *__restrict__ d_w, float *__restrict__ d_sig,
                                                                   float *__restrict__ d_sig_s, float *__restrict__ d_sig_d,
                                                                   float *__restrict__ d_rgb_s, float *__restrict__ d_rgb_d,
                                                                   float *__restrict__ d_shadow) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRaysPerBlockC + wave;
    if (r >= R) return;
    const float g0 = g_rgb ? g_rgb[r * 3 + 0] : 0.0f, g1 = g_rgb ? g_rgb[r * 3 + 1] : 0.0f, g2 = g_rgb ? g_rgb[r * 3 + 2] : 0.0f;
    const float gs = g_shadow ? g_shadow[r] : 0.0f;
    for (int32_t s = lane; s < S; s += kWave) {
        const int64_t i = r * S + s;
        const float wi = w[i], ss = sig_s[i], sd = sig_d[i];
        const BlendRatios q = blend_ratios(sig[i], ss, sd);
        const float sh = shadow ? shadow[i] : 0.0f;
        const float s0 = rgb_s[i * 3 + 0], s1 = rgb_s[i * 3 + 1], s2 = rgb_s[i * 3 + 2];
        const float e0 = rgb_d[i * 3 + 0], e1 = rgb_d[i * 3 + 1], e2 = rgb_d[i * 3 + 2];
        const float ka = q.a * (1.0f - sh);
        const float gS = g0 * s0 + g1 * s1 + g2 * s2;  // <g, rgb_s>
        const float gD = g0 * e0 + g1 * e1 + g2 * e2;  // <g, rgb_d>
        if (d_w) d_w[i] = ka * gS + q.b * gD + gs * sh * sh;
        const float wka = wi * ka, wb = wi * q.b;
        if (d_rgb_s) { d_rgb_s[i * 3 + 0] = g0 * wka; d_rgb_s[i * 3 + 1] = g1 * wka; d_rgb_s[i * 3 + 2] = g2 * wka; }
        if (d_rgb_d) { d_rgb_d[i * 3 + 0] = g0 * wb; d_rgb_d[i * 3 + 1] = g1 * wb; d_rgb_d[i * 3 + 2] = g2 * wb; }
        if (d_shadow) d_shadow[i] = wi * (2.0f * gs * sh - q.a * gS);
        const float da = wi * (1.0f - sh) * gS, db = wi * gD;   // dL/da, dL/db (twin: the tail of blend_accumulate_wide_bwd_kernel)
        if (d_sig_s) d_sig_s[i] = da * q.inv;
        if (d_sig_d) d_sig_d[i] = db * q.inv;
        if (d_sig) d_sig[i] = -(da * ss + db * sd) * q.inv * q.inv;
    }
}

// [r4] The same blend for the WIDE feature channels of the decomposed feature head (render_utils.py:247-252):
//   acc[r][c] = sum_s w * (a * feat_s[c] + b * feat_d[c]),  a, b as above.
// The reference materialises both ratios with a trailing axis, two [R,S,C] products, their sum and the accumulation -- with autograd,
// ~15 elementwise launches on 67 MB tensors at the 2048-ray shard.  One wave owns a ray, lanes walk the channels (coalesced rows), the
// per-sample scalars are wave-uniform loads; the backward needs two wave reductions per sample (<g, feat_s>, <g, feat_d>).
__global__ __launch_bounds__(256) void blend_accumulate_wide_fwd_kernel(const float *__restrict__ w, const float *__restrict__ sig,
                                                                        const float *__restrict__ sig_s, const float *__restrict__ sig_d,
                                                                        const float *__restrict__ f_s, const float *__restrict__ f_d, int64_t R,
                                                                        int32_t S, int32_t C, float *__restrict__ acc) {
    // one workgroup per ray: wave k takes the samples k, k + 4, ... (two at a time: two independent chains), the four partial sums meet in LDS
    __shared__ float part[4][kWave];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = blockIdx.x;
    for (int32_t c0 = 0; c0 < C; c0 += kWave) {
        const int32_t c = c0 + lane;
        const bool on = c < C;
        float a0 = 0.0f, a1 = 0.0f;
        int32_t s = wave;
        for (; s + 4 < S; s += 8) {
            const int64_t i = r * S + s, i2 = i + 4;
            const BlendRatios q0 = blend_ratios(sig[i], sig_s[i], sig_d[i]), q1 = blend_ratios(sig[i2], sig_s[i2], sig_d[i2]);
            const float fs0 = on ? f_s[i * C + c] : 0.0f, fd0 = on ? f_d[i * C + c] : 0.0f;
            const float fs1 = on ? f_s[i2 * C + c] : 0.0f, fd1 = on ? f_d[i2 * C + c] : 0.0f;
            a0 += w[i] * (q0.a * fs0 + q0.b * fd0);
            a1 += w[i2] * (q1.a * fs1 + q1.b * fd1);
        }
        if (s < S) {
            const int64_t i = r * S + s;
            const BlendRatios q0 = blend_ratios(sig[i], sig_s[i], sig_d[i]);
            const float fs0 = on ? f_s[i * C + c] : 0.0f, fd0 = on ? f_d[i * C + c] : 0.0f;
            a0 += w[i] * (q0.a * fs0 + q0.b * fd0);
        }
        part[wave][lane] = a0 + a1;
        __syncthreads();
        if (wave == 0 && on) acc[r * (int64_t)C + c] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void blend_accumulate_wide_bwd_kernel(const float *__restrict__ w, const float *__restrict__ sig,
                                                                        const float *__restrict__ sig_s, const float *__restrict__ sig_d,
                                                                        const float *__restrict__ f_s, const float *__restrict__ f_d,
                                                                        const float *__restrict__ g_acc, int64_t R, int32_t S, int32_t C,
                                                                        float *__restrict__ d_w, float *__restrict__ d_sig,
                                                                        float *__restrict__ d_sig_s, float *__restrict__ d_sig_d,
                                                                        float *__restrict__ d_f_s, float *__restrict__ d_f_d) {
    // samples are independent in the backward: a wave takes FOUR consecutive samples at a time (flat over (ray, sample); their eight
    // feature rows are in flight together, the eight dot products reduce interleaved, lanes 0..3 write the per-sample scalars)
    const int lane = threadIdx.x & 63;
    const int64_t n = R * (int64_t)S, n_quads = (n + 3) >> 2, n_waves = (int64_t)gridDim.x * 4;
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < n_quads; q += n_waves) {
        float gS[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gD[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wa[4], wb[4];
        int64_t rr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = q * 4 + u < n ? q * 4 + u : n - 1;
            rr[u] = i / S;
            const float inv = 1.0f / (sig[i] + 1e-6f);  // (w * sigma_s) * inv: the feature gradients' own order, not blend_ratios'
            wa[u] = w[i] * sig_s[i] * inv;
            wb[u] = w[i] * sig_d[i] * inv;
        }
        for (int32_t c = lane; c < C; c += kWave) {
            float fs[4], fd[4], g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = q * 4 + u < n ? q * 4 + u : n - 1;
                g[u] = g_acc[rr[u] * (int64_t)C + c];
                fs[u] = f_s[i * C + c];
                fd[u] = f_d[i * C + c];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t i = q * 4 + u;
                gS[u] += g[u] * fs[u];
                gD[u] += g[u] * fd[u];
                if (i < n) {
                    if (d_f_s) d_f_s[i * C + c] = g[u] * wa[u];
                    if (d_f_d) d_f_d[i * C + c] = g[u] * wb[u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { gS[u] = wave_sum(gS[u]); gD[u] = wave_sum(gD[u]); }
        const int u = lane & 3;
        const int64_t i = q * 4 + u;
        if (lane < 4 && i < n) {
            const float mS = u == 0 ? gS[0] : u == 1 ? gS[1] : u == 2 ? gS[2] : gS[3];
            const float mD = u == 0 ? gD[0] : u == 1 ? gD[1] : u == 2 ? gD[2] : gD[3];
            // twin of blend_ratios and of the d_sig tail of blend_accumulate_bwd_kernel, written out: through shared helpers this
            // kernel read 3 to 5 % above its parent in two sessions, like this it compiles to the parent's instructions
            // (profiles/composite_dedup_ab.json); change both copies alike
            const float wi = w[i], ss = sig_s[i], sd = sig_d[i], inv = 1.0f / (sig[i] + 1e-6f);
            const float a_ = ss * inv, b_ = sd * inv;
            if (d_w) d_w[i] = a_ * mS + b_ * mD;
            const float da = wi * mS, db = wi * mD;
            if (d_sig_s) d_sig_s[i] = da * inv;
            if (d_sig_d) d_sig_d[i] = db * inv;
            if (d_sig) d_sig[i] = -(da * ss + db * sd) * inv * inv;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ [r4]
// The static model's `rendering` (render_utils.py:73-122,158-159,217-220) as ONE launch each way: weights / transmittance scan,
// accumulation of the 3-channel colour, and the per-ray epilogue (opacity clamp, expected depth, median depth, sky composite) --
// three launches forward and three backward before, on tensors of a few MB.  Same arithmetic, same order as the three kernels
// (render_weights_fwd / accumulate_fwd_small<3> / ray_epilogue_fwd): results are bitwise theirs.  rgb == nullptr: geometry only
// (the density-only render of the lidar step).
__global__ __launch_bounds__(256) void composite_rgb_fwd_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                                const float *__restrict__ sigma, const float *__restrict__ rgb,
                                                                const float *__restrict__ rgb_sky, int64_t R, int32_t S,
                                                                float *__restrict__ weights, float *__restrict__ trans,
                                                                float *__restrict__ t_mid, float *__restrict__ t_dist,
                                                                float *__restrict__ ray_stats, float *__restrict__ opacity,
                                                                float *__restrict__ depth, float *__restrict__ median_out,
                                                                float *__restrict__ rgb_out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRaysPerBlockC + wave;
    if (r >= R) return;
    float carry = 0.0f;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    RayStats stats;
    for (int32_t base = 0; base < S; base += kWave) {
        ScanChunk k = load_chunk(ts, te, sigma, r, S, base, lane);
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
        if (k.ok && rgb) { c0 = rgb[k.i * 3 + 0]; c1 = rgb[k.i * 3 + 1]; c2 = rgb[k.i * 3 + 2]; }
        scan_chunk(k, lane, carry, true);
        const float w = k.ok ? k.T * (1.0f - k.e) : 0.0f;
        if (k.ok) {
            weights[k.i] = w;
            if (trans) trans[k.i] = k.T;
            if (t_mid) t_mid[k.i] = k.mid;
            if (t_dist) t_dist[k.i] = k.dt;
            acc[0] += w * c0; acc[1] += w * c1; acc[2] += w * c2;   // accumulate_fwd_small<3>: lanes walk samples
        }
        carry += __shfl(k.incl, kWave - 1, kWave);
        stats.step(w, k.mid, k.ok, base, S, lane);
    }
    const float4 st = stats.finish();
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) {
        *reinterpret_cast<float4 *>(ray_stats + r * 4) = st;
        epilogue_fwd(st, acc, 0, rgb_sky, r, opacity, depth, median_out, rgb_out);
    }
}

// Reverse of the above: ray_epilogue_bwd (per ray, by every lane), accumulate_bwd_small<3> and render_weights_bwd in one pass.
// d_weights / d_trans: gradients that reach the extras from other consumers (may be null).
__global__ __launch_bounds__(256) void composite_rgb_bwd_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                                const float *__restrict__ sigma, const float *__restrict__ rgb,
                                                                const float *__restrict__ rgb_sky, const float *__restrict__ weights,
                                                                const float *__restrict__ ray_stats, const float *__restrict__ d_rgb_out,
                                                                const float *__restrict__ d_opacity, const float *__restrict__ d_depth,
                                                                const float *__restrict__ d_weights, const float *__restrict__ d_trans,
                                                                int64_t R, int32_t S, float *__restrict__ d_sigma,
                                                                float *__restrict__ d_rgb, float *__restrict__ d_rgb_sky) {
    __shared__ float chunk_base[kRaysPerBlockC][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRaysPerBlockC + wave;
    const bool active = r < R;
    if (active) fill_chunk_base(ts, te, sigma, r, S, lane, chunk_base[wave]);
    __syncthreads();
    if (!active) return;
    // per-ray part (ray_epilogue_bwd, by every lane): gradient of (sum w, sum w mid) and of the accumulated colour
    const EpilogueGrad eg = epilogue_bwd(*reinterpret_cast<const float4 *>(ray_stats + r * 4), rgb_sky, d_opacity, d_depth, d_rgb_out, r,
                                         lane == 0, d_rgb_sky);
    float suffix = 0.0f;
    for (int32_t c = (S + kWave - 1) / kWave - 1; c >= 0; --c) {
        ScanChunk k = load_chunk(ts, te, sigma, r, S, c * kWave, lane);
        scan_chunk(k, lane, chunk_base[wave][c], false);
        float gw = (k.ok && d_weights) ? d_weights[k.i] : 0.0f;
        if (k.ok && rgb && d_rgb_out) {   // accumulate_bwd: d_w += sum_c g_c rgb_c,  d_rgb = w g
            float acc = 0.0f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc += eg.g[ch] * rgb[k.i * 3 + ch];
            gw += acc;
            if (d_rgb) {
                const float ws = weights[k.i];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) d_rgb[k.i * 3 + ch] = ws * eg.g[ch];
            }
        }
        gw += eg.g0 + eg.g1 * k.mid;
        const float gT = (k.ok && d_trans) ? d_trans[k.i] : 0.0f;
        const float da = reverse_chunk(k, gw, gT, lane, suffix);
        if (k.ok) d_sigma[k.i] = k.dt * da;
    }
}

}  // namespace emer

using namespace emer;

// What every entry point ends in: `blocks` workgroups of 256 threads on `stream`, then the launch check under the entry's name.
template <class K, class... A>
static int launch256(const char *what, K kern, int64_t blocks, void *stream, A... args) {
    hipLaunchKernelGGL(kern, dim3((uint32_t)blocks), dim3(256), 0, as_stream(stream), args...);
    return check_launch(what);
}
static int64_t ray_blocks(int64_t R) { return ceil_div(R, kRaysPerBlockC); }  // one wave per ray

extern "C" int emer_composite_rgb_fwd(const float *ts, const float *te, const float *sigma, const float *rgb, const float *rgb_sky, int64_t R,
                                      int32_t S, float *weights, float *trans, float *t_mid, float *t_dist, float *ray_stats, float *opacity,
                                      float *depth, float *median_depth, float *rgb_out, void *stream) {
    EMER_REQUIRE(R >= 0 && S >= 1, "composite_rgb_fwd: bad sizes R=%lld S=%d", (long long)R, S);
    if (R == 0) return EMER_OK;
    EMER_REQUIRE(ts && te && sigma && weights && ray_stats && opacity && depth && (!rgb_out || rgb), "composite_rgb_fwd: null pointer");
    return launch256("composite_rgb_fwd", composite_rgb_fwd_kernel, ray_blocks(R), stream, ts, te, sigma, rgb_out ? rgb : nullptr, rgb_sky, R, S,
                     weights, trans, t_mid, t_dist, ray_stats, opacity, depth, median_depth, rgb_out);
}

extern "C" int emer_composite_rgb_bwd(const float *ts, const float *te, const float *sigma, const float *rgb, const float *rgb_sky,
                                      const float *weights, const float *ray_stats, const float *d_rgb_out, const float *d_opacity,
                                      const float *d_depth, const float *d_weights, const float *d_trans, int64_t R, int32_t S,
                                      float *d_sigma, float *d_rgb, float *d_rgb_sky, void *stream) {
    EMER_REQUIRE(R >= 0 && S >= 1 && S <= 4096, "composite_rgb_bwd: bad sizes R=%lld S=%d (S <= 4096)", (long long)R, S);
    if (R == 0) return EMER_OK;
    EMER_REQUIRE(ts && te && sigma && ray_stats && d_sigma && (!d_rgb || (rgb && weights && d_rgb_out)), "composite_rgb_bwd: null pointer");
    return launch256("composite_rgb_bwd", composite_rgb_bwd_kernel, ray_blocks(R), stream, ts, te, sigma, rgb, rgb_sky, weights, ray_stats,
                     d_rgb_out, d_opacity, d_depth, d_weights, d_trans, R, S, d_sigma, d_rgb, d_rgb_sky);
}

extern "C" int emer_blend_accumulate_wide_fwd(const float *weights, const float *density, const float *static_density, const float *dynamic_density,
                                             const float *static_feat, const float *dynamic_feat, int64_t R, int32_t S, int32_t C, float *acc,
                                             void *stream) {
    EMER_REQUIRE(R >= 0 && S >= 1 && C >= 1, "blend_accumulate_wide_fwd: bad sizes");
    if (R == 0) return EMER_OK;
    EMER_REQUIRE(weights && density && static_density && dynamic_density && static_feat && dynamic_feat && acc, "blend_accumulate_wide_fwd: null pointer");
    return launch256("blend_accumulate_wide_fwd", blend_accumulate_wide_fwd_kernel, R, stream, weights, density, static_density, dynamic_density,
                     static_feat, dynamic_feat, R, S, C, acc);   // one workgroup per ray
}

extern "C" int emer_blend_accumulate_wide_bwd(const float *weights, const float *density, const float *static_density, const float *dynamic_density,
                                             const float *static_feat, const float *dynamic_feat, const float *d_acc, int64_t R, int32_t S, int32_t C,
                                             float *d_weights, float *d_density, float *d_static_density, float *d_dynamic_density,
                                             float *d_static_feat, float *d_dynamic_feat, void *stream) {
    EMER_REQUIRE(R >= 0 && S >= 1 && C >= 1, "blend_accumulate_wide_bwd: bad sizes");
    if (R == 0) return EMER_OK;
    EMER_REQUIRE(weights && density && static_density && dynamic_density && static_feat && dynamic_feat && d_acc, "blend_accumulate_wide_bwd: null pointer");
    const int64_t wg = ceil_div(R * (int64_t)S, 4 * 8);   // ~two quads of samples per wave
    return launch256("blend_accumulate_wide_bwd", blend_accumulate_wide_bwd_kernel, wg > 16384 ? 16384 : wg, stream, weights, density, static_density,
                     dynamic_density, static_feat, dynamic_feat, d_acc, R, S, C, d_weights, d_density, d_static_density, d_dynamic_density,
                     d_static_feat, d_dynamic_feat);
}

extern "C" int emer_render_weights_fwd(const float *ts, const float *te, const float *sigma, int64_t R, int32_t S,
                                       float *weights, float *trans, float *alphas, float *cdfs, float *ray_stats,
                                       float *t_mid, float *t_dist, void *stream) {
    EMER_REQUIRE(R >= 0 && S >= 1, "render_weights_fwd: bad sizes R=%lld S=%d", (long long)R, S);
    if (R == 0) return EMER_OK;
    EMER_REQUIRE(ts && te && sigma, "render_weights_fwd: null input");
    return launch256("render_weights_fwd", render_weights_fwd_kernel, ray_blocks(R), stream, ts, te, sigma, R, S, weights, trans, alphas, cdfs,
                     ray_stats, t_mid, t_dist);
}

extern "C" int emer_render_weights_bwd(const float *ts, const float *te, const float *sigma, const float *d_weights,
                                       const float *d_trans, const float *d_alphas, const float *d_ray_stats, int64_t R,
                                       int32_t S, float *d_sigma, void *stream) {
    EMER_REQUIRE(R >= 0 && S >= 1 && S <= 4096, "render_weights_bwd: bad sizes R=%lld S=%d (S <= 4096)", (long long)R, S);
    if (R == 0) return EMER_OK;
    EMER_REQUIRE(ts && te && sigma && d_sigma, "render_weights_bwd: null pointer");
    return launch256("render_weights_bwd", render_weights_bwd_kernel, ray_blocks(R), stream, ts, te, sigma, d_weights, d_trans, d_alphas,
                     d_ray_stats, R, S, d_sigma);
}

extern "C" int emer_accumulate_fwd(const float *w, const float *v, int64_t R, int32_t S, int32_t C, float *out,
                                   void *stream) {
    EMER_REQUIRE(R >= 0 && S >= 1 && C >= 1, "accumulate_fwd: bad sizes");
    if (R == 0) return EMER_OK;
    EMER_REQUIRE(w && out, "accumulate_fwd: null pointer");
    EMER_REQUIRE(v || C == 1, "accumulate_fwd: values == NULL requires n_channels == 1");
    switch (C) {
#define EMER_ACC(c) case c: return launch256("accumulate_fwd", accumulate_fwd_small_kernel<c>, ray_blocks(R), stream, w, v, R, S, out);
        EMER_ACC(1) EMER_ACC(2) EMER_ACC(3) EMER_ACC(4) EMER_ACC(5) EMER_ACC(6) EMER_ACC(7) EMER_ACC(8)
#undef EMER_ACC
    }
    return launch256("accumulate_fwd", accumulate_fwd_wide_kernel, ray_blocks(R), stream, w, v, R, S, C, out);
}

extern "C" int emer_accumulate_bwd(const float *w, const float *v, const float *d_out, int64_t R, int32_t S, int32_t C,
                                   float *d_w, float *d_v, void *stream) {
    EMER_REQUIRE(R >= 0 && S >= 1 && C >= 1, "accumulate_bwd: bad sizes");
    if (R == 0) return EMER_OK;
    EMER_REQUIRE(w && d_out, "accumulate_bwd: null pointer");
    EMER_REQUIRE(v || (C == 1 && !d_v), "accumulate_bwd: values == NULL requires n_channels == 1 and d_values == NULL");
    switch (C) {   // small: one thread per (ray, sample)
#define EMER_ACC(c) case c: return launch256("accumulate_bwd", accumulate_bwd_small_kernel<c>, ceil_div(R * S, 256), stream, w, v, d_out, R, S, d_w, d_v);
        EMER_ACC(1) EMER_ACC(2) EMER_ACC(3) EMER_ACC(4) EMER_ACC(5) EMER_ACC(6) EMER_ACC(7) EMER_ACC(8)
#undef EMER_ACC
    }
    return launch256("accumulate_bwd", accumulate_bwd_wide_kernel, ray_blocks(R), stream, w, v, d_out, R, S, C, d_w, d_v);
}

extern "C" int emer_blend_accumulate_fwd(const float *weights, const float *density, const float *static_density,
                                         const float *dynamic_density, const float *static_rgb, const float *dynamic_rgb,
                                         const float *shadow_ratio, int64_t R, int32_t S, float *acc_rgb, float *acc_shadow_sq,
                                         void *stream) {
    EMER_REQUIRE(R >= 0 && S >= 1, "blend_accumulate_fwd: bad sizes");
    if (R == 0) return EMER_OK;
    EMER_REQUIRE(weights && density && static_density && dynamic_density && static_rgb && dynamic_rgb && acc_rgb, "blend_accumulate_fwd: null pointer");
    EMER_REQUIRE(!acc_shadow_sq || shadow_ratio, "blend_accumulate_fwd: acc_shadow_sq needs shadow_ratio");
    return launch256("blend_accumulate_fwd", blend_accumulate_fwd_kernel, ray_blocks(R), stream, weights, density, static_density, dynamic_density,
                     static_rgb, dynamic_rgb, shadow_ratio, R, S, acc_rgb, acc_shadow_sq);
}

extern "C" int emer_blend_accumulate_bwd(const float *weights, const float *density, const float *static_density,
                                         const float *dynamic_density, const float *static_rgb, const float *dynamic_rgb,
                                         const float *shadow_ratio, const float *d_acc_rgb, const float *d_acc_shadow_sq, int64_t R,
                                         int32_t S, float *d_weights, float *d_density, float *d_static_density,
                                         float *d_dynamic_density, float *d_static_rgb, float *d_dynamic_rgb, float *d_shadow_ratio,
                                         void *stream) {
    EMER_REQUIRE(R >= 0 && S >= 1, "blend_accumulate_bwd: bad sizes");
    if (R == 0) return EMER_OK;
    EMER_REQUIRE(weights && density && static_density && dynamic_density && static_rgb && dynamic_rgb, "blend_accumulate_bwd: null pointer");
    EMER_REQUIRE(!d_shadow_ratio || shadow_ratio, "blend_accumulate_bwd: d_shadow_ratio needs shadow_ratio");
    return launch256("blend_accumulate_bwd", blend_accumulate_bwd_kernel, ray_blocks(R), stream, weights, density, static_density, dynamic_density,
                     static_rgb, dynamic_rgb, shadow_ratio, d_acc_rgb, d_acc_shadow_sq, R, S, d_weights, d_density, d_static_density,
                     d_dynamic_density, d_static_rgb, d_dynamic_rgb, d_shadow_ratio);
}
