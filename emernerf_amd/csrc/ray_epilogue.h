// Per-ray epilogue of `rendering` (radiance_fields/render_utils.py:102-105,217-226), the one copy of its arithmetic: opacity =
// clamp(sum w, 1e-6, 1), depth = sum(w mid) / opacity, rgb = acc_rgb + rgb_sky * (1 - opacity), and the reverse of the three.
// Used per thread by ray_epilogue_fwd/bwd_kernel (rayloss.hip) and per wave by composite_rgb_fwd/bwd_kernel (composite.hip), whose
// results are bitwise equal (tests/test_kernels_gpu.py).  st = (sum w, sum w*mid, median depth, -) of ray r.
#pragma once
#include "common.h"

namespace emer {

__device__ __forceinline__ float epilogue_opacity(float wsum) { return fminf(fmaxf(wsum, 1e-6f), 1.0f); }  // torch.clamp(1e-6, 1.0)

// acc: the ray's accumulated colour at acc[acc_off + c] (read only where rgb is wanted); median, rgb, rgb_sky may be null
__device__ __forceinline__ void epilogue_fwd(float4 st, const float *acc, int64_t acc_off, const float *__restrict__ rgb_sky, int64_t r,
                                             float *__restrict__ opacity, float *__restrict__ depth, float *__restrict__ median,
                                             float *__restrict__ rgb) {
    const float o = epilogue_opacity(st.x);
    opacity[r] = o;
    depth[r] = st.y / o;
    if (median) median[r] = st.z;
    if (rgb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = acc[acc_off + c];
            if (rgb_sky) v = v + rgb_sky[r * 3 + c] * (1.0f - o);
            rgb[r * 3 + c] = v;
        }
    }
}

// (g0, g1) = gradient of (sum w, sum w*mid); g[c] = d_rgb[r][c] (zero without d_rgb): the gradient of acc_rgb is d_rgb itself.
// d_rgb_sky [R,3] is written where `store` (one lane of a wave that owns the ray).  Every pointer but none of st may be null.
struct EpilogueGrad { float g0, g1, g[3]; };
__device__ __forceinline__ EpilogueGrad epilogue_bwd(float4 st, const float *__restrict__ rgb_sky, const float *__restrict__ d_opacity,
                                                     const float *__restrict__ d_depth, const float *__restrict__ d_rgb, int64_t r,
                                                     bool store, float *__restrict__ d_rgb_sky) {
    EpilogueGrad e = {0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
    const float o = epilogue_opacity(st.x);
    float go = d_opacity ? d_opacity[r] : 0.0f;
    const float gd = d_depth ? d_depth[r] : 0.0f;
    go -= gd * st.y / (o * o);
    if (d_rgb) {   // (the three loads together, ahead of the sky branch: a thread-per-ray caller waits on them once)
#pragma unroll
        for (int c = 0; c < 3; ++c) e.g[c] = d_rgb[r * 3 + c];
    }
    if (d_rgb && rgb_sky) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            go -= e.g[c] * rgb_sky[r * 3 + c];
            if (d_rgb_sky && store) d_rgb_sky[r * 3 + c] = e.g[c] * (1.0f - o);
        }
    }
    e.g0 = (st.x >= 1e-6f && st.x <= 1.0f) ? go : 0.0f;  // clamp passes the gradient where min <= x <= max (torch semantics, bounds included)
    e.g1 = gd / o;
    return e;
}

}  // namespace emer
