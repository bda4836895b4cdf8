// Evaluation metrics for gfx950: SSIM exactly as scikit-image computes it, and squared-error sums with an optional row mask.
// The reference evaluates with skimage.metrics.structural_similarity on the host (radiance_fields/video_utils.py:206-233)
// and torch mse_loss per image; here every image's metrics stay on the device until the eval loop is over.
//
//   * emer_ssim: structural_similarity(x, y, data_range=1, channel_axis=-1) with its defaults (7 x 7 uniform window,
//     K1 = 0.01, K2 = 0.03, sample covariance 49/48, scipy 'reflect' borders, mean over the map cropped by 3 pixels), the
//     full S map of full=True, and the sum / count of S over masked pixels (the masked variant:
//     structural_similarity(..., full=True)[1][mask].mean()).  One workgroup per 32 x 16 output tile, channels in turn:
//     tile + 3-pixel halo of both images staged in LDS, separable 7-tap box sums.  The five moments and S are computed in
//     fp64: uxx - ux^2 cancels badly on bright flat images (fp32 moments are off by ~2e-4 there); sums of 7 / 49 fp32 values
//     and their products are (near) exact in fp64.
//   * emer_sq_err_sums: (sum of (p - t)^2, the same over rows whose mask is nonzero, number of such rows) in fp64 --
//     masked_psnr on colours, feat_psnr / masked_feat_psnr on DINO features.
//
// Both write per-workgroup partials into a caller-owned workspace and reduce them in a second one-block launch in a fixed
// order: results are bitwise identical from run to run (no float atomics, no inter-workgroup hand-off inside a launch).
#include "common.h"

namespace emer {

constexpr int kSsimTW = 32, kSsimTH = 16, kSsimHalo = 3, kSsimWin = 7;
constexpr int kSsimRawW = kSsimTW + 2 * kSsimHalo, kSsimRawH = kSsimTH + 2 * kSsimHalo;  // 38 x 22
constexpr int kSsimThreads = 256;
constexpr int kSqErrThreads = 256, kSqErrMaxBlocks = 1024;
constexpr int kReduceThreads = 256;

// scipy.ndimage 'reflect' (d c b a | a b c d | d c b a); exact for -n <= i < 2n, clamped beyond (halo rows of a partial
// tile that no valid output reads)
__device__ __forceinline__ int reflect_idx(int i, int n) {
    i = i < 0 ? -i - 1 : i;
    i = i >= n ? 2 * n - 1 - i : i;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// block-wide sum of three doubles in a fixed order (wave butterfly, then the waves in index order); thread 0 gets the result
template <int kThreads>
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c, double (*red)[3]) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, kWave);
        b += __shfl_xor(b, off, kWave);
        c += __shfl_xor(c, off, kWave);
    }
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) { red[wave][0] = a; red[wave][1] = b; red[wave][2] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0][0]; b = red[0][1]; c = red[0][2];
        for (int w = 1; w < kThreads / kWave; ++w) { a += red[w][0]; b += red[w][1]; c += red[w][2]; }
    }
}

__global__ __launch_bounds__(kSsimThreads) void ssim_tile_kernel(const float *__restrict__ xs, const float *__restrict__ ys,
                                                                 const float *__restrict__ mask, int32_t H, int32_t W, int32_t C,
                                                                 float *__restrict__ smap, double *__restrict__ partials) {
    __shared__ float raw_x[kSsimRawH][kSsimRawW + 1], raw_y[kSsimRawH][kSsimRawW + 1];
    __shared__ double hs[5][kSsimRawH][kSsimTW];   // horizontal 7-tap sums of x, y, x^2, y^2, xy
    __shared__ double red[kSsimThreads / kWave][3];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kSsimTW, y0 = blockIdx.y * kSsimTH;
    // this thread's two output pixels: column tid % 32, rows 2 * (tid / 32) and the one below
    const int col = tid % kSsimTW, r0 = 2 * (tid / kSsimTW);
    const int gx = x0 + col;
    bool valid[2], crop[2], masked[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int gy = y0 + r0 + k;
        valid[k] = gx < W && gy < H;
        crop[k] = valid[k] && gx >= kSsimHalo && gx < W - kSsimHalo && gy >= kSsimHalo && gy < H - kSsimHalo;
        masked[k] = valid[k] && mask != nullptr && mask[(int64_t)gy * W + gx] != 0.0f;
    }
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03, cov_norm = 49.0 / 48.0, inv_np = 1.0 / 49.0;
    double acc_crop = 0.0, acc_mask = 0.0, n_mask = 0.0;
    for (int c = 0; c < C; ++c) {
        for (int e = tid; e < kSsimRawH * kSsimRawW; e += kSsimThreads) {
            const int r = e / kSsimRawW, q = e - r * kSsimRawW;
            const int64_t g = ((int64_t)reflect_idx(y0 - kSsimHalo + r, H) * W + reflect_idx(x0 - kSsimHalo + q, W)) * C + c;
            raw_x[r][q] = xs[g];
            raw_y[r][q] = ys[g];
        }
        __syncthreads();
        for (int e = tid; e < kSsimRawH * kSsimTW; e += kSsimThreads) {
            const int r = e / kSsimTW, q = e - r * kSsimTW;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
            for (int j = 0; j < kSsimWin; ++j) {
                const double a = raw_x[r][q + j], b = raw_y[r][q + j];
                sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
            }
            hs[0][r][q] = sx; hs[1][r][q] = sy; hs[2][r][q] = sxx; hs[3][r][q] = syy; hs[4][r][q] = sxy;
        }
        __syncthreads();
        double m[5][2];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            double s = 0.0;
#pragma unroll
            for (int j = 1; j < kSsimWin; ++j) s += hs[i][r0 + j][col];
            m[i][0] = s + hs[i][r0][col];
            m[i][1] = s + hs[i][r0 + kSsimWin][col];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double ux = m[0][k] * inv_np, uy = m[1][k] * inv_np;
            const double uxx = m[2][k] * inv_np, uyy = m[3][k] * inv_np, uxy = m[4][k] * inv_np;
            const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
            const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
            const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
            const double S = (A1 * A2) / (B1 * B2);
            if (valid[k] && smap != nullptr) smap[((int64_t)(y0 + r0 + k) * W + gx) * C + c] = (float)S;
            if (crop[k]) acc_crop += S;
            if (masked[k]) { acc_mask += S; n_mask += 1.0; }
        }
        __syncthreads();   // the next channel overwrites raw_* / hs
    }
    block_sum3<kSsimThreads>(acc_crop, acc_mask, n_mask, red);
    if (tid == 0) {
        double *p = partials + 3 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x);
        p[0] = acc_crop; p[1] = acc_mask; p[2] = n_mask;
    }
}

__global__ __launch_bounds__(kSqErrThreads) void sq_err_partial_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                                       const float *__restrict__ mask, int64_t rows, int32_t cols,
                                                                       bool vec4, double *__restrict__ partials) {
    __shared__ double red[kSqErrThreads / kWave][3];
    const int64_t total = rows * cols, stride = (int64_t)gridDim.x * kSqErrThreads;
    double s_all = 0.0, s_mask = 0.0, n_mask = 0.0;
    if (vec4) {   // 16-byte loads; total % 4 == 0 and both bases 16-byte aligned
        const float4 *p4 = reinterpret_cast<const float4 *>(pred), *t4 = reinterpret_cast<const float4 *>(target);
        for (int64_t v = (int64_t)blockIdx.x * kSqErrThreads + threadIdx.x; v < total / 4; v += stride) {
            const float4 a = p4[v], b = t4[v];
            const float pa[4] = {a.x, a.y, a.z, a.w}, tb[4] = {b.x, b.y, b.z, b.w};
            int64_t r = (4 * v) / cols, q = 4 * v - r * cols;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double d = (double)pa[k] - (double)tb[k], d2 = d * d;
                s_all += d2;
                if (mask != nullptr && mask[r] != 0.0f) { s_mask += d2; n_mask += q == 0 ? 1.0 : 0.0; }
                if (++q == cols) { q = 0; ++r; }
            }
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * kSqErrThreads + threadIdx.x; i < total; i += stride) {
            const double d = (double)pred[i] - (double)target[i], d2 = d * d;
            s_all += d2;
            if (mask != nullptr) {
                const int64_t r = i / cols;
                if (mask[r] != 0.0f) { s_mask += d2; n_mask += i == r * cols ? 1.0 : 0.0; }
            }
        }
    }
    block_sum3<kSqErrThreads>(s_all, s_mask, n_mask, red);
    if (threadIdx.x == 0) {
        double *p = partials + 3 * (int64_t)blockIdx.x;
        p[0] = s_all; p[1] = s_mask; p[2] = n_mask;
    }
}

// out[k] = (sum over blocks of partials[b][k]) in a fixed order; out[0] is then multiplied by scale0
__global__ __launch_bounds__(kReduceThreads) void sum3_finalize_kernel(const double *__restrict__ partials, int64_t n_blocks,
                                                                       double scale0, double *__restrict__ out) {
    __shared__ double red[kReduceThreads / kWave][3];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int64_t i = threadIdx.x; i < n_blocks; i += kReduceThreads) {
        a += partials[3 * i]; b += partials[3 * i + 1]; c += partials[3 * i + 2];
    }
    block_sum3<kReduceThreads>(a, b, c, red);
    if (threadIdx.x == 0) { out[0] = a * scale0; out[1] = b; out[2] = c; }
}

static int64_t ssim_blocks(int64_t H, int64_t W) { return ceil_div(W, kSsimTW) * ceil_div(H, kSsimTH); }

static int64_t sq_err_blocks(int64_t rows, int64_t cols) {
    int64_t b = ceil_div(rows * cols, kSqErrThreads * 4);
    return b < 1 ? 1 : (b > kSqErrMaxBlocks ? kSqErrMaxBlocks : b);
}

}  // namespace emer

using namespace emer;

extern "C" int64_t emer_ssim_workspace(int32_t height, int32_t width) {
    if (height < 1 || width < 1) return 0;
    return 3 * ssim_blocks(height, width);
}

extern "C" int emer_ssim(const float *pred, const float *gt, const float *mask, int32_t height, int32_t width, int32_t channels,
                         float *ssim_map, double *workspace, double *out, void *stream) {
    EMER_REQUIRE(height >= kSsimWin && width >= kSsimWin,
                 "ssim: the image (%d x %d) is smaller than the 7 x 7 window (scikit-image raises here too)", height, width);
    EMER_REQUIRE(channels >= 1, "ssim: need at least one channel");
    EMER_REQUIRE((int64_t)height * width * channels < (1ll << 40), "ssim: image too large");
    EMER_REQUIRE(pred && gt && workspace && out, "ssim: null pointer");
    hipStream_t st = as_stream(stream);
    const dim3 grid((uint32_t)ceil_div(width, kSsimTW), (uint32_t)ceil_div(height, kSsimTH));
    hipLaunchKernelGGL(ssim_tile_kernel, grid, dim3(kSsimThreads), 0, st, pred, gt, mask, height, width, channels, ssim_map, workspace);
    const double n_crop = (double)channels * (height - 2 * kSsimHalo) * (width - 2 * kSsimHalo);
    hipLaunchKernelGGL(sum3_finalize_kernel, dim3(1), dim3(kReduceThreads), 0, st, workspace, ssim_blocks(height, width), 1.0 / n_crop, out);
    return check_launch("ssim");
}

extern "C" int64_t emer_sq_err_sums_workspace(int64_t rows, int32_t cols) {
    if (rows < 0 || cols < 1) return 0;
    return 3 * sq_err_blocks(rows, cols);
}

extern "C" int emer_sq_err_sums(const float *pred, const float *target, const float *row_mask, int64_t rows, int32_t cols,
                                double *workspace, double *out, void *stream) {
    EMER_REQUIRE(rows >= 0 && cols >= 1 && rows * (int64_t)cols < (1ll << 48), "sq_err_sums: bad sizes");
    EMER_REQUIRE(workspace && out && (rows == 0 || (pred && target)), "sq_err_sums: null pointer");
    hipStream_t st = as_stream(stream);
    const int64_t blocks = sq_err_blocks(rows, cols);
    const bool vec4 = (rows * cols) % 4 == 0 && ((uintptr_t)pred & 15) == 0 && ((uintptr_t)target & 15) == 0;
    hipLaunchKernelGGL(sq_err_partial_kernel, dim3((uint32_t)blocks), dim3(kSqErrThreads), 0, st, pred, target, row_mask, rows, cols, vec4,
                       workspace);
    hipLaunchKernelGGL(sum3_finalize_kernel, dim3(1), dim3(kReduceThreads), 0, st, workspace, blocks, 1.0, out);
    return check_launch("sq_err_sums");
}
