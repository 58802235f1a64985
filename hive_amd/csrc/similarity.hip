// Scores a render against a held-out frame on the device: compare_images' SSIM and PSNR (scripts/compare_image_pair.py:110-133) and ms_ssim as called at
// scripts/experiments.py:1627-1635, for a batch of picture pairs, plain and with the frame whitened where the render shows background (:846-848).  gfx950 only.
// The rules are stated in include/hive_mi355x.h above hive_similarity_ssim_psnr; in short:
//
//   gray     g = (1868 c0 + 9617 c1 + 4899 c2 + 8192) >> 14 (the outer weights swapped for rgb_order), integer
//   mask     variant 1: a reference channel value reads as 255 where the estimate's value in that channel is 255 (per channel, while loading)
//   SSIM     five exact int32 sums over 7 x 7 windows (a horizontal 7-sum, then a vertical one, in LDS), then S in float64 in the stated order
//   sums     per thread in ascending tile order, a fixed tree per workgroup, one partial per workgroup; similarity_finish_kernel adds a picture's partials in
//            a fixed order: no floating-point atomic, the same bits on every run and in every batch
//   PSNR     the integer sum of squared gray differences (LDS integer atomic, then one 64-bit integer atomic per workgroup)
//   MS-SSIM  per level the five products filtered by the 11-tap window along H, then along W, through LDS in float64; 2 x 2 pooled planes for the next level
//
// Float64 without contraction (the Makefile's EXACT flags).
//
// Kernels: similarity_ssim_kernel (one workgroup per 32 x 32 tile of the map, per picture and variant), similarity_msssim_kernel (one workgroup per 16 x 32
// tile, per picture, variant and channel), similarity_pool_kernel (one thread per pooled value), similarity_finish_kernel (one workgroup per row of
// partials), similarity_combine_kernel (one thread per picture).
#include "hive_internal.hpp"

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_TILE = 32;              // the map tile of the SSIM kernel, SM_TILE x SM_TILE
constexpr int SM_WIN = 7;
constexpr int SM_IN = SM_TILE + SM_WIN - 1;  // 38: the tile with its halo
constexpr int MS_TAPS = 11;
constexpr int MS_TH = 16, MS_TW = 32;    // the map tile of the MS-SSIM kernel
constexpr int MS_IH = MS_TH + MS_TAPS - 1, MS_IW = MS_TW + MS_TAPS - 1;  // 26 x 42
constexpr int MS_LEVELS = 5;

__device__ __forceinline__ int sm_gray(int c0, int c1, int c2, int w0, int w2) { return (w0 * c0 + 9617 * c1 + w2 * c2 + 8192) >> 14; }

// grid (tiles_x, tiles_y, variants * N)
__global__ __launch_bounds__(SM_THREADS) void similarity_ssim_kernel(const uint8_t *__restrict__ ref, const uint8_t *__restrict__ est, int N, int H, int W, int w0,
                                                                     int w2, double *__restrict__ partials, unsigned long long *__restrict__ sse,
                                                                     double *__restrict__ map, uint8_t *__restrict__ gray_ref, uint8_t *__restrict__ gray_est) {
    __shared__ uint8_t gx[SM_IN][SM_IN + 2], gy[SM_IN][SM_IN + 2];
    __shared__ int hs[5][SM_IN][SM_TILE];
    __shared__ double red[SM_THREADS];
    __shared__ unsigned sse_tile;
    const int t = threadIdx.x;
    const int z = blockIdx.z, variant = z / N, n = z % N;
    const int i0 = blockIdx.y * SM_TILE, j0 = blockIdx.x * SM_TILE;
    // the last tile of a row / column also owns the picture's last 6 columns / rows (for the gray planes and the squared differences)
    const int own_r = blockIdx.y == gridDim.y - 1 ? SM_IN : SM_TILE, own_c = blockIdx.x == gridDim.x - 1 ? SM_IN : SM_TILE;
    if (t == 0) sse_tile = 0;
    __syncthreads();
    const size_t plane = (size_t)H * W;
    unsigned sq = 0;  // at most 6 pixels a thread: < 2^32
    for (int p = t; p < SM_IN * SM_IN; p += SM_THREADS) {
        const int r = p / SM_IN, c = p % SM_IN, i = i0 + r, j = j0 + c;
        int x = 0, y = 0;
        if (i < H && j < W) {
            const size_t px = (size_t)n * plane + (size_t)i * W + j;
            const uint8_t *a = ref + 3 * px, *b = est + 3 * px;
            int a0 = a[0], a1 = a[1], a2 = a[2];
            const int b0 = b[0], b1 = b[1], b2 = b[2];
            if (variant) a0 = b0 == 255 ? 255 : a0, a1 = b1 == 255 ? 255 : a1, a2 = b2 == 255 ? 255 : a2;
            x = sm_gray(a0, a1, a2, w0, w2), y = sm_gray(b0, b1, b2, w0, w2);
            if (r < own_r && c < own_c) {
                sq += (unsigned)((x - y) * (x - y));
                if (gray_ref) gray_ref[(size_t)variant * N * plane + px] = (uint8_t)x;
                if (gray_est && variant == 0) gray_est[px] = (uint8_t)y;
            }
        }
        gx[r][c] = (uint8_t)x, gy[r][c] = (uint8_t)y;
    }
    if (sq) atomicAdd(&sse_tile, sq);  // at most 38 * 38 * 255^2 < 2^32
    __syncthreads();
    for (int p = t; p < SM_IN * SM_TILE; p += SM_THREADS) {
        const int r = p / SM_TILE, c = p % SM_TILE;
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < SM_WIN; ++k) {
            const int x = gx[r][c + k], y = gy[r][c + k];
            sx += x, sy += y, sxx += x * x, syy += y * y, sxy += x * y;
        }
        hs[0][r][c] = sx, hs[1][r][c] = sy, hs[2][r][c] = sxx, hs[3][r][c] = syy, hs[4][r][c] = sxy;
    }
    __syncthreads();
    const int Hm = H - (SM_WIN - 1), Wm = W - (SM_WIN - 1);
    const double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255), cov_norm = 49.0 / 48.0;
    double acc = 0.0;
    for (int p = t; p < SM_TILE * SM_TILE; p += SM_THREADS) {
        const int r = p / SM_TILE, c = p % SM_TILE, i = i0 + r, j = j0 + c;
        if (i >= Hm || j >= Wm) continue;
        int s[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < SM_WIN; ++k)
#pragma unroll
            for (int q = 0; q < 5; ++q) s[q] += hs[q][r + k][c];
        const double ux = (double)s[0] / 49.0, uy = (double)s[1] / 49.0, uxx = (double)s[2] / 49.0, uyy = (double)s[3] / 49.0, uxy = (double)s[4] / 49.0;
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        const double S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
        acc = acc + S;
        if (map) map[((size_t)z * Hm + i) * Wm + j] = S;
    }
    red[t] = acc;
    block_tree_sum<SM_THREADS, 1>(&red);
    if (t == 0) {
        partials[((size_t)z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = red[0];
        if (sse_tile) atomicAdd(sse + z, (unsigned long long)sse_tile);
    }
}

struct MsWindow {
    double g[MS_TAPS];
};

// the reference picture's channel value at byte `at` as float64 c / 255.0, read as 255 where `masked` and the estimate's byte there is 255
__device__ __forceinline__ double ms_u8(const uint8_t *__restrict__ pic, const uint8_t *__restrict__ est, bool masked, size_t at) {
    const int v = pic[at];
    return (double)((masked && est[at] == 255) ? 255 : v) / 255.0;
}

// grid (tiles_x, tiles_y, variants * N * 3); partials [2][gridDim.z][tiles]
__global__ __launch_bounds__(SM_THREADS) void similarity_msssim_kernel(const uint8_t *__restrict__ ref_u8, const uint8_t *__restrict__ est_u8,
                                                                       const double *__restrict__ xs, const double *__restrict__ ys, int N, int h, int w, MsWindow win,
                                                                       double *__restrict__ partials) {
    __shared__ double sx[MS_IH][MS_IW + 1], sy[MS_IH][MS_IW + 1];
    __shared__ double v[5][MS_TH][MS_IW + 1];
    __shared__ double red[SM_THREADS];
    const int t = threadIdx.x;
    const int z = blockIdx.z, ch = z % 3, n = (z / 3) % N, variant = z / (3 * N);
    const int i0 = blockIdx.y * MS_TH, j0 = blockIdx.x * MS_TW;
    const size_t plane = (size_t)h * w;
    for (int p = t; p < MS_IH * MS_IW; p += SM_THREADS) {
        const int r = p / MS_IW, c = p % MS_IW, i = i0 + r, j = j0 + c;
        double a = 0.0, b = 0.0;
        if (i < h && j < w) {
            if (ref_u8) {
                const size_t at = 3 * ((size_t)n * plane + (size_t)i * w + j) + ch;
                a = ms_u8(ref_u8, est_u8, variant != 0, at), b = (double)est_u8[at] / 255.0;
            } else {
                const size_t at = (size_t)i * w + j;
                a = xs[((size_t)z) * plane + at], b = ys[((size_t)n * 3 + ch) * plane + at];
            }
        }
        sx[r][c] = a, sy[r][c] = b;
    }
    __syncthreads();
    for (int p = t; p < MS_TH * MS_IW; p += SM_THREADS) {  // along H
        const int r = p / MS_IW, c = p % MS_IW;
        double m1 = 0.0, m2 = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
        for (int k = 0; k < MS_TAPS; ++k) {
            const double a = sx[r + k][c], b = sy[r + k][c], g = win.g[k];
            m1 = m1 + g * a, m2 = m2 + g * b, xx = xx + g * (a * a), yy = yy + g * (b * b), xy = xy + g * (a * b);
        }
        v[0][r][c] = m1, v[1][r][c] = m2, v[2][r][c] = xx, v[3][r][c] = yy, v[4][r][c] = xy;
    }
    __syncthreads();
    const int hm = h - (MS_TAPS - 1), wm = w - (MS_TAPS - 1);
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double acc_cs = 0.0, acc_ssim = 0.0;
    for (int p = t; p < MS_TH * MS_TW; p += SM_THREADS) {  // along W
        const int r = p / MS_TW, c = p % MS_TW;
        if (i0 + r >= hm || j0 + c >= wm) continue;
        double f[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < MS_TAPS; ++k)
#pragma unroll
            for (int q = 0; q < 5; ++q) f[q] = f[q] + win.g[k] * v[q][r][c + k];
        const double mu1 = f[0], mu2 = f[1];
        const double s1 = f[2] - mu1 * mu1, s2 = f[3] - mu2 * mu2, s12 = f[4] - mu1 * mu2;
        const double cs = (2 * s12 + C2) / (s1 + s2 + C2);
        const double ssim = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs;
        acc_cs = acc_cs + cs, acc_ssim = acc_ssim + ssim;
    }
    const size_t tiles = (size_t)gridDim.x * gridDim.y, tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    red[t] = acc_cs;
    block_tree_sum<SM_THREADS, 1>(&red);
    if (t == 0) partials[(size_t)z * tiles + tile] = red[0];
    __syncthreads();
    red[t] = acc_ssim;
    block_tree_sum<SM_THREADS, 1>(&red);
    if (t == 0) partials[((size_t)gridDim.z + z) * tiles + tile] = red[0];
}

// one thread per pooled value: groups 0 .. variants - 1 are the X planes of the variants, group `variants` the Y planes; each group holds [N][3][h2][w2]
__global__ __launch_bounds__(SM_THREADS) void similarity_pool_kernel(const uint8_t *__restrict__ ref_u8, const uint8_t *__restrict__ est_u8,
                                                                     const double *__restrict__ xs, const double *__restrict__ ys, int N, int h, int w, int variants,
                                                                     double *__restrict__ x_next, double *__restrict__ y_next) {
    const int h2 = (h + 1) / 2, w2 = (w + 1) / 2, ph = h & 1, pw = w & 1;
    const long long per_group = (long long)N * 3 * h2 * w2;
    const long long e = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    if (e >= per_group * (variants + 1)) return;
    const int group = (int)(e / per_group);
    const long long q = e % per_group;
    const int j2 = (int)(q % w2), i2 = (int)((q / w2) % h2);
    const long long nc = q / ((long long)w2 * h2);  // n * 3 + ch
    const int ch = (int)(nc % 3);
    const long long n = nc / 3;
    const bool is_y = group == variants;
    const size_t plane = (size_t)h * w;
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int i = 2 * i2 - ph + a, j = 2 * j2 - pw + b;
            double val = 0.0;  // the padding
            if (i >= 0 && j >= 0) {  // (i < h and j < w always)
                if (ref_u8) {
                    const size_t at = 3 * ((size_t)n * plane + (size_t)i * w + j) + ch;
                    val = is_y ? (double)est_u8[at] / 255.0 : ms_u8(ref_u8, est_u8, group != 0, at);
                } else {
                    const size_t at = (size_t)i * w + j;
                    val = is_y ? ys[(size_t)nc * plane + at] : xs[((size_t)group * N * 3 + (size_t)nc) * plane + at];
                }
            }
            sum = sum + val;
        }
    (is_y ? y_next : x_next + (size_t)group * per_group)[q] = sum / 4.0;
}

// one workgroup per row
__global__ __launch_bounds__(SM_THREADS) void similarity_finish_kernel(const double *__restrict__ partials, long long per_row, double divisor, double *__restrict__ out) {
    __shared__ double red[SM_THREADS];
    const double *row = partials + (size_t)blockIdx.x * per_row;
    double acc = 0.0;
    for (long long k = threadIdx.x; k < per_row; k += SM_THREADS) acc = acc + row[k];
    red[threadIdx.x] = acc;
    block_tree_sum<SM_THREADS, 1>(&red);
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] / divisor;
}

// means [5][2][count][3] -> out [count]
__global__ __launch_bounds__(SM_THREADS) void similarity_combine_kernel(const double *__restrict__ means, long long count, double *__restrict__ out) {
    const long long e = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    if (e >= count) return;
    const double weight[MS_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    double sum = 0.0;
    for (int ch = 0; ch < 3; ++ch) {
        double prod = 1.0;
        for (int l = 0; l < MS_LEVELS; ++l) {
            const int kind = l == MS_LEVELS - 1 ? 1 : 0;
            const double value = means[(((size_t)l * 2 + kind) * count + e) * 3 + ch];
            prod = prod * pow(fmax(value, 0.0), weight[l]);
        }
        sum = sum + prod;
    }
    out[e] = sum / 3.0;
}

}  // namespace

extern "C" {

int hive_similarity_ssim_psnr(hive_ctx *ctx, const uint8_t *d_ref, const uint8_t *d_est, int N, int H, int W, int rgb_order, int variants, double *d_partials,
                              int64_t *d_sse, double *d_map, uint8_t *d_gray_ref, uint8_t *d_gray_est) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_ref && d_est && d_partials && d_sse, "similarity_ssim_psnr: NULL argument");
    HIVE_REQUIRE(ctx, N >= 1, "similarity_ssim_psnr: N = %d, need at least one pair", N);
    HIVE_REQUIRE(ctx, H >= SM_WIN && W >= SM_WIN, "similarity_ssim_psnr: %d x %d is smaller than the 7 x 7 window", H, W);
    HIVE_REQUIRE(ctx, (long long)H * W < (1ll << 31), "similarity_ssim_psnr: %d x %d pixels do not fit below 2^31", H, W);
    HIVE_REQUIRE(ctx, variants == 1 || variants == 2, "similarity_ssim_psnr: variants = %d, need 1 (plain) or 2 (plain and masked)", variants);
    HIVE_REQUIRE(ctx, (long long)variants * N <= 65535, "similarity_ssim_psnr: variants * N = %lld exceeds 65535", (long long)variants * N);
    HIVE_REQUIRE(ctx, rgb_order == 0 || rgb_order == 1, "similarity_ssim_psnr: rgb_order = %d, need 0 (bgr) or 1 (rgb)", rgb_order);
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(d_sse, 0, (size_t)variants * N * sizeof(int64_t), ctx->stream));
    const dim3 grid((unsigned)hive_div_up(W - (SM_WIN - 1), SM_TILE), (unsigned)hive_div_up(H - (SM_WIN - 1), SM_TILE), (unsigned)(variants * N));
    HIVE_REQUIRE(ctx, grid.y <= 65535, "similarity_ssim_psnr: H = %d has too many tile rows", H);
    hipLaunchKernelGGL(similarity_ssim_kernel, grid, dim3(SM_THREADS), 0, ctx->stream, d_ref, d_est, N, H, W, rgb_order ? 4899 : 1868, rgb_order ? 1868 : 4899,
                       d_partials, (unsigned long long *)d_sse, d_map, d_gray_ref, d_gray_est);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_similarity_msssim_level(hive_ctx *ctx, const uint8_t *d_ref_u8, const uint8_t *d_est_u8, const double *d_x, const double *d_y, int N, int h, int w,
                                 int variants, const double window[11], double *d_partials, double *d_x_next, double *d_y_next) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    const bool from_u8 = d_ref_u8 && d_est_u8 && !d_x && !d_y, from_f64 = d_x && d_y && !d_ref_u8 && !d_est_u8;
    HIVE_REQUIRE(ctx, from_u8 || from_f64, "similarity_msssim_level: give the two u8 pictures or the two float64 planes");
    HIVE_REQUIRE(ctx, window && d_partials, "similarity_msssim_level: NULL argument");
    HIVE_REQUIRE(ctx, (d_x_next == nullptr) == (d_y_next == nullptr), "similarity_msssim_level: both next planes or neither");
    HIVE_REQUIRE(ctx, N >= 1, "similarity_msssim_level: N = %d, need at least one pair", N);
    HIVE_REQUIRE(ctx, h >= MS_TAPS && w >= MS_TAPS, "similarity_msssim_level: %d x %d is smaller than the 11-tap window", h, w);
    HIVE_REQUIRE(ctx, (long long)h * w < (1ll << 31), "similarity_msssim_level: %d x %d values do not fit below 2^31", h, w);
    HIVE_REQUIRE(ctx, variants == 1 || variants == 2, "similarity_msssim_level: variants = %d, need 1 or 2", variants);
    HIVE_REQUIRE(ctx, (long long)variants * N * 3 <= 65535, "similarity_msssim_level: variants * N * 3 = %lld exceeds 65535", (long long)variants * N * 3);
    MsWindow win;
    memcpy(win.g, window, sizeof(win.g));
    const dim3 grid((unsigned)hive_div_up(w - (MS_TAPS - 1), MS_TW), (unsigned)hive_div_up(h - (MS_TAPS - 1), MS_TH), (unsigned)(variants * N * 3));
    HIVE_REQUIRE(ctx, grid.y <= 65535, "similarity_msssim_level: h = %d has too many tile rows", h);
    const long long n = (long long)(variants + 1) * N * 3 * ((h + 1) / 2) * ((w + 1) / 2);  // pooled values
    HIVE_REQUIRE(ctx, (n + SM_THREADS - 1) / SM_THREADS < (1ll << 31), "similarity_msssim_level: %lld pooled values are too many for one launch", n);
    hipLaunchKernelGGL(similarity_msssim_kernel, grid, dim3(SM_THREADS), 0, ctx->stream, d_ref_u8, d_est_u8, d_x, d_y, N, h, w, win, d_partials);
    if (d_x_next) {
        hipLaunchKernelGGL(similarity_pool_kernel, dim3((unsigned)((n + SM_THREADS - 1) / SM_THREADS)), dim3(SM_THREADS), 0, ctx->stream, d_ref_u8, d_est_u8, d_x, d_y, N,
                           h, w, variants, d_x_next, d_y_next);
    }
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_similarity_finish(hive_ctx *ctx, const double *d_partials, int64_t rows, int64_t per_row, double divisor, double *d_out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_partials && d_out, "similarity_finish: NULL argument");
    HIVE_REQUIRE(ctx, rows >= 1 && rows < (1ll << 31) && per_row >= 1, "similarity_finish: bad shape %lld x %lld", (long long)rows, (long long)per_row);
    HIVE_REQUIRE(ctx, divisor > 0.0, "similarity_finish: the divisor must be > 0");
    hipLaunchKernelGGL(similarity_finish_kernel, dim3((unsigned)rows), dim3(SM_THREADS), 0, ctx->stream, d_partials, (long long)per_row, divisor, d_out);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_similarity_msssim_combine(hive_ctx *ctx, const double *d_means, int64_t count, double *d_out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_means && d_out, "similarity_msssim_combine: NULL argument");
    HIVE_REQUIRE(ctx, count >= 1 && count < (1ll << 31), "similarity_msssim_combine: bad count %lld", (long long)count);
    hipLaunchKernelGGL(similarity_combine_kernel, dim3((unsigned)((count + SM_THREADS - 1) / SM_THREADS)), dim3(SM_THREADS), 0, ctx->stream, d_means, (long long)count,
                       d_out);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

}  // extern "C"
