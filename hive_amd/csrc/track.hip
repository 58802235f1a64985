// Frame-to-model camera tracking: the depth pyramid with vertex and normal maps of the live frame (hive_frame_maps) and one Gauss-Newton step of
// point-to-plane ICP against ray-cast model maps (hive_icp_step: projective association, the 6 x 6 normal equations reduced on the device).  gfx950 only.
// The rules are stated in include/hive_mi355x.h above hive_frame_maps; in short:
//
//   pyramid   level l + 1 pixel (u, v) from the 2 x 2 block at (2u, 2v): m = the smallest sample > 0; the mean, summed in row-major order, of the samples > 0
//             with d - m <= pyr_delta; 0 for a block without a sample (float32)
//   maps      V = ((d (u - cx)) / fx, (d (v - cy)) / fy, d); N = (V(u+1, v) - V) x (V(u, v+1) - V) normalised and turned to face the camera (float32)
//   ICP       per live pixel in float64 from the float32 maps: q = R V + t, n = R N, projected into the model camera, rounded to a pixel with the context's
//             rounding; distance and angle gates; r = N_m . (V_m - q), J = [q x N_m, N_m]; 21 + 6 + 1 sums and the pair count
//   sums      one pixel per thread, the fixed tree v[t] += v[t + off], off = 128 .. 1, per workgroup, one row of partials per workgroup; icp_finish_kernel adds
//             the rows in ascending order: no floating-point atomic, the same bits on every run
//   colour    hive_gray_pyramid: Y / 255 of the live frame (float32, the JPEG encoder's integer luma), halved by plain 2 x 2 means.  hive_rgbd_icp_step adds the
//             photometric term in the same launch: the live pixel projected into the model picture without rounding, the model's gray value (from its
//             ray-cast colour, on the fly) and central-difference gradients sampled bilinearly at the 2 x 2 cell, an occlusion gate on the model's depth;
//             r = I_live - I_model, J = [q x g_w, g_w] with g_w the image gradient carried to the world frame.  Its 29 sums follow the geometric ones in a
//             workgroup's row of partials (the LDS rows are used twice); the host adds A_geo + w^2 A_photo
//
// Float64 / float32 without contraction (the Makefile's EXACT flags).
#include "hive_internal.hpp"

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_SUMS = 28;            // 21 upper-triangle J^T J, 6 J^T r, r^2
constexpr int TK_COLS = TK_SUMS + 1;   // ... and the pair count (a whole number: exact in float64)
constexpr int TK_MAX_LEVELS = 8;

__global__ __launch_bounds__(TK_THREADS) void pyr_down_kernel(const float *__restrict__ src, int Ws, float *__restrict__ dst, int Hd, int Wd, float delta) {
    const long long e = (long long)blockIdx.x * TK_THREADS + threadIdx.x;
    if (e >= (long long)Hd * Wd) return;
    const int v = (int)(e / Wd), u = (int)(e % Wd);
    const float *s = src + (size_t)(2 * v) * Ws + 2 * u;
    const float d[4] = {s[0], s[1], s[Ws], s[Ws + 1]};
    float m = 0.f;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (d[k] > 0.f && (!any || d[k] < m)) m = d[k], any = true;
    float sum = 0.f, n = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (d[k] > 0.f && d[k] - m <= delta) sum = sum + d[k], n = n + 1.f;
    dst[e] = any ? sum / n : 0.f;
}

struct MapCam {
    float fx, fy, cx, cy;
};

__device__ __forceinline__ void tk_vertex(float d, int u, int v, const MapCam &c, float V[3]) {
    V[0] = (d * ((float)u - c.cx)) / c.fx, V[1] = (d * ((float)v - c.cy)) / c.fy, V[2] = d;
}

__global__ __launch_bounds__(TK_THREADS) void frame_maps_kernel(const float *__restrict__ depth, int H, int W, MapCam c, float *__restrict__ vertex,
                                                                float *__restrict__ normal) {
    const long long e = (long long)blockIdx.x * TK_THREADS + threadIdx.x;
    if (e >= (long long)H * W) return;
    const int v = (int)(e / W), u = (int)(e % W);
    const float d = depth[e];
    float V[3], N[3] = {0.f, 0.f, 0.f};
    tk_vertex(d, u, v, c, V);
    if (u + 1 < W && v + 1 < H) {
        const float dr = depth[e + 1], dd = depth[e + W];
        if (d > 0.f && dr > 0.f && dd > 0.f) {
            float A[3], B[3];
            tk_vertex(dr, u + 1, v, c, A);
            tk_vertex(dd, u, v + 1, c, B);
#pragma unroll
            for (int r = 0; r < 3; ++r) A[r] = A[r] - V[r], B[r] = B[r] - V[r];
            const float x = A[1] * B[2] - A[2] * B[1], y = A[2] * B[0] - A[0] * B[2], z = A[0] * B[1] - A[1] * B[0];
            const float len = sqrtf((x * x + y * y) + z * z);
            if (len > 0.f && len < __builtin_inff()) {
                N[0] = x / len, N[1] = y / len, N[2] = z / len;
                const float dot = (N[0] * V[0] + N[1] * V[1]) + N[2] * V[2];
                if (dot > 0.f) N[0] = -N[0], N[1] = -N[1], N[2] = -N[2];
            }
        }
    }
    if (!(d > 0.f)) V[0] = V[1] = V[2] = 0.f;
    vertex[3 * e + 0] = V[0], vertex[3 * e + 1] = V[1], vertex[3 * e + 2] = V[2];
    normal[3 * e + 0] = N[0], normal[3 * e + 1] = N[1], normal[3 * e + 2] = N[2];
}

struct IcpParams {
    double R[9], t[3];    // the estimate, camera-to-world
    double Mi[9], Mt[3];  // the model pose inverted: world-to-model-camera
    double fx, fy, cx, cy;
    double dist, cos_min;
    int H, W, round_mode;
};

// the terms of one pair: 21 of J_i J_j, 6 of J_i r, r r and the pair flag
__device__ __forceinline__ void tk_pair_terms(const double J[6], double r, double term[TK_COLS]) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) term[k++] = J[i] * J[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) term[21 + i] = J[i] * r;
    term[27] = r * r;
    term[28] = 1.0;
}

// the point-to-plane terms of live pixel e < H W into `term`, which comes in as zeros (left so, and false, for a pixel without a pair): shared by hive_icp_step
// and hive_rgbd_icp_step
__device__ __forceinline__ bool icp_geo_terms(const IcpParams &p, long long e, const float *__restrict__ live_v, const float *__restrict__ live_n,
                                              const float *__restrict__ model_v, const float *__restrict__ model_n, double term[TK_COLS]) {
    bool pair = false;
    const double N[3] = {(double)live_n[3 * e], (double)live_n[3 * e + 1], (double)live_n[3 * e + 2]};
    if (N[0] != 0.0 || N[1] != 0.0 || N[2] != 0.0) {
        const double V[3] = {(double)live_v[3 * e], (double)live_v[3 * e + 1], (double)live_v[3 * e + 2]};
        double q[3], n[3], c[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            q[r] = ((p.R[3 * r] * V[0] + p.R[3 * r + 1] * V[1]) + p.R[3 * r + 2] * V[2]) + p.t[r];
            n[r] = (p.R[3 * r] * N[0] + p.R[3 * r + 1] * N[1]) + p.R[3 * r + 2] * N[2];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) c[r] = ((p.Mi[3 * r] * q[0] + p.Mi[3 * r + 1] * q[1]) + p.Mi[3 * r + 2] * q[2]) + p.Mt[r];
        if (c[2] > 0.0) {
            const double su = p.fx * (c[0] / c[2]) + p.cx, sv = p.fy * (c[1] / c[2]) + p.cy;
            const double pu = p.round_mode == HIVE_ROUND_HALF_EVEN ? rint(su) : round(su), pv = p.round_mode == HIVE_ROUND_HALF_EVEN ? rint(sv) : round(sv);
            if (pu >= 0.0 && pu < (double)p.W && pv >= 0.0 && pv < (double)p.H) {  // (NaN: false)
                const size_t m = (size_t)(int)pv * p.W + (size_t)(int)pu;
                const double Nm[3] = {(double)model_n[3 * m], (double)model_n[3 * m + 1], (double)model_n[3 * m + 2]};
                if (Nm[0] != 0.0 || Nm[1] != 0.0 || Nm[2] != 0.0) {
                    const double d[3] = {(double)model_v[3 * m] - q[0], (double)model_v[3 * m + 1] - q[1], (double)model_v[3 * m + 2] - q[2]};
                    const double dist = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
                    const double cosine = (n[0] * Nm[0] + n[1] * Nm[1]) + n[2] * Nm[2];
                    if (dist <= p.dist && cosine >= p.cos_min) {
                        pair = true;
                        const double r = (Nm[0] * d[0] + Nm[1] * d[1]) + Nm[2] * d[2];
                        const double J[6] = {q[1] * Nm[2] - q[2] * Nm[1], q[2] * Nm[0] - q[0] * Nm[2], q[0] * Nm[1] - q[1] * Nm[0], Nm[0], Nm[1], Nm[2]};
                        tk_pair_terms(J, r, term);
                    }
                }
            }
        }
    }
    return pair;
}

// Y / 255 of one u8 [3] pixel, Y the integer luma of the JPEG encoder
__device__ __forceinline__ float tk_gray(const uint8_t *__restrict__ c) {
    const unsigned y = (19595u * c[0] + 38470u * c[1] + 7471u * c[2] + 32768u) >> 16;
    return (float)y / 255.f;
}

// the photometric terms of live pixel e < H W against the model's ray-cast depth and colour into `term`, which comes in as zeros (left so, and false, for a
// pixel that is not kept)
__device__ __forceinline__ bool icp_photo_terms(const IcpParams &p, long long e, const float *__restrict__ live_v, const float *__restrict__ live_i,
                                                const float *__restrict__ model_d, const uint8_t *__restrict__ model_c, double term[TK_COLS]) {
    if (!(live_v[3 * e + 2] > 0.f)) return false;
    const double V[3] = {(double)live_v[3 * e], (double)live_v[3 * e + 1], (double)live_v[3 * e + 2]};
    double q[3], c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = ((p.R[3 * r] * V[0] + p.R[3 * r + 1] * V[1]) + p.R[3 * r + 2] * V[2]) + p.t[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = ((p.Mi[3 * r] * q[0] + p.Mi[3 * r + 1] * q[1]) + p.Mi[3 * r + 2] * q[2]) + p.Mt[r];
    if (!(c[2] > 0.0)) return false;
    const double pu = p.fx * (c[0] / c[2]) + p.cx, pv = p.fy * (c[1] / c[2]) + p.cy;
    const double x0f = floor(pu), y0f = floor(pv);
    if (!(x0f >= 1.0 && x0f <= (double)(p.W - 3) && y0f >= 1.0 && y0f <= (double)(p.H - 3))) return false;  // (NaN: false; H < 4 or W < 4: nothing is kept)
    const int x0 = (int)x0f, y0 = (int)y0f;
    const double a = pu - x0f, b = pv - y0f;
    // the 4 x 4 window (x0 - 1 .. x0 + 2, y0 - 1 .. y0 + 2) without its corners: the cell's four pixels and their neighbours, all inside the picture
    double I[4][4];
    float D[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if ((j == 0 || j == 3) && (i == 0 || i == 3)) {
                I[j][i] = 0.0, D[j][i] = 0.f;
                continue;
            }
            const size_t m = (size_t)(y0 - 1 + j) * p.W + (size_t)(x0 - 1 + i);
            D[j][i] = model_d[m], I[j][i] = (double)tk_gray(model_c + 3 * m);
        }
    double gx[2][2], gy[2][2];
    bool usable = true;
#pragma unroll
    for (int j = 1; j <= 2; ++j)
#pragma unroll
        for (int i = 1; i <= 2; ++i) {
            usable = usable && D[j][i] > 0.f && D[j][i - 1] > 0.f && D[j][i + 1] > 0.f && D[j - 1][i] > 0.f && D[j + 1][i] > 0.f;
            gx[j - 1][i - 1] = 0.5 * (I[j][i + 1] - I[j][i - 1]);
            gy[j - 1][i - 1] = 0.5 * (I[j + 1][i] - I[j - 1][i]);
        }
    if (!usable) return false;
    const double depth_near = (double)(b >= 0.5 ? (a >= 0.5 ? D[2][2] : D[2][1]) : (a >= 0.5 ? D[1][2] : D[1][1]));  // (selects: the window stays in registers)
    if (!(fabs(depth_near - c[2]) <= p.dist)) return false;
    double top, bot;
    top = I[1][1] + a * (I[1][2] - I[1][1]), bot = I[2][1] + a * (I[2][2] - I[2][1]);
    const double Im = top + b * (bot - top);
    top = gx[0][0] + a * (gx[0][1] - gx[0][0]), bot = gx[1][0] + a * (gx[1][1] - gx[1][0]);
    const double sgx = top + b * (bot - top);
    top = gy[0][0] + a * (gy[0][1] - gy[0][0]), bot = gy[1][0] + a * (gy[1][1] - gy[1][0]);
    const double sgy = top + b * (bot - top);
    const double r = (double)live_i[e] - Im;
    const double gfx = sgx * p.fx, gfy = sgy * p.fy;
    const double gc[3] = {gfx / c[2], gfy / c[2], -((gfx * c[0] + gfy * c[1]) / (c[2] * c[2]))};
    double gw[3];  // R_m g_c: R_m is the transpose of Mi
#pragma unroll
    for (int k = 0; k < 3; ++k) gw[k] = (p.Mi[k] * gc[0] + p.Mi[3 + k] * gc[1]) + p.Mi[6 + k] * gc[2];
    const double J[6] = {q[1] * gw[2] - q[2] * gw[1], q[2] * gw[0] - q[0] * gw[2], q[0] * gw[1] - q[1] * gw[0], gw[0], gw[1], gw[2]};
    tk_pair_terms(J, r, term);
    return true;
}

// the workgroup's TK_COLS sums of `term` into `row`
__device__ __forceinline__ void tk_block_sums(double (*red)[TK_THREADS], const double term[TK_COLS], double *__restrict__ row) {
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < TK_COLS; ++q) red[q][t] = term[q];
    block_tree_sum<TK_THREADS, TK_COLS>(red);
    if (t < TK_COLS) row[t] = red[t][0];
}

__global__ __launch_bounds__(TK_THREADS) void icp_terms_kernel(IcpParams p, const float *__restrict__ live_v, const float *__restrict__ live_n,
                                                               const float *__restrict__ model_v, const float *__restrict__ model_n, double *__restrict__ partials,
                                                               uint8_t *__restrict__ pair_mask) {
    __shared__ double red[TK_COLS][TK_THREADS];
    const long long e = (long long)blockIdx.x * TK_THREADS + threadIdx.x, n_px = (long long)p.H * p.W;
    double term[TK_COLS];
#pragma unroll
    for (int q = 0; q < TK_COLS; ++q) term[q] = 0.0;
    if (e < n_px) {
        const bool pair = icp_geo_terms(p, e, live_v, live_n, model_v, model_n, term);
        if (pair_mask) pair_mask[e] = pair ? 1 : 0;
    }
    tk_block_sums(red, term, partials + (size_t)blockIdx.x * TK_COLS);
}

// both terms in one pass: a workgroup's row holds the geometric partials, then the photometric ones; the LDS rows are used twice
__global__ __launch_bounds__(TK_THREADS) void rgbd_terms_kernel(IcpParams p, const float *__restrict__ live_v, const float *__restrict__ live_n,
                                                                const float *__restrict__ model_v, const float *__restrict__ model_n,
                                                                const float *__restrict__ live_i, const float *__restrict__ model_d,
                                                                const uint8_t *__restrict__ model_c, double *__restrict__ partials, uint8_t *__restrict__ pair_mask,
                                                                uint8_t *__restrict__ photo_mask) {
    __shared__ double red[TK_COLS][TK_THREADS];
    const long long e = (long long)blockIdx.x * TK_THREADS + threadIdx.x, n_px = (long long)p.H * p.W;
    double *row = partials + (size_t)blockIdx.x * (2 * TK_COLS);
    double term[TK_COLS];
#pragma unroll
    for (int q = 0; q < TK_COLS; ++q) term[q] = 0.0;
    if (e < n_px) {
        const bool pair = icp_geo_terms(p, e, live_v, live_n, model_v, model_n, term);
        if (pair_mask) pair_mask[e] = pair ? 1 : 0;
    }
    tk_block_sums(red, term, row);
    __syncthreads();  // red[.][0] has been read
#pragma unroll
    for (int q = 0; q < TK_COLS; ++q) term[q] = 0.0;
    if (e < n_px) {
        const bool kept = icp_photo_terms(p, e, live_v, live_i, model_d, model_c, term);
        if (photo_mask) photo_mask[e] = kept ? 1 : 0;
    }
    tk_block_sums(red, term, row + TK_COLS);
}

// one workgroup: thread q adds column q (of `cols` <= 64) of the rows in ascending order
__global__ __launch_bounds__(64) void icp_finish_kernel(const double *__restrict__ partials, long long rows, int cols, double *__restrict__ out) {
    const int q = threadIdx.x;
    if (q >= cols) return;
    double acc = 0.0;
    for (long long b = 0; b < rows; ++b) acc = acc + partials[(size_t)b * cols + q];
    out[q] = acc;
}

__global__ __launch_bounds__(TK_THREADS) void gray_kernel(const uint8_t *__restrict__ color, long long n_px, float *__restrict__ gray) {
    const long long e = (long long)blockIdx.x * TK_THREADS + threadIdx.x;
    if (e < n_px) gray[e] = tk_gray(color + 3 * e);
}

__global__ __launch_bounds__(TK_THREADS) void gray_down_kernel(const float *__restrict__ src, int Ws, float *__restrict__ dst, int Hd, int Wd) {
    const long long e = (long long)blockIdx.x * TK_THREADS + threadIdx.x;
    if (e >= (long long)Hd * Wd) return;
    const int v = (int)(e / Wd), u = (int)(e % Wd);
    const float *s = src + (size_t)(2 * v) * Ws + 2 * u;
    dst[e] = ((s[0] + s[1]) + (s[Ws] + s[Ws + 1])) * 0.25f;
}

// hive_icp_step (d_live_gray == NULL: 29 numbers come back) and hive_rgbd_icp_step (58 numbers): one launch pair, one copy
int icp_step_run(hive_ctx *ctx, int H, int W, const float K[9], const float *d_live_vertex, const float *d_live_normal, const float *d_model_vertex,
                 const float *d_model_normal, const float *d_live_gray, const float *d_model_depth, const uint8_t *d_model_color, const double model_pose[16],
                 const double est_pose[16], float dist_thresh, float cos_thresh, double *h_sums, int64_t *h_pairs, uint8_t *d_pair_mask, uint8_t *d_photo_mask) {
    HIVE_REQUIRE(ctx, K && d_live_vertex && d_live_normal && d_model_vertex && d_model_normal && model_pose && est_pose && h_sums && h_pairs,
                 "icp_step: NULL argument");
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && (long long)H * W < (1ll << 31), "icp_step: bad image size %d x %d", H, W);
    HIVE_REQUIRE(ctx, dist_thresh >= 0.f, "icp_step: dist_thresh must be >= 0");
    const int terms = d_live_gray ? 2 : 1, cols = terms * TK_COLS;
    IcpParams p;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) p.R[3 * r + c] = est_pose[4 * r + c], p.Mi[3 * r + c] = model_pose[4 * c + r];  // the transpose
        p.t[r] = est_pose[4 * r + 3];
    }
    const double mt[3] = {model_pose[3], model_pose[7], model_pose[11]};
    for (int r = 0; r < 3; ++r) p.Mt[r] = -((p.Mi[3 * r] * mt[0] + p.Mi[3 * r + 1] * mt[1]) + p.Mi[3 * r + 2] * mt[2]);
    p.fx = K[0], p.fy = K[4], p.cx = K[2], p.cy = K[5];
    p.dist = dist_thresh, p.cos_min = cos_thresh;
    p.H = H, p.W = W, p.round_mode = ctx->round_mode;
    const long long n_px = (long long)H * W, rows = (n_px + TK_THREADS - 1) / TK_THREADS;
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, (size_t)(rows + 1) * cols * sizeof(double));
    if (rc) return rc;
    double *partials = (double *)ctx->d_scratch, *out = partials + (size_t)rows * cols;
    double *back = nullptr;  // 512 bytes: 58 numbers fit
    if ((rc = hive_pinned_small(ctx, (void **)&back))) return rc;
    if (d_live_gray)
        hipLaunchKernelGGL(rgbd_terms_kernel, dim3((unsigned)rows), dim3(TK_THREADS), 0, ctx->stream, p, d_live_vertex, d_live_normal, d_model_vertex, d_model_normal,
                           d_live_gray, d_model_depth, d_model_color, partials, d_pair_mask, d_photo_mask);
    else
        hipLaunchKernelGGL(icp_terms_kernel, dim3((unsigned)rows), dim3(TK_THREADS), 0, ctx->stream, p, d_live_vertex, d_live_normal, d_model_vertex, d_model_normal,
                           partials, d_pair_mask);
    hipLaunchKernelGGL(icp_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double *)partials, rows, cols, out);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(back, out, cols * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < terms; ++k) {
        memcpy(h_sums + k * TK_SUMS, back + k * TK_COLS, TK_SUMS * sizeof(double));
        h_pairs[k] = (int64_t)back[k * TK_COLS + TK_SUMS];
    }
    return HIVE_OK;
}

}  // namespace

extern "C" {

int hive_frame_maps(hive_ctx *ctx, const float *d_depth, int H, int W, const float K[9], int levels, float pyr_delta, float *d_depth_pyr, float *d_vertex_pyr,
                    float *d_normal_pyr, float *K_levels) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_depth && K && d_depth_pyr && d_vertex_pyr && d_normal_pyr && K_levels, "frame_maps: NULL argument");
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && (long long)H * W < (1ll << 31), "frame_maps: bad image size %d x %d", H, W);
    HIVE_REQUIRE(ctx, levels >= 1 && levels <= TK_MAX_LEVELS, "frame_maps: levels = %d, need 1 .. %d", levels, TK_MAX_LEVELS);
    HIVE_REQUIRE(ctx, (H >> (levels - 1)) > 0 && (W >> (levels - 1)) > 0, "frame_maps: %d x %d has no level %d", H, W, levels - 1);
    HIVE_REQUIRE(ctx, K[0] != 0.f && K[4] != 0.f, "frame_maps: fx and fy must not be 0");
    HIVE_REQUIRE(ctx, pyr_delta >= 0.f, "frame_maps: pyr_delta must be >= 0");
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(d_depth_pyr, d_depth, (size_t)H * W * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    size_t at = 0;
    int h = H, w = W;
    for (int l = 0; l < levels; ++l) {
        if (l > 0) {
            const int hs = h, ws = w;
            const size_t from = at;
            at += (size_t)hs * ws, h = hs / 2, w = ws / 2;
            fx = fx / 2.0, fy = fy / 2.0, cx = (cx - 0.5) / 2.0, cy = (cy - 0.5) / 2.0;
            hipLaunchKernelGGL(pyr_down_kernel, dim3((unsigned)hive_div_up((long long)h * w, TK_THREADS)), dim3(TK_THREADS), 0, ctx->stream, (const float *)(d_depth_pyr + from), ws, d_depth_pyr + at, h,
                               w, pyr_delta);
        }
        float *Kl = K_levels + 9 * l;
        Kl[0] = (float)fx, Kl[1] = 0.f, Kl[2] = (float)cx, Kl[3] = 0.f, Kl[4] = (float)fy, Kl[5] = (float)cy, Kl[6] = 0.f, Kl[7] = 0.f, Kl[8] = 1.f;
        const MapCam c = {Kl[0], Kl[4], Kl[2], Kl[5]};
        hipLaunchKernelGGL(frame_maps_kernel, dim3((unsigned)hive_div_up((long long)h * w, TK_THREADS)), dim3(TK_THREADS), 0, ctx->stream, (const float *)(d_depth_pyr + at), h, w, c,
                           d_vertex_pyr + 3 * at, d_normal_pyr + 3 * at);
    }
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_icp_step(hive_ctx *ctx, int H, int W, const float K[9], const float *d_live_vertex, const float *d_live_normal, const float *d_model_vertex,
                  const float *d_model_normal, const double model_pose[16], const double est_pose[16], float dist_thresh, float cos_thresh, double *h_sums,
                  int64_t *h_pairs, uint8_t *d_pair_mask) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    return icp_step_run(ctx, H, W, K, d_live_vertex, d_live_normal, d_model_vertex, d_model_normal, nullptr, nullptr, nullptr, model_pose, est_pose, dist_thresh,
                        cos_thresh, h_sums, h_pairs, d_pair_mask, nullptr);
}

int hive_rgbd_icp_step(hive_ctx *ctx, int H, int W, const float K[9], const float *d_live_vertex, const float *d_live_normal, const float *d_live_gray,
                       const float *d_model_vertex, const float *d_model_normal, const float *d_model_depth, const uint8_t *d_model_color,
                       const double model_pose[16], const double est_pose[16], float dist_thresh, float cos_thresh, double *h_sums, int64_t *h_pairs,
                       uint8_t *d_pair_mask, uint8_t *d_photo_mask) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_live_gray && d_model_depth && d_model_color, "rgbd_icp_step: NULL argument");
    return icp_step_run(ctx, H, W, K, d_live_vertex, d_live_normal, d_model_vertex, d_model_normal, d_live_gray, d_model_depth, d_model_color, model_pose, est_pose,
                        dist_thresh, cos_thresh, h_sums, h_pairs, d_pair_mask, d_photo_mask);
}

int hive_gray_pyramid(hive_ctx *ctx, const uint8_t *d_color, int H, int W, int levels, float *d_gray_pyr) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_color && d_gray_pyr, "gray_pyramid: NULL argument");
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && (long long)H * W < (1ll << 31), "gray_pyramid: bad image size %d x %d", H, W);
    HIVE_REQUIRE(ctx, levels >= 1 && levels <= TK_MAX_LEVELS, "gray_pyramid: levels = %d, need 1 .. %d", levels, TK_MAX_LEVELS);
    HIVE_REQUIRE(ctx, (H >> (levels - 1)) > 0 && (W >> (levels - 1)) > 0, "gray_pyramid: %d x %d has no level %d", H, W, levels - 1);
    hipLaunchKernelGGL(gray_kernel, dim3((unsigned)hive_div_up((long long)H * W, TK_THREADS)), dim3(TK_THREADS), 0, ctx->stream, d_color, (long long)H * W, d_gray_pyr);
    size_t at = 0;
    int h = H, w = W;
    for (int l = 1; l < levels; ++l) {
        const int ws = w;
        const size_t from = at;
        at += (size_t)h * w, h = h / 2, w = w / 2;
        hipLaunchKernelGGL(gray_down_kernel, dim3((unsigned)hive_div_up((long long)h * w, TK_THREADS)), dim3(TK_THREADS), 0, ctx->stream, (const float *)(d_gray_pyr + from), ws,
                           d_gray_pyr + at, h, w);
    }
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

}  // extern "C"
