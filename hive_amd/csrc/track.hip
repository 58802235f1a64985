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

__global__ __launch_bounds__(TK_THREADS) void icp_terms_kernel(IcpParams p, const float *__restrict__ live_v, const float *__restrict__ live_n,
                                                               const float *__restrict__ model_v, const float *__restrict__ model_n, double *__restrict__ partials,
                                                               uint8_t *__restrict__ pair_mask) {
    __shared__ double red[TK_COLS][TK_THREADS];
    const int t = threadIdx.x;
    const long long e = (long long)blockIdx.x * TK_THREADS + t, n_px = (long long)p.H * p.W;
    double term[TK_COLS];
#pragma unroll
    for (int q = 0; q < TK_COLS; ++q) term[q] = 0.0;
    bool pair = false;
    if (e < n_px) {
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
                    }
                }
            }
        }
        if (pair_mask) pair_mask[e] = pair ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < TK_COLS; ++q) red[q][t] = term[q];
    block_tree_sum<TK_THREADS, TK_COLS>(red);
    if (t < TK_COLS) partials[(size_t)blockIdx.x * TK_COLS + t] = red[t][0];
}

// one workgroup: thread q adds column q of the rows in ascending order
__global__ __launch_bounds__(64) void icp_finish_kernel(const double *__restrict__ partials, long long rows, double *__restrict__ out) {
    const int q = threadIdx.x;
    if (q >= TK_COLS) return;
    double acc = 0.0;
    for (long long b = 0; b < rows; ++b) acc = acc + partials[(size_t)b * TK_COLS + q];
    out[q] = acc;
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
    HIVE_REQUIRE(ctx, K && d_live_vertex && d_live_normal && d_model_vertex && d_model_normal && model_pose && est_pose && h_sums && h_pairs,
                 "icp_step: NULL argument");
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && (long long)H * W < (1ll << 31), "icp_step: bad image size %d x %d", H, W);
    HIVE_REQUIRE(ctx, dist_thresh >= 0.f, "icp_step: dist_thresh must be >= 0");
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
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, (size_t)(rows + 1) * TK_COLS * sizeof(double));
    if (rc) return rc;
    double *partials = (double *)ctx->d_scratch, *out = partials + (size_t)rows * TK_COLS;
    double *back = nullptr;
    if ((rc = hive_pinned_small(ctx, (void **)&back))) return rc;
    hipLaunchKernelGGL(icp_terms_kernel, dim3((unsigned)rows), dim3(TK_THREADS), 0, ctx->stream, p, d_live_vertex, d_live_normal, d_model_vertex, d_model_normal,
                       partials, d_pair_mask);
    hipLaunchKernelGGL(icp_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, (const double *)partials, rows, out);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(back, out, TK_COLS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(h_sums, back, TK_SUMS * sizeof(double));
    *h_pairs = (int64_t)back[TK_SUMS];
    return HIVE_OK;
}

}  // extern "C"
