// Foreground trajectory smoothing (ForegroundPoseOptimiser, hive/pose_optimisation.py:1618-1711).  gfx950 only.
//
//   hive_fg_centroids  -> centroids[i] = np.mean(point_cloud_from_depth(depth_i, mask_i > 0, K), axis=0)     (:1626-1634, 1654-1657)
//   hive_fts_optimise  -> the Adam loop over the camera poses (:1669-1709), every epoch inside ONE launch
//
// Float64 throughout, compiled without contraction, every sum in a fixed order that depends on the problem alone (never on the device or the launch): results are
// bit-identical from run to run.
//
// Centroids.  Per point the arithmetic of hive_unproject with R = I, t = 0: x_r = d * (Kinv[r][0] * u + Kinv[r][1] * v + Kinv[r][2]).  A frame is cut into tiles of
// 4096 pixels, one workgroup each: a thread adds its 16 pixels (tile + j * 256 + thread, j ascending), the 64 lanes of a wave combine in a butterfly (xor 32, 16,
// .. 1), the four waves in order.  One workgroup per frame then adds the tiles the same way (thread k takes tiles k, k + 256, ..) and divides by the count.
//
// Optimiser.  Parameters p_i = (q_i, t_i), q scalar-last.  With u = q / |q| = (a, s), v = c_i - t_i and the Hamilton product written out,
//   w_i = conj(u) (v, 0) u = (s^2 - a.a) v + 2 (a.v) a - 2 s (a x v),
// the loss of a chunk of m consecutive frames is
//   0.01 * mean_i |gt_i - w_i|  +  0.1 * |t[:-2] - 2 t[1:-1] + t[2:]|_F  +  0.1 * |t[:-1] - t[1:]|_F
// (each temporal term ONE Frobenius norm over the chunk's difference matrix), summed over the chunks; gt_i = w_i at the initial parameters.  Gradients, by hand:
//   g_i   = dL/dw_i = -(0.01 / m) (gt_i - w_i) / |gt_i - w_i|                      (0 where the residual is 0, as torch.norm's)
//   dL/dt = -[(s^2 - a.a) g + 2 (a.g) a + 2 s (a x g)]  +  0.1 / |D2|_F (D2_i - 2 D2_{i-1} + D2_{i-2})  +  0.1 / |D1|_F (D1_i - D1_{i-1})
//   dL/ds = g . (2 s v - 2 (a x v)),   dL/da = -2 (g.v) a + 2 (a.v) g + 2 (g.a) v - 2 s (v x g),   dL/dq = (dL/du - u (u . dL/du)) / |q|
// (D terms that do not exist at a chunk's ends are left out; a term whose norm is 0 contributes 0), then torch.optim.Adam: g += 1e-4 p for EVERY parameter
// (frames of no chunk decay too), m += (1 - b1) (g - m), v = b2 v + (1 - b2) g g, p -= lr / (1 - b1^k) * m / (sqrt(v) / sqrt(1 - b2^k) + eps).
// One workgroup of 1024 threads runs all epochs; per epoch three phases separated by __syncthreads(): per-frame terms, per-chunk sums (one wave per chunk: lanes
// take elements lane, lane + 64, .. in order, then the butterfly), gradients and update.  The state (14 N doubles of moments, 10 N of per-frame terms) is global
// memory that stays in L2.
#include "hive_internal.hpp"
#include "pose_math.hpp"

#include <algorithm>
#include <cmath>

namespace {

// ------------------------------------------------------------------------------------------------ centroids
constexpr int CT_THREADS = 256;
constexpr int CT_PER_THREAD = 16;
constexpr int CT_TILE = CT_THREADS * CT_PER_THREAD;

struct CentroidParams {
    double Kinv[9];
    int H, W, tiles;
};

// grid (tiles, frames): partial[frame][tile] = {sum x, sum y, sum z, count} (counts are exact in a double: < 2^30 pixels)
__global__ __launch_bounds__(CT_THREADS) void centroid_tile_kernel(const float *__restrict__ depth, const uint8_t *__restrict__ mask, CentroidParams p,
                                                                   double *__restrict__ partial) {
    __shared__ double lds[4][4];
    const long long n = (long long)p.H * p.W;
    const float *d = depth + (size_t)blockIdx.y * n;
    const uint8_t *m = mask + (size_t)blockIdx.y * n;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < CT_PER_THREAD; ++j) {
        const long long i = (long long)blockIdx.x * CT_TILE + j * CT_THREADS + threadIdx.x;
        if (i < n && m[i] && d[i] > 0.0f) {
            const double z = (double)d[i];
            const double pu = (double)(i % p.W), pv = (double)(i / p.W);
            for (int r = 0; r < 3; ++r) s[r] += z * (p.Kinv[3 * r + 0] * pu + p.Kinv[3 * r + 1] * pv + p.Kinv[3 * r + 2]);
            s[3] += 1.0;
        }
    }
    block_butterfly_sum<4>(s, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) partial[((size_t)blockIdx.y * p.tiles + blockIdx.x) * 4 + k] = s[k];
}

// grid (frames): out[frame] = {mean x, mean y, mean z, count}; a frame without a valid object pixel: all 0
__global__ __launch_bounds__(CT_THREADS) void centroid_frame_kernel(const double *__restrict__ partial, int tiles, double *__restrict__ out) {
    __shared__ double lds[4][4];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < tiles; t += CT_THREADS)
        for (int k = 0; k < 4; ++k) s[k] += partial[((size_t)blockIdx.x * tiles + t) * 4 + k];
    block_butterfly_sum<4>(s, lds);
    if (threadIdx.x == 0) {
        const double c = s[3];
        for (int k = 0; k < 3; ++k) out[(size_t)blockIdx.x * 4 + k] = c > 0.0 ? s[k] / c : 0.0;
        out[(size_t)blockIdx.x * 4 + 3] = c;
    }
}

// ------------------------------------------------------------------------------------------------ optimiser
constexpr int FTS_THREADS = 1024;
constexpr int FTS_WAVES = FTS_THREADS / 64;

struct FtsArgs {
    double *params;          // [N][7] in / out
    const double *gt_params; // [N][7] the parameters gt is taken at
    const double *centroids; // [N][3]
    const int *chunk_of;     // [N] chunk of the frame, -1 = none
    const int *chunk_start;  // [C]
    const int *chunk_len;    // [C]
    double *gt;              // [N][3]
    double *terms;           // [N][10]: |residual|, |D1|^2, |D2|^2, D1 (3), D2 (3), unused
    double *chunk_sums;      // [C][4]: |D1|_F, |D2|_F, loss of the chunk, unused
    double *moments;         // [N][14]: first and second moments
    double *losses;          // [epochs + 1]
    double *gradient;        // [N][7] or NULL: dL/dp at the final parameters (no weight decay)
    int N, C, epochs;
    double lr, beta1, beta2, eps, weight_decay;
};

using namespace hive_pose;  // Vec3, Pose, load_pose, rotate_inverse, rotate_forward

// per-frame terms of the loss at the current parameters
__device__ __forceinline__ void fts_terms(const FtsArgs &a) {
    for (int i = threadIdx.x; i < a.N; i += FTS_THREADS) {
        double *out = a.terms + (size_t)i * 10;
        const int c = a.chunk_of[i];
        double rn = 0.0;
        Vec3 d1 = {0.0, 0.0, 0.0}, d2 = {0.0, 0.0, 0.0};
        if (c >= 0) {
            const Pose u = load_pose(a.params + (size_t)i * 7);
            const Vec3 r = load3(a.gt + (size_t)i * 3) - rotate_inverse(u, load3(a.centroids + (size_t)i * 3) - u.t);
            rn = sqrt(dot(r, r));
            const int left = a.chunk_start[c] + a.chunk_len[c] - 1 - i;  // frames of the chunk behind this one
            if (left >= 1) {
                const Vec3 t1 = load3(a.params + (size_t)(i + 1) * 7 + 4);
                d1 = u.t - t1;
                if (left >= 2) d2 = (u.t - 2.0 * t1) + load3(a.params + (size_t)(i + 2) * 7 + 4);
            }
        }
        out[0] = rn;
        out[1] = dot(d1, d1);
        out[2] = dot(d2, d2);
        store3(out + 3, d1);
        store3(out + 6, d2);
    }
}

// per-chunk sums (one wave per chunk), then the loss (wave 0)
__device__ __forceinline__ void fts_chunk_sums(const FtsArgs &a, int slot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < a.C; c += FTS_WAVES) {
        const int start = a.chunk_start[c], m = a.chunk_len[c];
        double sr = 0.0, s1 = 0.0, s2 = 0.0;
        for (int k = lane; k < m; k += 64) {
            const double *t = a.terms + (size_t)(start + k) * 10;
            sr += t[0];
            s1 += t[1];
            s2 += t[2];
        }
        sr = wave_butterfly_sum(sr);
        s1 = wave_butterfly_sum(s1);
        s2 = wave_butterfly_sum(s2);
        if (lane == 0) {
            const double n1 = sqrt(s1), n2 = sqrt(s2);
            a.chunk_sums[(size_t)c * 4 + 0] = n1;
            a.chunk_sums[(size_t)c * 4 + 1] = n2;
            a.chunk_sums[(size_t)c * 4 + 2] = (0.01 * (sr / (double)m) + 0.1 * n2) + 0.1 * n1;
        }
    }
    __syncthreads();
    if (wave == 0) {
        double s = 0.0;
        for (int c = lane; c < a.C; c += 64) s += a.chunk_sums[(size_t)c * 4 + 2];
        s = wave_butterfly_sum(s);
        if (lane == 0) a.losses[slot] = s;
    }
}

// dL/dp of frame i (its terms and its chunk's sums are current)
__device__ __forceinline__ void fts_gradient(const FtsArgs &a, int i, double g[7]) {
    for (int k = 0; k < 7; ++k) g[k] = 0.0;
    const int c = a.chunk_of[i];
    if (c < 0) return;
    const double *terms = a.terms + (size_t)i * 10;
    const int start = a.chunk_start[c], m = a.chunk_len[c];
    const int pos = i - start;
    const Pose u = load_pose(a.params + (size_t)i * 7);
    Vec3 gt = {0.0, 0.0, 0.0};
    const double rn = terms[0];
    if (rn > 0.0) {
        const Vec3 v = load3(a.centroids + (size_t)i * 3) - u.t;
        const Vec3 r = load3(a.gt + (size_t)i * 3) - rotate_inverse(u, v);
        const Vec3 gw = (-(0.01 / (double)m) / rn) * r;
        gt = -1.0 * rotate_forward(u, gw);
        const double gs = dot(gw, (2.0 * u.s) * v - 2.0 * cross(u.a, v));
        const Vec3 ga = (((-2.0 * dot(gw, v)) * u.a + (2.0 * dot(u.a, v)) * gw) + (2.0 * dot(gw, u.a)) * v) - (2.0 * u.s) * cross(v, gw);
        const double radial = dot(u.a, ga) + u.s * gs;
        g[0] = (ga.x - u.a.x * radial) / u.norm;
        g[1] = (ga.y - u.a.y * radial) / u.norm;
        g[2] = (ga.z - u.a.z * radial) / u.norm;
        g[3] = (gs - u.s * radial) / u.norm;
    }
    const double n1 = a.chunk_sums[(size_t)c * 4 + 0], n2 = a.chunk_sums[(size_t)c * 4 + 1];
    if (n2 > 0.0) {  // D2_j = t_j - 2 t_{j+1} + t_{j+2} exists for j = start .. start + m - 3
        Vec3 acc = {0.0, 0.0, 0.0};
        if (pos <= m - 3) acc = acc + load3(terms + 6);
        if (pos >= 1 && pos <= m - 2) acc = acc - 2.0 * load3(terms - 10 + 6);
        if (pos >= 2) acc = acc + load3(terms - 20 + 6);
        gt = gt + (0.1 / n2) * acc;
    }
    if (n1 > 0.0) {  // D1_j = t_j - t_{j+1} exists for j = start .. start + m - 2
        Vec3 acc = {0.0, 0.0, 0.0};
        if (pos <= m - 2) acc = acc + load3(terms + 3);
        if (pos >= 1) acc = acc - load3(terms - 10 + 3);
        gt = gt + (0.1 / n1) * acc;
    }
    g[4] = gt.x;
    g[5] = gt.y;
    g[6] = gt.z;
}

__global__ __launch_bounds__(FTS_THREADS) void fts_kernel(FtsArgs a) {
    for (int i = threadIdx.x; i < a.N; i += FTS_THREADS) {  // gt = conj(u) (c - t, 0) u at gt_params, every frame
        const Pose u = load_pose(a.gt_params + (size_t)i * 7);
        store3(a.gt + (size_t)i * 3, rotate_inverse(u, load3(a.centroids + (size_t)i * 3) - u.t));
    }
    __syncthreads();
    double b1k = 1.0, b2k = 1.0;  // beta^k
    for (int epoch = 0; epoch < a.epochs; ++epoch) {
        fts_terms(a);
        __syncthreads();
        fts_chunk_sums(a, epoch);
        __syncthreads();
        b1k *= a.beta1;
        b2k *= a.beta2;
        const double step = a.lr / (1.0 - b1k), root2 = sqrt(1.0 - b2k);
        for (int i = threadIdx.x; i < a.N; i += FTS_THREADS) {
            double g[7];
            fts_gradient(a, i, g);
            double *p = a.params + (size_t)i * 7, *mom = a.moments + (size_t)i * 14;
            for (int k = 0; k < 7; ++k) {
                const double gk = g[k] + a.weight_decay * p[k];
                const double m1 = mom[k] + (1.0 - a.beta1) * (gk - mom[k]);
                const double m2 = a.beta2 * mom[7 + k] + (1.0 - a.beta2) * (gk * gk);
                mom[k] = m1;
                mom[7 + k] = m2;
                g[k] = p[k] - step * (m1 / (sqrt(m2) / root2 + a.eps));
            }
            for (int k = 0; k < 7; ++k) p[k] = g[k];
        }
        __syncthreads();
    }
    fts_terms(a);  // the loss (and, on request, its gradient) at the final parameters
    __syncthreads();
    fts_chunk_sums(a, a.epochs);
    __syncthreads();
    if (a.gradient)
        for (int i = threadIdx.x; i < a.N; i += FTS_THREADS) {
            double g[7];
            fts_gradient(a, i, g);
            for (int k = 0; k < 7; ++k) a.gradient[(size_t)i * 7 + k] = g[k];
        }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int hive_fg_centroids(hive_ctx *ctx, const float *d_depth, const uint8_t *d_mask, int n_frames, int H, int W, const double Kinv[9], double *out_centroids,
                      int64_t *out_counts) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_depth && d_mask && Kinv && out_centroids && out_counts, "fg_centroids: NULL argument");
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && (long long)H * W < (1ll << 30), "fg_centroids: bad image size %dx%d", H, W);
    HIVE_REQUIRE(ctx, n_frames >= 0 && n_frames <= 65535, "fg_centroids: %d frames (at most 65535 per call)", n_frames);
    if (n_frames == 0) return HIVE_OK;
    CentroidParams p;
    memcpy(p.Kinv, Kinv, sizeof(p.Kinv));
    p.H = H;
    p.W = W;
    p.tiles = (int)(((long long)H * W + CT_TILE - 1) / CT_TILE);
    const size_t off_out = align256((size_t)n_frames * p.tiles * 4 * 8);
    int rc;
    if ((rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, off_out + (size_t)n_frames * 4 * 8))) return rc;
    double *partial = (double *)ctx->d_scratch, *d_out = (double *)((char *)ctx->d_scratch + off_out);
    hipLaunchKernelGGL(centroid_tile_kernel, dim3(p.tiles, n_frames), dim3(CT_THREADS), 0, ctx->stream, d_depth, d_mask, p, partial);
    hipLaunchKernelGGL(centroid_frame_kernel, dim3(n_frames), dim3(CT_THREADS), 0, ctx->stream, (const double *)partial, p.tiles, d_out);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    std::vector<double> back((size_t)n_frames * 4);
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(back.data(), d_out, back.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n_frames; ++i) {
        for (int k = 0; k < 3; ++k) out_centroids[3 * i + k] = back[4 * (size_t)i + k];
        out_counts[i] = (int64_t)back[4 * (size_t)i + 3];
    }
    return HIVE_OK;
}

int hive_fts_optimise(hive_ctx *ctx, double *params, const double *gt_params, const double *centroids, int n_frames, const int32_t *chunk_start,
                      const int32_t *chunk_len, int n_chunks, double learning_rate, int num_epochs, double *losses, double *gradient) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, params && centroids && losses, "fts_optimise: NULL argument");
    HIVE_REQUIRE(ctx, n_frames > 0 && n_frames <= (1 << 20), "fts_optimise: bad frame count %d", n_frames);
    HIVE_REQUIRE(ctx, n_chunks >= 0 && (n_chunks == 0 || (chunk_start && chunk_len)), "fts_optimise: bad chunk list");
    HIVE_REQUIRE(ctx, num_epochs >= 0 && num_epochs <= (1 << 20), "fts_optimise: bad epoch count %d", num_epochs);
    const int N = n_frames, C = n_chunks;
    std::vector<int32_t> chunk_of((size_t)N, -1);
    int prev_end = 0;
    for (int c = 0; c < C; ++c) {  // ascending, disjoint, inside the trajectory, at least 3 frames (the temporal terms need them)
        HIVE_REQUIRE(ctx, chunk_len[c] >= 3 && chunk_start[c] >= prev_end && (long long)chunk_start[c] + chunk_len[c] <= N,
                     "fts_optimise: chunk %d = [%d, +%d) is out of order, too short or outside the %d frames", c, chunk_start[c], chunk_len[c], N);
        prev_end = chunk_start[c] + chunk_len[c];
        for (int i = chunk_start[c]; i < prev_end; ++i) chunk_of[(size_t)i] = c;
    }
    // scratch: params | gt_params | centroids | chunk_of | chunk_start | chunk_len | gt | terms | chunk sums | moments | losses | gradient
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return at;
    };
    const size_t o_params = take((size_t)N * 56), o_gtp = take((size_t)N * 56), o_cent = take((size_t)N * 24), o_of = take((size_t)N * 4);
    const size_t o_start = take((size_t)std::max(C, 1) * 4), o_len = take((size_t)std::max(C, 1) * 4), o_gt = take((size_t)N * 24);
    const size_t o_terms = take((size_t)N * 80), o_sums = take((size_t)std::max(C, 1) * 32), o_mom = take((size_t)N * 112);
    const size_t o_loss = take((size_t)(num_epochs + 1) * 8), o_grad = take((size_t)N * 56);
    int rc;
    if ((rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, off))) return rc;
    char *base = (char *)ctx->d_scratch;
    if ((rc = hive_upload(ctx, base + o_params, params, (size_t)N * 56))) return rc;
    if (gt_params && (rc = hive_upload(ctx, base + o_gtp, gt_params, (size_t)N * 56))) return rc;
    if ((rc = hive_upload(ctx, base + o_cent, centroids, (size_t)N * 24))) return rc;
    if ((rc = hive_upload(ctx, base + o_of, chunk_of.data(), (size_t)N * 4))) return rc;
    if (C && (rc = hive_upload(ctx, base + o_start, chunk_start, (size_t)C * 4))) return rc;
    if (C && (rc = hive_upload(ctx, base + o_len, chunk_len, (size_t)C * 4))) return rc;
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(base + o_mom, 0, (size_t)N * 112, ctx->stream));
    FtsArgs a;
    a.params = (double *)(base + o_params);
    a.gt_params = gt_params ? (const double *)(base + o_gtp) : a.params;
    a.centroids = (const double *)(base + o_cent);
    a.chunk_of = (const int *)(base + o_of);
    a.chunk_start = (const int *)(base + o_start);
    a.chunk_len = (const int *)(base + o_len);
    a.gt = (double *)(base + o_gt);
    a.terms = (double *)(base + o_terms);
    a.chunk_sums = (double *)(base + o_sums);
    a.moments = (double *)(base + o_mom);
    a.losses = (double *)(base + o_loss);
    a.gradient = gradient ? (double *)(base + o_grad) : nullptr;
    a.N = N;
    a.C = C;
    a.epochs = num_epochs;
    a.lr = learning_rate;
    a.beta1 = 0.9;
    a.beta2 = 0.999;
    a.eps = 1e-8;
    a.weight_decay = 1e-4;
    hipLaunchKernelGGL(fts_kernel, dim3(1), dim3(FTS_THREADS), 0, ctx->stream, a);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(params, a.params, (size_t)N * 56, hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(losses, a.losses, (size_t)(num_epochs + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (gradient) HIVE_CHECK_HIP(ctx, hipMemcpyAsync(gradient, a.gradient, (size_t)N * 56, hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return HIVE_OK;
}

}  // extern "C"
