// Frame registration from 3-D feature matches: a rigid (optionally similarity) RANSAC on the back-projected rows of hive_pairs_match, written like the homography
// RANSAC of pairs.hip.  It stands where the reference shells out to COLMAP (estimate_pose) and names BundleFusion ("3D correspondence guided frame
// registration"); both are external programs and absent, as are cv2's estimateAffine3D and Open3D's correspondence RANSAC: the rules are this project's own, stated
// in include/hive_mi355x.h above hive_ransac_rigid and restated in numpy in tests/rigid_restatement.py.  gfx950 only.
//
//   points    with a camera a row's side gives Z = depth, X = ((x - cx) Z) / fx, Y = ((y - cy) Z) / fy; without one a row is X_i Y_i Z_i X_j Y_j Z_j
//   RANSAC    float64, one rounding per operation (the Makefile's EXACT flags): `trials` samples of three correspondences drawn by lowbias32 of (seed, frame
//             pair, trial, draw); near-collinear samples rejected by a scale-free rule; Horn's closed form (the eigenvector of a symmetric 4 x 4 matrix by cyclic
//             Jacobi with a fixed number of sweeps); the integer count of residuals within the threshold; the winner by one 64-bit integer atomic maximum of
//             count << 32 | (0xFFFFFFFF - trial); one refit by the same solver over the winner's inliers from lane-ordered sums
//
// Kernels: rigid_trial_kernel (one lane per trial; the pair's points go through LDS in chunks of 512, every lane reads the same address), rigid_finish_kernel (one
// wave per pair).  No floating-point atomic: the same bits on every run, in every batch and at every place in it.
#include <cmath>

#include "hive_internal.hpp"
#include "ransac_core.hpp"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_CHUNK = 512;   // points staged at a time: 24 KiB of LDS
// Sweeps of the cyclic Jacobi.  Measured on the CPU with the restatement over every committed case (tests/register_cases.py, SWEEPS_MEASURED): after 5 sweeps the
// off-diagonal norm is at most 2^-52 of the matrix's Frobenius norm on all of them; two more.
constexpr int RG_SWEEPS = 7;
constexpr double RG_DEGENERATE = 0x1p-20;

struct RgCamera {
    double fx, fy, cx, cy;
    int on;
};

struct RgModel {
    double A[9], t[3], scale;  // A = scale R, row-major
};

// both sides of a correspondence
__device__ __forceinline__ void rg_point(const float *__restrict__ row, const RgCamera &cam, double p[3], double q[3]) {
    if (cam.on) {
        const double zi = (double)row[4], zj = (double)row[5];
        p[0] = (((double)row[0] - cam.cx) * zi) / cam.fx, p[1] = (((double)row[1] - cam.cy) * zi) / cam.fy, p[2] = zi;
        q[0] = (((double)row[2] - cam.cx) * zj) / cam.fx, q[1] = (((double)row[3] - cam.cy) * zj) / cam.fy, q[2] = zj;
    } else {
        p[0] = (double)row[0], p[1] = (double)row[1], p[2] = (double)row[2];
        q[0] = (double)row[3], q[1] = (double)row[4], q[2] = (double)row[5];
    }
}

__device__ __forceinline__ double rg_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// rule `degenerate` for one side
__device__ __forceinline__ bool rg_degenerate(const double p0[3], const double p1[3], const double p2[3]) {
    const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    return rg_dot(n, n) <= (RG_DEGENERATE * rg_dot(e1, e1)) * rg_dot(e2, e2);
}

// the eleven terms of one centred point: p'_a q'_b row-major, |p'|^2, |q'|^2
__device__ __forceinline__ void rg_accumulate(const double dp[3], const double dq[3], double acc[11]) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[3 * a + b] = acc[3 * a + b] + dp[a] * dq[b];
    acc[9] = acc[9] + rg_dot(dp, dp);
    acc[10] = acc[10] + rg_dot(dq, dq);
}

__device__ __forceinline__ bool rg_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN

// rule `horn`: centroids, centred sums S[3 a + b] = sum p'_a q'_b, sp = sum |p'|^2, sq = sum |q'|^2 -> the model.  Only the upper triangle of the symmetric
// matrix is kept (10 + 16 doubles with the eigenvectors); every index is static after unrolling, so the state stays in registers.
__device__ __forceinline__ bool rg_horn(const double cp[3], const double cq[3], const double S[11], bool with_scale, RgModel &m) {
    const double xx = S[0], xy = S[1], xz = S[2], yx = S[3], yy = S[4], yz = S[5], zx = S[6], zy = S[7], zz = S[8], sp = S[9], sq = S[10];
    double a[4][4], v[4][4];
    a[0][0] = (xx + yy) + zz, a[1][1] = (xx - yy) - zz, a[2][2] = (yy - xx) - zz, a[3][3] = (zz - xx) - yy;
    a[0][1] = yz - zy, a[0][2] = zx - xz, a[0][3] = xy - yx;
    a[1][2] = xy + yx, a[1][3] = zx + xz, a[2][3] = yz + zy;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < RG_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq != 0.0) {
                    const double app = a[p][p], aqq = a[q][q];
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    a[p][p] = app - t * apq, a[q][q] = aqq + t * apq, a[p][q] = 0.0;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (r != p && r != q) {
                            double &rp = a[r < p ? r : p][r < p ? p : r], &rq = a[r < q ? r : q][r < q ? q : r];
                            const double arp = rp, arq = rq;
                            rp = c * arp - s * arq, rq = s * arp + c * arq;
                        }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double vrp = v[r][p], vrq = v[r][q];
                        v[r][p] = c * vrp - s * vrq, v[r][q] = s * vrp + c * vrq;
                    }
                }
            }
    }
    // the eigenvector of the largest diagonal entry, the lowest index on a tie
    double best = a[0][0], w = v[0][0], x = v[1][0], y = v[2][0], z = v[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool sel = a[k][k] > best;
        best = sel ? a[k][k] : best;
        w = sel ? v[0][k] : w, x = sel ? v[1][k] : x, y = sel ? v[2][k] : y, z = sel ? v[3][k] : z;
    }
    const double first = x != 0.0 ? x : (y != 0.0 ? y : z);
    const double sg = (w < 0.0 || (w == 0.0 && first < 0.0)) ? -1.0 : 1.0;
    w = sg * w, x = sg * x, y = sg * y, z = sg * z;
    const double n = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / n, x = x / n, y = y / n, z = z / n;
    double R[9];
    R[0] = ((w * w + x * x) - y * y) - z * z, R[1] = 2.0 * (x * y - w * z), R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z), R[4] = ((w * w - x * x) + y * y) - z * z, R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y), R[7] = 2.0 * (y * z + w * x), R[8] = ((w * w - x * x) - y * y) + z * z;
    m.scale = with_scale ? sqrt(sq / sp) : 1.0;
    bool ok = sp != 0.0 && sq != 0.0 && rg_finite(sp) && rg_finite(sq) && rg_finite(m.scale);
#pragma unroll
    for (int k = 0; k < 9; ++k) m.A[k] = m.scale * R[k], ok = ok && rg_finite(m.A[k]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        m.t[r] = cq[r] - ((m.A[3 * r] * cp[0] + m.A[3 * r + 1] * cp[1]) + m.A[3 * r + 2] * cp[2]);
        ok = ok && rg_finite(m.t[r]);
    }
    return ok;
}

// the model of the minimal sample of trial t
__device__ __forceinline__ bool rg_minimal(const float *__restrict__ rows, int row_words, const RgCamera &cam, unsigned base, unsigned t, int M, bool with_scale, RgModel &m) {
    int s[3];
    rs_draw3(base, t, (unsigned)M, s[0], s[1], s[2]);
    double p[3][3], q[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) rg_point(rows + (size_t)s[k] * row_words, cam, p[k], q[k]);
    const bool bad = rg_degenerate(p[0], p[1], p[2]) || rg_degenerate(q[0], q[1], q[2]);
    double cp[3], cq[3], acc[11];
#pragma unroll
    for (int a = 0; a < 3; ++a) cp[a] = ((p[0][a] + p[1][a]) + p[2][a]) / 3.0, cq[a] = ((q[0][a] + q[1][a]) + q[2][a]) / 3.0;
#pragma unroll
    for (int n = 0; n < 11; ++n) acc[n] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double dp[3] = {p[k][0] - cp[0], p[k][1] - cp[1], p[k][2] - cp[2]}, dq[3] = {q[k][0] - cq[0], q[k][1] - cq[1], q[k][2] - cq[2]};
        rg_accumulate(dp, dq, acc);
    }
    const bool ok = rg_horn(cp, cq, acc, with_scale, m);
    return ok && !bad;
}

// rule `inlier`: d . d of d = (A p + t) - q
__device__ __forceinline__ double rg_dist2(const RgModel &m, const double p[3], const double q[3]) {
    double d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = (((m.A[3 * r] * p[0] + m.A[3 * r + 1] * p[1]) + m.A[3 * r + 2] * p[2]) + m.t[r]) - q[r];
    return rg_dot(d, d);
}

__device__ __forceinline__ bool rg_inlier_row(const RgModel &m, const float *__restrict__ row, const RgCamera &cam, double thr2, double *d2 = nullptr) {
    double p[3], q[3];
    rg_point(row, cam, p, q);
    const double e = rg_dist2(m, p, q);
    if (d2) *d2 = e;
    return e <= thr2;  // false for NaN
}

// grid (ceil(trials / 256), P), one lane per trial
__global__ __launch_bounds__(RG_THREADS) void rigid_trial_kernel(const float *__restrict__ rows, int row_words, const int32_t *__restrict__ counts, int count_stride,
                                                                 const int32_t *__restrict__ keys, int stride, int need, RgCamera cam, double threshold, int trials,
                                                                 unsigned seed, int with_scale, unsigned long long *__restrict__ best) {
    __shared__ double pts[RG_CHUNK][6];
    const int p = blockIdx.y, M = rs_count(counts, count_stride, p, stride);
    if (M < need) return;  // the whole workgroup
    const float *mine = rows + (size_t)p * stride * row_words;
    const int t = blockIdx.x * RG_THREADS + threadIdx.x;
    RgModel m;
#pragma unroll
    for (int k = 0; k < 9; ++k) m.A[k] = 0.0;
    m.t[0] = m.t[1] = m.t[2] = 0.0, m.scale = 0.0;
    bool live = t < trials;
    if (live) live = rg_minimal(mine, row_words, cam, rs_base(seed, keys + 2 * p), (unsigned)t, M, with_scale != 0, m);
    const double thr2 = threshold * threshold;
    unsigned count = 0;
    for (int k0 = 0; k0 < M; k0 += RG_CHUNK) {
        const int n = min(RG_CHUNK, M - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < n; e += RG_THREADS) {
            double a[3], b[3];
            rg_point(mine + (size_t)(k0 + e) * row_words, cam, a, b);
            pts[e][0] = a[0], pts[e][1] = a[1], pts[e][2] = a[2], pts[e][3] = b[0], pts[e][4] = b[1], pts[e][5] = b[2];
        }
        __syncthreads();
        if (live)
            for (int e = 0; e < n; ++e) {
                const double a[3] = {pts[e][0], pts[e][1], pts[e][2]}, b[3] = {pts[e][3], pts[e][4], pts[e][5]};
                count += rg_dist2(m, a, b) <= thr2 ? 1u : 0u;
            }
    }
    unsigned long long key = live ? ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)t) : 0ull;
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0 && key != 0ull) atomicMax(best + p, key);
}

// grid (P), one wave: the winner's mask, the refit in two passes, the re-score, T, scale and rms
__global__ __launch_bounds__(64) void rigid_finish_kernel(const float *__restrict__ rows, int row_words, const int32_t *__restrict__ counts, int count_stride,
                                                          const int32_t *__restrict__ keys, int stride, int need, RgCamera cam, double threshold, unsigned seed,
                                                          int with_scale, const unsigned long long *__restrict__ best, double *__restrict__ T, double *__restrict__ scale,
                                                          double *__restrict__ rms, uint8_t *__restrict__ mask, int32_t *__restrict__ result) {
    __shared__ double lds[64];
    const int p = blockIdx.x, lane = threadIdx.x, M = rs_count(counts, count_stride, p, stride);
    const float *mine = rows + (size_t)p * stride * row_words;
    uint8_t *mk = mask + (size_t)p * stride;
    const unsigned long long key = best[p];
    if (M < need || key == 0ull) {  // no model
        for (int k = lane; k < stride; k += 64) mk[k] = 0;
        if (lane < 16) T[(size_t)p * 16 + lane] = (double)NAN;
        if (lane == 0) scale[p] = (double)NAN, rms[p] = (double)NAN, result[3 * p] = M < 0 ? -2 : -1, result[3 * p + 1] = 0, result[3 * p + 2] = 0;
        return;
    }
    const unsigned t = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    const int winner_count = (int)(key >> 32);
    RgModel mw, mr;
    (void)rg_minimal(mine, row_words, cam, rs_base(seed, keys + 2 * p), t, M, with_scale != 0, mw);
    const double thr2 = threshold * threshold;
    // pass 1: the winner's mask and the centroids of its inliers
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int n_in = 0;
    for (int k = lane; k < stride; k += 64) {
        bool in = false;
        if (k < M) {
            double a[3], b[3];
            rg_point(mine + (size_t)k * row_words, cam, a, b);
            in = rg_dist2(mw, a, b) <= thr2;
            if (in) {
#pragma unroll
                for (int r = 0; r < 3; ++r) c[r] = c[r] + a[r], c[3 + r] = c[3 + r] + b[r];
                ++n_in;
            }
        }
        mk[k] = in ? 1 : 0;
    }
    for (int off = 32; off >= 1; off >>= 1) n_in += __shfl_xor(n_in, off);
    double cp[3], cq[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cp[r] = rs_lane_sum(c[r], lds) / (double)n_in, cq[r] = rs_lane_sum(c[3 + r], lds) / (double)n_in;
    // pass 2: the centred sums
    double acc[11], total[11];
#pragma unroll
    for (int n = 0; n < 11; ++n) acc[n] = 0.0;
    for (int k = lane; k < M; k += 64) {
        double a[3], b[3];
        rg_point(mine + (size_t)k * row_words, cam, a, b);
        if (rg_dist2(mw, a, b) <= thr2) {
            const double dp[3] = {a[0] - cp[0], a[1] - cp[1], a[2] - cp[2]}, dq[3] = {b[0] - cq[0], b[1] - cq[1], b[2] - cq[2]};
            rg_accumulate(dp, dq, acc);
        }
    }
#pragma unroll
    for (int n = 0; n < 11; ++n) total[n] = rs_lane_sum(acc[n], lds);
    const bool solved = rg_horn(cp, cq, total, with_scale != 0, mr);
    int refit_count = 0;
    for (int k0 = 0; k0 < M; k0 += 64) {
        const int k = k0 + lane;
        const bool in = solved && k < M && rg_inlier_row(mr, mine + (size_t)min(k, M - 1) * row_words, cam, thr2);
        refit_count += __popcll(__ballot(in));
    }
    const bool refit = solved && refit_count >= winner_count;
    const RgModel &m = refit ? mr : mw;
    const int final_count = refit ? refit_count : winner_count;
    double e2 = 0.0;
    for (int k = lane; k < M; k += 64) {
        double d2;
        const bool in = rg_inlier_row(m, mine + (size_t)k * row_words, cam, thr2, &d2);
        if (refit) mk[k] = in ? 1 : 0;
        if (in) e2 = e2 + d2;
    }
    const double sum2 = rs_lane_sum(e2, lds);
    if (lane != 0) return;
    double *out = T + (size_t)p * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) out[4 * r] = m.A[3 * r], out[4 * r + 1] = m.A[3 * r + 1], out[4 * r + 2] = m.A[3 * r + 2], out[4 * r + 3] = m.t[r];
    out[12] = 0.0, out[13] = 0.0, out[14] = 0.0, out[15] = 1.0;
    scale[p] = m.scale, rms[p] = sqrt(sum2 / (double)final_count);
    result[3 * p] = (int)t, result[3 * p + 1] = winner_count, result[3 * p + 2] = final_count;
}

}  // namespace

extern "C" {

int hive_ransac_rigid(hive_ctx *ctx, const float *d_rows, int row_words, const int32_t *d_counts, int count_stride, const int32_t *d_keys, int P, int stride,
                      const double *camera, double threshold, int trials, unsigned seed, int min_count, int with_scale, double *d_T, double *d_scale, double *d_rms,
                      uint8_t *d_mask, int32_t *d_result) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_rows && d_counts && d_keys && d_T && d_scale && d_rms && d_mask && d_result, "ransac_rigid: NULL argument");
    HIVE_REQUIRE(ctx, P >= 1 && P <= 65535, "ransac_rigid: P = %d pairs, need 1 .. 65535", P);
    HIVE_REQUIRE(ctx, stride >= 1 && stride < (1 << 24) && row_words >= 6 && row_words <= 64 && count_stride >= 1,
                 "ransac_rigid: stride = %d rows (1 .. 2^24 - 1) of %d words (6 .. 64), counts %d words apart", stride, row_words, count_stride);
    HIVE_REQUIRE(ctx, trials >= 1 && trials <= (1 << 24) && threshold > 0.0, "ransac_rigid: trials = %d (1 .. 2^24), threshold = %g (positive)", trials, threshold);
    RgCamera cam = {1.0, 1.0, 0.0, 0.0, 0};
    if (camera) {
        cam = {camera[0], camera[1], camera[2], camera[3], 1};
        HIVE_REQUIRE(ctx, std::isfinite(cam.fx) && std::isfinite(cam.fy) && cam.fx != 0.0 && cam.fy != 0.0 && std::isfinite(cam.cx) && std::isfinite(cam.cy),
                     "ransac_rigid: camera fx = %g, fy = %g (finite, not 0), cx = %g, cy = %g (finite)", cam.fx, cam.fy, cam.cx, cam.cy);
    }
    const int need = min_count > 3 ? min_count : 3;  // fewer correspondences: no model
    const size_t best_bytes = (size_t)P * sizeof(unsigned long long);
    if (int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, best_bytes)) return rc;
    unsigned long long *best = (unsigned long long *)ctx->d_scratch;
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(best, 0, best_bytes, ctx->stream));
    hipLaunchKernelGGL(rigid_trial_kernel, dim3((unsigned)hive_div_up(trials, RG_THREADS), (unsigned)P), dim3(RG_THREADS), 0, ctx->stream, d_rows, row_words, d_counts,
                       count_stride, d_keys, stride, need, cam, threshold, trials, seed, with_scale, best);
    hipLaunchKernelGGL(rigid_finish_kernel, dim3((unsigned)P), dim3(64), 0, ctx->stream, d_rows, row_words, d_counts, count_stride, d_keys, stride, need, cam, threshold, seed,
                       with_scale, best, d_T, d_scale, d_rms, d_mask, d_result);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

}  // extern "C"
