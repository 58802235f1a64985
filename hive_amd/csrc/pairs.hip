// The front half of hive/pose_optimisation.py's FeatureExtractor (:437-578) behind hive_sift_detect: the exact 2-nearest-neighbour match over an arbitrary list
// of picture pairs, the ratio-and-depth filter with its order-preserving compaction, a homography RANSAC in the place of cv2.findHomography(..., USAC_MAGSAC) and
// the second compaction by its inlier mask.  gfx950 only.  The rules are stated in include/hive_mi355x.h above hive_pairs_match and restated in numpy in
// tests/ransac_restatement.py.  cv2's USAC_MAGSAC is randomised and absent: the RANSAC here is a stated rule of its own and is not pinned against cv2.
//
//   match     rule `knn` (knn_match_kernel of knn_core.hpp, the kernel sift.hip launches too) between the two pictures a pair names
//   filter    a query survives when both pictures have min_features keypoints, not (double) d0 > ratio * (double) d1, and the depth at both rounded positions
//             is not 0; survivors keep the query order (a workgroup scan, no atomic decides an order)
//   RANSAC    float64, one rounding per operation (the Makefile's EXACT flags): Hartley normalisation of both sides with lane-order sums; `trials` minimal
//             samples drawn by lowbias32 of (seed, frame pair, trial, draw); an 8 x 8 elimination with partial pivoting; the integer count of forward transfer
//             errors within the threshold; the winner by one 64-bit integer atomic maximum of count << 32 | (0xFFFFFFFF - trial); one least-squares refit
//   compact   the rows of every kept pair, in pair order, inliers in row order
//
// Kernels: knn_match_kernel (knn_core.hpp: one thread per query), pair_filter_kernel (one workgroup per pair), ransac_norm_kernel (one wave per pair), ransac_trial_kernel (one
// lane per trial; the pair's normalised points go through LDS in chunks, every lane reads the same address), ransac_finish_kernel (one wave per pair),
// pair_offsets_kernel (one workgroup), pair_compact_kernel (one workgroup per pair).  No floating-point atomic: the same bits on every run and at every place.
#include <cmath>

#include "hive_internal.hpp"
#include "knn_core.hpp"
#include "ransac_core.hpp"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_ROW_WORDS = 8;       // x_i, y_i, x_j, y_j, depth_i, depth_j (f32); query index, train index (i32)
constexpr int RS_CHUNK = 512;         // normalised points staged at a time: 16 KiB of LDS
constexpr int RS_NORM_WORDS = 8;      // cx_i, cy_i, s_i, cx_j, cy_j, s_j, ok (1 / 0), unused
constexpr int RS_SUMS = 44;           // the upper triangle of the 8 x 8 normal equations and their right-hand side
constexpr double RS_EPS = 0x1p-40;    // a pivot with |a| <= 2^-40 rejects: normalised coordinates are of order 1

// depth at the rounded position, clamped into the picture
__device__ __forceinline__ float pr_depth_at(const float *__restrict__ depth, int H, int W, float x, float y) {
    const int r = (int)fminf(fmaxf(rintf(y), 0.0f), (float)(H - 1)), c = (int)fminf(fmaxf(rintf(x), 0.0f), (float)(W - 1));
    return depth[(size_t)r * W + c];
}

// grid (P): the filter and its compaction
__global__ __launch_bounds__(PR_THREADS) void pair_filter_kernel(const float *__restrict__ kps, const unsigned *__restrict__ counts, const int32_t *__restrict__ pairs,
                                                                 int N, int stride, const int32_t *__restrict__ idx, const float *__restrict__ dist,
                                                                 const float *__restrict__ depth, int H, int W, double ratio, int min_features,
                                                                 float *__restrict__ rows, int32_t *__restrict__ pair_counts) {
    __shared__ unsigned scan[PR_THREADS / 64];
    const int p = blockIdx.x, t = threadIdx.x;
    int pi, pj, Q, T;
    knn_pair(pairs, counts, N, stride, p, pi, pj, Q, T);
    if (min(Q, T) < max(min_features, 2)) Q = 0;
    const float *qk = kps + (size_t)pi * stride * KNN_KP_WORDS, *tk = kps + (size_t)pj * stride * KNN_KP_WORDS;
    const float *di = depth + (size_t)pi * H * W, *dj = depth + (size_t)pj * H * W;
    float *out = rows + (size_t)p * stride * PR_ROW_WORDS;
    unsigned kept = 0, passed = 0;
    for (int q0 = 0; q0 < Q; q0 += PR_THREADS) {
        const int q = q0 + t;
        bool by_ratio = false, keep = false;
        float xi = 0.f, yi = 0.f, xj = 0.f, yj = 0.f, zi = 0.f, zj = 0.f;
        int tr = -1;
        if (q < Q) {
            const size_t at = ((size_t)p * stride + q) * 2;
            tr = idx[at];
            by_ratio = tr >= 0 && idx[at + 1] >= 0 && !((double)dist[at] > ratio * (double)dist[at + 1]);
            if (by_ratio) {
                xi = qk[(size_t)q * KNN_KP_WORDS], yi = qk[(size_t)q * KNN_KP_WORDS + 1], xj = tk[(size_t)tr * KNN_KP_WORDS], yj = tk[(size_t)tr * KNN_KP_WORDS + 1];
                zi = pr_depth_at(di, H, W, xi, yi), zj = pr_depth_at(dj, H, W, xj, yj);
                keep = zi != 0.0f && zj != 0.0f;
            }
        }
        unsigned all_ratio, all_keep;
        (void)block_exclusive_total(by_ratio ? 1u : 0u, scan, &all_ratio);
        const unsigned at = kept + block_exclusive_total(keep ? 1u : 0u, scan, &all_keep);
        if (keep) {
            float *o = out + (size_t)at * PR_ROW_WORDS;
            o[0] = xi, o[1] = yi, o[2] = xj, o[3] = yj, o[4] = zi, o[5] = zj;
            ((int *)o)[6] = q, ((int *)o)[7] = tr;
        }
        kept += all_keep, passed += all_ratio;
    }
    if (t == 0) pair_counts[2 * p] = (int)passed, pair_counts[2 * p + 1] = (int)kept;
}

// ---- the homography RANSAC: float64, one rounding per operation (the hash, the draw, the count and the lane sum: ransac_core.hpp) ----
struct RsPoint {
    double X, Y, U, V;
};

// a correspondence in the normalised frames
__device__ __forceinline__ RsPoint rs_point(const float *__restrict__ row, const double *__restrict__ nm) {
    RsPoint p;
    p.X = ((double)row[0] - nm[0]) * nm[2], p.Y = ((double)row[1] - nm[1]) * nm[2];
    p.U = ((double)row[2] - nm[3]) * nm[5], p.V = ((double)row[3] - nm[4]) * nm[5];
    return p;
}

// the two equations of a correspondence, h33 = 1: r1 . h = b1, r2 . h = b2
__device__ __forceinline__ void rs_equations(const RsPoint &p, double r1[9], double r2[9]) {
    r1[0] = p.X, r1[1] = p.Y, r1[2] = 1.0, r1[3] = 0.0, r1[4] = 0.0, r1[5] = 0.0, r1[6] = -(p.U * p.X), r1[7] = -(p.U * p.Y), r1[8] = p.U;
    r2[0] = 0.0, r2[1] = 0.0, r2[2] = 0.0, r2[3] = p.X, r2[4] = p.Y, r2[5] = 1.0, r2[6] = -(p.V * p.X), r2[7] = -(p.V * p.Y), r2[8] = p.V;
}

// a[8][9] -> h by elimination with partial pivoting (the largest |a| of the column, the lowest row on a tie; a pivot <= RS_EPS rejects), then back
// substitution.  Every index is static after unrolling: the row exchange is a compare-and-select over the rows below, so the system stays in registers.
__device__ __forceinline__ bool rs_solve8(double a[8][9], double h[8]) {
    bool ok = true;
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        double best = fabs(a[col][col]);
        int piv = col;
#pragma unroll
        for (int r = col + 1; r < 8; ++r) {
            const double v = fabs(a[r][col]);
            if (v > best) best = v, piv = r;
        }
        ok = ok && best > RS_EPS;
#pragma unroll
        for (int r = col + 1; r < 8; ++r) {
            const bool sel = piv == r;
#pragma unroll
            for (int k = col; k < 9; ++k) {
                const double top = a[col][k], low = a[r][k];
                a[col][k] = sel ? low : top, a[r][k] = sel ? top : low;
            }
        }
#pragma unroll
        for (int r = col + 1; r < 8; ++r) {
            const double f = a[r][col] / a[col][col];
#pragma unroll
            for (int k = col + 1; k < 9; ++k) a[r][k] = a[r][k] - f * a[col][k];
        }
    }
#pragma unroll
    for (int r = 7; r >= 0; --r) {
        double acc = a[r][8];
#pragma unroll
        for (int k = r + 1; k < 8; ++k) acc = acc - a[r][k] * h[k];
        h[r] = acc / a[r][r];
    }
    return ok;
}

// the model of the minimal sample of trial t
__device__ __forceinline__ bool rs_minimal(const float *__restrict__ rows, int row_words, const double *__restrict__ nm, unsigned base, unsigned t, int M, double h[8]) {
    int s[4];
    rs_draw(base, t, (unsigned)M, s[0], s[1], s[2], s[3]);
    double a[8][9];
#pragma unroll
    for (int k = 0; k < 4; ++k) rs_equations(rs_point(rows + (size_t)s[k] * row_words, nm), a[2 * k], a[2 * k + 1]);
    return rs_solve8(a, h);
}

// forward transfer error in the normalised target frame within thr2, in front of the camera
__device__ __forceinline__ bool rs_inlier(const double h[8], const RsPoint &p, double thr2) {
    const double w = (h[6] * p.X + h[7] * p.Y) + 1.0;
    const double pu = (h[0] * p.X + h[1] * p.Y) + h[2], pv = (h[3] * p.X + h[4] * p.Y) + h[5];
    const double du = pu / w - p.U, dv = pv / w - p.V;
    const double e2 = du * du + dv * dv;
    return w > 0.0 && e2 <= thr2;
}

// grid (P), one wave: centroid, mean distance and scale of both sides over all M points
__global__ __launch_bounds__(64) void ransac_norm_kernel(const float *__restrict__ rows, int row_words, const int32_t *__restrict__ counts, int count_stride, int stride,
                                                         int need, double *__restrict__ norm) {
    __shared__ double lds[64];
    const int p = blockIdx.x, lane = threadIdx.x, M = rs_count(counts, count_stride, p, stride);
    const float *mine = rows + (size_t)p * stride * row_words;
    double *nm = norm + (size_t)p * RS_NORM_WORDS;
    if (M < need) {
        if (lane < RS_NORM_WORDS) nm[lane] = 0.0;
        return;
    }
    bool ok = true;
    for (int side = 0; side < 2; ++side) {
        double sx = 0.0, sy = 0.0;
        for (int k = lane; k < M; k += 64) sx = sx + (double)mine[(size_t)k * row_words + 2 * side], sy = sy + (double)mine[(size_t)k * row_words + 2 * side + 1];
        const double cx = rs_lane_sum(sx, lds) / (double)M, cy = rs_lane_sum(sy, lds) / (double)M;
        double sd = 0.0;
        for (int k = lane; k < M; k += 64) {
            const double dx = (double)mine[(size_t)k * row_words + 2 * side] - cx, dy = (double)mine[(size_t)k * row_words + 2 * side + 1] - cy;
            sd = sd + sqrt(dx * dx + dy * dy);
        }
        const double m = rs_lane_sum(sd, lds) / (double)M;
        ok = ok && m > 0.0;
        if (lane == 0) nm[3 * side] = cx, nm[3 * side + 1] = cy, nm[3 * side + 2] = 1.4142135623730951 / m;
    }
    if (lane == 0) nm[6] = ok ? 1.0 : 0.0, nm[7] = 0.0;
}

// grid (ceil(trials / 256), P), one lane per trial
__global__ __launch_bounds__(PR_THREADS) void ransac_trial_kernel(const float *__restrict__ rows, int row_words, const int32_t *__restrict__ counts, int count_stride,
                                                                  const int32_t *__restrict__ keys, int stride, int need, const double *__restrict__ norm, double threshold,
                                                                  int trials, unsigned seed, unsigned long long *__restrict__ best) {
    __shared__ double pts[RS_CHUNK][4];
    const int p = blockIdx.y, M = rs_count(counts, count_stride, p, stride);
    const double *nm = norm + (size_t)p * RS_NORM_WORDS;
    if (M < need || nm[6] == 0.0) return;  // the whole workgroup
    const float *mine = rows + (size_t)p * stride * row_words;
    const int t = blockIdx.x * PR_THREADS + threadIdx.x;
    double h[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool live = t < trials;
    if (live) live = rs_minimal(mine, row_words, nm, rs_base(seed, keys + 2 * p), (unsigned)t, M, h);
    const double thr = threshold * nm[5], thr2 = thr * thr;
    unsigned count = 0;
    for (int k0 = 0; k0 < M; k0 += RS_CHUNK) {
        const int n = min(RS_CHUNK, M - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < n; e += PR_THREADS) {
            const RsPoint q = rs_point(mine + (size_t)(k0 + e) * row_words, nm);
            pts[e][0] = q.X, pts[e][1] = q.Y, pts[e][2] = q.U, pts[e][3] = q.V;
        }
        __syncthreads();
        if (live)
            for (int e = 0; e < n; ++e) {
                RsPoint q;
                q.X = pts[e][0], q.Y = pts[e][1], q.U = pts[e][2], q.V = pts[e][3];
                count += rs_inlier(h, q, thr2) ? 1u : 0u;
            }
    }
    unsigned long long key = live ? ((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)t) : 0ull;
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0 && key != 0ull) atomicMax(best + p, key);
}

// grid (P), one wave: the winner's mask, the refit, the re-score, the denormalised H
__global__ __launch_bounds__(64) void ransac_finish_kernel(const float *__restrict__ rows, int row_words, const int32_t *__restrict__ counts, int count_stride,
                                                           const int32_t *__restrict__ keys, int stride, int need, const double *__restrict__ norm, double threshold,
                                                           unsigned seed, const unsigned long long *__restrict__ best, double *__restrict__ H, uint8_t *__restrict__ mask,
                                                           int32_t *__restrict__ result) {
    __shared__ double part[64][RS_SUMS + 1];
    __shared__ double total[RS_SUMS];
    const int p = blockIdx.x, lane = threadIdx.x, M = rs_count(counts, count_stride, p, stride);
    const double *nm = norm + (size_t)p * RS_NORM_WORDS;
    const float *mine = rows + (size_t)p * stride * row_words;
    uint8_t *mk = mask + (size_t)p * stride;
    const unsigned long long key = best[p];
    if (M < need || nm[6] == 0.0 || key == 0ull) {  // no model
        for (int k = lane; k < stride; k += 64) mk[k] = 0;
        if (lane < 9) H[(size_t)p * 9 + lane] = (double)NAN;
        if (lane == 0) result[3 * p] = M < 0 ? -2 : -1, result[3 * p + 1] = 0, result[3 * p + 2] = 0;
        return;
    }
    const unsigned t = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    const int winner_count = (int)(key >> 32);
    double hw[8], hr[8];
    (void)rs_minimal(mine, row_words, nm, rs_base(seed, keys + 2 * p), t, M, hw);
    const double thr = threshold * nm[5], thr2 = thr * thr;
    double acc[RS_SUMS];
#pragma unroll
    for (int n = 0; n < RS_SUMS; ++n) acc[n] = 0.0;
    for (int k = lane; k < stride; k += 64) {
        bool in = false;
        if (k < M) {
            const RsPoint q = rs_point(mine + (size_t)k * row_words, nm);
            in = rs_inlier(hw, q, thr2);
            if (in) {
                double r1[9], r2[9];
                rs_equations(q, r1, r2);
                int n = 0;
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int b = a; b < 8; ++b, ++n) {
                        acc[n] = acc[n] + r1[a] * r1[b];
                        acc[n] = acc[n] + r2[a] * r2[b];
                    }
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    acc[36 + a] = acc[36 + a] + r1[a] * r1[8];
                    acc[36 + a] = acc[36 + a] + r2[a] * r2[8];
                }
            }
        }
        mk[k] = in ? 1 : 0;
    }
#pragma unroll
    for (int n = 0; n < RS_SUMS; ++n) part[lane][n] = acc[n];
    __syncthreads();
    if (lane < RS_SUMS) {
        double s = 0.0;
        for (int l = 0; l < 64; ++l) s = s + part[l][lane];
        total[lane] = s;
    }
    __syncthreads();
    double a8[8][9];
    {
        int n = 0;
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = a; b < 8; ++b, ++n) a8[a][b] = total[n], a8[b][a] = total[n];
#pragma unroll
        for (int a = 0; a < 8; ++a) a8[a][8] = total[36 + a];
    }
    const bool solved = rs_solve8(a8, hr);
    int refit_count = 0;
    for (int k0 = 0; k0 < M; k0 += 64) {
        const int k = k0 + lane;
        const bool in = solved && k < M && rs_inlier(hr, rs_point(mine + (size_t)min(k, M - 1) * row_words, nm), thr2);
        refit_count += __popcll(__ballot(in));
    }
    const bool refit = solved && refit_count >= winner_count;
    if (refit)
        for (int k = lane; k < M; k += 64) mk[k] = rs_inlier(hr, rs_point(mine + (size_t)k * row_words, nm), thr2) ? 1 : 0;
    if (lane != 0) return;
    double h[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = refit ? hr[k] : hw[k];
    h[8] = 1.0;
    // T_j^-1 (H T_i), then over its h33
    double A[3][3], B[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        A[r][0] = h[3 * r] * nm[2], A[r][1] = h[3 * r + 1] * nm[2];
        A[r][2] = (h[3 * r + 2] - A[r][0] * nm[0]) - A[r][1] * nm[1];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        B[0][c] = A[0][c] / nm[5] + nm[3] * A[2][c];
        B[1][c] = A[1][c] / nm[5] + nm[4] * A[2][c];
        B[2][c] = A[2][c];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) H[(size_t)p * 9 + k] = B[k / 3][k % 3] / B[2][2];
    result[3 * p] = (int)t, result[3 * p + 1] = winner_count, result[3 * p + 2] = refit ? refit_count : winner_count;
}

// one workgroup: kept[p] = the final count of a pair with min_features survivors and inliers, else 0; offsets[p] = the rows before it; offsets[P] = all rows
__global__ __launch_bounds__(PR_THREADS) void pair_offsets_kernel(const int32_t *__restrict__ pair_counts, const int32_t *__restrict__ result, int P, int min_features,
                                                                  int32_t *__restrict__ kept, int64_t *__restrict__ offsets) {
    __shared__ unsigned scan[PR_THREADS / 64];
    long long before = 0;
    for (int p0 = 0; p0 < P; p0 += PR_THREADS) {
        const int p = p0 + threadIdx.x;
        unsigned n = 0;
        if (p < P && pair_counts[2 * p + 1] >= min_features && result[3 * p + 2] >= min_features) n = (unsigned)result[3 * p + 2];
        unsigned all;
        const unsigned at = block_exclusive_total(n, scan, &all);
        if (p < P) kept[p] = (int)n, offsets[p] = before + at;
        before += all;
    }
    if (threadIdx.x == 0) offsets[P] = before;
}

// grid (P): the inlier rows of a kept pair, in row order, at the pair's offset
__global__ __launch_bounds__(PR_THREADS) void pair_compact_kernel(const float *__restrict__ rows, const int32_t *__restrict__ pair_counts, const uint8_t *__restrict__ mask,
                                                                  int stride, const int32_t *__restrict__ kept, const int64_t *__restrict__ offsets,
                                                                  float *__restrict__ out) {
    __shared__ unsigned scan[PR_THREADS / 64];
    const int p = blockIdx.x;
    if (kept[p] == 0) return;
    const int M = min(max(pair_counts[2 * p + 1], 0), stride);
    const uint4 *src = (const uint4 *)(rows + (size_t)p * stride * PR_ROW_WORDS);
    uint4 *dst = (uint4 *)(out + (size_t)offsets[p] * PR_ROW_WORDS);
    unsigned before = 0;
    for (int k0 = 0; k0 < M; k0 += PR_THREADS) {
        const int k = k0 + threadIdx.x;
        const bool in = k < M && mask[(size_t)p * stride + k] != 0;
        unsigned all;
        const unsigned at = before + block_exclusive_total(in ? 1u : 0u, scan, &all);
        if (in && at < (unsigned)kept[p]) dst[2 * (size_t)at] = src[2 * (size_t)k], dst[2 * (size_t)at + 1] = src[2 * (size_t)k + 1];
        before += all;
    }
}

}  // namespace

extern "C" {

int hive_pairs_match(hive_ctx *ctx, const float *d_keypoints, const uint8_t *d_descriptors, const int32_t *d_counts, int capacity, int N, const int32_t *d_pairs, int P,
                     const float *d_depth, int H, int W, double ratio, int min_features, float *d_rows, int32_t *d_pair_counts, int32_t *d_indices, float *d_distances) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_keypoints && d_descriptors && d_counts && d_pairs && d_depth && d_rows && d_pair_counts, "pairs_match: NULL argument");
    HIVE_REQUIRE(ctx, (d_indices == nullptr) == (d_distances == nullptr), "pairs_match: NULL for one half of the 2-NN table; give both or neither");
    HIVE_REQUIRE(ctx, capacity >= 1 && capacity <= 65535 && N >= 1 && N <= 8192, "pairs_match: capacity = %d (1 .. 65535), N = %d pictures (1 .. 8192)", capacity, N);
    HIVE_REQUIRE(ctx, P >= 1 && P <= 65535, "pairs_match: P = %d pairs, need 1 .. 65535", P);
    HIVE_REQUIRE(ctx, H >= 1 && W >= 1 && (long long)H * W < (1ll << 27), "pairs_match: depth maps of %d x %d", H, W);
    HIVE_REQUIRE(ctx, ratio >= 0.0 && min_features >= 0, "pairs_match: ratio = %g and min_features = %d must not be negative", ratio, min_features);
    HIVE_REQUIRE(ctx, (uintptr_t)d_descriptors % 4 == 0 && (uintptr_t)d_rows % 16 == 0, "pairs_match: the descriptors must be 4-byte and the rows 16-byte aligned");
    if (!d_indices) {
        const size_t half = ((size_t)P * capacity * 2 * sizeof(int32_t) + 255) & ~(size_t)255;
        if (int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, 2 * half)) return rc;
        d_indices = (int32_t *)ctx->d_scratch, d_distances = (float *)((char *)ctx->d_scratch + half);
    }
    const KnnArgs a = {d_descriptors, d_descriptors, (const unsigned *)d_counts, d_pairs, N, 0, 0, capacity, 0, 0};
    hipLaunchKernelGGL(knn_match_kernel, dim3((unsigned)hive_div_up(capacity, KNN_TILE), (unsigned)P), dim3(KNN_TILE), 0, ctx->stream, a, d_indices, d_distances);
    hipLaunchKernelGGL(pair_filter_kernel, dim3((unsigned)P), dim3(PR_THREADS), 0, ctx->stream, d_keypoints, (const unsigned *)d_counts, d_pairs, N, capacity, d_indices,
                       d_distances, d_depth, H, W, ratio, min_features, d_rows, d_pair_counts);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_ransac_homography(hive_ctx *ctx, const float *d_rows, int row_words, const int32_t *d_counts, int count_stride, const int32_t *d_keys, int P, int stride,
                           double threshold, int trials, unsigned seed, int min_count, double *d_H, uint8_t *d_mask, int32_t *d_result) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_rows && d_counts && d_keys && d_H && d_mask && d_result, "ransac_homography: NULL argument");
    HIVE_REQUIRE(ctx, P >= 1 && P <= 65535, "ransac_homography: P = %d pairs, need 1 .. 65535", P);
    HIVE_REQUIRE(ctx, stride >= 1 && stride < (1 << 24) && row_words >= 4 && row_words <= 64 && count_stride >= 1,
                 "ransac_homography: stride = %d rows (1 .. 2^24 - 1) of %d words (4 .. 64), counts %d words apart", stride, row_words, count_stride);
    HIVE_REQUIRE(ctx, trials >= 1 && trials <= (1 << 24) && threshold > 0.0, "ransac_homography: trials = %d (1 .. 2^24), threshold = %g (positive)", trials, threshold);
    const int need = min_count > 4 ? min_count : 4;  // fewer correspondences: no model
    const size_t norm_bytes = ((size_t)P * RS_NORM_WORDS * sizeof(double) + 255) & ~(size_t)255, best_bytes = (size_t)P * sizeof(unsigned long long);
    if (int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, norm_bytes + best_bytes)) return rc;
    double *norm = (double *)ctx->d_scratch;
    unsigned long long *best = (unsigned long long *)((char *)ctx->d_scratch + norm_bytes);
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(best, 0, best_bytes, ctx->stream));
    hipLaunchKernelGGL(ransac_norm_kernel, dim3((unsigned)P), dim3(64), 0, ctx->stream, d_rows, row_words, d_counts, count_stride, stride, need, norm);
    hipLaunchKernelGGL(ransac_trial_kernel, dim3((unsigned)hive_div_up(trials, PR_THREADS), (unsigned)P), dim3(PR_THREADS), 0, ctx->stream, d_rows, row_words, d_counts,
                       count_stride, d_keys, stride, need, norm, threshold, trials, seed, best);
    hipLaunchKernelGGL(ransac_finish_kernel, dim3((unsigned)P), dim3(64), 0, ctx->stream, d_rows, row_words, d_counts, count_stride, d_keys, stride, need, norm, threshold, seed,
                       best, d_H, d_mask, d_result);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_pairs_compact(hive_ctx *ctx, const float *d_rows, const int32_t *d_pair_counts, const uint8_t *d_mask, const int32_t *d_result, int P, int stride,
                       int min_features, float *d_out, int32_t *d_kept, int64_t *d_offsets) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_rows && d_pair_counts && d_mask && d_result && d_out && d_kept && d_offsets, "pairs_compact: NULL argument");
    HIVE_REQUIRE(ctx, P >= 1 && P <= 65535 && stride >= 1 && stride <= 65535, "pairs_compact: P = %d pairs, stride = %d rows, need 1 .. 65535 each", P, stride);
    HIVE_REQUIRE(ctx, min_features >= 1, "pairs_compact: min_features = %d, need at least 1", min_features);
    HIVE_REQUIRE(ctx, ((uintptr_t)d_rows | (uintptr_t)d_out) % 16 == 0, "pairs_compact: the rows must be 16-byte aligned");
    hipLaunchKernelGGL(pair_offsets_kernel, dim3(1), dim3(PR_THREADS), 0, ctx->stream, d_pair_counts, d_result, P, min_features, d_kept, d_offsets);
    hipLaunchKernelGGL(pair_compact_kernel, dim3((unsigned)P), dim3(PR_THREADS), 0, ctx->stream, d_rows, d_pair_counts, d_mask, stride, d_kept, d_offsets, d_out);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

}  // extern "C"
