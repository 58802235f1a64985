// The fourth score of a render, MIFD (scripts/compare_image_pair.py:44-97): SIFT keypoints and descriptors of gray pictures, the exact 2-nearest-neighbour
// descriptor match, Lowe's ratio test and the mean distance between matched keypoint positions, on the device.  gfx950 only.  The detector is also the front
// half of hive/pose_optimisation.py's FeatureExtractor (:294, :426, :452).  The rules are stated in include/hive_mi355x.h above hive_sift_create and restated
// in numpy float32 in tests/sift_restatement.py; in short:
//
//   pyramid   gray -> float32, x2 bilinear (exact), octaves of nOctaveLayers + 3 Gaussian layers, each a separable blur of the previous one (row pass, then
//             column pass, one launch through an LDS tile with its halo; reflect-101 folded as often as needed; taps from the caller, products added in
//             ascending tap order), the next octave every second sample of layer nOctaveLayers
//   detect    DoG = layer differences taken where they are read; 26-neighbour extrema above the threshold, refined by up to 5 steps of the 3-D quadratic fit
//             (float32 elimination with partial pivoting); contrast, edge and mask tests; atomic append of the survivors
//   orient    one wave per candidate: 36-bin histogram, lane-private partials added in lane order, [1 4 6 4 1] / 16, every peak >= 0.8 max
//   order     keypoints ranked by (x, y, size, angle, response, octave), exact duplicates dropped: the output does not depend on the append order
//   describe  one wave per keypoint: 4 x 4 x 8 bins, lane-private partials added in lane order, clip at 0.2 norm, 512 / norm, bytes
//   match     squared L2 distances of byte descriptors as exact integers (packed byte dot products), the two nearest, ties to the lower train index
//
// atan2, exp, sin and cos are stated float32 polynomials (sift_atan2_deg, sift_exp, sift_sincos_deg): no library transcendental is called.  Float32 without
// contraction (the Makefile's EXACT flags); sqrt and / are correctly rounded.  No floating-point atomic: the same bits on every run, at every batch size and place.
//
// Kernels: sift_base_kernel (one thread per doubled pixel), sift_blur_kernel (one workgroup per 32 x 32 tile, per picture), sift_half_kernel, sift_detect_kernel
// (one thread per pixel, layer and picture), sift_orient_kernel and sift_describe_kernel (one wave per candidate / keypoint), sift_rank_kernel and
// sift_unique_kernel (one thread per keypoint), knn_match_kernel (knn_core.hpp: one thread per query), mifd_kernel (one thread per pair).
#include <cfloat>
#include <cmath>

#include "hive_internal.hpp"
#include "knn_core.hpp"

namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_TILE = 32;
constexpr int SF_MAX_RADIUS = 16;  // 33 taps: nOctaveLayers = 3, sigma = 1.6 needs 13
constexpr int SF_MAX_TAPS = 2 * SF_MAX_RADIUS + 1;
constexpr int SF_IN = SF_TILE + 2 * SF_MAX_RADIUS;
constexpr int SF_MAX_OCTAVES = 16;
constexpr int SF_BORDER = 5;
constexpr int SF_STEPS = 5;
constexpr int SF_ORI_BINS = 36;
constexpr int SF_D = 4, SF_N = 8;
static_assert(SF_D * SF_D * SF_N == KNN_DESC, "the matcher reads the descriptors the detector writes");
constexpr int SF_CAND_WORDS = 8;  // x, y, size, response (f32); packed octave, layer, r, c (i32)

struct SfTaps {
    float g[SF_MAX_TAPS];
    int n;
};

// ---- the stated polynomials: float32, one rounding per operation ----
// exp(x) for -87 <= x <= 88: n = rint(x log2 e), r = x - n ln2_hi - n ln2_lo (n ln2_hi is exact: ln2_hi has 15 significant bits), the degree-7 Taylor
// polynomial of exp(r) by Horner's rule, then ldexp
__device__ __forceinline__ float sift_exp(float x) {
    x = x < -87.0f ? -87.0f : x;
    const float n = rintf(x * (float)1.4426950408889634);
    float r = x - n * (float)0.693145751953125;
    r = r - n * (float)1.42860682030941723212e-6;
    float p = (float)(1.0 / 5040.0);
    p = p * r + (float)(1.0 / 720.0);
    p = p * r + (float)(1.0 / 120.0);
    p = p * r + (float)(1.0 / 24.0);
    p = p * r + (float)(1.0 / 6.0);
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    return ldexpf(p, (int)n);
}

// atan2(y, x) in degrees, [0, 360]: cv2's fastAtan2 form, an odd degree-7 polynomial in min / max with the octant fix-ups
__device__ __forceinline__ float sift_atan2_deg(float y, float x) {
    const float p1 = (float)(0.9997878412794807 * 57.29577951308232), p3 = (float)(-0.3258083974640975 * 57.29577951308232);
    const float p5 = (float)(0.1555786518463281 * 57.29577951308232), p7 = (float)(-0.04432655554792128 * 57.29577951308232);
    const float ax = fabsf(x), ay = fabsf(y);
    float a;
    if (ax >= ay) {
        const float c = ay / (ax + (float)2.220446049250313e-16), c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        const float c = ax / (ay + (float)2.220446049250313e-16), c2 = c * c;
        a = 90.0f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0.0f) a = 180.0f - a;
    if (y < 0.0f) a = 360.0f - a;
    return a;
}

// cos and sin of an angle in degrees, 0 <= a <= 360: q = rint(a / 90), r = a - 90 q, t = r pi / 180, Taylor polynomials in t (degrees 10 and 9), quadrant turn
__device__ __forceinline__ void sift_sincos_deg(float a, float *cs, float *sn) {
    const float q = rintf(a * (float)(1.0 / 90.0));
    const float t = (a - q * 90.0f) * (float)(3.141592653589793 / 180.0), t2 = t * t;
    float s = (float)(1.0 / 362880.0);
    s = s * t2 + (float)(-1.0 / 5040.0);
    s = s * t2 + (float)(1.0 / 120.0);
    s = s * t2 + (float)(-1.0 / 6.0);
    s = s * t2 + 1.0f;
    s = s * t;
    float c = (float)(-1.0 / 3628800.0);
    c = c * t2 + (float)(1.0 / 40320.0);
    c = c * t2 + (float)(-1.0 / 720.0);
    c = c * t2 + (float)(1.0 / 24.0);
    c = c * t2 + -0.5f;
    c = c * t2 + 1.0f;
    const int k = (int)q & 3;
    *cs = k == 0 ? c : k == 1 ? -s : k == 2 ? -c : s;
    *sn = k == 0 ? s : k == 1 ? c : k == 2 ? -s : -c;
}

// reflect-101 of any index into [0, n): folded as often as needed
__device__ __forceinline__ int sift_reflect(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int m = i % period;
    if (m < 0) m += period;
    return m < n ? m : period - m;
}

// gray u8 [N][H][W] -> float32 [N][2H][2W]: INTER_LINEAR, source coordinate (d + 0.5) / 2 - 0.5, edge samples replicated; weights 0.25 / 0.75: exact
__global__ __launch_bounds__(SF_THREADS) void sift_base_kernel(const uint8_t *__restrict__ gray, int H, int W, float *__restrict__ out) {
    const int h2 = 2 * H, w2 = 2 * W;
    const long long e = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (e >= (long long)h2 * w2) return;
    const int n = blockIdx.y, r = (int)(e / w2), c = (int)(e % w2);
    const float sy = ((float)r + 0.5f) * 0.5f - 0.5f, sx = ((float)c + 0.5f) * 0.5f - 0.5f;
    const int y0 = (int)floorf(sy), x0 = (int)floorf(sx);
    const float fy = sy - (float)y0, fx = sx - (float)x0;
    const int ya = max(y0, 0), yb = min(y0 + 1, H - 1), xa = max(x0, 0), xb = min(x0 + 1, W - 1);
    const uint8_t *p = gray + (size_t)n * H * W;
    const float top = (float)p[(size_t)ya * W + xa] * (1.0f - fx) + (float)p[(size_t)ya * W + xb] * fx;
    const float bot = (float)p[(size_t)yb * W + xa] * (1.0f - fx) + (float)p[(size_t)yb * W + xb] * fx;
    out[(size_t)n * h2 * w2 + (size_t)e] = top * (1.0f - fy) + bot * fy;
}

// one workgroup per 32 x 32 tile; grid (tiles_x, tiles_y, N).  src / dst: planes of h x w, one picture src_stride / dst_stride floats after the other
__global__ __launch_bounds__(SF_THREADS) void sift_blur_kernel(const float *__restrict__ src, size_t src_stride, float *__restrict__ dst, size_t dst_stride, int h, int w,
                                                               SfTaps taps) {
    __shared__ float in[SF_IN][SF_IN + 1];
    __shared__ float mid[SF_IN][SF_TILE + 1];
    const int t = threadIdx.x, R = taps.n / 2, span = SF_TILE + 2 * R;
    const int i0 = blockIdx.y * SF_TILE, j0 = blockIdx.x * SF_TILE;
    const float *s = src + (size_t)blockIdx.z * src_stride;
    for (int p = t; p < span * span; p += SF_THREADS) {
        const int r = p / span, c = p % span;
        in[r][c] = s[(size_t)sift_reflect(i0 - R + r, h) * w + sift_reflect(j0 - R + c, w)];
    }
    __syncthreads();
    for (int p = t; p < span * SF_TILE; p += SF_THREADS) {  // along the row
        const int r = p / SF_TILE, c = p % SF_TILE;
        float acc = taps.g[0] * in[r][c];
        for (int k = 1; k < taps.n; ++k) acc = acc + taps.g[k] * in[r][c + k];
        mid[r][c] = acc;
    }
    __syncthreads();
    float *d = dst + (size_t)blockIdx.z * dst_stride;
    for (int p = t; p < SF_TILE * SF_TILE; p += SF_THREADS) {  // along the column
        const int r = p / SF_TILE, c = p % SF_TILE;
        if (i0 + r >= h || j0 + c >= w) continue;
        float acc = taps.g[0] * mid[r][c];
        for (int k = 1; k < taps.n; ++k) acc = acc + taps.g[k] * mid[r + k][c];
        d[(size_t)(i0 + r) * w + (j0 + c)] = acc;
    }
}

// every second row and column; grid (blocks, N)
__global__ __launch_bounds__(SF_THREADS) void sift_half_kernel(const float *__restrict__ src, size_t src_stride, int w, float *__restrict__ dst, size_t dst_stride,
                                                               int h2, int w2) {
    const long long e = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (e >= (long long)h2 * w2) return;
    const int r = (int)(e / w2), c = (int)(e % w2);
    dst[(size_t)blockIdx.y * dst_stride + (size_t)e] = src[(size_t)blockIdx.y * src_stride + (size_t)(2 * r) * w + 2 * c];
}

struct SfDetect {
    int octave, h, w, layers;  // layers = nOctaveLayers
    int H, W;                  // the picture
    int capacity;
    float threshold, contrast_threshold, edge_threshold, sigma;
};

// DoG i of a picture's octave (pic: layer 0), i = 0 .. layers + 1
__device__ __forceinline__ float sift_dog(const float *__restrict__ pic, size_t plane, int w, int i, int r, int c) {
    const size_t at = (size_t)r * w + c;
    return pic[(size_t)(i + 1) * plane + at] - pic[(size_t)i * plane + at];
}

// X = H^-1 b by elimination with partial pivoting (the largest |a| of the column, the lowest row on a tie); false on a zero pivot
__device__ __forceinline__ bool sift_solve3(float a[3][4], float X[3]) {
#pragma unroll
    for (int col = 0; col < 3; ++col) {
        int piv = col;
#pragma unroll
        for (int rr = col + 1; rr < 3; ++rr)
            if (fabsf(a[rr][col]) > fabsf(a[piv][col])) piv = rr;
        if (a[piv][col] == 0.0f) return false;
        if (piv != col) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float tmp = a[col][k];
                a[col][k] = a[piv][k], a[piv][k] = tmp;
            }
        }
#pragma unroll
        for (int rr = col + 1; rr < 3; ++rr) {
            const float f = a[rr][col] / a[col][col];
#pragma unroll
            for (int k = col + 1; k < 4; ++k) a[rr][k] = a[rr][k] - f * a[col][k];
        }
    }
    X[2] = a[2][3] / a[2][2];
    X[1] = (a[1][3] - a[1][2] * X[2]) / a[1][1];
    X[0] = (a[0][3] - a[0][1] * X[1] - a[0][2] * X[2]) / a[0][0];
    return true;
}

// grid (ceil(h w / 256), N * layers)
__global__ __launch_bounds__(SF_THREADS) void sift_detect_kernel(const float *__restrict__ gauss, size_t pic_stride, SfDetect a, const uint8_t *__restrict__ mask,
                                                                 unsigned *__restrict__ counts, float *__restrict__ cand) {
    const long long e = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (e >= (long long)a.h * a.w) return;
    const int n = blockIdx.y / a.layers;
    int layer = 1 + blockIdx.y % a.layers, r = (int)(e / a.w), c = (int)(e % a.w);
    const int h = a.h, w = a.w;
    if (r < SF_BORDER || r >= h - SF_BORDER || c < SF_BORDER || c >= w - SF_BORDER) return;
    const float *pic = gauss + (size_t)n * pic_stride;
    const size_t plane = (size_t)h * w;
    const float val = sift_dog(pic, plane, w, layer, r, c);
    if (!(fabsf(val) > a.threshold)) return;
    bool is_max = val > 0.0f, is_min = val < 0.0f;
    for (int dl = -1; dl <= 1 && (is_max || is_min); ++dl)
        for (int dr = -1; dr <= 1; ++dr)
            for (int dc = -1; dc <= 1; ++dc) {
                const float v = sift_dog(pic, plane, w, layer + dl, r + dr, c + dc);
                is_max = is_max && val >= v, is_min = is_min && val <= v;
            }
    if (!is_max && !is_min) return;

    const float img_scale = (float)(1.0 / 255.0), deriv_scale = img_scale * 0.5f, cross_scale = img_scale * 0.25f;
    float xi = 0.0f, xr = 0.0f, xc = 0.0f;
    int step = 0;
    for (; step < SF_STEPS; ++step) {
#define D(l, y, x) sift_dog(pic, plane, w, (l), (y), (x))
        const float v2 = D(layer, r, c) * 2.0f;
        const float dxx = (D(layer, r, c + 1) + D(layer, r, c - 1) - v2) * img_scale, dyy = (D(layer, r + 1, c) + D(layer, r - 1, c) - v2) * img_scale;
        const float dss = (D(layer + 1, r, c) + D(layer - 1, r, c) - v2) * img_scale;
        const float dxy = (D(layer, r + 1, c + 1) - D(layer, r + 1, c - 1) - D(layer, r - 1, c + 1) + D(layer, r - 1, c - 1)) * cross_scale;
        const float dxs = (D(layer + 1, r, c + 1) - D(layer + 1, r, c - 1) - D(layer - 1, r, c + 1) + D(layer - 1, r, c - 1)) * cross_scale;
        const float dys = (D(layer + 1, r + 1, c) - D(layer + 1, r - 1, c) - D(layer - 1, r + 1, c) + D(layer - 1, r - 1, c)) * cross_scale;
        float m[3][4] = {{dxx, dxy, dxs, (D(layer, r, c + 1) - D(layer, r, c - 1)) * deriv_scale},
                         {dxy, dyy, dys, (D(layer, r + 1, c) - D(layer, r - 1, c)) * deriv_scale},
                         {dxs, dys, dss, (D(layer + 1, r, c) - D(layer - 1, r, c)) * deriv_scale}};
        float X[3];
        if (!sift_solve3(m, X)) return;
        xc = -X[0], xr = -X[1], xi = -X[2];
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
        const float big = 536870912.0f;  // 2^29; a NaN fails too
        if (!(fabsf(xi) <= big && fabsf(xr) <= big && fabsf(xc) <= big)) return;
        c += (int)rintf(xc), r += (int)rintf(xr), layer += (int)rintf(xi);
        if (layer < 1 || layer > a.layers || c < SF_BORDER || c >= w - SF_BORDER || r < SF_BORDER || r >= h - SF_BORDER) return;
    }
    if (step >= SF_STEPS) return;
    const float d0 = (D(layer, r, c + 1) - D(layer, r, c - 1)) * deriv_scale, d1 = (D(layer, r + 1, c) - D(layer, r - 1, c)) * deriv_scale;
    const float d2 = (D(layer + 1, r, c) - D(layer - 1, r, c)) * deriv_scale;
    const float tdot = d0 * xc + d1 * xr + d2 * xi;
    const float contr = D(layer, r, c) * img_scale + tdot * 0.5f;
    if (fabsf(contr) * (float)a.layers < a.contrast_threshold) return;
    const float v2 = D(layer, r, c) * 2.0f;
    const float dxx = (D(layer, r, c + 1) + D(layer, r, c - 1) - v2) * img_scale, dyy = (D(layer, r + 1, c) + D(layer, r - 1, c) - v2) * img_scale;
    const float dxy = (D(layer, r + 1, c + 1) - D(layer, r + 1, c - 1) - D(layer, r - 1, c + 1) + D(layer, r - 1, c - 1)) * cross_scale;
#undef D
    const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
    if (det <= 0.0f || tr * tr * a.edge_threshold >= (a.edge_threshold + 1.0f) * (a.edge_threshold + 1.0f) * det) return;
    const float oct_scale = (float)(1 << a.octave);
    const float x = ((float)c + xc) * oct_scale, y = ((float)r + xr) * oct_scale;
    const int packed = a.octave + (layer << 8) + ((int)rintf((xi + 0.5f) * 255.0f) << 16);
    const float size = a.sigma * sift_exp((((float)layer + xi) / (float)a.layers) * (float)0.6931471805599453) * oct_scale * 2.0f;
    if (mask) {  // the rounded position in the picture: the base is doubled
        const int mx = min(max((int)(x * 0.5f + 0.5f), 0), a.W - 1), my = min(max((int)(y * 0.5f + 0.5f), 0), a.H - 1);
        if (mask[(size_t)n * a.H * a.W + (size_t)my * a.W + mx] == 0) return;
    }
    const unsigned slot = atomicAdd(counts + 3 * n, 1u);
    if (slot >= (unsigned)a.capacity) return;  // counted, not stored: the caller reads the count
    float *o = cand + ((size_t)n * a.capacity + slot) * SF_CAND_WORDS;
    o[0] = x, o[1] = y, o[2] = size, o[3] = fabsf(contr);
    ((int *)o)[4] = packed, ((int *)o)[5] = layer, ((int *)o)[6] = r, ((int *)o)[7] = c;
}

struct SfPyramid {
    const float *gauss[SF_MAX_OCTAVES];
    int h[SF_MAX_OCTAVES], w[SF_MAX_OCTAVES];
    int octaves, layers;  // layers = nOctaveLayers
};

// one wave per candidate; grid (capacity, N)
__global__ __launch_bounds__(64) void sift_orient_kernel(SfPyramid pyr, const float *__restrict__ cand, int capacity, int nfeatures, unsigned *__restrict__ counts,
                                                         float *__restrict__ raw) {
    __shared__ float part[64][SF_ORI_BINS + 1];
    __shared__ float tmp[SF_ORI_BINS], hist[SF_ORI_BINS];
    __shared__ int greater;
    const int lane = threadIdx.x, n = blockIdx.y;
    const int total = (int)min(counts[3 * n], (unsigned)capacity);
    if ((int)blockIdx.x >= total) return;
    const float *all = cand + (size_t)n * capacity * SF_CAND_WORDS, *me = all + (size_t)blockIdx.x * SF_CAND_WORDS;
    if (nfeatures > 0) {  // retainBest: the nfeatures largest responses and whatever equals the last of them
        if (lane == 0) greater = 0;
        __syncthreads();
        int g = 0;
        for (int j = lane; j < total; j += 64) g += all[(size_t)j * SF_CAND_WORDS + 3] > me[3] ? 1 : 0;
        if (g) atomicAdd(&greater, g);
        __syncthreads();
        if (greater >= nfeatures) return;
    }
    const int packed = ((const int *)me)[4], o = packed & 255, layer = ((const int *)me)[5], r = ((const int *)me)[6], c = ((const int *)me)[7];
    const int h = pyr.h[o], w = pyr.w[o];
    const float *img = pyr.gauss[o] + ((size_t)n * (pyr.layers + 3) + layer) * h * w;
    const float scl = me[2] * 0.5f / (float)(1 << o);
    const int radius = (int)rintf(4.5f * scl);
    const float sigma = 1.5f * scl, exp_scale = -1.0f / (2.0f * sigma * sigma);
    for (int b = 0; b < SF_ORI_BINS; ++b) part[lane][b] = 0.0f;
    const int len = 2 * radius + 1;
    for (int p = lane; p < len * len; p += 64) {
        const int i = p / len - radius, j = p % len - radius, y = r + i, x = c + j;
        if (y <= 0 || y >= h - 1 || x <= 0 || x >= w - 1) continue;
        const float dx = img[(size_t)y * w + x + 1] - img[(size_t)y * w + x - 1], dy = img[(size_t)(y - 1) * w + x] - img[(size_t)(y + 1) * w + x];
        const float wgt = sift_exp((float)(i * i + j * j) * exp_scale);
        const float ori = sift_atan2_deg(dy, dx), mag = sqrtf(dx * dx + dy * dy);
        int bin = (int)rintf((float)(36.0 / 360.0) * ori);
        if (bin >= SF_ORI_BINS) bin -= SF_ORI_BINS;
        if (bin < 0) bin += SF_ORI_BINS;
        part[lane][bin] = part[lane][bin] + wgt * mag;
    }
    __syncthreads();
    if (lane < SF_ORI_BINS) {
        float acc = 0.0f;
        for (int l = 0; l < 64; ++l) acc = acc + part[l][lane];
        tmp[lane] = acc;
    }
    __syncthreads();
    if (lane < SF_ORI_BINS) {
        const int b = lane, m2 = (b + SF_ORI_BINS - 2) % SF_ORI_BINS, m1 = (b + SF_ORI_BINS - 1) % SF_ORI_BINS, p1 = (b + 1) % SF_ORI_BINS, p2 = (b + 2) % SF_ORI_BINS;
        hist[b] = (tmp[m2] + tmp[p2]) * (1.0f / 16.0f) + (tmp[m1] + tmp[p1]) * (4.0f / 16.0f) + tmp[b] * (6.0f / 16.0f);
    }
    __syncthreads();
    if (lane != 0) return;
    float omax = hist[0];
    for (int b = 1; b < SF_ORI_BINS; ++b) omax = fmaxf(omax, hist[b]);
    const float mag_thr = omax * 0.8f;
    for (int j = 0; j < SF_ORI_BINS; ++j) {
        const int l = j > 0 ? j - 1 : SF_ORI_BINS - 1, r2 = j < SF_ORI_BINS - 1 ? j + 1 : 0;
        if (!(hist[j] > hist[l] && hist[j] > hist[r2] && hist[j] >= mag_thr)) continue;
        float bin = (float)j + 0.5f * (hist[l] - hist[r2]) / (hist[l] - 2.0f * hist[j] + hist[r2]);
        bin = bin < 0.0f ? (float)SF_ORI_BINS + bin : bin >= (float)SF_ORI_BINS ? bin - (float)SF_ORI_BINS : bin;
        float angle = 360.0f - (float)(360.0 / SF_ORI_BINS) * bin;
        if (fabsf(angle - 360.0f) < FLT_EPSILON) angle = 0.0f;
        const unsigned slot = atomicAdd(counts + 3 * n + 1, 1u);
        if (slot >= (unsigned)capacity) continue;
        float *k = raw + ((size_t)n * capacity + slot) * KNN_KP_WORDS;
        // the first octave is -1: positions and size halve, the octave byte becomes (o - 1) & 255
        k[0] = me[0] * 0.5f, k[1] = me[1] * 0.5f, k[2] = me[2] * 0.5f, k[3] = angle, k[4] = me[3];
        k[5] = (float)((packed & ~255) | ((packed - 1) & 255));
    }
}

// -1, 0, 1: the order of (x, y, size, angle, response, octave)
__device__ __forceinline__ int sift_key_cmp(const float *a, const float *b) {
#pragma unroll
    for (int k = 0; k < KNN_KP_WORDS; ++k) {
        if (a[k] < b[k]) return -1;
        if (a[k] > b[k]) return 1;
    }
    return 0;
}

// sorted[rank(i)] = raw[i], rank by the key, then by the slot; grid (ceil(capacity / 256), N)
__global__ __launch_bounds__(SF_THREADS) void sift_rank_kernel(const float *__restrict__ raw, int capacity, const unsigned *__restrict__ counts,
                                                               float *__restrict__ sorted) {
    const int n = blockIdx.y, i = blockIdx.x * SF_THREADS + threadIdx.x;
    const int total = (int)min(counts[3 * n + 1], (unsigned)capacity);
    if (i >= total) return;
    const float *base = raw + (size_t)n * capacity * KNN_KP_WORDS;
    float me[KNN_KP_WORDS];
    for (int k = 0; k < KNN_KP_WORDS; ++k) me[k] = base[(size_t)i * KNN_KP_WORDS + k];
    int rank = 0;
    for (int j = 0; j < total; ++j) {
        const int cmp = sift_key_cmp(base + (size_t)j * KNN_KP_WORDS, me);
        rank += (cmp < 0 || (cmp == 0 && j < i)) ? 1 : 0;
    }
    float *o = sorted + ((size_t)n * capacity + rank) * KNN_KP_WORDS;
    for (int k = 0; k < KNN_KP_WORDS; ++k) o[k] = me[k];
}

// drops every keypoint equal to the one before it; grid (ceil(capacity / 256), N)
__global__ __launch_bounds__(SF_THREADS) void sift_unique_kernel(const float *__restrict__ sorted, int capacity, unsigned *__restrict__ counts, float *__restrict__ out) {
    const int n = blockIdx.y, i = blockIdx.x * SF_THREADS + threadIdx.x;
    const int total = (int)min(counts[3 * n + 1], (unsigned)capacity);
    if (total == 0 && i == 0) counts[3 * n + 2] = 0;
    if (i >= total) return;
    const float *base = sorted + (size_t)n * capacity * KNN_KP_WORDS;
    int before = 0;
    for (int j = 1; j <= i; ++j) before += sift_key_cmp(base + (size_t)j * KNN_KP_WORDS, base + (size_t)(j - 1) * KNN_KP_WORDS) != 0 ? 1 : 0;
    const bool first = i == 0 || sift_key_cmp(base + (size_t)i * KNN_KP_WORDS, base + (size_t)(i - 1) * KNN_KP_WORDS) != 0;
    // `before` counts the distinct keys among 1 .. i; slot 0 is always distinct
    const int slot = first ? (i == 0 ? 0 : before) : -1;
    if (slot >= 0)
        for (int k = 0; k < KNN_KP_WORDS; ++k) out[((size_t)n * capacity + slot) * KNN_KP_WORDS + k] = base[(size_t)i * KNN_KP_WORDS + k];
    if (i == total - 1) counts[3 * n + 2] = (unsigned)(before + 1);
}

// one wave per keypoint; grid (capacity, N)
__global__ __launch_bounds__(64) void sift_describe_kernel(SfPyramid pyr, const float *__restrict__ kps, int capacity, const unsigned *__restrict__ counts,
                                                           uint8_t *__restrict__ desc) {
    __shared__ float part[64][KNN_DESC + 1];
    __shared__ float dst[KNN_DESC];
    const int lane = threadIdx.x, n = blockIdx.y;
    if (blockIdx.x >= counts[3 * n + 2]) return;
    const float *kp = kps + ((size_t)n * capacity + blockIdx.x) * KNN_KP_WORDS;
    const int packed = (int)kp[5], ob = packed & 255, layer = (packed >> 8) & 255;
    const int octave = ob < 128 ? ob : ob - 256, o = octave + 1;
    const float scale = ldexpf(1.0f, -octave);
    const float px = kp[0] * scale, py = kp[1] * scale, scl = kp[2] * scale * 0.5f;
    float ori = 360.0f - kp[3];
    if (fabsf(ori - 360.0f) < FLT_EPSILON) ori = 0.0f;
    const int h = pyr.h[o], w = pyr.w[o];
    const float *img = pyr.gauss[o] + ((size_t)n * (pyr.layers + 3) + layer) * h * w;
    const int ptx = (int)rintf(px), pty = (int)rintf(py);
    float cos_t, sin_t;
    sift_sincos_deg(ori, &cos_t, &sin_t);
    const float bins_per_deg = (float)(SF_N / 360.0), exp_scale = -1.0f / ((float)(SF_D * SF_D) * 0.5f), hist_width = 3.0f * scl;
    int radius = (int)rintf(hist_width * (float)1.4142135623730951 * (float)(SF_D + 1) * 0.5f);
    radius = min(radius, (int)sqrt((double)h * h + (double)w * w));
    cos_t = cos_t / hist_width, sin_t = sin_t / hist_width;
    for (int b = 0; b < KNN_DESC; ++b) part[lane][b] = 0.0f;
    const int len = 2 * radius + 1;
    for (int p = lane; p < len * len; p += 64) {
        const int i = p / len - radius, j = p % len - radius;
        const float c_rot = (float)j * cos_t - (float)i * sin_t, r_rot = (float)j * sin_t + (float)i * cos_t;
        float rbin = r_rot + (float)(SF_D / 2) - 0.5f, cbin = c_rot + (float)(SF_D / 2) - 0.5f;
        const int r = pty + i, c = ptx + j;
        if (!(rbin > -1.0f && rbin < (float)SF_D && cbin > -1.0f && cbin < (float)SF_D && r > 0 && r < h - 1 && c > 0 && c < w - 1)) continue;
        const float dx = img[(size_t)r * w + c + 1] - img[(size_t)r * w + c - 1], dy = img[(size_t)(r - 1) * w + c] - img[(size_t)(r + 1) * w + c];
        const float wgt = sift_exp((c_rot * c_rot + r_rot * r_rot) * exp_scale);
        float obin = (sift_atan2_deg(dy, dx) - ori) * bins_per_deg;
        const float mag = sqrtf(dx * dx + dy * dy) * wgt;
        const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);
        rbin = rbin - r0f, cbin = cbin - c0f, obin = obin - o0f;
        const int r0 = (int)r0f, c0 = (int)c0f;
        int o0 = (int)o0f;
        if (o0 < 0) o0 += SF_N;
        if (o0 >= SF_N) o0 -= SF_N;
        const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
        const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11, v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
        const float v111 = v_rc11 * obin, v110 = v_rc11 - v111, v101 = v_rc10 * obin, v100 = v_rc10 - v101;
        const float v011 = v_rc01 * obin, v010 = v_rc01 - v011, v001 = v_rc00 * obin, v000 = v_rc00 - v001;
        const int o1 = (o0 + 1) & (SF_N - 1);
        // the eight bins in the order 000 001 010 011 100 101 110 111 (row, column, orientation); rows and columns outside 0 .. 3 take nothing
        const float v[8] = {v000, v001, v010, v011, v100, v101, v110, v111};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int rr = r0 + (q >> 2), cc = c0 + ((q >> 1) & 1), oo = (q & 1) ? o1 : o0;
            if (rr < 0 || rr >= SF_D || cc < 0 || cc >= SF_D) continue;
            const int b = (rr * SF_D + cc) * SF_N + oo;
            part[lane][b] = part[lane][b] + v[q];
        }
    }
    __syncthreads();
    for (int b = lane; b < KNN_DESC; b += 64) {
        float acc = 0.0f;
        for (int l = 0; l < 64; ++l) acc = acc + part[l][b];
        dst[b] = acc;
    }
    __syncthreads();
    if (lane != 0) return;
    float nrm2 = 0.0f;
    for (int k = 0; k < KNN_DESC; ++k) nrm2 = nrm2 + dst[k] * dst[k];
    const float thr = sqrtf(nrm2) * 0.2f;
    nrm2 = 0.0f;
    for (int k = 0; k < KNN_DESC; ++k) {
        const float v = fminf(dst[k], thr);
        dst[k] = v, nrm2 = nrm2 + v * v;
    }
    const float s = 512.0f / fmaxf(sqrtf(nrm2), FLT_EPSILON);
    uint8_t *out = desc + ((size_t)n * capacity + blockIdx.x) * KNN_DESC;
    for (int k = 0; k < KNN_DESC; ++k) out[k] = (uint8_t)fminf(fmaxf(rintf(dst[k] * s), 0.0f), 255.0f);
}

// the ratio test and the mean distance of a pair; one thread per pair
__global__ __launch_bounds__(64) void mifd_kernel(const float *__restrict__ kps, const unsigned *__restrict__ counts, int q_base, int t_base, int stride, int pairs,
                                                  const int32_t *__restrict__ idx, const float *__restrict__ dist, float ratio, int min_matches,
                                                  double *__restrict__ score, int32_t *__restrict__ matches) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= pairs) return;
    const int Q = knn_count(counts, q_base + p, stride), T = knn_count(counts, t_base + p, stride);
    const float *qk = kps + (size_t)(q_base + p) * stride * KNN_KP_WORDS, *tk = kps + (size_t)(t_base + p) * stride * KNN_KP_WORDS;
    int kept = 0;
    double sum = 0.0;
    if (Q >= 2 && T >= 2)
        for (int q = 0; q < Q; ++q) {
            const size_t at = ((size_t)p * stride + q) * 2;
            if (!(dist[at] < ratio * dist[at + 1])) continue;
            const int j = idx[at];
            const float dx = qk[(size_t)q * KNN_KP_WORDS] - tk[(size_t)j * KNN_KP_WORDS], dy = qk[(size_t)q * KNN_KP_WORDS + 1] - tk[(size_t)j * KNN_KP_WORDS + 1];
            const double ddx = (double)dx, ddy = (double)dy;
            sum = sum + sqrt(ddx * ddx + ddy * ddy);
            ++kept;
        }
    matches[p] = kept;
    score[p] = (Q < 2 || T < 2 || kept < min_matches || kept == 0) ? (double)NAN : sum / (double)kept;
}

}  // namespace

struct hive_sift {
    hive_ctx *ctx = nullptr;
    int H = 0, W = 0, max_images = 0, capacity = 0, nfeatures = 0, layers = 0, octaves = 0;
    float contrast_threshold = 0.f, edge_threshold = 0.f, sigma = 0.f;
    int oh[SF_MAX_OCTAVES] = {}, ow[SF_MAX_OCTAVES] = {};
    float *gauss[SF_MAX_OCTAVES] = {};  // [max_images][layers + 3][oh][ow]
    float *base = nullptr;              // [max_images][2H][2W]
    float *cand = nullptr, *raw = nullptr, *sorted = nullptr;
    std::vector<SfTaps> taps;           // [0] the base blur, [i] the blur from layer i - 1 to layer i
    void *mem = nullptr;
    int last_stage = 0;                 // hive_sift_set_last_stage: 0 = everything
};

extern "C" {

int hive_sift_create(hive_ctx *ctx, int H, int W, int max_images, int nfeatures, int n_octave_layers, double contrast_threshold, double edge_threshold, double sigma,
                     const float *const *taps, const int *tap_counts, int capacity, hive_sift **out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, out && taps && tap_counts, "sift_create: NULL argument");
    HIVE_REQUIRE(ctx, H >= 6 && W >= 6, "sift_create: %d x %d is smaller than 6 x 6, the smallest picture whose doubled base reaches past the 5-pixel border", H, W);
    HIVE_REQUIRE(ctx, (long long)H * W < (1ll << 27), "sift_create: %d x %d pixels are too many", H, W);
    HIVE_REQUIRE(ctx, max_images >= 1 && max_images <= 8192, "sift_create: max_images = %d, need 1 .. 8192", max_images);
    HIVE_REQUIRE(ctx, n_octave_layers >= 1 && n_octave_layers <= 5, "sift_create: nOctaveLayers = %d, need 1 .. 5", n_octave_layers);
    HIVE_REQUIRE(ctx, nfeatures >= 0 && capacity >= 1 && capacity <= 65535, "sift_create: nfeatures = %d, capacity = %d (1 .. 65535)", nfeatures, capacity);
    HIVE_REQUIRE(ctx, contrast_threshold >= 0 && edge_threshold > 0 && sigma > 0, "sift_create: thresholds and sigma must be positive");
    hive_sift *s = new hive_sift;
    s->ctx = ctx, s->H = H, s->W = W, s->max_images = max_images, s->capacity = capacity, s->nfeatures = nfeatures, s->layers = n_octave_layers;
    s->contrast_threshold = (float)contrast_threshold, s->edge_threshold = (float)edge_threshold, s->sigma = (float)sigma;
    for (int i = 0; i < n_octave_layers + 3; ++i) {
        const int n = tap_counts[i];
        if (n < 1 || n > SF_MAX_TAPS || n % 2 == 0 || !taps[i]) {
            delete s;
            return hive_fail(ctx, HIVE_ERR_INVALID, "sift_create: blur %d has %d taps, need an odd number up to %d", i, n, SF_MAX_TAPS);
        }
        SfTaps t = {};
        t.n = n;
        memcpy(t.g, taps[i], n * sizeof(float));
        s->taps.push_back(t);
    }
    const int smaller = 2 * (H < W ? H : W);
    s->octaves = (int)lrint(std::log((double)smaller) / std::log(2.0) - 2.0) + 1;
    if (s->octaves < 1) s->octaves = 1;
    if (s->octaves > SF_MAX_OCTAVES) s->octaves = SF_MAX_OCTAVES;
    hive_scratch_layout lay;
    const int L3 = n_octave_layers + 3;
    for (int pass = 0; pass < 2; ++pass) {
        lay.off = 0;
        int h = 2 * H, w = 2 * W;
        s->base = lay.take<float>((size_t)max_images * h * w);
        for (int o = 0; o < s->octaves; ++o) {
            if (h < 1 || w < 1) {
                s->octaves = o;
                break;
            }
            s->oh[o] = h, s->ow[o] = w;
            s->gauss[o] = lay.take<float>((size_t)max_images * L3 * h * w);
            h /= 2, w /= 2;
        }
        s->cand = lay.take<float>((size_t)max_images * capacity * SF_CAND_WORDS);
        s->raw = lay.take<float>((size_t)max_images * capacity * KNN_KP_WORDS);
        s->sorted = lay.take<float>((size_t)max_images * capacity * KNN_KP_WORDS);
        if (pass == 0) {
            const hipError_t e = hipMalloc(&s->mem, lay.bytes());
            if (e != hipSuccess) {
                const size_t bytes = lay.bytes();
                delete s;
                return hive_fail(ctx, HIVE_ERR_NOMEM, "sift_create: %zu bytes for %d pictures of %d x %d: %s", bytes, max_images, H, W, hipGetErrorString(e));
            }
            lay.base = (char *)s->mem;
        }
    }
    *out = s;
    return HIVE_OK;
}

int hive_sift_destroy(hive_sift *sift) {
    HIVE_ENTER(sift ? sift->ctx : nullptr);
    if (!sift) return HIVE_OK;
    (void)hipStreamSynchronize(sift->ctx->stream);
    if (sift->mem) (void)hipFree(sift->mem);
    delete sift;
    return HIVE_OK;
}

int hive_sift_detect(hive_sift *sift, const uint8_t *d_gray, const uint8_t *d_mask, int N, float *d_keypoints, uint8_t *d_descriptors, int32_t *d_counts) {
    HIVE_ENTER(sift ? sift->ctx : nullptr);
    if (!sift) return hive_fail(nullptr, HIVE_ERR_INVALID, "sift is NULL");
    hive_ctx *ctx = sift->ctx;
    HIVE_REQUIRE(ctx, d_gray && d_keypoints && d_descriptors && d_counts, "sift_detect: NULL argument");
    HIVE_REQUIRE(ctx, N >= 1 && N <= sift->max_images, "sift_detect: N = %d, the object holds 1 .. %d pictures", N, sift->max_images);
    hipStream_t st = ctx->stream;
    const int H = sift->H, W = sift->W, L = sift->layers, L3 = L + 3, cap = sift->capacity;
    unsigned *counts = (unsigned *)d_counts;
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(counts, 0, (size_t)N * 3 * sizeof(unsigned), st));
    hipLaunchKernelGGL(sift_base_kernel, dim3((unsigned)hive_div_up(4ll * H * W, SF_THREADS), (unsigned)N), dim3(SF_THREADS), 0, st, d_gray, H, W, sift->base);
    SfPyramid pyr = {};
    pyr.octaves = sift->octaves, pyr.layers = L;
    for (int o = 0; o < sift->octaves; ++o) {
        const int h = sift->oh[o], w = sift->ow[o];
        const size_t plane = (size_t)h * w, stride = plane * L3;
        const dim3 tiles((unsigned)hive_div_up(w, SF_TILE), (unsigned)hive_div_up(h, SF_TILE), (unsigned)N);
        pyr.gauss[o] = sift->gauss[o], pyr.h[o] = h, pyr.w[o] = w;
        if (o == 0) {
            hipLaunchKernelGGL(sift_blur_kernel, tiles, dim3(SF_THREADS), 0, st, sift->base, plane, sift->gauss[0], stride, h, w, sift->taps[0]);
        } else {
            const int ph = sift->oh[o - 1], pw = sift->ow[o - 1];
            hipLaunchKernelGGL(sift_half_kernel, dim3((unsigned)hive_div_up((long long)plane, SF_THREADS), (unsigned)N), dim3(SF_THREADS), 0, st,
                               sift->gauss[o - 1] + (size_t)L * ph * pw, (size_t)ph * pw * L3, pw, sift->gauss[o], stride, h, w);
        }
        for (int i = 1; i < L3; ++i)
            hipLaunchKernelGGL(sift_blur_kernel, tiles, dim3(SF_THREADS), 0, st, sift->gauss[o] + (size_t)(i - 1) * plane, stride, sift->gauss[o] + (size_t)i * plane, stride,
                               h, w, sift->taps[i]);
    }
    if (sift->last_stage == 1) {
        HIVE_CHECK_HIP(ctx, hipGetLastError());
        return HIVE_OK;
    }
    for (int o = 0; o < sift->octaves; ++o) {
        const int h = sift->oh[o], w = sift->ow[o];
        if (h <= 2 * SF_BORDER || w <= 2 * SF_BORDER) continue;
        SfDetect a = {};
        a.octave = o, a.h = h, a.w = w, a.layers = L, a.H = H, a.W = W, a.capacity = cap;
        a.threshold = (float)std::floor(0.5 * (double)sift->contrast_threshold / L * 255.0);
        a.contrast_threshold = sift->contrast_threshold, a.edge_threshold = sift->edge_threshold, a.sigma = sift->sigma;
        hipLaunchKernelGGL(sift_detect_kernel, dim3((unsigned)hive_div_up((long long)h * w, SF_THREADS), (unsigned)(N * L)), dim3(SF_THREADS), 0, st, sift->gauss[o],
                           (size_t)h * w * L3, a, d_mask, counts, sift->cand);
    }
    hipLaunchKernelGGL(sift_orient_kernel, dim3((unsigned)cap, (unsigned)N), dim3(64), 0, st, pyr, sift->cand, cap, sift->nfeatures, counts, sift->raw);
    const dim3 per_kp((unsigned)hive_div_up(cap, SF_THREADS), (unsigned)N);
    hipLaunchKernelGGL(sift_rank_kernel, per_kp, dim3(SF_THREADS), 0, st, sift->raw, cap, counts, sift->sorted);
    hipLaunchKernelGGL(sift_unique_kernel, per_kp, dim3(SF_THREADS), 0, st, sift->sorted, cap, counts, d_keypoints);
    if (sift->last_stage != 2) hipLaunchKernelGGL(sift_describe_kernel, dim3((unsigned)cap, (unsigned)N), dim3(64), 0, st, pyr, d_keypoints, cap, counts, d_descriptors);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_sift_set_last_stage(hive_sift *sift, int stage) {
    if (!sift) return hive_fail(nullptr, HIVE_ERR_INVALID, "sift is NULL");
    HIVE_REQUIRE(sift->ctx, stage >= 0 && stage <= 2, "sift_set_last_stage: stage = %d, need 0 (everything), 1 (the pyramid) or 2 (the keypoints)", stage);
    sift->last_stage = stage;
    return HIVE_OK;
}

int hive_sift_read_layer(hive_sift *sift, int octave, int layer, int N, float *d_out) {
    HIVE_ENTER(sift ? sift->ctx : nullptr);
    if (!sift) return hive_fail(nullptr, HIVE_ERR_INVALID, "sift is NULL");
    hive_ctx *ctx = sift->ctx;
    HIVE_REQUIRE(ctx, d_out, "sift_read_layer: NULL argument");
    HIVE_REQUIRE(ctx, octave >= 0 && octave < sift->octaves && layer >= 0 && layer < sift->layers + 3, "sift_read_layer: octave %d of %d, layer %d of %d", octave,
                 sift->octaves, layer, sift->layers + 3);
    HIVE_REQUIRE(ctx, N >= 1 && N <= sift->max_images, "sift_read_layer: N = %d, the object holds 1 .. %d pictures", N, sift->max_images);
    const size_t plane = (size_t)sift->oh[octave] * sift->ow[octave] * sizeof(float);
    HIVE_CHECK_HIP(ctx, hipMemcpy2DAsync(d_out, plane, sift->gauss[octave] + (size_t)layer * (plane / sizeof(float)), plane * (sift->layers + 3), plane, (size_t)N,
                                         hipMemcpyDeviceToDevice, ctx->stream));
    return HIVE_OK;
}

int hive_sift_read_candidates(hive_sift *sift, int N, void *d_out) {
    HIVE_ENTER(sift ? sift->ctx : nullptr);
    if (!sift) return hive_fail(nullptr, HIVE_ERR_INVALID, "sift is NULL");
    hive_ctx *ctx = sift->ctx;
    HIVE_REQUIRE(ctx, d_out, "sift_read_candidates: NULL argument");
    HIVE_REQUIRE(ctx, N >= 1 && N <= sift->max_images, "sift_read_candidates: N = %d, the object holds 1 .. %d pictures", N, sift->max_images);
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(d_out, sift->cand, (size_t)N * sift->capacity * SF_CAND_WORDS * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return HIVE_OK;
}

int hive_knn_match(hive_ctx *ctx, const uint8_t *d_query, int Q, const uint8_t *d_train, int T, int32_t *d_indices, float *d_distances) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_query && d_train && d_indices && d_distances, "knn_match: NULL argument");
    HIVE_REQUIRE(ctx, Q >= 1 && T >= 1 && Q < (1 << 24) && T < (1 << 24), "knn_match: Q = %d, T = %d, need 1 .. 2^24 - 1", Q, T);
    HIVE_REQUIRE(ctx, ((uintptr_t)d_query | (uintptr_t)d_train) % 4 == 0, "knn_match: the descriptors must be 4-byte aligned");
    const KnnArgs a = {d_query, d_train, nullptr, nullptr, 0, 0, 0, Q > T ? Q : T, Q, T};
    hipLaunchKernelGGL(knn_match_kernel, dim3((unsigned)hive_div_up(Q, KNN_TILE), 1u), dim3(KNN_TILE), 0, ctx->stream, a, d_indices, d_distances);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_mifd(hive_ctx *ctx, const float *d_keypoints, const uint8_t *d_descriptors, const int32_t *d_counts, int capacity, int query_first, int train_first, int pairs,
              float ratio_threshold, int min_matches, int32_t *d_indices, float *d_distances, double *d_scores, int32_t *d_matches) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_keypoints && d_descriptors && d_counts && d_indices && d_distances && d_scores && d_matches, "mifd: NULL argument");
    HIVE_REQUIRE(ctx, capacity >= 1 && capacity <= 65535 && pairs >= 1 && pairs <= 65535 && query_first >= 0 && train_first >= 0,
                 "mifd: capacity = %d, pairs = %d (1 .. 65535 each), first pictures %d and %d", capacity, pairs, query_first, train_first);
    HIVE_REQUIRE(ctx, (uintptr_t)d_descriptors % 4 == 0, "mifd: the descriptors must be 4-byte aligned");
    const KnnArgs a = {d_descriptors, d_descriptors, (const unsigned *)d_counts, nullptr, 0, query_first, train_first, capacity, 0, 0};
    hipLaunchKernelGGL(knn_match_kernel, dim3((unsigned)hive_div_up(capacity, KNN_TILE), (unsigned)pairs), dim3(KNN_TILE), 0, ctx->stream, a, d_indices, d_distances);
    hipLaunchKernelGGL(mifd_kernel, dim3((unsigned)hive_div_up(pairs, 64)), dim3(64), 0, ctx->stream, d_keypoints, (const unsigned *)d_counts, query_first, train_first, capacity,
                       pairs, d_indices, d_distances, ratio_threshold, min_matches, d_scores, d_matches);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

}  // extern "C"
