// What texture.hip and texture_level.hip share: the camera of a fill, the projection and the bilinear sample of include/hive_mi355x.h's `fill` rule, the byte
// rule.  Float64 without contraction (the Makefile's EXACT flags), in the order written.
#pragma once
#include "hive_internal.hpp"

#include <cmath>

struct TextureCam {
    double K[9];
    double near;
};

__device__ __forceinline__ bool tx_ids_ok(int a, int b, int c, long long nv) {
    return (unsigned long long)a < (unsigned long long)nv && (unsigned long long)b < (unsigned long long)nv && (unsigned long long)c < (unsigned long long)nv;
}

__device__ __forceinline__ uint8_t tx_byte(double c) { return (uint8_t)fmin(255.0, fmax(0.0, floor(c + 0.5))); }

// hive_project's order: Rt = a view's R row-major then t
__device__ __forceinline__ void tx_project(const TextureCam &cam, const double *__restrict__ Rt, const double P[3], double c[3]) {
    const double *R = Rt, *t = Rt + 9;
    double q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = R[3 * r + 0] * P[0] + R[3 * r + 1] * P[1] + R[3 * r + 2] * P[2] + t[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = cam.K[3 * r + 0] * q[0] + cam.K[3 * r + 1] * q[1] + cam.K[3 * r + 2] * q[2];
}

// the clamped bilinear sample of `frame` u8 [H][W][3] at (c_0 / c_2, c_1 / c_2), unrounded
__device__ __forceinline__ void tx_bilinear(const uint8_t *__restrict__ frame, int H, int W, const double c[3], double out[3]) {
    const double u = fmin(fmax(c[0] / c[2], 0.0), (double)(W - 1)), v = fmin(fmax(c[1] / c[2], 0.0), (double)(H - 1));
    const double fu = floor(u), fv = floor(v), ax = u - fu, ay = v - fv;
    const int j0 = (int)fu, i0 = (int)fv, j1 = min(j0 + 1, W - 1), i1 = min(i0 + 1, H - 1);
    const uint8_t *p00 = frame + 3 * ((size_t)i0 * W + j0), *p01 = frame + 3 * ((size_t)i0 * W + j1), *p10 = frame + 3 * ((size_t)i1 * W + j0),
                  *p11 = frame + 3 * ((size_t)i1 * W + j1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double c00 = (double)p00[ch], c01 = (double)p01[ch], c10 = (double)p10[ch], c11 = (double)p11[ch];
        const double top = c00 + ax * (c01 - c00), bottom = c10 + ax * (c11 - c10);
        out[ch] = top + ay * (bottom - top);
    }
}
