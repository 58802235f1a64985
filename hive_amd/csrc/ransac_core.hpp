// What the two RANSACs share (pairs.hip: the homography; register.hip: the rigid transform): the hash and the draw of a trial's sample, a pair's count and the
// lane-ordered float64 sum of a wave.  The rules are stated in include/hive_mi355x.h above hive_pairs_match (`draw`, `lane sum`) and restated in numpy in
// tests/ransac_restatement.py.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ unsigned rs_mix(unsigned x) {  // lowbias32
    x ^= x >> 16, x *= 0x7feb352du;
    x ^= x >> 15, x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ unsigned rs_base(unsigned seed, const int32_t *__restrict__ key) {
    return rs_mix(rs_mix(rs_mix(seed) ^ (unsigned)key[0]) ^ (unsigned)key[1]);
}

// four distinct indices below M >= 4, in the order drawn: draw k takes the mulhi(x_k, M - k)-th index not yet chosen, in ascending order
__device__ __forceinline__ void rs_draw(unsigned base, unsigned t, unsigned M, int &d0, int &d1, int &d2, int &d3) {
    const unsigned h = rs_mix(base ^ t);
    const unsigned a = __umulhi(rs_mix(h), M);
    unsigned b = __umulhi(rs_mix(h ^ 1u), M - 1u);
    b += b >= a ? 1u : 0u;
    const unsigned s0 = min(a, b), s1 = max(a, b);
    unsigned c = __umulhi(rs_mix(h ^ 2u), M - 2u);
    c += c >= s0 ? 1u : 0u;
    c += c >= s1 ? 1u : 0u;
    const unsigned u0 = min(s0, c), u1 = min(max(s0, c), s1), u2 = max(s1, c);
    unsigned d = __umulhi(rs_mix(h ^ 3u), M - 3u);
    d += d >= u0 ? 1u : 0u;
    d += d >= u1 ? 1u : 0u;
    d += d >= u2 ? 1u : 0u;
    d0 = (int)a, d1 = (int)b, d2 = (int)c, d3 = (int)d;
}

// the first three of those draws alone, for M >= 3
__device__ __forceinline__ void rs_draw3(unsigned base, unsigned t, unsigned M, int &d0, int &d1, int &d2) {
    const unsigned h = rs_mix(base ^ t);
    const unsigned a = __umulhi(rs_mix(h), M);
    unsigned b = __umulhi(rs_mix(h ^ 1u), M - 1u);
    b += b >= a ? 1u : 0u;
    const unsigned s0 = min(a, b), s1 = max(a, b);
    unsigned c = __umulhi(rs_mix(h ^ 2u), M - 2u);
    c += c >= s0 ? 1u : 0u;
    c += c >= s1 ? 1u : 0u;
    d0 = (int)a, d1 = (int)b, d2 = (int)c;
}

// a pair's number of correspondences; -1 for a count outside 0 .. stride: such a pair is refused (result -2), never cut
__device__ __forceinline__ int rs_count(const int32_t *__restrict__ counts, int count_stride, int p, int stride) {
    const int c = counts[(size_t)p * count_stride];
    return c < 0 || c > stride ? -1 : c;
}

// total = 0 + lane 0 + lane 1 + ... + lane 63, on every lane of a one-wave workgroup
__device__ __forceinline__ double rs_lane_sum(double mine, double *lds) {
    __syncthreads();
    lds[threadIdx.x] = mine;
    __syncthreads();
    double acc = 0.0;
    for (int l = 0; l < 64; ++l) acc = acc + lds[l];
    return acc;
}

}  // namespace
