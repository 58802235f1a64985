// The exact 2-nearest-neighbour matcher (rule `knn` of include/hive_mi355x.h): squared L2 distances of 128-byte descriptors as exact integers, the two nearest, a
// tie to the lower train index.  knn_match_kernel is the one launch kernel: hive_knn_match and hive_mifd (sift.hip) name a pair's pictures by q_base + p and
// t_base + p, hive_pairs_match (pairs.hip) by a pair list.  Also here: what the units share about hive_sift_detect's rows (KNN_DESC, KNN_KP_WORDS) and the
// one clamp of a picture's keypoint count (knn_count).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

constexpr int KNN_TILE = 64;
constexpr int KNN_DESC = 128;     // a descriptor's bytes
constexpr int KNN_WORDS = KNN_DESC / 4;
constexpr int KNN_KP_WORDS = 6;   // hive_sift_detect's keypoint row: x, y, size, angle, response, octave (all f32)

// a picture's keypoint count from hive_sift_detect's counts, never more than the `stride` rows the picture has
__device__ __forceinline__ int knn_count(const unsigned *__restrict__ counts, int picture, int stride) { return (int)min(counts[3 * picture + 2], (unsigned)stride); }

// sum over the four bytes of a[i] * b[i], added to acc
__device__ __forceinline__ unsigned knn_dot4(unsigned a, unsigned b, unsigned acc) {
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    return acc + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) + (a >> 24) * (b >> 24);
#endif
}

// One thread per query, KNN_TILE threads a workgroup, every thread of it calls this (it holds barriers).  Query q of the Q descriptors at qd (a thread with
// q >= Q scans zeros and its result is not used) against the T descriptors at td, staged through `tile`: the two smallest squared distances b0 <= b1 and
// their train indices (-1 where T has fewer).
__device__ __forceinline__ void knn_two_nearest(const unsigned *__restrict__ qd, const unsigned *__restrict__ td, int Q, int T, int q,
                                                unsigned (*tile)[KNN_WORDS + 1], unsigned &b0, unsigned &b1, int &i0, int &i1) {
    const int t = threadIdx.x;
    unsigned mine[KNN_WORDS], nq = 0;
#pragma unroll
    for (int k = 0; k < KNN_WORDS; ++k) {
        mine[k] = q < Q ? qd[(size_t)q * KNN_WORDS + k] : 0u;
        nq = knn_dot4(mine[k], mine[k], nq);
    }
    b0 = 0xffffffffu, b1 = 0xffffffffu;
    i0 = -1, i1 = -1;
    for (int t0 = 0; t0 < T; t0 += KNN_TILE) {
        const int rows = min(KNN_TILE, T - t0);
        __syncthreads();
        for (int e = t; e < rows * KNN_WORDS; e += KNN_TILE) tile[e / KNN_WORDS][e % KNN_WORDS] = td[(size_t)t0 * KNN_WORDS + e];
        __syncthreads();
        for (int d = 0; d < rows; ++d) {
            unsigned dot = 0, nt = 0;
#pragma unroll
            for (int k = 0; k < KNN_WORDS; ++k) {
                const unsigned v = tile[d][k];
                dot = knn_dot4(mine[k], v, dot), nt = knn_dot4(v, v, nt);
            }
            const unsigned d2 = nq + nt - 2u * dot;  // the exact squared distance, at most 128 * 255^2
            if (d2 < b0) b1 = b0, i1 = i0, b0 = d2, i0 = t0 + d;
            else if (d2 < b1) b1 = d2, i1 = t0 + d;
        }
    }
}

// What pair p matches: queries of picture pairs[2 p] against trains of picture pairs[2 p + 1] of the N pictures when a pair list is given (a pair naming a
// picture outside 0 .. N - 1 has Q = T = 0), else of pictures q_base + p and t_base + p; `stride` descriptors a picture; a picture's number of descriptors
// from `counts` when given, else Q and T
struct KnnArgs {
    const uint8_t *query, *train;
    const unsigned *counts;
    const int32_t *pairs;
    int N, q_base, t_base, stride, Q, T;
};

// the pictures of pair p of a pair list and their keypoint counts; 0 and 0 for a pair that names a picture outside 0 .. N - 1
__device__ __forceinline__ void knn_pair(const int32_t *__restrict__ pairs, const unsigned *__restrict__ counts, int N, int stride, int p, int &pi, int &pj, int &Q, int &T) {
    pi = pairs[2 * p], pj = pairs[2 * p + 1];
    const bool ok = pi >= 0 && pi < N && pj >= 0 && pj < N;
    if (!ok) pi = pj = 0;
    Q = ok ? knn_count(counts, pi, stride) : 0;
    T = ok ? knn_count(counts, pj, stride) : 0;
}

// The two nearest train descriptors of every query descriptor; one thread per query, grid (ceil(max Q / 64), pairs): idx / dist [pair][stride][2], -1 and
// inf where T has fewer than two.  (static: each unit that launches it holds its own copy of this one definition)
static __global__ __launch_bounds__(KNN_TILE) void knn_match_kernel(KnnArgs a, int32_t *__restrict__ idx, float *__restrict__ dist) {
    __shared__ unsigned tile[KNN_TILE][KNN_WORDS + 1];
    const int p = blockIdx.y, q = blockIdx.x * KNN_TILE + threadIdx.x;
    int pi = a.q_base + p, pj = a.t_base + p, Q = a.Q, T = a.T;
    if (a.pairs)
        knn_pair(a.pairs, a.counts, a.N, a.stride, p, pi, pj, Q, T);
    else if (a.counts)
        Q = knn_count(a.counts, pi, a.stride), T = knn_count(a.counts, pj, a.stride);
    if ((int)blockIdx.x * KNN_TILE >= Q) return;
    const unsigned *qd = (const unsigned *)(a.query + (size_t)pi * a.stride * KNN_DESC), *td = (const unsigned *)(a.train + (size_t)pj * a.stride * KNN_DESC);
    unsigned b0, b1;
    int i0, i1;
    knn_two_nearest(qd, td, Q, T, q, tile, b0, b1, i0, i1);
    if (q >= Q) return;
    const size_t at = ((size_t)p * a.stride + q) * 2;
    idx[at] = i0, idx[at + 1] = i1;
    dist[at] = i0 < 0 ? INFINITY : sqrtf((float)b0), dist[at + 1] = i1 < 0 ? INFINITY : sqrtf((float)b1);
}
