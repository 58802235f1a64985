// The inner loop of the exact 2-nearest-neighbour matcher (rule `knn` of include/hive_mi355x.h), shared by sift.hip (hive_knn_match, hive_mifd) and pairs.hip
// (hive_pairs_match): squared L2 distances of 128-byte descriptors as exact integers, the two nearest, a tie to the lower train index.
#pragma once
#include <hip/hip_runtime.h>

constexpr int KNN_TILE = 64;
constexpr int KNN_WORDS = 32;  // a descriptor: 128 bytes as 32 words

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
