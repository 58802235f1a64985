// Order-preserving compaction of a mesh on the device, shared by the clean-up (fgmesh.hip) and the decimation (decimate.hip): the kept vertices get
// consecutive rows in input order, the kept faces follow in input order and index those rows.  Four launches: count, scan, vertex map, faces; the scan is
// block_scan_counts of hive_internal.hpp, the one scan of every compaction.
//
// The params struct P says what is kept:
//   nv(), nf()            vertices / faces of the input (device counts, bounded by the capacities the scratch was laid out for)
//   keep_vertex(i)        vertex i survives
//   keep_face(f)          face f survives
//   face_vertex(f, k)     output row of corner k of a kept face f (already through vmap), or -1
//   vmap                  [nv] i32, written here: output row of every input vertex, or -1
#pragma once
#include "hive_internal.hpp"

#include <algorithm>

namespace {

constexpr int TILE = 1024;  // items per workgroup of 256 (4 consecutive items per thread keep the input order)

// scan_counts_kernel of the two block-count arrays (totals[0..1] = their sums), and box = the texture window's empty box (INT_MAX, INT_MAX, INT_MIN,
// INT_MIN) for the atomics of window_project_kernel (no host-to-device copy in the call)
__global__ __launch_bounds__(SCAN_THREADS) void scan_counts_box_kernel(unsigned *__restrict__ a, unsigned *__restrict__ b, int nb, unsigned *totals, int *box) {
    unsigned *const arrays[] = {a, b};
    block_scan_counts(arrays, nb, totals);
    if (threadIdx.x < 4) box[threadIdx.x] = threadIdx.x < 2 ? 0x7fffffff : (int)0x80000000;
}

inline void scan_counts_box(hive_ctx *ctx, unsigned *a, unsigned *b, int nb, unsigned *totals, int *box) {
    hipLaunchKernelGGL(scan_counts_box_kernel, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, a, b, nb, totals, box);
}

// per block of TILE: kept vertices -> bv, kept faces -> bf (both arrays cover max(face blocks, vertex blocks))
template <class P>
__global__ __launch_bounds__(256) void compact_count_kernel(P p, unsigned *__restrict__ bv, unsigned *__restrict__ bf) {
    __shared__ unsigned lds[8];
    const long long nf = p.nf(), nv = p.nv();
    unsigned c[2] = {0, 0};  // kept vertices, kept faces
    for (int j = 0; j < TILE / 256; ++j) {
        const long long i = (long long)blockIdx.x * TILE + threadIdx.x * (TILE / 256) + j;
        if (i < nf) c[1] += p.keep_face(i);
        if (i < nv) c[0] += p.keep_vertex(i);
    }
    block_sum(c, lds);
    if (threadIdx.x == 0) {
        bv[blockIdx.x] = c[0];
        bf[blockIdx.x] = c[1];
    }
}

// vmap[v] = output row of a kept vertex (else -1); out_vertex_index (optional) = the kept input ids in order
template <class P>
__global__ __launch_bounds__(256) void compact_vmap_kernel(P p, const unsigned *__restrict__ bv, int32_t *__restrict__ out_vertex_index) {
    __shared__ unsigned lds[4];
    const long long nv = p.nv();
    const long long base = (long long)blockIdx.x * TILE + threadIdx.x * (TILE / 256);
    bool ok[TILE / 256];
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
        ok[j] = base + j < nv && p.keep_vertex(base + j);
        c += ok[j];
    }
    long long o = (long long)bv[blockIdx.x] + block_exclusive(c, lds);
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
        if (base + j >= nv) continue;
        p.vmap[base + j] = ok[j] ? (int)o : -1;
        if (ok[j]) {
            if (out_vertex_index) out_vertex_index[o] = (int32_t)(base + j);
            ++o;
        }
    }
}

// the kept faces in order, through the vertex map; rows past out_cap are counted but not written
template <class P>
__global__ __launch_bounds__(256) void compact_faces_kernel(P p, const unsigned *__restrict__ bf, int32_t *__restrict__ out, long long out_cap) {
    __shared__ unsigned lds[4];
    const long long nf = p.nf();
    const long long base = (long long)blockIdx.x * TILE + threadIdx.x * (TILE / 256);
    bool ok[TILE / 256];
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
        ok[j] = base + j < nf && p.keep_face(base + j);
        c += ok[j];
    }
    long long o = (long long)bf[blockIdx.x] + block_exclusive(c, lds);
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j)
        if (ok[j]) {
            if (o < out_cap)
                for (int k = 0; k < 3; ++k) out[3 * o + k] = p.face_vertex(base + j, k);
            ++o;
        }
}

// the four launches on ctx->stream: bv / bf hold nb block counts each; out_counts[0..1] = vertices / faces kept; box = four words for the scan's empty box
template <class P>
void launch_compaction(hive_ctx *ctx, const P &p, unsigned *bv, unsigned *bf, int nb, unsigned *out_counts, int *box, int32_t *out_faces, long long out_cap,
                       int32_t *out_vertex_index) {
    hipLaunchKernelGGL(compact_count_kernel<P>, dim3(nb), dim3(256), 0, ctx->stream, p, bv, bf);
    scan_counts_box(ctx, bv, bf, nb, out_counts, box);
    hipLaunchKernelGGL(compact_vmap_kernel<P>, dim3(nb), dim3(256), 0, ctx->stream, p, (const unsigned *)bv, out_vertex_index);
    hipLaunchKernelGGL(compact_faces_kernel<P>, dim3(nb), dim3(256), 0, ctx->stream, p, (const unsigned *)bf, out_faces, out_cap);
}

}  // namespace
