// Motion segmentation of depth frames against the static model (hive_amd/segmentation.py): rules `motion`, `open`, `label` of include/hive_mi355x.h.
//   hive_motion_mask       -> motion_kernel: one thread per pixel, seg_moving (segment_core.hpp)
//   hive_mask_open         -> box_kernel<false> then box_kernel<true>: a (2 it + 1)^2 box minimum, then the box maximum, each separable through LDS
//   hive_label_components  -> label_run: six launches for any batch, none of which waits for another workgroup
//        label_tile_kernel    a workgroup labels a SEG_TILE_H x SEG_TILE_W tile in LDS (row runs by ballot, unions with the row above) and writes raster indices
//        label_border_kernel  unions across tile borders and corners with atomicMin on the label plane
//        label_flatten_kernel every pixel to its root; areas by integer atomicAdd, one per root and wave for a wave's first roots
//        label_count_kernel   the kept roots of every chunk of 4096 pixels
//        label_number_kernel  the scan over the root flags in raster order, a chunk per workgroup: numbers, count, areas
//        label_write_kernel   the numbers as int32 or uint8
//   hive_motion_segment    -> the three in one call, one read-back at its end (the uint8 limit)
// Everything is integers but the motion predicate, which states its float32 order; built without contraction like every stated rule.
#include "hive_internal.hpp"
#include "segment_core.hpp"

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_SCAN_ITEMS = 16;  // consecutive pixels per thread of the numbering's two kernels: 4096 a workgroup
constexpr int SEG_AREA_ROUNDS = 4;  // label_flatten_kernel: roots a wave adds the lane count of, before single adds
constexpr int BOX_H = 16, BOX_W = 64;  // output tile of a box pass
constexpr unsigned SEG_NO_FRAME = 0xffffffffu;

__global__ __launch_bounds__(SEG_THREADS) void motion_kernel(const float *__restrict__ live, const float *__restrict__ model, size_t total, float min_difference,
                                                             float relative_difference, uint8_t *__restrict__ mask) {
    const size_t i = (size_t)blockIdx.x * SEG_THREADS + threadIdx.x;
    if (i < total) mask[i] = seg_moving(live[i], model[i], min_difference, relative_difference) ? 1 : 0;
}

// out = the box minimum (MAX = false) or maximum of `in != 0` over the pixels of the picture within r in both directions; grid (tiles x, tiles y, frame).
// Pixels outside the picture hold the pass's identity in LDS, so they take no part.
template <bool MAX>
__global__ __launch_bounds__(SEG_THREADS) void box_kernel(const uint8_t *__restrict__ in, int H, int W, int r, uint8_t *__restrict__ out) {
    __shared__ uint8_t src[(BOX_H + 2 * SEG_MAX_OPEN) * (BOX_W + 2 * SEG_MAX_OPEN)], rows[(BOX_H + 2 * SEG_MAX_OPEN) * BOX_W];
    const size_t base = (size_t)blockIdx.z * H * W;
    const int v0 = blockIdx.y * BOX_H, u0 = blockIdx.x * BOX_W, sh = BOX_H + 2 * r, sw = BOX_W + 2 * r;
    for (int e = threadIdx.x; e < sh * sw; e += SEG_THREADS) {
        const int v = v0 - r + e / sw, u = u0 - r + e % sw;
        const bool inside = v >= 0 && v < H && u >= 0 && u < W;
        src[e] = inside ? (in[base + (size_t)v * W + u] != 0) : (MAX ? 0 : 1);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < sh * BOX_W; e += SEG_THREADS) {
        const uint8_t *s = src + (e / BOX_W) * sw + e % BOX_W;
        uint8_t acc = s[0];
        for (int k = 1; k <= 2 * r; ++k) acc = MAX ? (acc | s[k]) : (acc & s[k]);
        rows[e] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < BOX_H * BOX_W; e += SEG_THREADS) {
        const int v = v0 + e / BOX_W, u = u0 + e % BOX_W;
        if (v >= H || u >= W) continue;
        uint8_t acc = rows[e];
        for (int k = 1; k <= 2 * r; ++k) acc = MAX ? (acc | rows[e + k * BOX_W]) : (acc & rows[e + k * BOX_W]);
        out[base + (size_t)v * W + u] = acc;
    }
}

struct LdsMin {
    __device__ int operator()(int *p, int v) const { return atomicMin(p, v); }
};

// One tile in LDS; grid (tiles x, tiles y, frame).  labels: the raster index v * W + u of the smallest pixel (raster order) of the pixel's component WITHIN
// the tile, -1 for a clear pixel.
__global__ __launch_bounds__(SEG_THREADS) void label_tile_kernel(const uint8_t *__restrict__ mask, int H, int W, int connectivity, int *__restrict__ labels) {
    __shared__ int lab[SEG_TILE_H * SEG_TILE_W];
    __shared__ uint64_t rowmask[SEG_TILE_H];
    const size_t base = (size_t)blockIdx.z * H * W;
    const int v0 = blockIdx.y * SEG_TILE_H, u0 = blockIdx.x * SEG_TILE_W, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = u0 + lane;
    // row runs: every pixel of a run starts at the run's first pixel
    for (int r = wave; r < SEG_TILE_H; r += SEG_THREADS / 64) {
        const int v = v0 + r;
        const bool set = v < H && u < W && mask[base + (size_t)v * W + u] != 0;
        const uint64_t m = __ballot(set);
        if (lane == 0) rowmask[r] = m;
        lab[r * SEG_TILE_W + lane] = set ? r * SEG_TILE_W + seg_run_start(m, lane) : -1;
    }
    __syncthreads();
    // each run with the runs of the row above (seg_links names the pixel pairs); the loops inside seg_union end as segment_core.hpp argues
    for (int r = wave + SEG_THREADS / 64 * (wave == 0); r < SEG_TILE_H; r += SEG_THREADS / 64) {
        const uint64_t m = rowmask[r];
        if (!((m >> lane) & 1)) continue;
        const int links = seg_links(m, rowmask[r - 1], lane, connectivity), p = r * SEG_TILE_W + lane;
        if (links & SEG_LINK_UP) seg_union(lab, p, p - SEG_TILE_W, LdsMin());
        if (links & SEG_LINK_UP_LEFT) seg_union(lab, p, p - SEG_TILE_W - 1, LdsMin());
        if (links & SEG_LINK_UP_RIGHT) seg_union(lab, p, p - SEG_TILE_W + 1, LdsMin());
    }
    __syncthreads();
    // no label changes any more: the root, as a raster index of the picture
    for (int r = wave; r < SEG_TILE_H; r += SEG_THREADS / 64) {
        const int v = v0 + r;
        if (v >= H || u >= W) continue;
        int root = lab[r * SEG_TILE_W + lane];
        if (root >= 0) {
            root = seg_find(lab, root);
            root = (v0 + root / SEG_TILE_W) * W + u0 + root % SEG_TILE_W;
        }
        labels[base + (size_t)v * W + u] = root;
    }
}

struct GlobalMin {
    __device__ int operator()(int *p, int v) const { return atomicMin(p, v); }
};

// Every pair of neighbouring set pixels that lie in different tiles: the later pixel of the pair (raster order) unions itself with the earlier.  One thread
// per pixel, grid (ceil(H W / 256), frame); a pixel inside its tile has no such neighbour and leaves at once.  The corner case is here too: (v - 1, u - 1)
// and (v - 1, u + 1) are tested against the pixel's own tile, not against a row or a column alone.
__global__ __launch_bounds__(SEG_THREADS) void label_border_kernel(int H, int W, int connectivity, int *__restrict__ labels) {
    const int i = blockIdx.x * SEG_THREADS + threadIdx.x;
    if (i >= H * W) return;
    const int v = i / W, u = i % W, tv = v % SEG_TILE_H, tu = u % SEG_TILE_W;
    if (tv != 0 && tu != 0 && tu != SEG_TILE_W - 1) return;
    int *L = labels + (size_t)blockIdx.y * H * W;
    if (L[i] < 0) return;
    const auto join = [&](int dv, int du) {
        const int qv = v + dv, qu = u + du;
        if (qv < 0 || qu < 0 || qu >= W) return;
        if (qv / SEG_TILE_H == v / SEG_TILE_H && qu / SEG_TILE_W == u / SEG_TILE_W) return;  // the tile launch's pair
        const int q = qv * W + qu;
        if (seg_load(L + q) >= 0) seg_union(L, i, q, GlobalMin());
    };
    join(-1, 0);
    join(0, -1);
    if (connectivity == 8) {
        join(-1, -1);
        join(-1, 1);
    }
}

// Every set pixel to its root, and the areas at the roots; grid (ceil(H W / 256), frame), every thread of a wave stays to the end (ballot).  A pixel written
// here holds its root, which is what any other thread's seg_find through it would reach: the invariant of seg_find holds throughout.  Areas: up to
// SEG_AREA_ROUNDS times the first lane still holding a root adds the number of lanes that hold the same one (a large component fills most of a wave, and
// one add per pixel to one address is what this launch would otherwise wait for); lanes left after that add their own 1.  Integer adds: any order, one sum.
__global__ __launch_bounds__(SEG_THREADS) void label_flatten_kernel(int H, int W, int *__restrict__ labels, int *__restrict__ areas) {
    const int i = blockIdx.x * SEG_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const size_t base = (size_t)blockIdx.y * H * W;
    int *L = labels + base;
    int root = -1;
    if (i < H * W && L[i] >= 0) {
        root = seg_find(L, i);
        __atomic_store_n(L + i, root, __ATOMIC_RELAXED);
    }
    uint64_t todo = __ballot(root >= 0);  // the same in every lane: the loop is uniform
    for (int round = 0; round < SEG_AREA_ROUNDS && todo; ++round) {
        const int leader = __ffsll((long long)todo) - 1, theirs = __shfl(root, leader);
        const uint64_t same = __ballot(root == theirs);  // (theirs >= 0: lanes without a root never match)
        if (lane == leader) atomicAdd(areas + base + theirs, __popcll(same));
        if (root == theirs) root = -1;
        todo &= ~same;
    }
    if (root >= 0) atomicAdd(areas + base + root, 1);
}

// The numbering is a scan over the root flags in raster order, a chunk of SEG_THREADS * SEG_SCAN_ITEMS pixels per workgroup, grid (chunks, frame), in two
// launches: label_count_kernel leaves each chunk's count, label_number_kernel adds the counts of the chunks before its own and numbers its chunk.
// A thread's SEG_SCAN_ITEMS consecutive pixels from `at`: bit k of *roots = pixel at + k is a root (labels[x] == x), of the result = it also has the area
__device__ __forceinline__ unsigned scan_flags(const int *__restrict__ L, const int *__restrict__ A, int at, int total, int min_area, unsigned *roots) {
    unsigned keep = 0;
    *roots = 0;
#pragma unroll
    for (int k = 0; k < SEG_SCAN_ITEMS; ++k) {
        const int x = at + k;
        if (x < total && L[x] == x) {
            *roots |= 1u << k;
            if (A[x] >= min_area) keep |= 1u << k;
        }
    }
    return keep;
}

__global__ __launch_bounds__(SEG_THREADS) void label_count_kernel(int H, int W, int min_area, const int *__restrict__ labels, const int *__restrict__ areas,
                                                                  unsigned *__restrict__ partial) {
    __shared__ unsigned lds[SEG_THREADS / 64];
    const size_t base = (size_t)blockIdx.y * H * W;
    unsigned roots, chunk;
    const unsigned keep = scan_flags(labels + base, areas + base, ((int)blockIdx.x * SEG_THREADS + (int)threadIdx.x) * SEG_SCAN_ITEMS, H * W, min_area, &roots);
    block_exclusive_total((unsigned)__popc(keep), lds, &chunk);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = chunk;
}

// A root (labels[x] == x) whose area is at least min_area gets the next number, in raster order, written over its area; other roots get 0.  The frame's last
// chunk also writes counts[frame] = the numbers given and the zeros behind them in out_areas (optional) [frame][area_capacity], where the area of number j is
// at j - 1; with limit > 0, a frame whose count exceeds it lowers *over_frame to its index.
__global__ __launch_bounds__(SEG_THREADS) void label_number_kernel(int H, int W, int min_area, const int *__restrict__ labels, int *__restrict__ areas,
                                                                   const unsigned *__restrict__ partial, int *__restrict__ counts, int *__restrict__ out_areas,
                                                                   int area_capacity, int limit, unsigned *__restrict__ over_frame) {
    __shared__ unsigned lds[SEG_THREADS / 64];
    const size_t base = (size_t)blockIdx.y * H * W;
    int *A = areas + base, *O = out_areas ? out_areas + (size_t)blockIdx.y * area_capacity : nullptr;
    const unsigned *before = partial + (size_t)blockIdx.y * gridDim.x;
    unsigned mine = 0, carry, chunk, roots;
    for (unsigned c = threadIdx.x; c < blockIdx.x; c += SEG_THREADS) mine += before[c];
    block_exclusive_total(mine, lds, &carry);
    const int at = ((int)blockIdx.x * SEG_THREADS + (int)threadIdx.x) * SEG_SCAN_ITEMS;
    const unsigned keep = scan_flags(labels + base, A, at, H * W, min_area, &roots);
    unsigned number = carry + block_exclusive_total((unsigned)__popc(keep), lds, &chunk);
#pragma unroll
    for (int k = 0; k < SEG_SCAN_ITEMS; ++k) {
        if (!((roots >> k) & 1)) continue;
        const int x = at + k;
        if ((keep >> k) & 1) {
            ++number;
            if (O && number <= (unsigned)area_capacity) O[number - 1] = A[x];
            A[x] = (int)number;
        } else {
            A[x] = 0;
        }
    }
    if (blockIdx.x != gridDim.x - 1) return;
    const unsigned count = carry + chunk;
    if (O)
        for (unsigned j = count + threadIdx.x; j < (unsigned)area_capacity; j += SEG_THREADS) O[j] = 0;
    if (threadIdx.x == 0) {
        counts[blockIdx.y] = (int)count;
        if (limit > 0 && count > (unsigned)limit) atomicMin(over_frame, blockIdx.y);
    }
}

// the number of every pixel's root; `labels` may be the int32 output itself (a thread reads its own pixel's label alone)
template <class Out>
__global__ __launch_bounds__(SEG_THREADS) void label_write_kernel(size_t per_frame, const int *labels, const int *__restrict__ numbers, Out *out) {
    const size_t i = (size_t)blockIdx.x * SEG_THREADS + threadIdx.x;
    if (i >= per_frame) return;
    const size_t base = (size_t)blockIdx.y * per_frame;
    const int root = labels[base + i];
    out[base + i] = root >= 0 ? (Out)numbers[base + root] : (Out)0;
}

int check_frames(hive_ctx *ctx, const char *name, int n, int H, int W) {
    HIVE_REQUIRE(ctx, n >= 1 && n <= 65535 && H >= 1 && W >= 1 && (long long)H * W < (1ll << 30) && hive_div_up(H, BOX_H) <= 65535, "%s: bad sizes n=%d %dx%d", name, n, H, W);
    return HIVE_OK;
}

int motion_run(hive_ctx *ctx, const float *d_live, const float *d_model, size_t total, float min_difference, float relative_difference, uint8_t *d_mask) {
    HIVE_REQUIRE(ctx, min_difference >= 0.0f && relative_difference >= 0.0f && min_difference <= 3.0e38f && relative_difference <= 3.0e38f,
                 "motion_mask: min_difference = %g, relative_difference = %g (finite, not negative)", (double)min_difference, (double)relative_difference);
    hipLaunchKernelGGL(motion_kernel, dim3((unsigned)((total + SEG_THREADS - 1) / SEG_THREADS)), dim3(SEG_THREADS), 0, ctx->stream, d_live, d_model, total,
                       min_difference, relative_difference, d_mask);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

// tmp: a plane of n * H * W bytes that is neither d_mask nor d_out; d_out may be d_mask
int open_run(hive_ctx *ctx, const uint8_t *d_mask, int n, int H, int W, int iterations, uint8_t *tmp, uint8_t *d_out) {
    HIVE_REQUIRE(ctx, iterations >= 0 && iterations <= SEG_MAX_OPEN, "mask_open: %d iterations (0 .. %d)", iterations, SEG_MAX_OPEN);
    if (iterations == 0) {
        if (d_out != d_mask) HIVE_CHECK_HIP(ctx, hipMemcpyAsync(d_out, d_mask, (size_t)n * H * W, hipMemcpyDeviceToDevice, ctx->stream));
        return HIVE_OK;
    }
    const dim3 grid(hive_div_up(W, BOX_W), hive_div_up(H, BOX_H), n), blk(SEG_THREADS);
    hipLaunchKernelGGL(box_kernel<false>, grid, blk, 0, ctx->stream, d_mask, H, W, iterations, tmp);
    hipLaunchKernelGGL(box_kernel<true>, grid, blk, 0, ctx->stream, (const uint8_t *)tmp, H, W, iterations, d_out);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

struct LabelJob {
    const uint8_t *mask;
    int n, H, W, connectivity, min_area;
    int *labels, *numbers;  // two planes of n * H * W int32; `labels` may be out_i32
    unsigned *partial;      // n * scan_chunks(H, W) words
    int32_t *out_i32 = nullptr;
    uint8_t *out_u8 = nullptr;
    int32_t *counts = nullptr, *areas = nullptr;
    int area_capacity = 0;
};
int scan_chunks(int H, int W) { return hive_div_up((long long)H * W, SEG_THREADS * SEG_SCAN_ITEMS); }
// The six launches; with a uint8 output, the one read-back: the first frame with more than 255 components fails the call
int label_run(hive_ctx *ctx, const LabelJob &j) {
    HIVE_REQUIRE(ctx, j.connectivity == 4 || j.connectivity == 8, "label_components: connectivity %d (4 or 8)", j.connectivity);
    HIVE_REQUIRE(ctx, j.min_area >= 0 && j.area_capacity >= 0, "label_components: min_area = %d, area_capacity = %d", j.min_area, j.area_capacity);
    const size_t per_frame = (size_t)j.H * j.W;
    hipStream_t st = ctx->stream;
    unsigned *over = ctx->d_scalars + SEG_SCALARS;
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(j.numbers, 0, per_frame * j.n * sizeof(int), st));
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(over, 0xff, sizeof(unsigned), st));
    const dim3 blk(SEG_THREADS), pixels(hive_div_up((long long)per_frame, SEG_THREADS), j.n);
    hipLaunchKernelGGL(label_tile_kernel, dim3(hive_div_up(j.W, SEG_TILE_W), hive_div_up(j.H, SEG_TILE_H), j.n), blk, 0, st, j.mask, j.H, j.W, j.connectivity, j.labels);
    hipLaunchKernelGGL(label_border_kernel, pixels, blk, 0, st, j.H, j.W, j.connectivity, j.labels);
    hipLaunchKernelGGL(label_flatten_kernel, pixels, blk, 0, st, j.H, j.W, j.labels, j.numbers);
    const dim3 chunks(scan_chunks(j.H, j.W), j.n);
    hipLaunchKernelGGL(label_count_kernel, chunks, blk, 0, st, j.H, j.W, j.min_area, (const int *)j.labels, (const int *)j.numbers, j.partial);
    hipLaunchKernelGGL(label_number_kernel, chunks, blk, 0, st, j.H, j.W, j.min_area, (const int *)j.labels, j.numbers, (const unsigned *)j.partial, j.counts, j.areas,
                       j.area_capacity, j.out_u8 ? 255 : 0, over);
    if (j.out_u8)
        hipLaunchKernelGGL(label_write_kernel<uint8_t>, pixels, blk, 0, st, per_frame, (const int *)j.labels, (const int *)j.numbers, j.out_u8);
    else
        hipLaunchKernelGGL(label_write_kernel<int32_t>, pixels, blk, 0, st, per_frame, (const int *)j.labels, (const int *)j.numbers, j.out_i32);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    if (!j.out_u8) return HIVE_OK;
    unsigned *h;
    int rc = hive_pinned_small(ctx, (void **)&h);
    if (rc) return rc;
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(h, over, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(st));
    const unsigned frame = h[0];
    if (frame == SEG_NO_FRAME) return HIVE_OK;
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(h, j.counts + frame, sizeof(int), hipMemcpyDeviceToHost, st));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(st));
    return hive_fail(ctx, HIVE_ERR_INVALID, "label_components: frame %u has %d components, more than the 255 a uint8 label holds; ask for int32 labels or a larger min_area",
                     frame, (int)h[0]);
}

// the context's generic scratch, at least lay.bytes() of it, as lay's base
int reserve(hive_ctx *ctx, hive_scratch_layout &lay) {
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, lay.bytes());
    if (rc) return rc;
    lay = hive_scratch_layout();
    lay.base = (char *)ctx->d_scratch;
    return HIVE_OK;
}

}  // namespace

extern "C" {

int hive_motion_mask(hive_ctx *ctx, const float *d_live, const float *d_model, int n, int H, int W, float min_difference, float relative_difference, uint8_t *d_mask) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_live && d_model && d_mask, "motion_mask: NULL argument");
    int rc = check_frames(ctx, "motion_mask", n, H, W);
    if (rc) return rc;
    return motion_run(ctx, d_live, d_model, (size_t)n * H * W, min_difference, relative_difference, d_mask);
}

int hive_mask_open(hive_ctx *ctx, const uint8_t *d_mask, int n, int H, int W, int iterations, uint8_t *d_out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_mask && d_out, "mask_open: NULL argument");
    int rc = check_frames(ctx, "mask_open", n, H, W);
    if (rc) return rc;
    const size_t total = (size_t)n * H * W;
    hive_scratch_layout lay;
    lay.take<uint8_t>(total);
    if ((rc = reserve(ctx, lay))) return rc;
    return open_run(ctx, d_mask, n, H, W, iterations, lay.take<uint8_t>(total), d_out);
}

int hive_label_components(hive_ctx *ctx, const uint8_t *d_mask, int n, int H, int W, int connectivity, int min_area, int label_bytes, void *d_labels,
                          int32_t *d_counts, int32_t *d_areas, int area_capacity) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_mask && d_labels && d_counts, "label_components: NULL argument");
    HIVE_REQUIRE(ctx, label_bytes == 1 || label_bytes == 4, "label_components: label_bytes = %d (4: int32, 1: uint8)", label_bytes);
    HIVE_REQUIRE(ctx, d_areas || area_capacity == 0, "label_components: area_capacity = %d without d_areas", area_capacity);
    int rc = check_frames(ctx, "label_components", n, H, W);
    if (rc) return rc;
    const size_t total = (size_t)n * H * W;
    hive_scratch_layout lay;
    const size_t words = (size_t)n * scan_chunks(H, W);
    lay.take<int>(total), lay.take<unsigned>(words);
    if (label_bytes == 1) lay.take<int>(total);
    if ((rc = reserve(ctx, lay))) return rc;
    LabelJob j{d_mask, n, H, W, connectivity, min_area};
    j.numbers = lay.take<int>(total), j.partial = lay.take<unsigned>(words);
    j.labels = label_bytes == 1 ? lay.take<int>(total) : (int *)d_labels;
    if (label_bytes == 1)
        j.out_u8 = (uint8_t *)d_labels;
    else
        j.out_i32 = (int32_t *)d_labels;
    j.counts = d_counts, j.areas = d_areas, j.area_capacity = area_capacity;
    return label_run(ctx, j);
}

int hive_motion_segment(hive_ctx *ctx, const float *d_live, const float *d_model, int n, int H, int W, float min_difference, float relative_difference,
                        int opening_iterations, int connectivity, int min_area, uint8_t *d_ids, int32_t *d_counts) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_live && d_model && d_ids && d_counts, "motion_segment: NULL argument");
    int rc = check_frames(ctx, "motion_segment", n, H, W);
    if (rc) return rc;
    const size_t total = (size_t)n * H * W;
    hive_scratch_layout lay;
    const size_t words = (size_t)n * scan_chunks(H, W);
    lay.take<int>(total), lay.take<int>(total), lay.take<unsigned>(words), lay.take<uint8_t>(total), lay.take<uint8_t>(total);
    if ((rc = reserve(ctx, lay))) return rc;
    LabelJob j{nullptr, n, H, W, connectivity, min_area};
    j.numbers = lay.take<int>(total), j.labels = lay.take<int>(total), j.partial = lay.take<unsigned>(words);
    uint8_t *raw = lay.take<uint8_t>(total), *tmp = lay.take<uint8_t>(total);
    // the raw mask, opened in place (open_run reads it into tmp first), labelled into d_ids
    if ((rc = motion_run(ctx, d_live, d_model, total, min_difference, relative_difference, raw))) return rc;
    if ((rc = open_run(ctx, raw, n, H, W, opening_iterations, tmp, raw))) return rc;
    j.mask = raw, j.out_u8 = d_ids, j.counts = d_counts;
    return label_run(ctx, j);
}

}  // extern "C"
