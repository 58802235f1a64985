// Internal declarations shared by the translation units of libhive_mi355x.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hive_mi355x.h"

#define HIVE_WAVE 64

struct hive_staging_slot {
    void *pinned = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool in_flight = false;
};

struct hive_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    int round_mode = HIVE_ROUND_HALF_EVEN;
    std::string last_error;

    // host -> device staging ring (pinned), so that a HOST call may return before the copy lands
    static constexpr int kSlots = 4;
    hive_staging_slot slots[kSlots];
    int next_slot = 0;

    // generic device scratch (grown on demand, never shrunk)
    void *d_scratch = nullptr;
    size_t scratch_bytes = 0;
    // packed frame {depth bits, rgb} + per-frame scalars
    void *d_frame = nullptr;
    size_t frame_bytes = 0;
    void *d_batch = nullptr;  // texels + tile maxima of a prepared batch of frames (tsdf.hip prepare_batch)
    size_t batch_bytes = 0;
    void *d_in = nullptr;  // device copy of host inputs
    size_t in_bytes = 0;
    int tsdf_scalars = 0;           // which of the two TSDF scalar blocks the frame in flight uses (tsdf.hip prepare_frame)
    int tsdf_multi_scalars = 0;     // the same for the fused sweep's blocks (SC_TSDF_SWEEP_A / _B)
    unsigned *d_scalars = nullptr;  // HIVE_SCALAR_WORDS words of small results and counters: the map of its regions is below (SC_*)
    void *h_pinned_small = nullptr;  // 512 bytes of pinned host memory for small read-backs (mesh totals, the tracker's 58 sums), allocated on first use: hive_pinned_small
    void *d_zeros = nullptr;        // 256 bytes of zeros: the source of padding taps in the implicit-GEMM convolutions
    // split-K of the MFMA tile kernels at small batches (mfma_pipe.hpp splitk_*): f32 partial tiles + one arrival counter per tile (zero between launches)
    void *d_splitk = nullptr;
    size_t splitk_bytes = 0;
    unsigned *d_splitk_count = nullptr;
    void *d_gram = nullptr;  // partial Gram matrices / sums / quadratic forms of gram.hip (GroupNorm statistics of 1 x 1 convolutions)
    size_t gram_bytes = 0;

    // hive_ctx_set_deterministic: no split-K, no key split inside the attention workgroup, no Gram-matrix GroupNorm statistics (the three paths whose use
    // depends on the batch size and the CU count)
    bool deterministic = false;
    // launches of the small-launch paths since creation / the last reset (hive_ctx_launch_stats): split-K items, four-stage-ring kernels
    int64_t n_splitk_launches = 0, n_deep_ring_launches = 0;

    // HIP-event timing of the dominant kernel
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    hipEvent_t last_start = nullptr, last_stop = nullptr;
};

// The map of hive_ctx::d_scalars: every region, offset and extent in words, in ascending order.  A new user takes a gap (or the tail) and adds its
// line here and to HIVE_SCALAR_MAP; the static_assert below refuses regions that overlap or leave the allocation.  Offsets INSIDE a region
// (MS_NITEMS, MS_HIST, ... of a sweep block, the [4] of a per-frame block) belong to the kernels that use them and stay beside those kernels.
constexpr int HIVE_SCALAR_WORDS = 4096;                // what hive_ctx_create allocates and zeroes
constexpr int COUNT_SLOTS = 64, COUNT_STRIDE = 16;     // update counters of the TSDF COUNT kernels: 64 x u64, 128 bytes apart
constexpr int MS_STRIDE = 512;                         // words of one scalar block of a fused TSDF sweep
constexpr int SC_TSDF_FRAME_WORDS = 8;                 // words of one per-frame TSDF block (prep_frame_kernel clears the other block: this many)
constexpr int SC_TSDF_FRAME_A = 0;                     // tsdf.hip: the two per-frame blocks alternate (A here, B below)
constexpr int SC_MC_TOTALS = 8, SC_MC_TOTALS_WORDS = 4;            // mcubes.hip: vertex and face totals of an extraction (2 x u64)
constexpr int SC_UNPROJECT_TOTAL = 20, SC_UNPROJECT_TOTAL_WORDS = 2;  // geometry.hip hive_unproject: the point count (u64)
constexpr int SC_PROJECT_BBOX = 24, SC_PROJECT_BBOX_WORDS = 5;     // geometry.hip hive_project_bbox: min u, max u, min v, max v, count
constexpr int SC_GRID_TOTALS = 32, SC_GRID_TOTALS_WORDS = 2;       // fgmesh.hip hive_grid_mesh: vertices, faces
constexpr int SC_FILTER_TOTAL = 34, SC_FILTER_TOTAL_WORDS = 1;     // fgmesh.hip hive_filter_faces: faces kept
constexpr int SC_WINDOW_BOX = 40, SC_WINDOW_BOX_WORDS = 4;         // fgmesh.hip hive_texture_window: the box of the projected points
constexpr int SC_TSDF_FRAME_B = 48;                                // tsdf.hip: the other per-frame block
constexpr int SC_TSDF_COUNTERS = 128, SC_TSDF_COUNTERS_WORDS = COUNT_SLOTS * COUNT_STRIDE * 2;  // tsdf.hip: COUNT_SLOTS * COUNT_STRIDE u64s
constexpr int MS_BASE = 2304;                          // tsdf.hip: the two alternating blocks of the fused sweep, MS_STRIDE words each
constexpr int CC_SCALARS = 3584, CC_SCALARS_WORDS = 14;            // fgmesh.hip: the clean-up's / the frame mesh runner's block, [0..13]
constexpr int DEC_SCALARS = 3712, DEC_SCALARS_WORDS = 20;          // decimate.hip: [0..15] hive_decimate_run, [16..19] hive_mesh_decimate's counts
constexpr int SEG_SCALARS = 3744, SEG_SCALARS_WORDS = 1;           // segment.hip: the first frame with more components than a uint8 label holds
constexpr int TXS_SCALARS = 3752, TXS_SCALARS_WORDS = 24;         // texture_smooth.hip: 9 x u64 of hive_texture_smooth, behind them 2 x u64 of hive_mesh_face_neighbours
struct hive_scalar_region {
    int at, words;
};
constexpr hive_scalar_region HIVE_SCALAR_MAP[] = {
    {SC_TSDF_FRAME_A, SC_TSDF_FRAME_WORDS},          {SC_MC_TOTALS, SC_MC_TOTALS_WORDS},       {SC_UNPROJECT_TOTAL, SC_UNPROJECT_TOTAL_WORDS},
    {SC_PROJECT_BBOX, SC_PROJECT_BBOX_WORDS},        {SC_GRID_TOTALS, SC_GRID_TOTALS_WORDS},   {SC_FILTER_TOTAL, SC_FILTER_TOTAL_WORDS},
    {SC_WINDOW_BOX, SC_WINDOW_BOX_WORDS},            {SC_TSDF_FRAME_B, SC_TSDF_FRAME_WORDS},   {SC_TSDF_COUNTERS, SC_TSDF_COUNTERS_WORDS},
    {MS_BASE, MS_STRIDE},                            {MS_BASE + MS_STRIDE, MS_STRIDE},         {CC_SCALARS, CC_SCALARS_WORDS},
    {DEC_SCALARS, DEC_SCALARS_WORDS},                {SEG_SCALARS, SEG_SCALARS_WORDS},         {TXS_SCALARS, TXS_SCALARS_WORDS},
};
constexpr bool hive_scalar_map_ok() {
    int end = 0;
    for (const hive_scalar_region &r : HIVE_SCALAR_MAP) {
        if (r.at < end || r.words <= 0) return false;
        end = r.at + r.words;
    }
    return end <= HIVE_SCALAR_WORDS;
}
static_assert(hive_scalar_map_ok(), "hive_ctx::d_scalars: each region starts at or after the end of the one before it, and the last ends inside the allocation");

int hive_fail(hive_ctx *ctx, int code, const char *fmt, ...);

// Every extern "C" entry point runs with its context's device current and puts the caller's device back on
// return: a context (or a volume / ViT engine built on it) may belong to a GPU other than the calling
// thread's current one -- kernels, copies and allocations must land on the context's GPU, and the caller's
// (PyTorch's) current device must not change behind its back.
struct hive_device_guard {
    int prev = -1;
    bool switched = false;
    explicit hive_device_guard(const hive_ctx *ctx) {
        if (!ctx) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != ctx->device) switched = hipSetDevice(ctx->device) == hipSuccess;
    }
    ~hive_device_guard() {
        if (switched) (void)hipSetDevice(prev);
    }
    hive_device_guard(const hive_device_guard &) = delete;
    hive_device_guard &operator=(const hive_device_guard &) = delete;
};
#define HIVE_ENTER(ctx) hive_device_guard _hive_device_guard(ctx)
void hive_set_global_error(const char *msg);

#define HIVE_CHECK_HIP(ctx, expr)                                                                        \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess)                                                                            \
            return hive_fail((ctx), _e == hipErrorOutOfMemory ? HIVE_ERR_NOMEM : HIVE_ERR_DEVICE,        \
                             "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

#define HIVE_REQUIRE(ctx, cond, ...)                                   \
    do {                                                               \
        if (!(cond)) return hive_fail((ctx), HIVE_ERR_INVALID, __VA_ARGS__); \
    } while (0)

// Once per device: the latch of a launcher's hipFuncSetAttribute block (a function-local static: hipFuncAttributeMaxDynamicSharedMemorySize is a property of
// the kernel ON a device).  `if (!latch.done(ctx)) { ... set the attributes ...; latch.mark(ctx); }`; devices past 63 set them every time.
struct hive_device_latch {
    bool set[64] = {};
    bool done(const hive_ctx *ctx) const { return ctx->device < 64 && set[ctx->device]; }
    void mark(const hive_ctx *ctx) {
        if (ctx->device < 64) set[ctx->device] = true;
    }
};

// grows *ptr to at least `bytes` of device memory
int hive_reserve_device(hive_ctx *ctx, void **ptr, size_t *cur, size_t bytes);
// the context's 512 bytes of pinned host memory for small read-backs (allocated on first use)
int hive_pinned_small(hive_ctx *ctx, void **out);
// copies `bytes` from host memory to device memory `dst` through the pinned ring; returns once the
// host buffer may be reused by the caller
int hive_upload(hive_ctx *ctx, void *dst, const void *src, size_t bytes);
// dpt_ops.hip: (mean, rstd) per (sample, group) from the per-tile channel sums a GN convolution epilogue left (conv.hip)
int hive_gn_finalize_tiles(hive_ctx *ctx, const float *d_partial, int N, int HW, int C, int G, int tile_rows, float eps, float *d_stats);
// conv.hip: THE eligibility of the two-pass conv + GroupNorm, for its launchers hive_nhwc_conv_gn_apply and hive_nhwc_conv_gn_apply_gram (declared in
// hive_mi355x.h; *fused = 0 otherwise), for hive_gn_gram_preferred and for the network object, which allocates the pair's intermediate where it fails:
// whole 256-channel tiles, a lane's 8 channels inside one group, a tile inside two samples
inline bool hive_conv_gn_two_pass_eligible(int C_out, int G, long long hw_out) {
    return G > 0 && C_out % 256 == 0 && C_out % G == 0 && (C_out / G) % 8 == 0 && hw_out >= 256;
}
// split-K workspace of at least `bytes` and the (zeroed) arrival counters (HIVE_SPLITK_TILES of them)
constexpr int HIVE_SPLITK_TILES = 4096;
int hive_splitk_workspace(hive_ctx *ctx, size_t bytes, void **ws, unsigned **count);
// gram.hip: (mean, rstd)[N][G] of GroupNorm(conv1x1(x, w)) from the Gram matrices of x and the tables hive_gn_gram_prepare made of w
int hive_gram_gn_stats(hive_ctx *ctx, const void *d_x, int dtype, int N, int H, int W, int C_in, int C_out, int stride, int Ho, int Wo, int G, const float *d_tables,
                       float eps, float *d_stats, float *d_S_out, float *d_s_out);
// block-wide exclusive offset of this thread's count `c` in a 256-thread workgroup (4 consecutive items per thread keep row-major order)
__device__ __forceinline__ unsigned block_exclusive(unsigned c, unsigned *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = c;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += lds[w];
    __syncthreads();
    return before + inc - c;
}
// block_exclusive, and the workgroup's total in *total (every thread gets it)
__device__ __forceinline__ unsigned block_exclusive_total(unsigned c, unsigned *lds, unsigned *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = c;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int w = 0; w < 256 / 64; ++w) {
        if (w < wave) before += lds[w];
        all += lds[w];
    }
    __syncthreads();
    *total = all;
    return before + inc - c;
}
// ---- the two float64 workgroup sums whose order include/hive_mi355x.h states; float64 without contraction, so the bits depend on the values alone ----
// The fixed tree: v[q][0] = the sum of v[q][0 .. THREADS) for each of the COLS columns by v[q][t] += v[q][t + off], off = THREADS / 2 .. 1, one barrier per
// level for all columns.  Every thread of the THREADS-thread workgroup calls it after writing its own v[q][threadIdx.x]; the sums are there for every thread
// on return (similarity.hip, lpips.hip, track.hip)
template <int THREADS, int COLS>
__device__ __forceinline__ void block_tree_sum(double (*v)[THREADS]) {
    const int t = threadIdx.x;
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int q = 0; q < COLS; ++q) v[q][t] = v[q][t] + v[q][t + off];
        }
        __syncthreads();
    }
}
// the butterfly over the 64 lanes of a wave, s = s + s[lane ^ off], off = 32 .. 1: every lane gets the same total (fts.hip: a chunk's sums, one wave each)
__device__ __forceinline__ double wave_butterfly_sum(double s) {
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
// s[0 .. COUNT) over a 256-thread workgroup: the butterfly in every wave, then the four waves left to right; valid in thread 0 alone.  `lds` holds a row per
// wave.  No barrier behind the sum: no caller (fts.hip's centroid kernels, poseopt.hip's loss and step kernels) touches `lds` again or reads another
// thread's result; one that did would put its own barrier in between.  The butterfly is wave_butterfly_sum per value with the offsets outermost: value by
// value the same additions, but po_step_kernel<false, true> needs 166 VGPRs in place of 120 when the values are outermost
template <int COUNT, int WIDTH>
__device__ __forceinline__ void block_butterfly_sum(double *s, double (*lds)[WIDTH]) {
    static_assert(COUNT <= WIDTH, "a row of lds holds every value");
    for (int off = 32; off > 0; off >>= 1)
        for (int j = 0; j < COUNT; ++j) s[j] += __shfl_xor(s[j], off);
    if ((threadIdx.x & 63) == 0)
        for (int j = 0; j < COUNT; ++j) lds[threadIdx.x >> 6][j] = s[j];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int j = 0; j < COUNT; ++j) s[j] = ((lds[0][j] + lds[1][j]) + lds[2][j]) + lds[3][j];
}
// a bijection of the 32-bit integers that scatters neighbouring ids: the tie-break of the decimation's collapse keys (decimate.hip) and of the label smoothing's
// appliers (texture_smooth.hip), neither of which may follow the numbering of the mesh
__device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    return x ^ (x >> 16);
}
// ceil(a / b) for launch grids
inline int hive_div_up(long long a, int b) { return (int)((a + b - 1) / b); }
// A 256-thread workgroup scans `count` values 256 at a time: store(i, the sum of load(0 .. i - 1)) for every i < count; returns the sum of all (in every
// thread).  Every thread of the workgroup calls it with the same count
template <class Load, class Store>
__device__ __forceinline__ unsigned block_scan_chunks(unsigned count, unsigned *lds, Load load, Store store) {
    unsigned carry = 0;
    for (unsigned base = 0; base < count; base += 256) {
        const unsigned i = base + threadIdx.x;
        unsigned chunk;
        const unsigned at = block_exclusive_total(i < count ? load(i) : 0u, lds, &chunk);
        if (i < count) store(i, carry + at);
        carry += chunk;
    }
    return carry;
}
// ---- the order-preserving compactions (geometry, fgmesh, mesh_compact, merge, mcubes): count per workgroup, scan the block counts, place ----
// The count step.  Sums of N per-thread counts over a 256-thread workgroup: the butterfly in every wave, then the four waves; the sums are in c[] of thread 0
// alone.  `lds` holds 4 N words; no barrier behind the sum, as in block_butterfly_sum
template <int N>
__device__ __forceinline__ void block_sum(unsigned (&c)[N], unsigned *lds) {
    for (int off = 32; off > 0; off >>= 1)
        for (int k = 0; k < N; ++k) c[k] += (unsigned)__shfl_xor((int)c[k], off);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < N; ++k) lds[4 * k + (threadIdx.x >> 6)] = c[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < N; ++k) c[k] = lds[4 * k] + lds[4 * k + 1] + lds[4 * k + 2] + lds[4 * k + 3];
}
// The scan step.  ONE workgroup of SCAN_THREADS scans (exclusive, in place) N arrays of nb block counts each; total[k] = the sum of array k.  Thread t sums
// its run [t per, t per + per), per = ceil(nb / SCAN_THREADS), of every array; the first lane of wave k walks array k's partials serially, so the N walks run
// side by side and two arrays cost what one costs (the walk ends behind the last thread that has a run); then every thread rewrites its runs.  Partials and
// totals are of type Total (unsigned or unsigned long long; an offset is what fits the array's 32 bits).  The arrays must not overlap
constexpr int SCAN_THREADS = 1024;
template <int N, class Total>
__device__ __forceinline__ void block_scan_counts(unsigned *const (&a)[N], int nb, Total *total) {
    static_assert(N <= SCAN_THREADS / 64, "a wave walks each array");
    __shared__ Total part[N][SCAN_THREADS];
    const int t = threadIdx.x;
    const int per = max((nb + SCAN_THREADS - 1) / SCAN_THREADS, 1);
    const int lo = min(t * per, nb), hi = min(lo + per, nb);
    const int used = (nb + per - 1) / per;  // threads with a run: the ones behind them add zeros and read no offset
    Total r[N] = {};
    for (int i = lo; i < hi; ++i) {
        unsigned v[N];
        for (int k = 0; k < N; ++k) v[k] = a[k][i];
        for (int k = 0; k < N; ++k) r[k] += v[k];
    }
    for (int k = 0; k < N; ++k) part[k][t] = r[k];
    __syncthreads();
    if ((t & 63) == 0 && (t >> 6) < N) {
        Total *p = part[t >> 6], sum = 0;
        // over the partials of the threads with a run, in whole chunks of 32 (the loads of a chunk are issued together)
        for (int i = 0; i < used; i += 32)
#pragma unroll
            for (int j = i; j < i + 32; ++j) {
                const Total v = p[j];
                p[j] = sum;
                sum += v;
            }
        total[t >> 6] = sum;
    }
    __syncthreads();
    for (int k = 0; k < N; ++k) r[k] = part[k][t];
    for (int i = lo; i < hi; ++i) {
        unsigned v[N];
        for (int k = 0; k < N; ++k) v[k] = a[k][i];
        for (int k = 0; k < N; ++k) {
            a[k][i] = (unsigned)r[k];
            r[k] += v[k];
        }
    }
}
// (one parameter per array: __restrict__ on each lets a run's loads pass the stores of the count before)
template <class Total, class... Counts>
__global__ __launch_bounds__(SCAN_THREADS) void scan_counts_kernel(int nb, Total *total, Counts *__restrict__... a) {
    unsigned *const arrays[] = {a...};
    block_scan_counts(arrays, nb, total);
}
template <class Total, class... Counts>
inline void hive_scan_counts(hive_ctx *ctx, int nb, Total *total, Counts *... a) {
    hipLaunchKernelGGL((scan_counts_kernel<Total, Counts...>), dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, nb, total, a...);
}
// ---- the exclusive scan of n counts behind the vertex -> faces lists (texture_smooth.hip, texture_level.hip): tile sums, hive_scan_counts over them, offsets ----
constexpr int HIVE_SCAN_TILE = 1024;  // items per 256-thread workgroup (4 consecutive items per thread keep the order)
// the sum of c[0 .. n) per tile; the grid covers item n as well (an empty item), so that tile_offsets_kernel writes out[n] = the total
template <int TILE>
__global__ __launch_bounds__(256) void tile_sums_kernel(const unsigned *__restrict__ c, long long n, unsigned *__restrict__ tiles) {
    __shared__ unsigned lds[4];
    unsigned s[1] = {0};
    for (int j = 0; j < TILE / 256; ++j) {
        const long long i = (long long)blockIdx.x * TILE + threadIdx.x * (TILE / 256) + j;
        if (i < n) s[0] += c[i];
    }
    block_sum(s, lds);
    if (threadIdx.x == 0) tiles[blockIdx.x] = s[0];
}
// out[i] = the sum of c[0 .. i) for i in [0, n]; tiles: the scanned tile sums
template <int TILE, class Out>
__global__ __launch_bounds__(256) void tile_offsets_kernel(const unsigned *__restrict__ c, long long n, const unsigned *__restrict__ tiles, Out *__restrict__ out) {
    __shared__ unsigned lds[4];
    const long long base = (long long)blockIdx.x * TILE + threadIdx.x * (TILE / 256);
    unsigned v[TILE / 256], mine = 0;
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
        v[j] = base + j < n ? c[base + j] : 0u;
        mine += v[j];
    }
    unsigned long long o = (unsigned long long)tiles[blockIdx.x] + block_exclusive(mine, lds);
#pragma unroll
    for (int j = 0; j < TILE / 256; ++j) {
        if (base + j <= n) out[base + j] = (Out)o;
        o += v[j];
    }
}
// the last of n >= 1 table rows whose first element first_of(row) is not after `at` (rows ascend; row 0 starts at or before every `at` asked for)
template <class At, class FirstOf>
__device__ __forceinline__ int last_not_after(int n, At at, FirstOf first_of) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first_of(mid) <= at)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
// regions of one block of device scratch, 256-byte aligned, in the order they are taken.  With a null base the layout only sizes: take() returns
// null, bytes() is what to reserve; the same takes over the reserved block then give the pointers.
struct hive_scratch_layout {
    char *base = nullptr;
    size_t off = 0;
    template <class T>
    T *take(size_t count) {
        T *at = base ? (T *)(base + off) : nullptr;
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return at;
    }
    size_t bytes() const { return off; }
};
// ---- the host frame the picture encoders share (jpeg.hip, png.hip); `name` is "jpeg" / "png" in the error texts ----
inline int hive_picture_sides(hive_ctx *ctx, const char *name, int i, int height, int width) {
    HIVE_REQUIRE(ctx, height >= 1 && height <= 65535 && width >= 1 && width <= 65535, "%s: picture %d is %d x %d (sides of 1 .. 65535)", name, i, height, width);
    return HIVE_OK;
}
inline int hive_picture_room(hive_ctx *ctx, const char *name, int64_t out_bytes, int64_t total_bytes) {
    HIVE_REQUIRE(ctx, out_bytes >= total_bytes, "%s_encode: out_bytes = %lld is too small: hive_%s_layout asks for %lld bytes", name, (long long)out_bytes, name,
                 (long long)total_bytes);
    return HIVE_OK;
}
// the picture table and, behind it in the same block of scratch, the tables struct: one upload
template <class Row, class Tables>
int hive_upload_tables(hive_ctx *ctx, Row *d_rows, const std::vector<Row> &rows, Tables *d_tab, const Tables &tables) {
    const size_t tab_at = (size_t)((char *)d_tab - (char *)d_rows);
    std::vector<uint8_t> both(tab_at + sizeof(Tables), 0);
    memcpy(both.data(), rows.data(), rows.size() * sizeof(Row));
    memcpy(both.data() + tab_at, &tables, sizeof(Tables));
    return hive_upload(ctx, d_rows, both.data(), both.size());
}
// behind the launches: the files' sizes into the caller's array, and the stream drained
inline int hive_read_sizes(hive_ctx *ctx, const long long *d_sizes, int n, int64_t *sizes) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the kernels write long long, the caller reads int64_t");
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(sizes, d_sizes, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return HIVE_OK;
}
// decimate.hip: quadric edge collapse of a device-resident mesh (hive_mesh_decimate), for the entry points of any translation unit
struct hive_dec_job {
    const double *pos;                   // [V][3]
    const int32_t *faces;                // [F][3]
    const unsigned *counts;              // device: [0] = V, [1] = F (at most vert_cap / face_cap)
    long long vert_cap = 0, face_cap = 0;
    long long budget = 0;
    double max_error = 0.0;
    int32_t *out_faces = nullptr;        // [F][3] room for out_face_cap rows
    long long out_face_cap = 0;
    int32_t *out_vertex_index = nullptr; // optional [V]: input ids of the surviving vertices in order
    unsigned *out_counts = nullptr;      // device: [0] = vertices out, [1] = faces out
};
// bytes of scratch a job of these capacities needs; the vertex map (input id -> output row or -1, [V] i32) is at hive_decimate_vmap(scratch)
size_t hive_decimate_scratch_bytes(long long vert_cap, long long face_cap);
int32_t *hive_decimate_vmap(void *scratch, long long vert_cap, long long face_cap);
// runs every round (polling the device between batches of rounds) and the output compaction on ctx->stream; stats = {rounds, collapses, locked vertices}
int hive_decimate_run(hive_ctx *ctx, const hive_dec_job &job, void *scratch, int64_t stats[3]);
// geometry.hip: hive_dilate_mask_se over n frames on the device (se in host memory).  a, b: two planes of n * H * W bytes; the dilated masks
// (0 / 1) are left in b
int hive_dilate_frames(hive_ctx *ctx, const uint8_t *d_mask, int n, int H, int W, const uint8_t *se, int kh, int kw, int iterations, uint8_t *a, uint8_t *b);
// event helpers for kernel timing
int hive_time_begin(hive_ctx *ctx);
int hive_time_end(hive_ctx *ctx);

struct hive_tsdf {
    hive_ctx *ctx = nullptr;
    int64_t dim[3] = {0, 0, 0};
    int64_t n = 0;
    int64_t x_off = 0;      // x-slab of a larger scene grid: this volume holds grid voxels x_off <= x < x_off + dim[0]
    int64_t grid_dim0 = 0;  // x dimension of the whole grid
    double bnds[6] = {0, 0, 0, 0, 0, 0};
    float origin[3] = {0, 0, 0};
    float voxel_size = 0.f;
    float trunc = 0.f;
    float *d_tsdf = nullptr, *d_weight = nullptr, *d_color = nullptr;
    bool owns = false;
    // pixel / colour rounding of integrate, finalize and the mesh colour lookup of THIS volume (hive_round_mode):
    // a property of the volume, not of the context, so that two volumes of one thread may differ
    int round_mode = HIVE_ROUND_HALF_EVEN;
    // frames per sweep of the most recent hive_tsdf_integrate_batch (1 = the single-frame kernel), in launch order
    std::vector<int> last_groups;
    // true while every weight of the volume is a whole number of unit observations: set by create / reset, kept by integrate calls with
    // obs_weight == 1 (at most 65533 frames: unit_frames), cleared by anything else that writes the planes (other observation weights,
    // set_volume / set_volume_range / set_volume_segments / accum_finalize, hive_tsdf_planes_modified).  Selects the division-free colour update (tsdf.hip).
    bool unit_weights = true;
    int64_t unit_frames = 0;
    // frames handed to the integrate entry points / integrate launches since creation or the last reset (hive_tsdf_stats)
    int64_t frames_seen = 0, launches_seen = 0;
    // device word holding the work-list length of the most recent sweep (valid until the next sweep but one on this context)
    const unsigned *last_n_items = nullptr;
    // mesh extraction results (device)
    int64_t n_verts = -1, n_faces = -1;
    int64_t cap_verts = 0, cap_faces = 0;  // capacity of the result arrays below (kept between extractions, grown on demand)
    float *d_verts = nullptr, *d_norms = nullptr, *d_verts_vox = nullptr;
    int32_t *d_faces = nullptr;
    uint8_t *d_vcolors = nullptr;
    // mesh scratch
    uint32_t *d_vbase = nullptr;  // per voxel: first vertex id | axis mask << 29
    size_t vbase_bytes = 0;
    uint32_t *d_blk = nullptr;  // per block counts / offsets
    size_t blk_bytes = 0;
};

void hive_tsdf_free_mesh(hive_tsdf *vol);

// rounding shared by device code: RM = 0 half-even (np.round), 1 half-away (roundf)
template <int RM>
__device__ __forceinline__ float hive_round(float x) {
    if (RM == 0) return rintf(x);
    return roundf(x);
}

// One voxel of a running-average volume (tsdf t, weight w, packed colour c) -> its five sums [t * w, w, r * w, g * w, b * w] at o[0], o[plane], ... o[4 * plane]:
// what a rank contributes to the merge.  ONE statement of these products for every layout the sums are written in (tsdf.hip, merge.hip): the dense and the
// sparse merge are bit-identical only as long as they share it.
__device__ __forceinline__ void hive_voxel_sums(float t, float w, unsigned c, float *__restrict__ o, long long plane) {
    o[0] = t * w;  // w == 0 (never observed): tsdf is 1, the sum is 0
    o[plane] = w;
    o[2 * plane] = (float)(c & 255u) * w;
    o[3 * plane] = (float)((c >> 8) & 255u) * w;
    o[4 * plane] = (float)(c >> 16) * w;
}
