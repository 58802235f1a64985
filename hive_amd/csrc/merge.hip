// Sparse multi-GPU merge of TSDF volumes (hive_amd.distributed.fuse_sharded(merge="sparse")): only the observed SEGMENTS go through the collectives.  gfx950 only.
//
// A segment is a run of L consecutive voxels of the linear C-order index (z fastest): segment s = [s * L, min((s + 1) * L, N)), S = ceil(N / L), L a power of
// two in 64 .. 4096.  A segment is INACTIVE iff every weight word in it has the bit pattern of +0.0f (decided on the bits: a -0.0f is active and goes through
// the same arithmetic as in the dense merge).  Contract: a voxel of weight +0.0f holds the initial values (tsdf 1, colour 0) -- true of every volume the integrate
// kernels produce, and exactly what finalize_kernel writes for w == 0 -- so leaving an inactive segment untouched equals what the dense merge writes there.
//
//   mark     hive_tsdf_mark_segments / hive_mark_segments   weight plane -> u8 flags [S]: a wave covers 64 words of a segment per step, __ballot of "bits != 0"
//   list     hive_segment_list                              flags -> ascending indices of the active segments: block count -> scan -> write (as geometry.hip)
//   pack     hive_tsdf_accum_from_volume_segments / hive_accum_pack_segments   the listed segments' five sums, piece-major [world][5][per * L]
//   scatter  hive_tsdf_set_volume_segments                  all-gathered [world][3][per * L] -> the listed segments' voxels
//
// The fold between pack and scatter is hive_tsdf_accum_finalize_to with plane_stride = per * L.  Every offset is 64-bit (5 * 1024^3 elements).  All HBM-bound, no atomics.
#include "hive_internal.hpp"

#include <algorithm>

static bool segment_ok(int L) { return L >= 64 && L <= 4096 && (L & (L - 1)) == 0; }
static int log2_of(int L) {
    int s = 0;
    while ((1 << s) < L) ++s;
    return s;
}

// A wave takes MARK_SEGS consecutive segments per trip (grid-stride), so that 64-voxel segments still keep several loads in flight per lane: lane l reads
// word s * L + step + l of each; a lane past n -- the tail of the last segment, or a segment past the last -- reads nothing.
constexpr int MARK_SEGS = 4;
__global__ __launch_bounds__(256) void mark_segments_kernel(const unsigned *__restrict__ weight_bits, long long n, int L, long long n_segments,
                                                            uint8_t *__restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * 4 * MARK_SEGS;
    for (long long s0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * MARK_SEGS; s0 < n_segments; s0 += stride) {
        unsigned bits[MARK_SEGS] = {};  // (OR of the lane's words per segment: the loads are independent of each other)
        for (int step = 0; step < L; step += 64) {
#pragma unroll
            for (int j = 0; j < MARK_SEGS; ++j) {
                const long long i = (s0 + j) * L + step + lane;
                bits[j] |= i < n ? weight_bits[i] : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < MARK_SEGS; ++j) {
            const unsigned long long any = __ballot(bits[j] != 0u);
            if (lane == 0 && s0 + j < n_segments) flags[s0 + j] = any ? 1 : 0;
        }
    }
}

constexpr int SL_VPT = 4;
constexpr int SL_TILE = 256 * SL_VPT;  // flags per workgroup; a thread takes SL_VPT consecutive ones, which keeps the order

__global__ __launch_bounds__(256) void segment_count_kernel(const uint8_t *__restrict__ flags, long long n_segments, unsigned *__restrict__ blk) {
    __shared__ unsigned lds[4];
    const long long base = (long long)blockIdx.x * SL_TILE + threadIdx.x * SL_VPT;
    unsigned c[1] = {0};
    for (int j = 0; j < SL_VPT; ++j)
        if (base + j < n_segments && flags[base + j]) ++c[0];
    block_sum(c, lds);
    if (threadIdx.x == 0) blk[blockIdx.x] = c[0];
}

__global__ __launch_bounds__(256) void segment_write_kernel(const uint8_t *__restrict__ flags, long long n_segments, const unsigned *__restrict__ blk,
                                                            int32_t *__restrict__ list) {
    __shared__ unsigned lds[4];
    const long long base = (long long)blockIdx.x * SL_TILE + threadIdx.x * SL_VPT;
    bool on[SL_VPT];
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < SL_VPT; ++j) {
        on[j] = base + j < n_segments && flags[base + j];
        c += on[j];
    }
    long long id = (long long)blk[blockIdx.x] + block_exclusive(c, lds);  // < n_segments: the list has room for every segment
#pragma unroll
    for (int j = 0; j < SL_VPT; ++j)
        if (on[j]) list[id++] = (int32_t)(base + j);
}

// Where the merge buffers keep list entry k (k < world * per): piece k / per, segment slot k % per of that piece's planes of per * L floats.
struct SegmentLayout {
    const int32_t *list;
    long long n_active, per, n, n_segments;  // n voxels in n_segments segments
    int shift, planes;                       // L = 1 << shift; planes per piece (5 sums or 3 results)
    __device__ __forceinline__ long long slot_offset(long long k, int e) const {
        const long long piece = k / per, j = k - piece * per;
        return (piece * planes * per + j) << shift | e;
    }
    // the voxel behind lane e of list entry k, or -1 for padding (k past the list, a lane past n, an index that is no segment)
    __device__ __forceinline__ long long voxel(long long k, int e) const {
        if (k >= n_active) return -1;
        const long long s = list[k];
        if (s < 0 || s >= n_segments) return -1;
        const long long i = (s << shift) | e;
        return i < n ? i : -1;
    }
};

// VOLUME: (tsdf, weight, colour) -> the five sums; otherwise a0 = accumulator planes [5][n], gathered as they are.  Padding is written as zeros.
template <bool VOLUME>
__global__ __launch_bounds__(256) void pack_segments_kernel(const float *__restrict__ a0, const float *__restrict__ weight, const float *__restrict__ color,
                                                            SegmentLayout lay, long long total, float *__restrict__ out) {
    const long long stride = (long long)gridDim.x * 256;
    const long long plane = lay.per << lay.shift;
    const int mask = (1 << lay.shift) - 1;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += stride) {
        const long long k = g >> lay.shift;
        const int e = (int)(g & mask);
        const long long i = lay.voxel(k, e);
        float *o = out + lay.slot_offset(k, e);
        if (VOLUME) {
            float w = 0.f, t = 0.f;
            unsigned c = 0u;
            if (i >= 0) {
                w = weight[i];
                t = a0[i];
                c = (unsigned)color[i];
            }
            hive_voxel_sums(t, w, c, o, plane);
        } else {
#pragma unroll
            for (int p = 0; p < 5; ++p) o[p * plane] = i >= 0 ? a0[p * lay.n + i] : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void scatter_segments_kernel(const float *__restrict__ in, SegmentLayout lay, long long total, float *__restrict__ tsdf,
                                                               float *__restrict__ weight, float *__restrict__ color) {
    const long long stride = (long long)gridDim.x * 256;
    const long long plane = lay.per << lay.shift;
    const int mask = (1 << lay.shift) - 1;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += stride) {
        const long long k = g >> lay.shift;
        const int e = (int)(g & mask);
        const long long i = lay.voxel(k, e);
        if (i < 0) continue;
        const float *src = in + lay.slot_offset(k, e);
        tsdf[i] = src[0];
        weight[i] = src[plane];
        color[i] = src[2 * plane];
    }
}

static int grid_for(long long items) { return (int)std::min<long long>((items + 255) / 256, 256 * 32); }

static int check_layout(hive_ctx *ctx, const char *who, const void *d_list, int64_t n_active, int L, int world, int64_t per, int64_t n, const void *buf,
                        int planes, SegmentLayout *lay) {
    HIVE_REQUIRE(ctx, segment_ok(L), "%s: segment length %d is not a power of two in 64 .. 4096", who, L);
    const int64_t n_segments = (n + L - 1) / L;
    HIVE_REQUIRE(ctx, n_active >= 0 && n_active <= n_segments, "%s: %lld active segments of %lld", who, (long long)n_active, (long long)n_segments);
    HIVE_REQUIRE(ctx, world > 0 && per >= 0 && (int64_t)world * per >= n_active, "%s: need world * per >= %lld segments (world %d, per %lld)", who, (long long)n_active,
                 world, (long long)per);
    HIVE_REQUIRE(ctx, n_active == 0 || (d_list && buf), "%s: NULL argument", who);
    lay->list = (const int32_t *)d_list;
    lay->n_active = n_active;
    lay->per = per;
    lay->n = n;
    lay->n_segments = n_segments;
    lay->shift = log2_of(L);
    lay->planes = planes;
    return HIVE_OK;
}

static int mark_segments(hive_ctx *ctx, const float *d_weight, int64_t n, int L, uint8_t *d_flags) {
    HIVE_REQUIRE(ctx, segment_ok(L), "mark_segments: segment length %d is not a power of two in 64 .. 4096", L);
    HIVE_REQUIRE(ctx, d_weight && d_flags && n > 0, "mark_segments: bad argument");
    const long long n_segments = (n + L - 1) / L;
    const int blocks = (int)std::min<long long>((n_segments + 4 * MARK_SEGS - 1) / (4 * MARK_SEGS), (long long)ctx->num_cus * 8);
    hipLaunchKernelGGL(mark_segments_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const unsigned *)d_weight, (long long)n, L, n_segments, d_flags);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

static int pack_segments(hive_ctx *ctx, bool volume, const float *a0, const float *weight, const float *color, const SegmentLayout &lay, int world, float *d_out) {
    if (lay.n_active == 0) return HIVE_OK;
    const long long total = ((long long)world * lay.per) << lay.shift;
    if (volume)
        hipLaunchKernelGGL(pack_segments_kernel<true>, dim3(grid_for(total)), dim3(256), 0, ctx->stream, a0, weight, color, lay, total, d_out);
    else
        hipLaunchKernelGGL(pack_segments_kernel<false>, dim3(grid_for(total)), dim3(256), 0, ctx->stream, a0, weight, color, lay, total, d_out);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

extern "C" {

int hive_mark_segments(hive_ctx *ctx, const float *d_weight, int64_t n, int L, uint8_t *d_flags) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    return mark_segments(ctx, d_weight, n, L, d_flags);
}

int hive_tsdf_mark_segments(hive_tsdf *v, int L, uint8_t *d_flags) {
    HIVE_ENTER(v ? v->ctx : nullptr);
    if (!v) return hive_fail(nullptr, HIVE_ERR_INVALID, "vol is NULL");
    return mark_segments(v->ctx, v->d_weight, v->n, L, d_flags);
}

int hive_segment_list(hive_ctx *ctx, const uint8_t *d_flags, int64_t n_segments, int32_t *d_list, int64_t *d_count) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_flags && d_list && d_count, "segment_list: NULL argument");
    HIVE_REQUIRE(ctx, n_segments > 0 && n_segments <= INT32_MAX, "segment_list: %lld segments", (long long)n_segments);
    const int nb = (int)((n_segments + SL_TILE - 1) / SL_TILE);
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, (size_t)nb * sizeof(unsigned));
    if (rc) return rc;
    unsigned *blk = (unsigned *)ctx->d_scratch;
    hipLaunchKernelGGL(segment_count_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_flags, (long long)n_segments, blk);
    hive_scan_counts(ctx, nb, (unsigned long long *)d_count, blk);  // (the total is below 2^31: the same bits as i64)
    hipLaunchKernelGGL(segment_write_kernel, dim3(nb), dim3(256), 0, ctx->stream, d_flags, (long long)n_segments, (const unsigned *)blk, d_list);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_tsdf_accum_from_volume_segments(hive_tsdf *v, const int32_t *d_list, int64_t n_active, int L, int world, int64_t per, float *d_out) {
    HIVE_ENTER(v ? v->ctx : nullptr);
    if (!v) return hive_fail(nullptr, HIVE_ERR_INVALID, "vol is NULL");
    SegmentLayout lay;
    int rc = check_layout(v->ctx, "accum_from_volume_segments", d_list, n_active, L, world, per, v->n, d_out, 5, &lay);
    if (rc) return rc;
    return pack_segments(v->ctx, true, v->d_tsdf, v->d_weight, v->d_color, lay, world, d_out);
}

int hive_accum_pack_segments(hive_ctx *ctx, const float *d_accum, int64_t n, const int32_t *d_list, int64_t n_active, int L, int world, int64_t per,
                             float *d_out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_accum && n > 0, "accum_pack_segments: bad argument");
    SegmentLayout lay;
    int rc = check_layout(ctx, "accum_pack_segments", d_list, n_active, L, world, per, n, d_out, 5, &lay);
    if (rc) return rc;
    return pack_segments(ctx, false, d_accum, nullptr, nullptr, lay, world, d_out);
}

int hive_tsdf_set_volume_segments(hive_tsdf *v, const int32_t *d_list, int64_t n_active, int L, int world, int64_t per, const float *d_in) {
    HIVE_ENTER(v ? v->ctx : nullptr);
    if (!v) return hive_fail(nullptr, HIVE_ERR_INVALID, "vol is NULL");
    hive_ctx *ctx = v->ctx;
    SegmentLayout lay;
    int rc = check_layout(ctx, "set_volume_segments", d_list, n_active, L, world, per, v->n, d_in, 3, &lay);
    if (rc) return rc;
    if (n_active == 0) return HIVE_OK;
    const long long total = (long long)n_active << lay.shift;
    hipLaunchKernelGGL(scatter_segments_kernel, dim3(grid_for(total)), dim3(256), 0, ctx->stream, d_in, lay, total, v->d_tsdf, v->d_weight, v->d_color);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    v->n_verts = v->n_faces = -1;
    v->unit_weights = false;
    return HIVE_OK;
}

}  // extern "C"
