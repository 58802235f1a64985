// Billboard: every foreground object flattened to the median camera-space depth of its vertices (hive/pipeline.py:439-447).  gfx950 only.
//
//   hive_fg_billboard -> camera_space_points = rotation @ (vertices.T + translation)
//                        camera_space_points[2, :] = np.median(camera_space_points[2, :])
//                        vertices = (rotation.T @ (camera_space_points - translation)).T
//
// The reference's map is R (p + t) and back R^T (c - t) -- NOT world2image's R p + t; for t != 0 the two are not inverses of each other.  It is
// restated literally.  Float64, compiled without contraction (no fused multiply-add), in this operation order (R row-major, p = (x, y, z)):
//
//   forward   c_r   = (R[r][0] * (x + t0) + R[r][1] * (y + t1)) + R[r][2] * (z + t2)          r = 0, 1, 2
//   median    m     = np.median(c_2)
//   back      out_j = (R[0][j] * (c_0 - t0) + R[1][j] * (c_1 - t1)) + R[2][j] * (m - t2)      j = 0, 1, 2
//
// The median is EXACT: a radix select over the order-preserving 64-bit integer image of the doubles (sign bit set -> all bits flipped, else the sign bit
// flipped: negative depths occur through the quirk above), 8 bits per pass, most significant byte first.  A pass counts, for each wanted rank, the elements
// that agree with the bytes chosen so far into a 256-bin histogram per workgroup in LDS and adds it to a global one with integer atomics, so the result does
// not depend on the launch shape or the arrival order.  The next pass starts by choosing the byte from the finished histogram (every workgroup does that for
// itself from the same numbers).  Odd V: the order statistic V / 2; even V: (a + b) / 2 of the statistics V / 2 - 1 and V / 2, numpy's arithmetic.  The
// integer keys order -0 before +0 (numpy's partition does not order the two zeros); NaNs are not supported (finite depths in, finite vertices out).
#include "hive_internal.hpp"

#include <algorithm>

namespace {

constexpr int BB_THREADS = 256;
constexpr int BB_PASSES = 8;

struct BBSelect {                 // the state of the select after p passes, for the two wanted ranks
    unsigned long long prefix[2]; // the p most significant bytes of the wanted key (in the low bits)
    unsigned long long rank[2];   // rank of the wanted key among the elements that share that prefix
};

struct BBParams {
    double R[9], t[3];
    long long n;
    int n_sel;  // 1: odd n (one rank), 2: even n
};

__device__ __forceinline__ unsigned long long bb_key(double z) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(z);
    return (b >> 63) ? ~b : (b ^ 0x8000000000000000ull);
}

__device__ __forceinline__ double bb_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    return __longlong_as_double((long long)b);
}

// one wave-wide histogram update: the lanes that share the first active lane's bin add their number at once (the upper bytes of an object's depths are nearly
// all equal), the others one by one
__device__ __forceinline__ void bb_count(unsigned *hist, bool take, unsigned bin) {
    const unsigned long long active = __ballot(take);
    if (!active) return;
    const int first = __ffsll((long long)active) - 1;
    const unsigned lead = (unsigned)__shfl((int)bin, first);
    const unsigned long long same = __ballot(take && bin == lead);
    if ((int)(threadIdx.x & 63) == first) atomicAdd(hist + lead, (unsigned)__popcll(same));
    if (take && bin != lead) atomicAdd(hist + bin, 1u);
}

// state[pass] from state[pass - 1] and the finished histogram of pass - 1 (pass >= 1); all 256 threads of the workgroup; returns it through LDS
__device__ __forceinline__ BBSelect bb_choose(const BBSelect *__restrict__ state, const unsigned *__restrict__ hist, int pass, int n_sel, unsigned *lds_scan,
                                              BBSelect *lds_sel) {
    const BBSelect prev = state[pass - 1];
    for (int s = 0; s < n_sel; ++s) {
        const unsigned c = hist[((pass - 1) * 2 + s) * 256 + threadIdx.x];
        const unsigned long long before = block_exclusive(c, lds_scan);
        if (prev.rank[s] >= before && prev.rank[s] < before + c) {  // exactly one bin holds the rank
            lds_sel->prefix[s] = (prev.prefix[s] << 8) | threadIdx.x;
            lds_sel->rank[s] = prev.rank[s] - before;
        }
    }
    __syncthreads();
    BBSelect cur = *lds_sel;
    if (n_sel == 1) {
        cur.prefix[1] = cur.prefix[0];
        cur.rank[1] = cur.rank[0];
    }
    return cur;
}

// pass 0 computes the keys from the vertices; passes 1 .. 7 read them back
__global__ __launch_bounds__(BB_THREADS) void bb_pass_kernel(const double *__restrict__ vertices, unsigned long long *__restrict__ keys, BBParams p, int pass,
                                                             BBSelect *__restrict__ state, unsigned *__restrict__ hist) {
    __shared__ unsigned lds_hist[2][256];
    __shared__ unsigned lds_scan[4];
    __shared__ BBSelect lds_sel;
    lds_hist[0][threadIdx.x] = 0;
    lds_hist[1][threadIdx.x] = 0;
    BBSelect cur;
    if (pass == 0) {
        cur.prefix[0] = cur.prefix[1] = 0;
        __syncthreads();
    } else {
        cur = bb_choose(state, hist, pass, p.n_sel, lds_scan, &lds_sel);  // (ends with a barrier)
        if (blockIdx.x == 0 && threadIdx.x == 0) state[pass] = cur;
    }
    const int shift = 56 - 8 * pass;
    const long long stride = (long long)gridDim.x * BB_THREADS;
    const long long rounds = (p.n + stride - 1) / stride;  // whole waves stay in the loop: the ballots of bb_count need them
    for (long long k = 0; k < rounds; ++k) {
        const long long i = k * stride + (long long)blockIdx.x * BB_THREADS + threadIdx.x;
        const bool in = i < p.n;
        unsigned long long key = 0;
        if (in) {
            if (pass == 0) {
                const double x = vertices[3 * i + 0] + p.t[0], y = vertices[3 * i + 1] + p.t[1], z = vertices[3 * i + 2] + p.t[2];
                key = bb_key((p.R[6] * x + p.R[7] * y) + p.R[8] * z);
                keys[i] = key;
            } else {
                key = keys[i];
            }
        }
        const unsigned bin = (unsigned)(key >> shift) & 255u;
        const unsigned long long head = pass == 0 ? 0ull : key >> (shift + 8);
        bb_count(lds_hist[0], in && head == cur.prefix[0], bin);
        if (p.n_sel == 2) bb_count(lds_hist[1], in && head == cur.prefix[1], bin);
    }
    __syncthreads();
    for (int s = 0; s < p.n_sel; ++s) {
        const unsigned c = lds_hist[s][threadIdx.x];
        if (c) atomicAdd(hist + (pass * 2 + s) * 256 + threadIdx.x, c);
    }
}

__global__ __launch_bounds__(BB_THREADS) void bb_write_kernel(double *__restrict__ vertices, BBParams p, BBSelect *__restrict__ state,
                                                              const unsigned *__restrict__ hist, double *__restrict__ median_out) {
    __shared__ unsigned lds_scan[4];
    __shared__ BBSelect lds_sel;
    const BBSelect fin = bb_choose(state, hist, BB_PASSES, p.n_sel, lds_scan, &lds_sel);
    const double a = bb_value(fin.prefix[0]);
    const double m = p.n_sel == 1 ? a : (a + bb_value(fin.prefix[1])) / 2.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) *median_out = m;
    const double cz = m - p.t[2];
    for (long long i = (long long)blockIdx.x * BB_THREADS + threadIdx.x; i < p.n; i += (long long)gridDim.x * BB_THREADS) {
        const double x = vertices[3 * i + 0] + p.t[0], y = vertices[3 * i + 1] + p.t[1], z = vertices[3 * i + 2] + p.t[2];
        const double cx = ((p.R[0] * x + p.R[1] * y) + p.R[2] * z) - p.t[0];
        const double cy = ((p.R[3] * x + p.R[4] * y) + p.R[5] * z) - p.t[1];
        vertices[3 * i + 0] = (p.R[0] * cx + p.R[3] * cy) + p.R[6] * cz;
        vertices[3 * i + 1] = (p.R[1] * cx + p.R[4] * cy) + p.R[7] * cz;
        vertices[3 * i + 2] = (p.R[2] * cx + p.R[5] * cy) + p.R[8] * cz;
    }
}

}  // namespace

extern "C" {

int hive_fg_billboard(hive_ctx *ctx, double *d_vertices, int64_t n, const double R[9], const double t[3], double *median_out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, R && t, "fg_billboard: NULL argument");
    HIVE_REQUIRE(ctx, n >= 0 && n < (1ll << 31) && (n == 0 || d_vertices), "fg_billboard: bad vertex count %lld", (long long)n);
    if (n == 0) {  // an object without vertices: nothing to flatten
        if (median_out) *median_out = 0.0;
        return HIVE_OK;
    }
    // scratch: keys u64 [n] | histograms u32 [8 passes][2 ranks][256] | select states [9] | median f64
    const size_t off_hist = ((size_t)n * 8 + 255) & ~(size_t)255;
    const size_t off_state = off_hist + (size_t)BB_PASSES * 2 * 256 * 4;
    const size_t off_median = off_state + (((BB_PASSES + 1) * sizeof(BBSelect) + 255) & ~(size_t)255);
    int rc;
    if ((rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, off_median + 256))) return rc;
    char *base = (char *)ctx->d_scratch;
    unsigned long long *keys = (unsigned long long *)base;
    unsigned *hist = (unsigned *)(base + off_hist);
    BBSelect *state = (BBSelect *)(base + off_state);
    double *d_median = (double *)(base + off_median);
    BBParams p;
    memcpy(p.R, R, sizeof(p.R));
    memcpy(p.t, t, sizeof(p.t));
    p.n = n;
    p.n_sel = (n & 1) ? 1 : 2;
    BBSelect first;
    first.prefix[0] = first.prefix[1] = 0;
    first.rank[0] = (n & 1) ? (unsigned long long)(n / 2) : (unsigned long long)(n / 2 - 1);
    first.rank[1] = (unsigned long long)(n / 2);
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(hist, 0, (size_t)BB_PASSES * 2 * 256 * 4, ctx->stream));
    if ((rc = hive_upload(ctx, state, &first, sizeof(first)))) return rc;
    const dim3 grid((unsigned)std::min<long long>((n + BB_THREADS - 1) / BB_THREADS, (long long)ctx->num_cus * 4));
    for (int pass = 0; pass < BB_PASSES; ++pass)
        hipLaunchKernelGGL(bb_pass_kernel, grid, dim3(BB_THREADS), 0, ctx->stream, (const double *)d_vertices, keys, p, pass, state, hist);
    hipLaunchKernelGGL(bb_write_kernel, grid, dim3(BB_THREADS), 0, ctx->stream, d_vertices, p, state, (const unsigned *)hist, d_median);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    if (median_out) {
        HIVE_CHECK_HIP(ctx, hipMemcpyAsync(median_out, d_median, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return HIVE_OK;
}

}  // extern "C"
