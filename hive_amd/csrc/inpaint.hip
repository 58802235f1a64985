// Telea inpainting of the background behind dynamic objects (hive/dataset_adaptors.py:473-571, `cv2.inpaint(image, mask, 30, cv2.INPAINT_TELEA)`), in the
// level order and operation order that include/hive_mi355x.h states for hive_inpaint_telea.  gfx950 only; float64, compiled without contraction.
//
//   inp_rows_kernel   per pixel, the distance along its row to the nearest pixel of the OTHER kind (hole <-> known); one thread per row, two sweeps
//   inp_cols_kernel   column minimum of row distance^2 + dy^2 -> exact squared distance to the other kind, the level, the (frame, level) histogram.
//                     One launch serves both polarities: a hole pixel gets d_in^2, a known pixel d_out^2.  d_out^2 is only ever read within radius + 1 of
//                     the hole (the window, and the four neighbours of a hole pixel), so the search of a known pixel stops at |dy| = radius + 1: values
//                     above (radius + 1)^2 are upper bounds that nothing reads.
//   (host)            reads the histogram back: refuses a frame without a known pixel, turns it into the start of every (level, frame) run
//   inp_sort_kernel   counting sort of the batch's hole pixels by (level, frame, y, x): one workgroup per frame walks it in row-major order with the
//                     run cursors in LDS; ranks inside a wave come from ballots, waves take their turn in order -- no atomics, the same list every run
//   inp_fill_kernel   one launch per level over all frames; one wave per hole pixel, lane j adds the window offsets k = j, j + 64, ... in ascending order,
//                     then the 64 partial sums go through the fixed tree (lanes j and j + 32, then + 16, ... + 1).  Colour and depth share the weights.
// Nothing here waits on the device for other workgroups; the host reads one histogram per batch.
#include "hive_internal.hpp"

#include <algorithm>

namespace {

constexpr int INP_NO_ROW = 1 << 20;       // row distance of a row without a pixel of the other kind
constexpr int INP_FAR = 0x7fffffff;       // squared distance of a frame without a pixel of the other kind
constexpr int INP_MAX_SIDE = 4096;        // frame sides: levels stay below 8192 (the sort's cursors fit in LDS), squared distances in int32

// ---- distances ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void inp_rows_kernel(const uint8_t *__restrict__ mask, int rows, int W, int *__restrict__ g) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;
    const uint8_t *m = mask + (size_t)r * W;
    int *out = g + (size_t)r * W;
    int last[2] = {-INP_NO_ROW, -INP_NO_ROW};  // last x seen of [0] known, [1] hole
    for (int x = 0; x < W; ++x) {
        const int kind = m[x] != 0;
        last[kind] = x;
        out[x] = min(x - last[kind ^ 1], INP_NO_ROW);
    }
    last[0] = last[1] = 2 * INP_NO_ROW;
    for (int x = W - 1; x >= 0; --x) {
        const int kind = m[x] != 0;
        last[kind] = x;
        out[x] = min(out[x], min(last[kind ^ 1] - x, INP_NO_ROW));
    }
}

// wave-wide histogram update (billboard.hip's bb_count): lanes that share the first active lane's bin add their number at once
__device__ __forceinline__ void inp_count(unsigned *hist, bool take, unsigned bin) {
    unsigned long long todo = __ballot(take);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const unsigned lead = (unsigned)__shfl((int)bin, first);
        const unsigned long long same = __ballot(take && bin == lead);
        if ((int)(threadIdx.x & 63) == first) atomicAdd(hist + lead, (unsigned)__popcll(same));
        todo &= ~same;
    }
}

__device__ __forceinline__ int inp_level_of(int d2) {  // smallest L with L * L >= d2, in integers
    int L = (int)sqrt((double)d2);
    while (L * L < d2) ++L;
    while (L > 0 && (L - 1) * (L - 1) >= d2) --L;
    return L;
}

// blockIdx.y = frame.  hist [n][level_stride]: [f][L] = hole pixels of level L >= 1, [f][0] = hole pixels of a frame without a known pixel
__global__ __launch_bounds__(256) void inp_cols_kernel(const uint8_t *__restrict__ mask, const int *__restrict__ g, int H, int W, int known_reach, int level_stride,
                                                       int *__restrict__ d2, uint16_t *__restrict__ lvl, unsigned *__restrict__ hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t fb = (size_t)blockIdx.y * H * W;
    const bool in = i < H * W;
    bool hole = false;
    int level = 0;
    if (in) {
        const int y = i / W, x = i % W;
        hole = mask[fb + i] != 0;
        const int reach = hole ? H : known_reach;
        int best = INP_FAR;
        for (int dy = 0; dy <= reach; ++dy) {
            const int dd = dy * dy;
            if (dd >= best || (y - dy < 0 && y + dy >= H)) break;
            for (int side = 0; side < 2; ++side) {
                const int yy = side ? y + dy : y - dy;
                if (yy < 0 || yy >= H) continue;
                const size_t q = fb + (size_t)yy * W + x;
                if ((mask[q] != 0) != hole) {
                    best = min(best, dd);
                } else {
                    const int gg = g[q];
                    if (gg < INP_NO_ROW) best = min(best, gg * gg + dd);
                }
            }
        }
        d2[fb + i] = best;
        if (hole) level = best == INP_FAR ? 0 : inp_level_of(best);
        lvl[fb + i] = hole ? (best == INP_FAR ? (uint16_t)0xffff : (uint16_t)level) : (uint16_t)0;
    }
    inp_count(hist + (size_t)blockIdx.y * level_stride, in && hole, (unsigned)level);
}

// ---- the sort -------------------------------------------------------------------------------------------------------------------------------
// cursor [n][level_stride]: where the run of (level, frame) starts in `items`.  items: pixel index in the batch (frame * H * W + y * W + x)
__global__ __launch_bounds__(256) void inp_sort_kernel(const uint16_t *__restrict__ lvl, int H, int W, int level_stride, int max_level,
                                                       const unsigned *__restrict__ cursor, uint32_t *__restrict__ items) {
    extern __shared__ unsigned cur[];  // [max_level + 1]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_px = H * W;
    const size_t fb = (size_t)blockIdx.x * n_px;
    for (int L = threadIdx.x; L <= max_level; L += 256) cur[L] = cursor[(size_t)blockIdx.x * level_stride + L];
    __syncthreads();
    for (int base = 0; base < n_px; base += 256) {
        const int i = base + threadIdx.x;
        const unsigned L = i < n_px ? lvl[fb + i] : 0u;
        if (!__syncthreads_or(L != 0)) continue;
        for (int turn = 0; turn < 4; ++turn) {
            if (wave == turn) {
                unsigned long long todo = __ballot(L != 0);
                while (todo) {
                    const int first = __ffsll((long long)todo) - 1;
                    const unsigned lead = (unsigned)__shfl((int)L, first);
                    const unsigned long long same = __ballot(L == lead);
                    const unsigned start = cur[lead];
                    if (L == lead) items[start + (unsigned)__popcll(same & ((1ull << lane) - 1ull))] = (uint32_t)(fb + i);
                    __builtin_amdgcn_wave_barrier();
                    if (lane == first) cur[lead] = start + (unsigned)__popcll(same);
                    todo &= ~same;
                }
            }
            __syncthreads();
        }
    }
}

// ---- the fill -------------------------------------------------------------------------------------------------------------------------------
struct InpFill {
    int H, W, eps, level;
    unsigned first, count;  // the level's run in items
    const uint32_t *items;
    const uint16_t *lvl;
    const int *d2;
    uint8_t *img8;    // [n][H][W][C8], filled in place
    uint16_t *img16;  // [n][H][W]
};

__device__ __forceinline__ double inp_T(const uint16_t *lvl, const int *d2, size_t i) {
    const double d = sqrt((double)d2[i]);
    return lvl[i] ? d : 1.0 - d;
}

__device__ __forceinline__ double inp_tree(double v) {  // lane 0: the fixed pairwise tree over the 64 lanes
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
    return v;
}

// one channel's I(q) + grad I(q) . r; l, r, u, d: which of q's four neighbours are usable
template <class T>
__device__ __forceinline__ double inp_sample(const T *img, size_t q, size_t row, int stride, bool l, bool r, bool u, bool d, double rx, double ry) {
    const double c = (double)img[q];
    double gx = 0.0, gy = 0.0;
    if (l && r)
        gx = ((double)img[q + stride] - (double)img[q - stride]) / 2.0;
    else if (r)
        gx = (double)img[q + stride] - c;
    else if (l)
        gx = c - (double)img[q - stride];
    if (u && d)
        gy = ((double)img[q + row] - (double)img[q - row]) / 2.0;
    else if (d)
        gy = (double)img[q + row] - c;
    else if (u)
        gy = c - (double)img[q - row];
    return c + (gx * rx + gy * ry);
}

template <int C8, bool D16>
__global__ __launch_bounds__(256) void inp_fill_kernel(InpFill p) {
    const int lane = threadIdx.x & 63;
    const unsigned item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= p.count) return;  // (the whole wave)
    const int H = p.H, W = p.W, eps = p.eps, side = 2 * p.eps + 1, L = p.level;
    const size_t n_px = (size_t)H * W;
    const size_t gi = p.items[p.first + item];
    const size_t fb = gi / n_px * n_px;
    const int pix = (int)(gi - fb), y = pix / W, x = pix % W;
    const uint16_t *lvl = p.lvl + fb;
    const int *d2 = p.d2 + fb;
    const double Tp = inp_T(lvl, d2, pix);
    const double gTx = (inp_T(lvl, d2, (size_t)y * W + min(x + 1, W - 1)) - inp_T(lvl, d2, (size_t)y * W + max(x - 1, 0))) / 2.0;
    const double gTy = (inp_T(lvl, d2, (size_t)min(y + 1, H - 1) * W + x) - inp_T(lvl, d2, (size_t)max(y - 1, 0) * W + x)) / 2.0;
    double s = 0.0, a8[C8 ? C8 : 1] = {}, a16 = 0.0;
    for (int k = lane; k < side * side; k += 64) {
        const int dy = k / side - eps, dx = k % side - eps;
        const int r2i = dx * dx + dy * dy;
        const int qx = x + dx, qy = y + dy;
        if (r2i == 0 || r2i > eps * eps || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const size_t q = (size_t)qy * W + qx;
        if (lvl[q] >= L) continue;
        const double rx = (double)-dx, ry = (double)-dy, r2 = (double)r2i;
        const double dst = 1.0 / (r2 * sqrt(r2));
        const double lev = 1.0 / (1.0 + fabs(inp_T(lvl, d2, q) - Tp));
        double dir = fabs(rx * gTx + ry * gTy);
        if (dir <= 0.01) dir = 1e-6;
        const double w = (dst * lev) * dir;
        const bool nl = qx > 0 && lvl[q - 1] < L, nr = qx < W - 1 && lvl[q + 1] < L;
        const bool nu = qy > 0 && lvl[q - W] < L, nd = qy < H - 1 && lvl[q + W] < L;
        if (C8) {
            const uint8_t *img = p.img8 + fb * C8;
#pragma unroll
            for (int c = 0; c < C8; ++c) a8[c] += w * inp_sample(img + c, q * C8, (size_t)W * C8, C8, nl, nr, nu, nd, rx, ry);
        }
        if (D16) a16 += w * inp_sample(p.img16 + fb, q, (size_t)W, 1, nl, nr, nu, nd, rx, ry);
        s += w;
    }
    s = inp_tree(s);
    if (C8) {
#pragma unroll
        for (int c = 0; c < C8; ++c) {
            const double v = floor(inp_tree(a8[c]) / s + 0.5);
            if (lane == 0) p.img8[(fb + pix) * C8 + c] = (uint8_t)fmin(fmax(v, 0.0), 255.0);
        }
    }
    if (D16) {
        const double v = floor(inp_tree(a16) / s + 0.5);
        if (lane == 0) p.img16[fb + pix] = (uint16_t)fmin(fmax(v, 0.0), 65535.0);
    }
}

// Fills img8 / img16 (either may be null) in place under d_holes (non-zero = hole) for n frames.  levels_out (host, optional): level count per frame.
int inpaint_run(hive_ctx *ctx, const uint8_t *d_holes, int n, int H, int W, int radius, uint8_t *img8, int C8, uint16_t *img16, char *scratch,
                int32_t *levels_out) {
    const size_t n_px = (size_t)H * W, total = n_px * (size_t)n;
    const int level_stride = H + W;
    hive_scratch_layout lay;
    lay.base = scratch;
    int *g = lay.take<int>(total);  // row distances, then (dead after the column pass) the sorted items
    int *d2 = lay.take<int>(total);
    uint16_t *lvl = lay.take<uint16_t>(total);
    unsigned *hist = lay.take<unsigned>((size_t)n * level_stride);
    unsigned *cursor = lay.take<unsigned>((size_t)n * level_stride);
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(hist, 0, (size_t)n * level_stride * sizeof(unsigned), ctx->stream));
    const int rows = n * H;
    hipLaunchKernelGGL(inp_rows_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, ctx->stream, d_holes, rows, W, g);
    hipLaunchKernelGGL(inp_cols_kernel, dim3((unsigned)((n_px + 255) / 256), n), dim3(256), 0, ctx->stream, d_holes, (const int *)g, H, W, radius + 1, level_stride,
                       d2, lvl, hist);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    std::vector<unsigned> h_hist((size_t)n * level_stride);
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(h_hist.data(), hist, h_hist.size() * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int max_level = 0;
    for (int f = 0; f < n; ++f) {
        HIVE_REQUIRE(ctx, h_hist[(size_t)f * level_stride] == 0, "inpaint: frame %d has no known pixel", f);
        int top = 0;
        for (int L = 1; L < level_stride; ++L)
            if (h_hist[(size_t)f * level_stride + L]) top = L;
        if (levels_out) levels_out[f] = top;
        max_level = std::max(max_level, top);
    }
    if (max_level == 0) return HIVE_OK;  // no hole anywhere: the copies stand
    // runs in (level, frame) order
    std::vector<unsigned> h_cursor((size_t)n * level_stride, 0u), level_first((size_t)max_level + 2, 0u);
    unsigned at = 0;
    for (int L = 1; L <= max_level; ++L) {
        level_first[L] = at;
        for (int f = 0; f < n; ++f) {
            h_cursor[(size_t)f * level_stride + L] = at;
            at += h_hist[(size_t)f * level_stride + L];
        }
    }
    level_first[max_level + 1] = at;
    int rc;
    if ((rc = hive_upload(ctx, cursor, h_cursor.data(), h_cursor.size() * sizeof(unsigned)))) return rc;
    uint32_t *items = (uint32_t *)g;
    hipLaunchKernelGGL(inp_sort_kernel, dim3(n), dim3(256), (size_t)(max_level + 1) * sizeof(unsigned), ctx->stream, (const uint16_t *)lvl, H, W, level_stride,
                       max_level, (const unsigned *)cursor, items);
    InpFill p;
    p.H = H, p.W = W, p.eps = radius;
    p.items = items, p.lvl = lvl, p.d2 = d2;
    p.img8 = img8, p.img16 = img16;
    for (int L = 1; L <= max_level; ++L) {
        p.level = L;
        p.first = level_first[L];
        p.count = level_first[L + 1] - level_first[L];
        if (!p.count) continue;
        const dim3 grid((p.count + 3) / 4);
        if (img8 && img16)
            hipLaunchKernelGGL((inp_fill_kernel<3, true>), grid, dim3(256), 0, ctx->stream, p);
        else if (img16)
            hipLaunchKernelGGL((inp_fill_kernel<0, true>), grid, dim3(256), 0, ctx->stream, p);
        else if (C8 == 3)
            hipLaunchKernelGGL((inp_fill_kernel<3, false>), grid, dim3(256), 0, ctx->stream, p);
        else
            hipLaunchKernelGGL((inp_fill_kernel<1, false>), grid, dim3(256), 0, ctx->stream, p);
    }
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

size_t inpaint_scratch_bytes(int n, int H, int W) {
    const size_t total = (size_t)H * W * (size_t)n;
    hive_scratch_layout lay;
    lay.take<int>(total);
    lay.take<int>(total);
    lay.take<uint16_t>(total);
    lay.take<unsigned>((size_t)n * (H + W));
    lay.take<unsigned>((size_t)n * (H + W));
    return lay.bytes();
}

int inpaint_check(hive_ctx *ctx, int n, int H, int W, int radius) {
    HIVE_REQUIRE(ctx, n > 0 && n <= 65535 && H > 0 && W > 0 && H <= INP_MAX_SIDE && W <= INP_MAX_SIDE, "inpaint: bad arguments n=%d %dx%d (sides up to %d)", n, H, W,
                 INP_MAX_SIDE);
    HIVE_REQUIRE(ctx, (size_t)n * H * W < ((size_t)1 << 31), "inpaint: %d frames of %dx%d are more than 2^31 pixels; pass fewer frames per call", n, H, W);
    HIVE_REQUIRE(ctx, radius >= 2 && radius <= 64, "inpaint: the radius must be 2 .. 64, got %d", radius);
    return HIVE_OK;
}

}  // namespace

extern "C" {

int hive_inpaint_telea(hive_ctx *ctx, const void *image, int H, int W, int channels, int bytes_per_sample, const uint8_t *mask, int radius, int mem, void *out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, image && mask && out, "inpaint_telea: NULL argument");
    HIVE_REQUIRE(ctx, (bytes_per_sample == 1 && (channels == 1 || channels == 3)) || (bytes_per_sample == 2 && channels == 1),
                 "inpaint_telea: u8 with 1 or 3 channels or u16 with 1 channel, got %d channels of %d bytes", channels, bytes_per_sample);
    int rc;
    if ((rc = inpaint_check(ctx, 1, H, W, radius))) return rc;
    const size_t n_px = (size_t)H * W, img_bytes = n_px * channels * bytes_per_sample;
    const bool host = mem == HIVE_MEM_HOST;
    hive_scratch_layout in;  // host calls: the mask and the image being filled
    in.take<uint8_t>(n_px);
    in.take<uint8_t>(img_bytes);
    if (host && (rc = hive_reserve_device(ctx, &ctx->d_in, &ctx->in_bytes, in.bytes()))) return rc;
    if ((rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, inpaint_scratch_bytes(1, H, W)))) return rc;
    in = hive_scratch_layout();
    in.base = (char *)ctx->d_in;
    const uint8_t *d_mask = mask;
    void *d_img = out;
    if (host) {
        uint8_t *m = in.take<uint8_t>(n_px);
        d_img = in.take<uint8_t>(img_bytes);
        if ((rc = hive_upload(ctx, m, mask, n_px))) return rc;
        if ((rc = hive_upload(ctx, d_img, image, img_bytes))) return rc;
        d_mask = m;
    }
    // device calls fill `out` in place: it starts as a copy of the image.  A refused frame leaves the copy behind, never a partial fill.
    if (!host && out != image) HIVE_CHECK_HIP(ctx, hipMemcpyAsync(out, image, img_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    rc = inpaint_run(ctx, d_mask, 1, H, W, radius, bytes_per_sample == 1 ? (uint8_t *)d_img : nullptr, channels, bytes_per_sample == 2 ? (uint16_t *)d_img : nullptr,
                     (char *)ctx->d_scratch, nullptr);
    if (rc) return rc;
    if (host) {
        HIVE_CHECK_HIP(ctx, hipMemcpyAsync(out, d_img, img_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIVE_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return HIVE_OK;
}

int hive_inpaint_frames(hive_ctx *ctx, const uint8_t *d_rgb, const uint16_t *d_depth, const uint8_t *d_mask, int n, int H, int W, int dilate_kh, int dilate_kw,
                        int dilate_iterations, int radius, uint8_t *d_rgb_out, uint16_t *d_depth_out, int32_t *levels_out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_mask && (d_rgb || d_depth), "inpaint_frames: NULL argument");
    HIVE_REQUIRE(ctx, (!d_rgb || d_rgb_out) && (!d_depth || d_depth_out), "inpaint_frames: an image without its output");
    HIVE_REQUIRE(ctx, dilate_iterations >= 0, "inpaint_frames: %d dilation iterations", dilate_iterations);
    int rc;
    if ((rc = inpaint_check(ctx, n, H, W, radius))) return rc;
    const size_t total = (size_t)H * W * (size_t)n;
    hive_scratch_layout lay;  // the two dilation planes, then inpaint_run's block
    lay.take<uint8_t>(total);
    lay.take<uint8_t>(total);
    const size_t run_at = lay.bytes();
    if ((rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, run_at + inpaint_scratch_bytes(n, H, W)))) return rc;
    lay = hive_scratch_layout();
    lay.base = (char *)ctx->d_scratch;
    uint8_t *a = lay.take<uint8_t>(total), *b = lay.take<uint8_t>(total);
    const uint8_t *d_holes = d_mask;
    if (dilate_iterations > 0) {
        HIVE_REQUIRE(ctx, dilate_kh >= 1 && dilate_kw >= 1 && dilate_kh <= 32 && dilate_kw <= 32, "inpaint_frames: dilation element %dx%d", dilate_kh, dilate_kw);
        uint8_t ones[32 * 32];
        memset(ones, 1, sizeof(ones));
        if ((rc = hive_dilate_frames(ctx, d_mask, n, H, W, ones, dilate_kh, dilate_kw, dilate_iterations, a, b))) return rc;
        d_holes = b;
    }
    if (d_rgb && d_rgb_out != d_rgb) HIVE_CHECK_HIP(ctx, hipMemcpyAsync(d_rgb_out, d_rgb, total * 3, hipMemcpyDeviceToDevice, ctx->stream));
    if (d_depth && d_depth_out != d_depth) HIVE_CHECK_HIP(ctx, hipMemcpyAsync(d_depth_out, d_depth, total * 2, hipMemcpyDeviceToDevice, ctx->stream));
    return inpaint_run(ctx, d_holes, n, H, W, radius, d_rgb ? d_rgb_out : nullptr, 3, d_depth ? d_depth_out : nullptr, (char *)ctx->d_scratch + run_at, levels_out);
}

}  // extern "C"
