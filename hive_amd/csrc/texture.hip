// Textures a mesh from posed frames: per face the view that sees it best, an atlas of two faces per S x S block, one gather per texel.  No counterpart in the
// reference (its background keeps the volume's vertex colours).  gfx950 only.  The rules are stated in include/hive_mi355x.h above hive_texture_select; in short:
//
//   select     per view, after that view's hive_render_draw and hive_render_resolve(depth): face f is a candidate iff its three vertices were kept by the draw,
//              its snapped area A != 0, and every vertex's nearest pixel (i, j) = ((Y + 128) >> 8, (X + 128) >> 8) is on the screen, unmasked and not hidden:
//              depth[i][j] == 0 || z <= (double)depth[i][j] + tolerance.  key = |A| << 16 | (65535 - view); best[f] = max(best[f], key).  One thread per face.
//   layout     faces 2k and 2k + 1 share block k; per_row = ceil(sqrt(blocks)); texel (x, y) of a block belongs to the even face iff x + y <= S - 1
//   unweld     three vertices of its own per face; uv at the corner texels (1, 1), (S - 4, 1), (1, S - 4) / (S - 2, S - 2), (3, S - 2), (S - 2, 3)
//   fill       b1, b2 from the block-local texel, b0 = (1 - b1) - b2; P = (b0 V0 + b1 V1) + b2 V2; hive_project's order with the winning view; bilinear in float64;
//              a face without a view: the same combination of its vertex colours.  One thread per texel.
//   adjusted fill   the same kernel with texture_level.hip's Q16 gain per view and channel and offsets per face corner: byte((c q) 2^-16 + interpolated offset);
//              exact, hence the plain atlas, at unit gains and zero offsets.  The projection and the bilinear sample are texture_core.hpp's, shared with the levelling.
//
// Float64 without contraction (the Makefile's EXACT flags).
//
// Kernels: texture_select_kernel and texture_unweld_kernel (one thread per face), texture_fill_kernel (one thread per texel, workgroups of TX_TILE x TX_TILE
// texels: DESIGN.md, "Texturing the background").
#include "texture_core.hpp"

namespace {

constexpr int TX_THREADS = 256;
constexpr int TX_TILE = 16;  // the fill kernel's workgroup: TX_TILE x TX_TILE texels (a performance knob)
constexpr int TX_MIN_CELL = 6, TX_MAX_CELL = 64, TX_MAX_ATLAS = 16384, TX_MAX_VIEWS = 65535;

struct TextureLayout {
    int S, per_row, Wt, Ht;
    long long blocks;
};

// false: nf or cell out of range, or an atlas side over TX_MAX_ATLAS (message in `why`)
bool tx_layout(long long nf, int cell, TextureLayout &l, const char *&why) {
    if (nf <= 0 || nf >= (1ll << 31)) return why = "texture_layout: the face count must be in [1, 2^31)", false;
    if (cell < TX_MIN_CELL || cell > TX_MAX_CELL) return why = "texture_layout: cell must be in [6, 64]", false;
    l.S = cell;
    l.blocks = (nf + 1) / 2;
    long long r = (long long)std::sqrt((double)l.blocks);  // ceil(sqrt(blocks)) in integers
    while (r * r < l.blocks) ++r;
    while (r > 1 && (r - 1) * (r - 1) >= l.blocks) --r;
    const long long rows = (l.blocks + r - 1) / r;
    if (r * cell > TX_MAX_ATLAS || rows * cell > TX_MAX_ATLAS) return why = "texture_layout: the atlas would exceed 16384 texels on a side", false;
    l.per_row = (int)r, l.Wt = (int)(r * cell), l.Ht = (int)(rows * cell);
    return true;
}

__global__ __launch_bounds__(TX_THREADS) void texture_select_kernel(const int32_t *__restrict__ faces, long long nf, long long nv, const int32_t *__restrict__ xy,
                                                                    const double *__restrict__ z, const float *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                                    int H, int W, unsigned view, double tolerance, unsigned long long *__restrict__ best) {
    const long long f = (long long)blockIdx.x * TX_THREADS + threadIdx.x;
    if (f >= nf) return;
    const int id[3] = {faces[3 * f + 0], faces[3 * f + 1], faces[3 * f + 2]};
    if (!tx_ids_ok(id[0], id[1], id[2], nv)) return;
    long long X[3], Y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double zk = z[id[k]];
        if (!(zk > 0.0)) return;  // a rejected vertex has z = 0
        X[k] = xy[2 * (long long)id[k]], Y[k] = xy[2 * (long long)id[k] + 1];
        const long long i = (Y[k] + 128) >> 8, j = (X[k] + 128) >> 8;  // (an arithmetic shift: floor)
        if (i < 0 || i >= H || j < 0 || j >= W) return;
        const long long px = i * W + j;
        if (mask && mask[px]) return;
        const float d = depth[px];
        if (!(d == 0.f || zk <= (double)d + tolerance)) return;
    }
    const long long A = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0]);
    if (A == 0) return;
    const unsigned long long key = ((unsigned long long)(A < 0 ? -A : A) << 16) | (unsigned long long)(65535u - view);
    if (key > best[f]) best[f] = key;  // (this thread alone touches best[f])
}

__global__ __launch_bounds__(TX_THREADS) void texture_unweld_kernel(const double *__restrict__ vertices, long long nv, const int32_t *__restrict__ faces, long long nf,
                                                                    TextureLayout l, const unsigned long long *__restrict__ best, double *__restrict__ vertices_out,
                                                                    int32_t *__restrict__ faces_out, double *__restrict__ uv, int32_t *__restrict__ views) {
    const long long f = (long long)blockIdx.x * TX_THREADS + threadIdx.x;
    if (f >= nf) return;
    const int id[3] = {faces[3 * f + 0], faces[3 * f + 1], faces[3 * f + 2]};
    const bool ok = tx_ids_ok(id[0], id[1], id[2], nv);  // (the callers check the ids; nothing is read out of bounds if they did not)
    const long long block = f >> 1;
    const int S = l.S, col0 = (int)(block % l.per_row) * S, row0 = (int)(block / l.per_row) * S;
    const bool odd = f & 1;
    const int cx[3] = {odd ? S - 2 : 1, odd ? 3 : S - 4, odd ? S - 2 : 1}, cy[3] = {odd ? S - 2 : 1, odd ? S - 2 : 1, odd ? 3 : S - 4};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long o = 3 * f + k;
#pragma unroll
        for (int r = 0; r < 3; ++r) vertices_out[3 * o + r] = ok ? vertices[3 * (long long)id[k] + r] : 0.0;
        faces_out[o] = (int32_t)o;
        uv[2 * o + 0] = (double)(col0 + cx[k]) / (double)l.Wt;
        uv[2 * o + 1] = 1.0 - (double)(row0 + cy[k]) / (double)l.Ht;
    }
    if (views) views[f] = best && best[f] ? (int32_t)(65535u - (unsigned)(best[f] & 0xffffull)) : -1;
}

// ADJUST: hive_texture_fill_adjusted's gains u32 [n][3] (Q16) and offsets f64 [nf][3][3] on a texel with a view; the plain fill passes neither
template <bool ADJUST>
__global__ __launch_bounds__(TX_TILE *TX_TILE) void texture_fill_kernel(const double *__restrict__ vertices, long long nv, const uint8_t *__restrict__ colors,
                                                                        const int32_t *__restrict__ faces, long long nf, const unsigned long long *__restrict__ best,
                                                                        const uint8_t *__restrict__ frames, int n, int H, int W, TextureCam cam,
                                                                        const double *__restrict__ poses, TextureLayout l, const unsigned *__restrict__ gains,
                                                                        const double *__restrict__ offsets, uint8_t *__restrict__ texture) {
    const int col = blockIdx.x * TX_TILE + threadIdx.x, row = blockIdx.y * TX_TILE + threadIdx.y;
    if (col >= l.Wt || row >= l.Ht) return;
    uint8_t *o = texture + 3 * ((size_t)row * l.Wt + col);
    const int S = l.S, x = col % S, y = row % S;
    const bool even = x + y <= S - 1;
    const long long f = 2 * ((long long)(row / S) * l.per_row + col / S) + (even ? 0 : 1);
    int id[3] = {0, 0, 0};
    if (f < nf) id[0] = faces[3 * f + 0], id[1] = faces[3 * f + 1], id[2] = faces[3 * f + 2];
    if (f >= nf || !tx_ids_ok(id[0], id[1], id[2], nv)) {
        o[0] = o[1] = o[2] = 0;
        return;
    }
    const double b1 = (double)(even ? x - 1 : S - 2 - x) / (double)(S - 5), b2 = (double)(even ? y - 1 : S - 2 - y) / (double)(S - 5);
    const double b0 = (1.0 - b1) - b2;
    const unsigned long long key = best[f];
    const int view = (int)(65535u - (unsigned)(key & 0xffffull));
    if (key == 0 || view >= n) {  // no view: the vertex colours
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            o[ch] = tx_byte((b0 * (double)colors[3 * (long long)id[0] + ch] + b1 * (double)colors[3 * (long long)id[1] + ch]) + b2 * (double)colors[3 * (long long)id[2] + ch]);
        return;
    }
    const double *Rt = poses + 12 * (long long)view;
    double c[3];
    for (int attempt = 0; attempt < 2; ++attempt) {  // the second time: vertex 0, which the draw kept
        double P[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double v0 = vertices[3 * (long long)id[0] + r];
            P[r] = attempt ? v0 : (b0 * v0 + b1 * vertices[3 * (long long)id[1] + r]) + b2 * vertices[3 * (long long)id[2] + r];
        }
        tx_project(cam, Rt, P, c);
        if (c[2] >= cam.near) break;
    }
    double s[3];
    tx_bilinear(frames + 3 * (size_t)view * H * W, H, W, c, s);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        if (ADJUST) {
            const double *h = offsets + 9 * f;
            o[ch] = tx_byte(((s[ch] * (double)gains[3 * view + ch]) * 0x1p-16) + ((b0 * h[ch] + b1 * h[3 + ch]) + b2 * h[6 + ch]));
        } else {
            o[ch] = tx_byte(s[ch]);
        }
    }
}

dim3 tx_grid(long long n) { return dim3((unsigned)((n + TX_THREADS - 1) / TX_THREADS)); }

}  // namespace

extern "C" {

int hive_texture_select(hive_ctx *ctx, const int32_t *d_faces, int64_t nf, int64_t nv, const int32_t *d_xy, const double *d_z, const float *d_depth,
                        const uint8_t *d_mask, int H, int W, int view_index, double depth_tolerance, uint64_t *d_best) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && ((long long)H + 1) * ((long long)W + 1) <= (1ll << 31), "texture_select: bad screen size %d x %d", H, W);
    HIVE_REQUIRE(ctx, nf >= 0 && nf < (1ll << 31) && nv >= 0 && nv < (1ll << 31), "texture_select: bad counts %lld faces, %lld vertices", (long long)nf, (long long)nv);
    HIVE_REQUIRE(ctx, view_index >= 0 && view_index < TX_MAX_VIEWS, "texture_select: view_index %d outside [0, 65535)", view_index);
    HIVE_REQUIRE(ctx, depth_tolerance >= 0.0, "texture_select: depth_tolerance must be >= 0");  // (false for a NaN)
    if (nf == 0 || nv == 0) return HIVE_OK;
    HIVE_REQUIRE(ctx, d_faces && d_xy && d_z && d_depth && d_best, "texture_select: NULL argument");
    hipLaunchKernelGGL(texture_select_kernel, tx_grid(nf), dim3(TX_THREADS), 0, ctx->stream, d_faces, (long long)nf, (long long)nv, d_xy, d_z, d_depth, d_mask, H, W,
                       (unsigned)view_index, depth_tolerance, (unsigned long long *)d_best);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_texture_layout(int64_t nf, int cell, int *Wt, int *Ht, int *per_row) {
    TextureLayout l;
    const char *why = nullptr;
    if (!tx_layout(nf, cell, l, why)) return hive_fail(nullptr, HIVE_ERR_INVALID, "%s (%lld faces, cell %d)", why, (long long)nf, cell);
    if (Wt) *Wt = l.Wt;
    if (Ht) *Ht = l.Ht;
    if (per_row) *per_row = l.per_row;
    return HIVE_OK;
}

int hive_texture_unweld(hive_ctx *ctx, const double *d_vertices, int64_t nv, const int32_t *d_faces, int64_t nf, int cell, const uint64_t *d_best,
                        double *d_vertices_out, int32_t *d_faces_out, double *d_uv, int32_t *d_views) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    TextureLayout l;
    const char *why = nullptr;
    HIVE_REQUIRE(ctx, tx_layout(nf, cell, l, why), "%s (%lld faces, cell %d)", why, (long long)nf, cell);
    HIVE_REQUIRE(ctx, 3 * nf < (1ll << 31), "texture_unweld: %lld faces need %lld vertices: the indices are int32", (long long)nf, (long long)(3 * nf));
    HIVE_REQUIRE(ctx, nv > 0 && nv < (1ll << 31) && d_vertices && d_faces && d_vertices_out && d_faces_out && d_uv, "texture_unweld: NULL argument or no vertices");
    hipLaunchKernelGGL(texture_unweld_kernel, tx_grid(nf), dim3(TX_THREADS), 0, ctx->stream, d_vertices, (long long)nv, d_faces, (long long)nf, l,
                       (const unsigned long long *)d_best, d_vertices_out, d_faces_out, d_uv, d_views);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

// the two fills: d_gains == NULL is the plain one
static int tx_fill(hive_ctx *ctx, const char *name, const double *d_vertices, int64_t nv, const uint8_t *d_vertex_colors, const int32_t *d_faces, int64_t nf,
                   const uint64_t *d_best, const uint8_t *d_frames, int n, int H, int W, const double K[9], const double *d_poses, double near, int cell,
                   const uint32_t *d_gains, const double *d_offsets, uint8_t *d_texture) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    TextureLayout l;
    const char *why = nullptr;
    HIVE_REQUIRE(ctx, tx_layout(nf, cell, l, why), "%s (%lld faces, cell %d)", why, (long long)nf, cell);
    HIVE_REQUIRE(ctx, n > 0 && n <= TX_MAX_VIEWS, "%s: %d views outside [1, 65535]", name, n);
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && (long long)H * W < (1ll << 31), "%s: bad frame size %d x %d", name, H, W);
    HIVE_REQUIRE(ctx, near > 0.0, "%s: near must be > 0", name);
    HIVE_REQUIRE(ctx, nv > 0 && nv < (1ll << 31) && d_vertices && d_vertex_colors && d_faces && d_best && d_frames && K && d_poses && d_texture,
                 "%s: NULL argument or no vertices", name);
    TextureCam cam;
    memcpy(cam.K, K, sizeof(cam.K));
    cam.near = near;
    const dim3 grid((unsigned)((l.Wt + TX_TILE - 1) / TX_TILE), (unsigned)((l.Ht + TX_TILE - 1) / TX_TILE));
    if (d_gains)
        hipLaunchKernelGGL(texture_fill_kernel<true>, grid, dim3(TX_TILE, TX_TILE), 0, ctx->stream, d_vertices, (long long)nv, d_vertex_colors, d_faces, (long long)nf,
                           (const unsigned long long *)d_best, d_frames, n, H, W, cam, d_poses, l, (const unsigned *)d_gains, d_offsets, d_texture);
    else
        hipLaunchKernelGGL(texture_fill_kernel<false>, grid, dim3(TX_TILE, TX_TILE), 0, ctx->stream, d_vertices, (long long)nv, d_vertex_colors, d_faces, (long long)nf,
                           (const unsigned long long *)d_best, d_frames, n, H, W, cam, d_poses, l, (const unsigned *)nullptr, (const double *)nullptr, d_texture);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_texture_fill(hive_ctx *ctx, const double *d_vertices, int64_t nv, const uint8_t *d_vertex_colors, const int32_t *d_faces, int64_t nf, const uint64_t *d_best,
                      const uint8_t *d_frames, int n, int H, int W, const double K[9], const double *d_poses, double near, int cell, uint8_t *d_texture) {
    return tx_fill(ctx, "texture_fill", d_vertices, nv, d_vertex_colors, d_faces, nf, d_best, d_frames, n, H, W, K, d_poses, near, cell, nullptr, nullptr, d_texture);
}

int hive_texture_fill_adjusted(hive_ctx *ctx, const double *d_vertices, int64_t nv, const uint8_t *d_vertex_colors, const int32_t *d_faces, int64_t nf,
                               const uint64_t *d_best, const uint8_t *d_frames, int n, int H, int W, const double K[9], const double *d_poses, double near, int cell,
                               const uint32_t *d_gains_q16, const double *d_offsets, uint8_t *d_texture) {
    if (ctx && !(d_gains_q16 && d_offsets)) return hive_fail(ctx, HIVE_ERR_INVALID, "texture_fill_adjusted: NULL gains or offsets");
    return tx_fill(ctx, "texture_fill_adjusted", d_vertices, nv, d_vertex_colors, d_faces, nf, d_best, d_frames, n, H, W, K, d_poses, near, cell, d_gains_q16, d_offsets,
                   d_texture);
}

}  // extern "C"
