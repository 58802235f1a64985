// Renders meshes from a camera pose: an exact z-buffer rasteriser (what render_mesh does with pyrender's RenderFlags.FLAT in the reference,
// scripts/experiments.py:861-883).  gfx950 only.  The rules are stated in include/hive_mi355x.h above hive_render_clear; in short:
//
//   vertex     cam_r = ((R[r][0] x + R[r][1] y) + R[r][2] z) + t_r;  c_r = (K[r][0] cam_0 + K[r][1] cam_1) + K[r][2] cam_2  -- hive_project's order;
//              sx = c_0 / c_2, sy = c_1 / c_2, z = c_2;  X = (int)floor(sx * 256 + 0.5), Y likewise (8 sub-pixel bits)
//   reject     a face with a vertex that has !(z >= near) or !(|sx| < 65536 && |sy| < 65536), or with snapped area A == 0 (no clipping, no culling)
//   coverage   int64 edge functions at the sample (x = j, y = i) of pixel (i, j), top-left rule; A < 0: vertices 1 and 2 swapped
//   depth      q_e = (double)w_e / z_e; den = (q0 + q1) + q2; depth = (float)(1.0 / (den / (double)A))
//   key        float_bits(depth) << 32 | global face index; the pixel keeps the MINIMUM (one 64-bit atomic): nearest surface, then smallest face index,
//              whatever the arrival order or the launch shape
//   shade      attribute a = ((q0 a0 + q1 a1) + q2 a2) / den, from the edge functions recomputed at the winner
//
// Float64 without contraction (the Makefile's EXACT flags).  The guard band keeps every edge function below 2^53, so int64 -> double is exact.
//
// Kernels: render_project_kernel (one thread per vertex), render_raster_kernel (one thread per face: boxes of at most RD_SMALL_BOX pixels are drawn on the
// spot, larger ones go to a list, compacted per wave), render_raster_large_kernel (one workgroup per listed face striding over its box),
// render_shade_kernel and render_resolve_kernel (one thread per pixel).
#include "hive_internal.hpp"

#include <algorithm>

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_SUB = 256;           // 8 sub-pixel bits
constexpr long long RD_SMALL_BOX = 64;  // pixels of the clipped bounding box up to which a face is drawn by its own thread (a performance knob)
constexpr unsigned long long RD_EMPTY = ~0ull;

struct RenderCam {
    double K[9], R[9], t[3];
    double near;
};

// a face ready to be sampled: snapped vertices (1 and 2 swapped when the area was negative), depths, |area| and the clipped box
struct RenderFace {
    long long X[3], Y[3];
    double z[3];
    long long A;
    int i0, i1, j0, j1;
    int id[3];  // the vertex of each slot
};

// false: the face is rejected or its clipped box is empty
__device__ __forceinline__ bool rd_setup(const int32_t *__restrict__ faces, long long f, long long nv, const int32_t *__restrict__ xy, const double *__restrict__ z,
                                         int H, int W, RenderFace &s) {
    int a = faces[3 * f + 0], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if ((unsigned long long)a >= (unsigned long long)nv || (unsigned long long)b >= (unsigned long long)nv || (unsigned long long)c >= (unsigned long long)nv)
        return false;  // (the callers check the ids; nothing is read out of bounds if they did not)
    const double za = z[a], zb = z[b], zc = z[c];
    if (!(za > 0.0 && zb > 0.0 && zc > 0.0)) return false;  // a rejected vertex has z = 0
    const long long Xa = xy[2 * a], Ya = xy[2 * a + 1], Xb = xy[2 * b], Yb = xy[2 * b + 1], Xc = xy[2 * c], Yc = xy[2 * c + 1];
    const long long A = (Xb - Xa) * (Yc - Ya) - (Xc - Xa) * (Yb - Ya);
    if (A == 0) return false;
    const bool swap = A < 0;
    s.X[0] = Xa, s.Y[0] = Ya, s.z[0] = za, s.id[0] = a;
    s.X[1] = swap ? Xc : Xb, s.Y[1] = swap ? Yc : Yb, s.z[1] = swap ? zc : zb, s.id[1] = swap ? c : b;
    s.X[2] = swap ? Xb : Xc, s.Y[2] = swap ? Yb : Yc, s.z[2] = swap ? zb : zc, s.id[2] = swap ? b : c;
    s.A = swap ? -A : A;
    const long long min_x = min(Xa, min(Xb, Xc)), max_x = max(Xa, max(Xb, Xc)), min_y = min(Ya, min(Yb, Yc)), max_y = max(Ya, max(Yb, Yc));
    // ceil(min / 256) .. floor(max / 256), clipped to the screen (>> on a negative value is an arithmetic shift: floor)
    s.j0 = (int)max(0ll, (min_x + (RD_SUB - 1)) >> 8), s.j1 = (int)min((long long)W - 1, max_x >> 8);
    s.i0 = (int)max(0ll, (min_y + (RD_SUB - 1)) >> 8), s.i1 = (int)min((long long)H - 1, max_y >> 8);
    return s.j0 <= s.j1 && s.i0 <= s.i1;
}

// the three edge functions at the sample of pixel (i, j): w[e] belongs to the edge opposite vertex e, from p = e + 1 to q = e + 2 (mod 3); true: inside
__device__ __forceinline__ bool rd_edges(const RenderFace &s, int i, int j, long long w[3]) {
    const long long px = (long long)j * RD_SUB, py = (long long)i * RD_SUB;
    bool inside = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int p = (e + 1) % 3, q = (e + 2) % 3;
        const long long dx = s.X[q] - s.X[p], dy = s.Y[q] - s.Y[p];
        w[e] = dx * (py - s.Y[p]) - dy * (px - s.X[p]);
        inside = inside && (w[e] > 0 || (w[e] == 0 && (dy < 0 || (dy == 0 && dx > 0))));  // top-left rule
    }
    return inside;
}

// q_e = w_e / z_e and den = (q0 + q1) + q2
__device__ __forceinline__ double rd_weights(const RenderFace &s, const long long w[3], double q[3]) {
#pragma unroll
    for (int e = 0; e < 3; ++e) q[e] = (double)w[e] / s.z[e];
    return (q[0] + q[1]) + q[2];
}

__device__ __forceinline__ void rd_sample(const RenderFace &s, int i, int j, unsigned face, unsigned long long *__restrict__ key_plane, int W) {
    long long w[3];
    if (!rd_edges(s, i, j, w)) return;
    double q[3];
    const double den = rd_weights(s, w, q);
    const float depth = (float)(1.0 / (den / (double)s.A));
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | face;
    unsigned long long *at = key_plane + (size_t)i * W + j;
    // keys only decrease, so a stale read can only let a needless atomic through
    if (key < *at) atomicMin(at, key);
}

__global__ __launch_bounds__(RD_THREADS) void render_clear_kernel(unsigned long long *__restrict__ key_plane, long long n) {
    const long long i = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (i < n) key_plane[i] = RD_EMPTY;
}

__global__ __launch_bounds__(RD_THREADS) void render_project_kernel(const double *__restrict__ vertices, long long nv, RenderCam p, int32_t *__restrict__ xy,
                                                                    double *__restrict__ z) {
    const long long i = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (i >= nv) return;
    const double X[3] = {vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]};
    double cam[3], c[3];
    for (int r = 0; r < 3; ++r) cam[r] = p.R[3 * r + 0] * X[0] + p.R[3 * r + 1] * X[1] + p.R[3 * r + 2] * X[2] + p.t[r];
    for (int r = 0; r < 3; ++r) c[r] = p.K[3 * r + 0] * cam[0] + p.K[3 * r + 1] * cam[1] + p.K[3 * r + 2] * cam[2];
    const double sx = c[0] / c[2], sy = c[1] / c[2];
    const bool keep = c[2] >= p.near && fabs(sx) < 65536.0 && fabs(sy) < 65536.0;
    xy[2 * i + 0] = keep ? (int32_t)floor(sx * RD_SUB + 0.5) : 0;
    xy[2 * i + 1] = keep ? (int32_t)floor(sy * RD_SUB + 0.5) : 0;
    z[i] = keep ? c[2] : 0.0;  // the reject flag: a kept vertex has z >= near > 0
}

// counts[0] = faces on the large list, counts[1] = faces drawn here
__global__ __launch_bounds__(RD_THREADS) void render_raster_kernel(const int32_t *__restrict__ faces, long long nf, long long nv, unsigned face_base,
                                                                   const int32_t *__restrict__ xy, const double *__restrict__ z, int H, int W,
                                                                   unsigned long long *__restrict__ key_plane, int32_t *__restrict__ large, unsigned *__restrict__ counts) {
    const long long f = (long long)blockIdx.x * RD_THREADS + threadIdx.x;  // (whole waves reach the ballots)
    RenderFace s;
    const bool live = f < nf && rd_setup(faces, f, nv, xy, z, H, W, s);
    const bool big = live && (long long)(s.i1 - s.i0 + 1) * (s.j1 - s.j0 + 1) > RD_SMALL_BOX;
    const int lane = threadIdx.x & 63;
    const unsigned long long big_mask = __ballot(big), small_mask = __ballot(live && !big);
    if (big_mask) {  // one slot range per wave
        const int leader = __ffsll((long long)big_mask) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(counts + 0, (unsigned)__popcll(big_mask));
        base = (unsigned)__shfl((int)base, leader);
        if (big) large[base + (unsigned)__popcll(big_mask & ((1ull << lane) - 1ull))] = (int32_t)f;
    }
    if (small_mask && lane == __ffsll((long long)small_mask) - 1) atomicAdd(counts + 1, (unsigned)__popcll(small_mask));
    if (!live || big) return;
    for (int i = s.i0; i <= s.i1; ++i)
        for (int j = s.j0; j <= s.j1; ++j) rd_sample(s, i, j, face_base + (unsigned)f, key_plane, W);
}

__global__ __launch_bounds__(RD_THREADS) void render_raster_large_kernel(const int32_t *__restrict__ faces, long long nf, long long nv, unsigned face_base,
                                                                         const int32_t *__restrict__ xy, const double *__restrict__ z, int H, int W,
                                                                         unsigned long long *__restrict__ key_plane, const int32_t *__restrict__ large,
                                                                         const unsigned *__restrict__ counts) {
    const unsigned n_large = min(counts[0], (unsigned)min(nf, 0x7fffffffll));
    for (unsigned e = blockIdx.x; e < n_large; e += gridDim.x) {
        const long long f = large[e];
        RenderFace s;
        if (f < 0 || f >= nf || !rd_setup(faces, f, nv, xy, z, H, W, s)) continue;  // (always passes: the list holds faces that did)
        const int bw = s.j1 - s.j0 + 1;
        const long long n_px = (long long)(s.i1 - s.i0 + 1) * bw;
        for (long long k = threadIdx.x; k < n_px; k += RD_THREADS) rd_sample(s, s.i0 + (int)(k / bw), s.j0 + (int)(k % bw), face_base + (unsigned)f, key_plane, W);
    }
}

// vertex colours (colors != NULL) or a nearest texel of `texture` through uv; only pixels whose winner is one of this mesh's faces
__global__ __launch_bounds__(RD_THREADS) void render_shade_kernel(const int32_t *__restrict__ faces, long long nf, long long nv, unsigned face_base,
                                                                  const int32_t *__restrict__ xy, const double *__restrict__ z, const uint8_t *__restrict__ colors,
                                                                  const double *__restrict__ uv, const uint8_t *__restrict__ texture, int Ht, int Wt,
                                                                  const unsigned long long *__restrict__ key_plane, int H, int W, uint8_t *__restrict__ out) {
    const long long px = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (px >= (long long)H * W) return;
    const unsigned long long key = key_plane[px];
    if (key == RD_EMPTY) return;
    const long long f = (long long)(unsigned)key - (long long)face_base;
    if (f < 0 || f >= nf) return;
    RenderFace s;
    if (!rd_setup(faces, f, nv, xy, z, H, W, s)) return;  // (always passes: the face won this pixel)
    long long w[3];
    rd_edges(s, (int)(px / W), (int)(px % W), w);
    double q[3];
    const double den = rd_weights(s, w, q);
    uint8_t *o = out + 3 * px;
    if (colors) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double a0 = (double)colors[3 * (long long)s.id[0] + ch], a1 = (double)colors[3 * (long long)s.id[1] + ch], a2 = (double)colors[3 * (long long)s.id[2] + ch];
            const double c = ((q[0] * a0 + q[1] * a1) + q[2] * a2) / den;
            o[ch] = (uint8_t)fmin(255.0, floor(c + 0.5));
        }
    } else {
        double a[2];
#pragma unroll
        for (int k = 0; k < 2; ++k)
            a[k] = ((q[0] * uv[2 * (long long)s.id[0] + k] + q[1] * uv[2 * (long long)s.id[1] + k]) + q[2] * uv[2 * (long long)s.id[2] + k]) / den;
        const int col = (int)fmin(fmax(floor(a[0] * (double)Wt + 0.5), 0.0), (double)(Wt - 1));
        const int row = (int)fmin(fmax(floor((1.0 - a[1]) * (double)Ht + 0.5), 0.0), (double)(Ht - 1));
        const uint8_t *texel = texture + 3 * ((size_t)row * Wt + col);
        o[0] = texel[0], o[1] = texel[1], o[2] = texel[2];
    }
}

struct RenderBackground {
    uint8_t rgb[3];
};

__global__ __launch_bounds__(RD_THREADS) void render_resolve_kernel(const unsigned long long *__restrict__ key_plane, long long n, RenderBackground bg,
                                                                    uint8_t *__restrict__ color, float *__restrict__ depth, int32_t *__restrict__ face) {
    const long long px = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (px >= n) return;
    const unsigned long long key = key_plane[px];
    const bool empty = key == RD_EMPTY;
    if (empty && color) color[3 * px + 0] = bg.rgb[0], color[3 * px + 1] = bg.rgb[1], color[3 * px + 2] = bg.rgb[2];
    if (depth) depth[px] = empty ? 0.f : __uint_as_float((unsigned)(key >> 32));
    if (face) face[px] = empty ? -1 : (int32_t)(unsigned)key;
}

dim3 rd_grid(long long n) { return dim3((unsigned)((n + RD_THREADS - 1) / RD_THREADS)); }

// what draw and shade require of a mesh and the screen
int rd_check_mesh(hive_ctx *ctx, const char *who, const void *vertices, int64_t nv, const void *faces, int64_t nf, int64_t face_base, int H, int W) {
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && (long long)H * W < (1ll << 31), "%s: bad screen size %d x %d", who, H, W);
    HIVE_REQUIRE(ctx, nv >= 0 && nv < (1ll << 31) && (nv == 0 || vertices), "%s: bad vertex count %lld", who, (long long)nv);
    HIVE_REQUIRE(ctx, nf >= 0 && nf < (1ll << 31) && (nf == 0 || faces), "%s: bad face count %lld", who, (long long)nf);
    HIVE_REQUIRE(ctx, face_base >= 0 && face_base + nf < 0xffffffffll, "%s: face indices [%lld, %lld) do not fit below 2^32 - 1", who, (long long)face_base,
                 (long long)(face_base + nf));
    return HIVE_OK;
}

}  // namespace

extern "C" {

int hive_render_clear(hive_ctx *ctx, uint64_t *d_key, int H, int W) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_key && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "render_clear: bad arguments");
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(render_clear_kernel, rd_grid(n), dim3(RD_THREADS), 0, ctx->stream, (unsigned long long *)d_key, n);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_render_draw(hive_ctx *ctx, const double *d_vertices, int64_t nv, const int32_t *d_faces, int64_t nf, int64_t face_base, const double K[9], const double R[9],
                     const double t[3], int H, int W, double near, int32_t *d_xy, double *d_z, int32_t *d_large, uint32_t *d_counts, uint64_t *d_key) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    int rc;
    if ((rc = rd_check_mesh(ctx, "render_draw", d_vertices, nv, d_faces, nf, face_base, H, W))) return rc;
    HIVE_REQUIRE(ctx, K && R && t && d_key && d_counts, "render_draw: NULL argument");
    HIVE_REQUIRE(ctx, near > 0.0, "render_draw: near must be > 0");
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(d_counts, 0, 2 * sizeof(uint32_t), ctx->stream));
    if (nv == 0 || nf == 0) return HIVE_OK;
    HIVE_REQUIRE(ctx, d_xy && d_z && d_large, "render_draw: NULL scratch");
    RenderCam p;
    memcpy(p.K, K, sizeof(p.K));
    memcpy(p.R, R, sizeof(p.R));
    memcpy(p.t, t, sizeof(p.t));
    p.near = near;
    hipLaunchKernelGGL(render_project_kernel, rd_grid(nv), dim3(RD_THREADS), 0, ctx->stream, d_vertices, (long long)nv, p, d_xy, d_z);
    hipLaunchKernelGGL(render_raster_kernel, rd_grid(nf), dim3(RD_THREADS), 0, ctx->stream, d_faces, (long long)nf, (long long)nv, (unsigned)face_base,
                       (const int32_t *)d_xy, (const double *)d_z, H, W, (unsigned long long *)d_key, d_large, d_counts);
    // the list's length stays on the device: enough workgroups for a screenful of large faces, each striding over the list
    const dim3 grid((unsigned)std::min<long long>(nf, (long long)ctx->num_cus * 8));
    hipLaunchKernelGGL(render_raster_large_kernel, grid, dim3(RD_THREADS), 0, ctx->stream, d_faces, (long long)nf, (long long)nv, (unsigned)face_base,
                       (const int32_t *)d_xy, (const double *)d_z, H, W, (unsigned long long *)d_key, (const int32_t *)d_large, (const unsigned *)d_counts);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_render_shade(hive_ctx *ctx, int64_t nv, const int32_t *d_faces, int64_t nf, int64_t face_base, const int32_t *d_xy, const double *d_z,
                      const uint8_t *d_vertex_colors, const double *d_uv, const uint8_t *d_texture, int Ht, int Wt, const uint64_t *d_key, int H, int W,
                      uint8_t *d_color) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    int rc;
    if ((rc = rd_check_mesh(ctx, "render_shade", d_xy, nv, d_faces, nf, face_base, H, W))) return rc;
    HIVE_REQUIRE(ctx, d_key && d_color, "render_shade: NULL argument");
    if (nv == 0 || nf == 0) return HIVE_OK;
    HIVE_REQUIRE(ctx, d_xy && d_z, "render_shade: NULL projected vertices");
    HIVE_REQUIRE(ctx, d_vertex_colors || (d_uv && d_texture && Ht > 0 && Wt > 0), "render_shade: vertex colours, or uv and a texture of at least one texel");
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(render_shade_kernel, rd_grid(n), dim3(RD_THREADS), 0, ctx->stream, d_faces, (long long)nf, (long long)nv, (unsigned)face_base, d_xy, d_z,
                       d_vertex_colors, d_uv, d_texture, Ht, Wt, (const unsigned long long *)d_key, H, W, d_color);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_render_resolve(hive_ctx *ctx, const uint64_t *d_key, int H, int W, const uint8_t background[3], uint8_t *d_color, float *d_depth, int32_t *d_face) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, d_key && H > 0 && W > 0 && (long long)H * W < (1ll << 31), "render_resolve: bad arguments");
    RenderBackground bg = {{255, 255, 255}};
    if (background) memcpy(bg.rgb, background, 3);
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(render_resolve_kernel, rd_grid(n), dim3(RD_THREADS), 0, ctx->stream, (const unsigned long long *)d_key, n, bg, d_color, d_depth, d_face);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

}  // extern "C"
