// What is left visible at the label changes of texture.hip / texture_smooth.hip: one multiplicative gain per key frame and channel (samples, sums; the solve is
// the host's), and additive offsets that close the step at every seam vertex and are harmonic inside each patch (level).  No counterpart in the reference.
// gfx950 only.  The rules are stated in include/hive_mi355x.h above hive_texture_samples and restated in tests/texture_levelling_restatement.py; in short:
//
//   samples  per view, after hive_texture_vote on the same d_xy: a face with area != 0 whose three nearest pixels hold nine bytes in [1, 254] gives the
//            per-channel sums of the three pixels, any other face (0, 0, 0).
//   sums     G[c][a][b] = sum_f s_af s_bf, D[c][a][b] = sum_f s_af^2, N[a][b] = #f over the faces valid in both a and b.  Integers: any order gives the same
//            words.  A workgroup owns view a and a run of faces, walks b > a, reduces in its waves and adds once per word.
//   level    node = (vertex, label) of a participating face; a vertex with two labels or more is a seam vertex, its nodes fixed at mean - own colour; every
//            other node: `sweeps` Jacobi steps towards the mean of its faces' other two corners.  The offsets live on the node's first corner (its lowest
//            face); one launch per sweep, ping-pong, no workgroup waits for another.
//
// Float64 without contraction (the Makefile's EXACT flags), sums in the order written.  256 threads (four wave64) a workgroup.
#include "texture_core.hpp"

#include <algorithm>

namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_TILE = HIVE_SCAN_TILE;  // items per workgroup of the scan
constexpr int EX_PER_THREAD = 8;     // faces per thread of the sums kernel: a workgroup owns EX_PER_THREAD * LV_THREADS faces of one view
constexpr int EX_MAX_VIEWS = 256, LV_MAX_VIEWS = 65535, LV_MAX_SWEEPS = 4096;
enum { LV_TOTAL = 0, LV_SEAM_VERTICES, LV_MAX_OFFSET, LV_WORDS };  // the u64 words of a levelling, in its scratch

dim3 lv_grid(long long n) { return dim3((unsigned)std::max<long long>(1, (n + LV_THREADS - 1) / LV_THREADS)); }

__device__ __forceinline__ unsigned long long lv_wave_sum(unsigned long long s) {
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// ------------------------------------------------------------------------------------------------------------------------ samples
__global__ __launch_bounds__(LV_THREADS) void texture_samples_kernel(const int32_t *__restrict__ faces, long long nf, long long nv, const int32_t *__restrict__ xy,
                                                                     const long long *__restrict__ area, const uint8_t *__restrict__ frame, int H, int W,
                                                                     uint16_t *__restrict__ row) {
    const long long f = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (f >= nf) return;
    unsigned s[3] = {0, 0, 0};
    const int id[3] = {faces[3 * f + 0], faces[3 * f + 1], faces[3 * f + 2]};
    bool ok = area[f] != 0 && tx_ids_ok(id[0], id[1], id[2], nv);
    for (int k = 0; k < 3 && ok; ++k) {
        const long long X = xy[2 * (long long)id[k]], Y = xy[2 * (long long)id[k] + 1];
        const long long i = (Y + 128) >> 8, j = (X + 128) >> 8;
        if (i < 0 || i >= H || j < 0 || j >= W) {  // (a candidate of the vote is on the screen: only a table from elsewhere gets here)
            ok = false;
            break;
        }
        const uint8_t *p = frame + 3 * (i * W + j);
        for (int ch = 0; ch < 3; ++ch) {
            ok = ok && p[ch] >= 1 && p[ch] <= 254;
            s[ch] += p[ch];
        }
    }
    for (int ch = 0; ch < 3; ++ch) row[3 * f + ch] = ok ? (uint16_t)s[ch] : (uint16_t)0;
}

// ------------------------------------------------------------------------------------------------------------------------ sums
// acc u64 [7][n][n]: planes 0 .. 2 G (entries a < b only: the host mirrors them), 3 .. 5 D, 6 N (a < b only)
__global__ __launch_bounds__(LV_THREADS) void exposure_sums_kernel(const uint16_t *__restrict__ samples, int n, long long nf, unsigned long long *__restrict__ acc) {
    __shared__ unsigned long long lds[4][10];
    const int a = blockIdx.y;
    const long long base = (long long)blockIdx.x * (EX_PER_THREAD * LV_THREADS) + threadIdx.x;
    unsigned sa[EX_PER_THREAD][3];
#pragma unroll
    for (int j = 0; j < EX_PER_THREAD; ++j) {
        const long long f = base + (long long)j * LV_THREADS;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) sa[j][ch] = f < nf ? samples[3 * ((long long)a * nf + f) + ch] : 0u;
        if (!(sa[j][0] && sa[j][1] && sa[j][2])) sa[j][0] = sa[j][1] = sa[j][2] = 0;
    }
    const long long nn = (long long)n * n;
    for (int b = a + 1; b < n; ++b) {  // (the same trip count for every thread of the workgroup: the barriers below are uniform)
        unsigned long long v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // G rgb, D[a][b] rgb, D[b][a] rgb, N
#pragma unroll
        for (int j = 0; j < EX_PER_THREAD; ++j) {
            const long long f = base + (long long)j * LV_THREADS;
            if (f >= nf || !sa[j][0]) continue;
            const uint16_t *p = samples + 3 * ((long long)b * nf + f);
            const unsigned sb[3] = {p[0], p[1], p[2]};
            if (!(sb[0] && sb[1] && sb[2])) continue;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                v[ch] += (unsigned long long)sa[j][ch] * sb[ch];
                v[3 + ch] += (unsigned long long)sa[j][ch] * sa[j][ch];
                v[6 + ch] += (unsigned long long)sb[ch] * sb[ch];
            }
            v[9] += 1;
        }
#pragma unroll
        for (int i = 0; i < 10; ++i) v[i] = lv_wave_sum(v[i]);
        if ((threadIdx.x & 63) == 0)
            for (int i = 0; i < 10; ++i) lds[threadIdx.x >> 6][i] = v[i];
        __syncthreads();
        if (threadIdx.x < 10) {
            const int i = threadIdx.x;
            const unsigned long long s = ((lds[0][i] + lds[1][i]) + lds[2][i]) + lds[3][i];
            const long long ab = (long long)a * n + b, ba = (long long)b * n + a;
            const long long at = i < 3 ? i * nn + ab : i < 6 ? i * nn + ab : i < 9 ? (i - 3) * nn + ba : 6 * nn + ab;
            if (s) atomicAdd(acc + at, s);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------------ level
struct LvParams {
    const double *vertices;  // [nv][3]
    long long nv;
    const int32_t *faces;  // [nf][3]
    long long nf;
    const unsigned long long *best;  // [nf]
    const uint8_t *frames;           // [n][H][W][3]
    int n, H, W;
    TextureCam cam;
    const double *poses;    // [n][12]
    const unsigned *gains;  // [n][3] Q16
    int32_t *label;         // [nf] the view of a participating face, -1 for any other
    unsigned *vcount;       // [nv] participating faces of a vertex
    unsigned *cursor;       // [nv]
    unsigned *vstart;       // [nv + 1]
    int32_t *vcorners;      // [3 nf] per vertex the corners 3 g + k that hold it, ascending
    unsigned *blocks;       // block sums of the scan
    int32_t *rep;           // [3 nf] the corner that holds the offsets of this corner's node: the node's lowest face
    uint8_t *moves;         // [3 nf] 1: this corner holds a node that the sweeps move
    double *h[2];           // [3 nf][3] each, valid at the corners that hold a node
    unsigned long long *words;
    // c(v, l): fill's sample at P = V_v for view l, then the gain
    __device__ void colour(int v, int l, double out[3]) const {
        const double P[3] = {vertices[3 * (long long)v], vertices[3 * (long long)v + 1], vertices[3 * (long long)v + 2]};
        double c[3], s[3];
        tx_project(cam, poses + 12 * (long long)l, P, c);
        tx_bilinear(frames + 3 * (size_t)l * H * W, H, W, c, s);
        for (int ch = 0; ch < 3; ++ch) out[ch] = (s[ch] * (double)gains[3 * l + ch]) * 0x1p-16;
    }
};

__global__ __launch_bounds__(LV_THREADS) void lv_label_kernel(LvParams p) {
    const long long f = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (f >= p.nf) return;
    const int id[3] = {p.faces[3 * f], p.faces[3 * f + 1], p.faces[3 * f + 2]};
    const unsigned long long key = p.best[f];
    const int view = (int)(65535u - (unsigned)(key & 0xffffull));
    const bool part = key != 0 && view < p.n && tx_ids_ok(id[0], id[1], id[2], p.nv) && id[0] != id[1] && id[1] != id[2] && id[0] != id[2];
    p.label[f] = part ? view : -1;
    if (part)
        for (int k = 0; k < 3; ++k) atomicAdd(p.vcount + id[k], 1u);
}

// (the scan of the counts: tile_sums_kernel and tile_offsets_kernel of hive_internal.hpp, as hive_mesh_face_neighbours uses them)
__global__ __launch_bounds__(LV_THREADS) void lv_fill_kernel(LvParams p) {
    const long long f = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (f >= p.nf || p.label[f] < 0) return;
    for (int k = 0; k < 3; ++k) {
        const int v = p.faces[3 * f + k];
        p.vcorners[p.vstart[v] + atomicAdd(p.cursor + v, 1u)] = (int32_t)(3 * f + k);
    }
}

// a vertex's list in ascending order (the fill's order depends on the run): an insertion sort, quadratic in the vertex's degree -- fine for surfaces
__global__ __launch_bounds__(LV_THREADS) void lv_sort_kernel(LvParams p) {
    const long long v = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (v >= p.nv) return;
    int32_t *mine = p.vcorners + p.vstart[v];
    const unsigned count = p.vstart[v + 1] - p.vstart[v];
    for (unsigned i = 1; i < count; ++i) {
        const int32_t x = mine[i];
        unsigned at = i;
        for (; at > 0 && mine[at - 1] > x; --at) mine[at] = mine[at - 1];
        mine[at] = x;
    }
}

// per corner: the node's holder, and at the holder the start offsets: mean - own colour at a seam vertex, else 0
__global__ __launch_bounds__(LV_THREADS) void lv_init_kernel(LvParams p) {
    const long long c = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    unsigned long long seam_vertex = 0;
    if (c < 3 * p.nf) {
        const long long f = c / 3;
        const int l = p.label[f];
        double start[3] = {0.0, 0.0, 0.0};
        int32_t rep = (int32_t)c;
        bool moves = false;
        if (l >= 0) {
            const int v = p.faces[c];
            const unsigned lo = p.vstart[v], hi = p.vstart[v + 1];
            bool found = false, seam = false;
            int lowest = l;
            for (unsigned e = lo; e < hi; ++e) {
                const int32_t cg = p.vcorners[e];
                const int lg = p.label[cg / 3];
                if (lg == l && !found) found = true, rep = cg;
                seam = seam || lg != l;
                lowest = min(lowest, lg);
            }
            if (rep == c) {
                moves = !seam;
                if (seam) {
                    double own[3], sum[3] = {0.0, 0.0, 0.0}, count = 0.0;
                    p.colour(v, l, own);
                    for (int cur = -1;;) {  // the vertex's labels in ascending order
                        int next = LV_MAX_VIEWS + 1;
                        for (unsigned e = lo; e < hi; ++e) {
                            const int lg = p.label[p.vcorners[e] / 3];
                            if (lg > cur && lg < next) next = lg;
                        }
                        if (next > LV_MAX_VIEWS) break;
                        double col[3];
                        p.colour(v, next, col);
                        for (int ch = 0; ch < 3; ++ch) sum[ch] = sum[ch] + col[ch];
                        count += 1.0;
                        cur = next;
                    }
                    for (int ch = 0; ch < 3; ++ch) start[ch] = sum[ch] / count - own[ch];
                    seam_vertex = l == lowest;
                }
            }
        }
        p.rep[c] = rep;
        p.moves[c] = moves;
        for (int ch = 0; ch < 3; ++ch) p.h[0][3 * c + ch] = p.h[1][3 * c + ch] = start[ch];
    }
    seam_vertex = lv_wave_sum(seam_vertex);
    if ((threadIdx.x & 63) == 0 && seam_vertex) atomicAdd(p.words + LV_SEAM_VERTICES, seam_vertex);
}

// one Jacobi sweep: reads `src` alone, writes the nodes that move to `dst` (a fixed node holds its value in both)
__global__ __launch_bounds__(LV_THREADS) void lv_sweep_kernel(LvParams p, const double *__restrict__ src, double *__restrict__ dst) {
    const long long c = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    if (c >= 3 * p.nf || !p.moves[c]) return;
    const int l = p.label[c / 3], v = p.faces[c];
    double s[3] = {0.0, 0.0, 0.0}, count = 0.0;
    for (unsigned e = p.vstart[v]; e < p.vstart[v + 1]; ++e) {  // the node's faces in ascending order
        const int32_t cg = p.vcorners[e];
        const int32_t g = cg / 3, k = cg - 3 * g;
        if (p.label[g] != l) continue;
        const long long one = p.rep[3 * (long long)g + (k + 1) % 3], two = p.rep[3 * (long long)g + (k + 2) % 3];
        for (int ch = 0; ch < 3; ++ch) s[ch] = (s[ch] + src[3 * one + ch]) + src[3 * two + ch];
        count += 1.0;
    }
    for (int ch = 0; ch < 3; ++ch) dst[3 * c + ch] = s[ch] / (2.0 * count);
}

// the offsets per face corner, 0 at a face that takes no part; the largest magnitude (a non-negative double's bits order as an integer's)
__global__ __launch_bounds__(LV_THREADS) void lv_finish_kernel(LvParams p, const double *__restrict__ h, double *__restrict__ out) {
    const long long c = (long long)blockIdx.x * LV_THREADS + threadIdx.x;
    double most = 0.0;
    if (c < 3 * p.nf) {
        const bool part = p.label[c / 3] >= 0;
        const long long at = part ? p.rep[c] : 0;
        for (int ch = 0; ch < 3; ++ch) {
            const double x = part ? h[3 * at + ch] : 0.0;
            out[3 * c + ch] = x;
            most = fmax(most, fabs(x));
        }
    }
    for (int off = 32; off > 0; off >>= 1) most = fmax(most, __shfl_xor(most, off));
    if ((threadIdx.x & 63) == 0 && most > 0.0) atomicMax(p.words + LV_MAX_OFFSET, (unsigned long long)__double_as_longlong(most));
}

}  // namespace

extern "C" {

int hive_texture_samples(hive_ctx *ctx, const int32_t *d_faces, int64_t nf, int64_t nv, const int32_t *d_xy, const int64_t *d_area, const uint8_t *d_frame, int H,
                         int W, int view_index, uint16_t *d_samples) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && ((long long)H + 1) * ((long long)W + 1) <= (1ll << 31), "texture_samples: bad screen size %d x %d", H, W);
    HIVE_REQUIRE(ctx, nf >= 0 && nf < (1ll << 31) && nv >= 0 && nv < (1ll << 31), "texture_samples: bad counts %lld faces, %lld vertices", (long long)nf, (long long)nv);
    HIVE_REQUIRE(ctx, view_index >= 0 && view_index < LV_MAX_VIEWS && ((long long)view_index + 1) * nf < (1ll << 31),
                 "texture_samples: row %d of %lld faces outside a table of fewer than 2^31 entries", view_index, (long long)nf);
    if (nf == 0) return HIVE_OK;
    HIVE_REQUIRE(ctx, d_faces && d_area && d_samples && d_frame && (nv == 0 || d_xy), "texture_samples: NULL argument");
    hipLaunchKernelGGL(texture_samples_kernel, lv_grid(nf), dim3(LV_THREADS), 0, ctx->stream, d_faces, (long long)nf, (long long)nv, d_xy,
                       (const long long *)d_area + (long long)view_index * nf, d_frame, H, W, d_samples + 3 * (long long)view_index * nf);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

int hive_texture_exposure_sums(hive_ctx *ctx, const uint16_t *d_samples, int n_views, int64_t nf, int64_t *G, int64_t *D, int64_t *N) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, n_views > 0 && n_views <= EX_MAX_VIEWS, "texture_exposure_sums: %d views outside [1, 256]: the pair sums are n^2 words and n^2 / 2 passes over the faces",
                 n_views);
    HIVE_REQUIRE(ctx, nf >= 0 && (long long)n_views * nf < (1ll << 31), "texture_exposure_sums: %d views x %lld faces: the table holds fewer than 2^31 entries", n_views,
                 (long long)nf);
    HIVE_REQUIRE(ctx, G && D && N, "texture_exposure_sums: NULL argument");
    const size_t nn = (size_t)n_views * n_views;
    memset(G, 0, 3 * nn * sizeof(int64_t)), memset(D, 0, 3 * nn * sizeof(int64_t)), memset(N, 0, nn * sizeof(int64_t));
    if (nf == 0 || n_views == 1) return HIVE_OK;
    HIVE_REQUIRE(ctx, d_samples, "texture_exposure_sums: NULL argument");
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, 7 * nn * sizeof(unsigned long long));
    if (rc) return rc;
    unsigned long long *acc = (unsigned long long *)ctx->d_scratch;
    hipStream_t s = ctx->stream;
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(acc, 0, 7 * nn * sizeof(unsigned long long), s));
    const dim3 grid((unsigned)hive_div_up(nf, EX_PER_THREAD * LV_THREADS), (unsigned)(n_views - 1));
    hipLaunchKernelGGL(exposure_sums_kernel, grid, dim3(LV_THREADS), 0, s, d_samples, n_views, (long long)nf, acc);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    std::vector<int64_t> back(7 * nn);  // one read-back
    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(back.data(), acc, 7 * nn * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIVE_CHECK_HIP(ctx, hipStreamSynchronize(s));
    memcpy(G, back.data(), 3 * nn * sizeof(int64_t)), memcpy(D, back.data() + 3 * nn, 3 * nn * sizeof(int64_t)), memcpy(N, back.data() + 6 * nn, nn * sizeof(int64_t));
    for (int a = 0; a < n_views; ++a)
        for (int b = a + 1; b < n_views; ++b) {
            const size_t ab = (size_t)a * n_views + b, ba = (size_t)b * n_views + a;
            for (int ch = 0; ch < 3; ++ch) G[ch * nn + ba] = G[ch * nn + ab];
            N[ba] = N[ab];
        }
    return HIVE_OK;
}

int hive_texture_level(hive_ctx *ctx, const double *d_vertices, int64_t nv, const int32_t *d_faces, int64_t nf, const uint64_t *d_best, const uint8_t *d_frames, int n,
                       int H, int W, const double K[9], const double *d_poses, const uint32_t *d_gains_q16, int sweeps, double *d_offsets, int64_t *seam_vertices,
                       double *max_offset) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, n > 0 && n <= LV_MAX_VIEWS, "texture_level: %d views outside [1, 65535]", n);
    HIVE_REQUIRE(ctx, H > 0 && W > 0 && (long long)H * W < (1ll << 31), "texture_level: bad frame size %d x %d", H, W);
    HIVE_REQUIRE(ctx, sweeps >= 0 && sweeps <= LV_MAX_SWEEPS, "texture_level: %d sweeps outside [0, 4096]", sweeps);
    HIVE_REQUIRE(ctx, nf > 0 && 3 * nf < (1ll << 31) && nv > 0 && nv < (1ll << 31), "texture_level: bad counts %lld faces, %lld vertices", (long long)nf, (long long)nv);
    HIVE_REQUIRE(ctx, d_vertices && d_faces && d_best && d_frames && K && d_poses && d_gains_q16 && d_offsets, "texture_level: NULL argument");
    LvParams p{};
    p.vertices = d_vertices, p.nv = nv, p.faces = d_faces, p.nf = nf, p.best = (const unsigned long long *)d_best;
    p.frames = d_frames, p.n = n, p.H = H, p.W = W, p.poses = d_poses, p.gains = (const unsigned *)d_gains_q16;
    memcpy(p.cam.K, K, sizeof(p.cam.K));
    p.cam.near = 0.0;  // (a node is a vertex its view's draw kept: no near test)
    const int nb_v = hive_div_up(nv + 1, LV_TILE);
    auto lay = [&](char *base) {
        hive_scratch_layout L{base};
        p.words = L.take<unsigned long long>(LV_WORDS);
        p.vcount = L.take<unsigned>(2 * (size_t)nv);  // the counts and, behind them, the cursors: one memset
        p.cursor = p.vcount ? p.vcount + nv : nullptr;
        p.vstart = L.take<unsigned>((size_t)nv + 1);
        p.blocks = L.take<unsigned>((size_t)nb_v);
        p.label = L.take<int32_t>((size_t)nf);
        p.vcorners = L.take<int32_t>(3 * (size_t)nf);
        p.rep = L.take<int32_t>(3 * (size_t)nf);
        p.moves = L.take<uint8_t>(3 * (size_t)nf);
        p.h[0] = L.take<double>(9 * (size_t)nf);
        p.h[1] = L.take<double>(9 * (size_t)nf);
        return L.bytes();
    };
    int rc = hive_reserve_device(ctx, &ctx->d_scratch, &ctx->scratch_bytes, lay(nullptr));
    if (rc) return rc;
    lay((char *)ctx->d_scratch);
    hipStream_t s = ctx->stream;
    const dim3 blk(LV_THREADS), faces_grid = lv_grid(nf), corners_grid = lv_grid(3 * nf);
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(p.words, 0, LV_WORDS * sizeof(unsigned long long), s));
    HIVE_CHECK_HIP(ctx, hipMemsetAsync(p.vcount, 0, 2 * (size_t)nv * sizeof(unsigned), s));
    hipLaunchKernelGGL(lv_label_kernel, faces_grid, blk, 0, s, p);
    hipLaunchKernelGGL(tile_sums_kernel<LV_TILE>, dim3(nb_v), blk, 0, s, (const unsigned *)p.vcount, (long long)nv, p.blocks);
    hive_scan_counts(ctx, nb_v, p.words + LV_TOTAL, p.blocks);
    hipLaunchKernelGGL((tile_offsets_kernel<LV_TILE, unsigned>), dim3(nb_v), blk, 0, s, (const unsigned *)p.vcount, (long long)nv, (const unsigned *)p.blocks, p.vstart);
    hipLaunchKernelGGL(lv_fill_kernel, faces_grid, blk, 0, s, p);
    hipLaunchKernelGGL(lv_sort_kernel, lv_grid(nv), blk, 0, s, p);
    hipLaunchKernelGGL(lv_init_kernel, corners_grid, blk, 0, s, p);
    for (int sweep = 0; sweep < sweeps; ++sweep) hipLaunchKernelGGL(lv_sweep_kernel, corners_grid, blk, 0, s, p, (const double *)p.h[sweep & 1], p.h[(sweep + 1) & 1]);
    hipLaunchKernelGGL(lv_finish_kernel, corners_grid, blk, 0, s, p, (const double *)p.h[sweeps & 1], d_offsets);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    if (seam_vertices || max_offset) {
        void *pinned;
        if ((rc = hive_pinned_small(ctx, &pinned))) return rc;
        HIVE_CHECK_HIP(ctx, hipMemcpyAsync(pinned, p.words, LV_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIVE_CHECK_HIP(ctx, hipStreamSynchronize(s));
        const volatile unsigned long long *back = (const volatile unsigned long long *)pinned;
        if (seam_vertices) *seam_vertices = (int64_t)back[LV_SEAM_VERTICES];
        if (max_offset) {
            const unsigned long long bits = back[LV_MAX_OFFSET];
            memcpy(max_offset, &bits, sizeof(double));
        }
    }
    return HIVE_OK;
}

}  // extern "C"
