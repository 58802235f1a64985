// LPIPS(net='alex', version 0.1) of a render against a held-out frame on the device: the third column of the reference's result tables
// (scripts/compare_image_pair.py:29-41,110-133, scripts/experiments.py:663-684,844-852,1384-1426, scripts/compare_image_pairs.py:40-84).  gfx950 only.
// The rules are stated in include/hive_mi355x.h above hive_lpips_create; in short:
//
//   input    a byte reads through the 3 x 256 float32 table the host built (value, then the scaling layer); variant 1 reads a reference byte as 255 where the
//            estimate's byte of the same pixel and channel is 255 (while loading: the whitened frame is never written)
//   conv     five float32 convolutions as implicit GEMMs on __builtin_amdgcn_mfma_f32_32x32x2f32: rows = output pixels of every picture, columns = output
//            channels, k = (ky, kx, ci) ascending.  One accumulator chain per output value, k ascending from 0.0, no split-K, no atomics: the bits of a
//            value depend on its receptive field and the weights alone.  Bias, then ReLU, in the epilogue
//   pool     maxpool 3 / 2 (floor, no padding) in front of layers 1 and 2, a pass of its own
//   tail     per pixel and layer, float64, c ascending: the two norms, then d = sum_c w_c * (a_c / (na + 1e-10) - b_c / (nb + 1e-10))^2
//   sums     a workgroup owns 256 consecutive pixels of one picture: the fixed tree gives its partial, hive_similarity_finish the layer's mean
//
// Float32 / float64 without contraction (the Makefile's EXACT flags); MFMA accumulators in VGPRs.
//
// Kernels: lpips_conv_kernel<MODE> (one workgroup per 64 x 64 tile of the [pixels][channels] output; MODE 0: a 16-wide k chunk lies inside one tap and is loaded
// as float4, Cin % 16 == 0; MODE 1: any Cin, scalar gathers, the K tail zero-filled in LDS; MODE 2: as 1 from the two u8 pictures through the table),
// lpips_pool_kernel (one thread per four channels of a pooled pixel), lpips_tail_kernel (one thread per pixel, the channels staged through LDS), lpips_sum_kernel (one thread per pair and
// variant), lpips_repack_kernel (OIHW -> [k][Cout], once per model).
#include <algorithm>

#include "hive_internal.hpp"

struct hive_lpips {
    hive_ctx *ctx = nullptr;
    float *d_w[5] = {}, *d_b[5] = {}, *d_lin[5] = {};  // [K][Cout], [Cout], [Cout]: regions of `mem`
    float *d_table = nullptr;                           // [3][256]
    void *mem = nullptr;
    void *ws = nullptr;  // features, pooled maps, partials and layer scores of one chunk of pictures: grown on demand, never shrunk
    size_t ws_bytes = 0;
};

namespace {

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

constexpr int LP_THREADS = 256;
constexpr int LP_BM = 64, LP_BN = 64, LP_BK = 16;  // the output tile (pixels x channels) and the k chunk of the convolution kernel
constexpr int LP_LD = LP_BM + 4;                   // LDS row: 68 floats (272 bytes, a multiple of 16)
constexpr int LP_TAIL_C = 16;                     // channels of 256 pixels the tail kernel holds in LDS at a time (every C_out is a multiple)
constexpr int LP_MIN_SIDE = 31;                    // conv1 gives 7, the pools 3 and 1
constexpr size_t LP_WS_CAP = (size_t)1 << 30;      // a chunk of pictures is sized to keep the workspace below this (one picture may exceed it)

struct LpLayer {
    int cin, cout, k, stride, pad, pool;
};
constexpr LpLayer LP_LAYERS[5] = {{3, 64, 11, 4, 2, 0}, {64, 192, 5, 1, 2, 1}, {192, 384, 3, 1, 1, 1}, {384, 256, 3, 1, 1, 0}, {256, 256, 3, 1, 1, 0}};

struct LpShape {
    int M;               // output pixels of every picture of the launch
    int H, W, Cin;       // the convolution's input (after the pool)
    int Ho, Wo, Cout;
    int KW, stride, pad, K;
};

// grid (ceil(M / 64), ceil(Cout / 64)).  MODE 0 / 1: `in` f32 [B][H][W][Cin].  MODE 2: ref / est u8 [nc][H][W][3]; picture b of the launch is set b / nc
// (sets 0 .. variants - 1 the reference, plain then masked; set `variants` the estimate), picture b % nc.
template <int MODE>
__global__ __launch_bounds__(LP_THREADS) void lpips_conv_kernel(const float *__restrict__ in, const uint8_t *__restrict__ ref, const uint8_t *__restrict__ est, int nc,
                                                                int variants, const float *__restrict__ table, const float *__restrict__ wk,
                                                                const float *__restrict__ bias, float *__restrict__ out, LpShape s) {
    __shared__ __attribute__((aligned(16))) float As[LP_BK][LP_LD];
    __shared__ __attribute__((aligned(16))) float Bs[LP_BK][LP_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = blockIdx.x * LP_BM, n0 = blockIdx.y * LP_BN;
    // the output pixel whose operand row this thread stages
    const int ar = MODE == 0 ? t >> 2 : t & 63;
    const int am = m0 + ar;
    const bool a_ok = am < s.M;
    int ab = 0, iy0 = 0, ix0 = 0;
    if (a_ok) {
        ab = am / (s.Ho * s.Wo);
        const int rem = am % (s.Ho * s.Wo);
        iy0 = (rem / s.Wo) * s.stride - s.pad, ix0 = (rem % s.Wo) * s.stride - s.pad;
    }
    const int bk = t >> 4, bc = n0 + (t & 15) * 4;  // the weight row (inside the chunk) and the first of four channels this thread stages

    float a_reg[4];
    float4 b_reg;
    auto fetch = [&](int k0) {
        if (MODE == 0) {  // the chunk [k0, k0 + 16) lies inside one tap: four consecutive channels
            const int tap = k0 / s.Cin, ci = k0 % s.Cin + (t & 3) * 4;
            const int iy = iy0 + tap / s.KW, ix = ix0 + tap % s.KW;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a_ok && iy >= 0 && iy < s.H && ix >= 0 && ix < s.W) v = *(const float4 *)(in + (((size_t)ab * s.H + iy) * s.W + ix) * s.Cin + ci);
            a_reg[0] = v.x, a_reg[1] = v.y, a_reg[2] = v.z, a_reg[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + wave + 4 * j;
                float v = 0.f;  // the zero padding of the convolution, the rows past M and the tail of K
                if (a_ok && k < s.K) {
                    const int row = s.KW * s.Cin, ky = k / row, r = k % row, kx = r / s.Cin, ci = r % s.Cin;
                    const int iy = iy0 + ky, ix = ix0 + kx;
                    if (iy >= 0 && iy < s.H && ix >= 0 && ix < s.W) {
                        if (MODE == 1) {
                            v = in[(((size_t)ab * s.H + iy) * s.W + ix) * s.Cin + ci];
                        } else {
                            const int set = ab / nc, n = ab % nc;
                            const size_t at = (((size_t)n * s.H + iy) * s.W + ix) * 3 + ci;
                            int byte;
                            if (set == variants) {
                                byte = est[at];
                            } else {
                                byte = ref[at];
                                if (set == 1 && est[at] == 255) byte = 255;
                            }
                            v = table[ci * 256 + byte];
                        }
                    }
                }
                a_reg[j] = v;
            }
        }
        b_reg = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 + bk < s.K && bc < s.Cout) b_reg = *(const float4 *)(wk + (size_t)(k0 + bk) * s.Cout + bc);  // (Cout % 4 == 0)
    };

    lp_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;  // this wave's 32 x 32 quarter of the tile
    const int li = lane & 31, lh = lane >> 5;
    const int chunks = (s.K + LP_BK - 1) / LP_BK;
    fetch(0);
    for (int kc = 0; kc < chunks; ++kc) {
        __syncthreads();  // the previous chunk has been read
        if (MODE == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) As[(t & 3) * 4 + j][ar] = a_reg[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) As[wave + 4 * j][ar] = a_reg[j];
        }
        *(float4 *)&Bs[bk][(t & 15) * 4] = b_reg;
        __syncthreads();
        if (kc + 1 < chunks) fetch((kc + 1) * LP_BK);  // in flight under the MFMAs below
#pragma unroll
        for (int kk = 0; kk < LP_BK / 2; ++kk)  // lanes 0-31 carry k = 2 kk, lanes 32-63 k = 2 kk + 1: the chain is k ascending
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * kk + lh][wm + li], Bs[2 * kk + lh][wn + li], acc, 0, 0, 0);
    }
    const int col = n0 + wn + li;
    if (col >= s.Cout) return;
    const float bv = bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m >= s.M) continue;
        const float v = acc[r] + bv;
        out[(size_t)m * s.Cout + col] = v > 0.f ? v : 0.f;
    }
}

// maxpool 3 / 2, floor, no padding: in f32 [B][h][w][C] -> out [B][hp][wp][C]; one thread per four channels, grid-stride
__global__ __launch_bounds__(LP_THREADS) void lpips_pool_kernel(const float *__restrict__ in, long long total4, int h, int w, int hp, int wp, int C,
                                                                float *__restrict__ out) {
    const int c4n = C / 4;
    for (long long e = (long long)blockIdx.x * LP_THREADS + threadIdx.x; e < total4; e += (long long)gridDim.x * LP_THREADS) {
        const int c4 = (int)(e % c4n);
        long long q = e / c4n;
        const int px = (int)(q % wp);
        q /= wp;
        const int py = (int)(q % hp);
        const long long b = q / hp;
        const float *base = in + (((size_t)b * h + 2 * py) * w + 2 * px) * C + 4 * c4;
        float4 m = *(const float4 *)base;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float4 v = *(const float4 *)(base + ((size_t)dy * w + dx) * C);
                m.x = v.x > m.x ? v.x : m.x, m.y = v.y > m.y ? v.y : m.y, m.z = v.z > m.z ? v.z : m.z, m.w = v.w > m.w ? v.w : m.w;
            }
        *(float4 *)(out + (size_t)e * 4) = m;
    }
}

// grid (ceil(hw / 256), variants * nc).  feat f32 [variants + 1][nc][hw][C], C % 16 == 0; partials f64 [variants][nc][gridDim.x]; dist (optional) f64 rows of hw
// values, the row of (variant v, picture n) at dist + (v * dist_pictures + n) * hw.  Thread t owns pixel blockIdx.x * 256 + t and adds over c ascending; the
// workgroup brings 16 channels of its 256 pixels at a time through LDS (35 KB) with coalesced loads, once for the norms and once for d.
__global__ __launch_bounds__(LP_THREADS) void lpips_tail_kernel(const float *__restrict__ feat, int nc, int variants, int hw, int C, const float *__restrict__ lin,
                                                                double *__restrict__ partials, double *__restrict__ dist, long long dist_pictures) {
    __shared__ float sa[LP_THREADS][LP_TAIL_C + 1], sb[LP_THREADS][LP_TAIL_C + 1];
    __shared__ double red[LP_THREADS];
    const int t = threadIdx.x, z = blockIdx.y, v = z / nc, n = z % nc;
    const int p0 = blockIdx.x * LP_THREADS, p = p0 + t;
    const float *a = feat + (((size_t)v * nc + n) * hw + p0) * C, *b = feat + (((size_t)variants * nc + n) * hw + p0) * C;
    auto stage = [&](int c0) {
        __syncthreads();  // the previous chunk has been read
#pragma unroll
        for (int j = 0; j < LP_TAIL_C / 4; ++j) {
            const int e = t + LP_THREADS * j, r = e / (LP_TAIL_C / 4), q = e % (LP_TAIL_C / 4);  // four consecutive threads read 64 consecutive bytes of a row
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
            if (p0 + r < hw) x = *(const float4 *)(a + (size_t)r * C + c0 + 4 * q), y = *(const float4 *)(b + (size_t)r * C + c0 + 4 * q);
            sa[r][4 * q] = x.x, sa[r][4 * q + 1] = x.y, sa[r][4 * q + 2] = x.z, sa[r][4 * q + 3] = x.w;
            sb[r][4 * q] = y.x, sb[r][4 * q + 1] = y.y, sb[r][4 * q + 2] = y.z, sb[r][4 * q + 3] = y.w;
        }
        __syncthreads();
    };
    double sum_a = 0.0, sum_b = 0.0;
    for (int c0 = 0; c0 < C; c0 += LP_TAIL_C) {
        stage(c0);
#pragma unroll
        for (int c = 0; c < LP_TAIL_C; ++c) {
            const double x = (double)sa[t][c], y = (double)sb[t][c];
            sum_a = sum_a + x * x, sum_b = sum_b + y * y;
        }
    }
    const double na = sqrt(sum_a) + 1e-10, nb = sqrt(sum_b) + 1e-10;
    double d = 0.0;
    for (int c0 = 0; c0 < C; c0 += LP_TAIL_C) {
        stage(c0);
#pragma unroll
        for (int c = 0; c < LP_TAIL_C; ++c) {
            const double q = (double)sa[t][c] / na - (double)sb[t][c] / nb;
            d = d + (double)lin[c0 + c] * (q * q);
        }
    }
    if (p >= hw) d = 0.0;  // (a pixel past the end saw zeros: 0 / 1e-10 - 0 / 1e-10)
    if (p < hw && dist) dist[((size_t)v * dist_pictures + n) * hw + p] = d;
    red[t] = d;
    block_tree_sum<LP_THREADS, 1>(&red);  // the fixed tree of the picture scores
    if (t == 0) partials[(size_t)z * gridDim.x + blockIdx.x] = red[0];
}

// layer_scores f64 [5][count] -> out[e] = l0 + l1 + l2 + l3 + l4, left to right
__global__ __launch_bounds__(LP_THREADS) void lpips_sum_kernel(const double *__restrict__ layer_scores, long long count, double *__restrict__ out) {
    const long long e = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (e >= count) return;
    double sum = layer_scores[e];
    for (int l = 1; l < 5; ++l) sum = sum + layer_scores[(size_t)l * count + e];
    out[e] = sum;
}

// OIHW [Cout][Cin][KH][KW] -> [(ky * KW + kx) * Cin + ci][Cout]
__global__ __launch_bounds__(LP_THREADS) void lpips_repack_kernel(const float *__restrict__ oihw, int Cout, int Cin, int KH, int KW, float *__restrict__ wk) {
    const long long total = (long long)Cout * Cin * KH * KW;
    const long long e = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (e >= total) return;
    const int co = (int)(e % Cout);
    long long k = e / Cout;
    const int ci = (int)(k % Cin);
    k /= Cin;
    const int kx = (int)(k % KW), ky = (int)(k / KW);
    wk[e] = oihw[(((size_t)co * Cin + ci) * KH + ky) * KW + kx];
}

struct LpSizes {
    int hp, wp;  // the convolution's input, after the pool when the layer has one
    int ho, wo;
};
// false when the layer has no output at this input size
bool lp_sizes(int layer, int h, int w, LpSizes *o) {
    const LpLayer &L = LP_LAYERS[layer];
    o->hp = h, o->wp = w;
    if (L.pool) {
        if (h < 3 || w < 3) return false;
        o->hp = (h - 3) / 2 + 1, o->wp = (w - 3) / 2 + 1;
    }
    const int eh = o->hp + 2 * L.pad - L.k, ew = o->wp + 2 * L.pad - L.k;
    if (eh < 0 || ew < 0) return false;
    o->ho = eh / L.stride + 1, o->wo = ew / L.stride + 1;
    return true;
}

// One row of the layer table over B pictures on the context's stream: `in` f32 [B][h][w][Cin], or (layer 0, in == NULL) the u8 pictures as lpips_conv_kernel
// MODE 2 reads them with B = (variants + 1) * nc.  `pooled`: room for B * hp * wp * Cin floats when the layer pools.  The caller keeps B * ho * wo <= 65535 * 64.
int lp_run_layer(hive_lpips *net, int layer, const float *in, const uint8_t *ref, const uint8_t *est, int nc, int variants, int B, int h, int w, float *pooled,
                 float *out) {
    hive_ctx *ctx = net->ctx;
    const LpLayer &L = LP_LAYERS[layer];
    LpSizes z;
    if (!lp_sizes(layer, h, w, &z)) return hive_fail(ctx, HIVE_ERR_INVALID, "lpips: layer %d has no output at %d x %d", layer, h, w);
    if (L.pool) {
        const long long total4 = (long long)B * z.hp * z.wp * (L.cin / 4);
        const long long blocks = (total4 + LP_THREADS - 1) / LP_THREADS;
        hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(LP_THREADS), 0, ctx->stream, in, total4, h, w, z.hp, z.wp, L.cin,
                           pooled);
        in = pooled;
    }
    LpShape s;
    s.M = B * z.ho * z.wo;
    s.H = z.hp, s.W = z.wp, s.Cin = L.cin, s.Ho = z.ho, s.Wo = z.wo, s.Cout = L.cout, s.KW = L.k, s.stride = L.stride, s.pad = L.pad, s.K = L.k * L.k * L.cin;
    const dim3 grid((unsigned)((s.M + LP_BM - 1) / LP_BM), (unsigned)((L.cout + LP_BN - 1) / LP_BN));
    if (!in)
        hipLaunchKernelGGL(lpips_conv_kernel<2>, grid, dim3(LP_THREADS), 0, ctx->stream, nullptr, ref, est, nc, variants, net->d_table, net->d_w[layer], net->d_b[layer],
                           out, s);
    else if (L.cin % LP_BK == 0)
        hipLaunchKernelGGL(lpips_conv_kernel<0>, grid, dim3(LP_THREADS), 0, ctx->stream, in, nullptr, nullptr, 1, 1, nullptr, net->d_w[layer], net->d_b[layer], out, s);
    else
        hipLaunchKernelGGL(lpips_conv_kernel<1>, grid, dim3(LP_THREADS), 0, ctx->stream, in, nullptr, nullptr, 1, 1, nullptr, net->d_w[layer], net->d_b[layer], out, s);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

}  // namespace

extern "C" {

int hive_lpips_create(hive_ctx *ctx, const float *const conv_w[5], const float *const conv_b[5], const float *const lin_w[5], hive_lpips **out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, conv_w && conv_b && lin_w && out, "lpips_create: NULL argument");
    for (int l = 0; l < 5; ++l) HIVE_REQUIRE(ctx, conv_w[l] && conv_b[l] && lin_w[l], "lpips_create: layer %d has a NULL weight pointer", l);
    *out = nullptr;
    // the input table: the value of a byte in float64 rounded to float32 (compare_image_pair.py:30-33), then the scaling layer in float32
    float table[3 * 256];
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    for (int k = 0; k < 3; ++k)
        for (int v = 0; v < 256; ++v) {
            const float x = (float)(((double)v / 255.0) * 2.0 - 1.0);
            table[k * 256 + v] = (x - shift[k]) / scale[k];
        }
    hive_scratch_layout lay;
    size_t biggest = 0;
    auto regions = [&](hive_lpips *net) {
        for (int l = 0; l < 5; ++l) {
            const LpLayer &L = LP_LAYERS[l];
            const size_t nw = (size_t)L.k * L.k * L.cin * L.cout;
            float *w = lay.take<float>(nw), *b = lay.take<float>(L.cout), *g = lay.take<float>(L.cout);
            if (net) net->d_w[l] = w, net->d_b[l] = b, net->d_lin[l] = g;
            biggest = nw > biggest ? nw : biggest;
        }
        float *tab = lay.take<float>(3 * 256);
        if (net) net->d_table = tab;
    };
    regions(nullptr);
    void *mem = nullptr;
    HIVE_CHECK_HIP(ctx, hipMalloc(&mem, lay.bytes()));
    hive_lpips *net = new hive_lpips();
    net->ctx = ctx;
    net->mem = mem;
    lay = hive_scratch_layout{(char *)mem, 0};
    regions(net);
    int rc = hive_reserve_device(ctx, &ctx->d_in, &ctx->in_bytes, biggest * sizeof(float));
    for (int l = 0; l < 5 && !rc; ++l) {
        const LpLayer &L = LP_LAYERS[l];
        const size_t nw = (size_t)L.k * L.k * L.cin * L.cout;
        rc = hive_upload(ctx, ctx->d_in, conv_w[l], nw * sizeof(float));
        if (rc) break;
        hipLaunchKernelGGL(lpips_repack_kernel, dim3((unsigned)((nw + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS), 0, ctx->stream, (const float *)ctx->d_in, L.cout,
                           L.cin, L.k, L.k, net->d_w[l]);
        rc = hive_upload(ctx, net->d_b[l], conv_b[l], L.cout * sizeof(float));
        if (!rc) rc = hive_upload(ctx, net->d_lin[l], lin_w[l], L.cout * sizeof(float));
    }
    if (!rc) rc = hive_upload(ctx, net->d_table, table, sizeof(table));
    if (!rc && hipGetLastError() != hipSuccess) rc = hive_fail(ctx, HIVE_ERR_DEVICE, "lpips_create: the repack launch failed");
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(mem);
        delete net;
        return rc;
    }
    *out = net;
    return HIVE_OK;
}

int hive_lpips_destroy(hive_lpips *net) {
    HIVE_ENTER(net ? net->ctx : nullptr);
    if (!net) return HIVE_OK;
    (void)hipStreamSynchronize(net->ctx->stream);
    if (net->ws) (void)hipFree(net->ws);
    if (net->mem) (void)hipFree(net->mem);
    delete net;
    return HIVE_OK;
}

int hive_lpips_layer(hive_lpips *net, int layer, const float *d_in, int N, int h, int w, float *d_out) {
    HIVE_ENTER(net ? net->ctx : nullptr);
    if (!net) return hive_fail(nullptr, HIVE_ERR_INVALID, "lpips is NULL");
    hive_ctx *ctx = net->ctx;
    HIVE_REQUIRE(ctx, layer >= 0 && layer < 5, "lpips_layer: layer = %d, need 0 .. 4", layer);
    HIVE_REQUIRE(ctx, d_in && d_out, "lpips_layer: NULL argument");
    HIVE_REQUIRE(ctx, ((uintptr_t)d_in | (uintptr_t)d_out) % 16 == 0, "lpips_layer: the tensors must be 16-byte aligned");
    HIVE_REQUIRE(ctx, N >= 1, "lpips_layer: N = %d, need at least one picture", N);
    LpSizes z;
    HIVE_REQUIRE(ctx, h >= 1 && w >= 1 && lp_sizes(layer, h, w, &z), "lpips_layer: layer %d has no output at %d x %d", layer, h, w);
    const LpLayer &L = LP_LAYERS[layer];
    HIVE_REQUIRE(ctx, (long long)h * w * L.cin < (1ll << 31), "lpips_layer: %d x %d x %d values do not fit below 2^31", h, w, L.cin);
    // pictures per launch: at most 65535 row tiles, and a pooled map below the workspace cap
    const long long out_px = (long long)z.ho * z.wo, pooled_floats = L.pool ? (long long)z.hp * z.wp * L.cin : 0;
    long long per = 65535ll * LP_BM / out_px;
    if (pooled_floats) per = std::min(per, std::max(1ll, (long long)(LP_WS_CAP / sizeof(float)) / pooled_floats));
    HIVE_REQUIRE(ctx, per >= 1, "lpips_layer: %d x %d is too large for one launch", h, w);
    per = std::min<long long>(per, N);
    float *pooled = nullptr;
    if (pooled_floats) {
        int rc = hive_reserve_device(ctx, &net->ws, &net->ws_bytes, (size_t)per * pooled_floats * sizeof(float));
        if (rc) return rc;
        pooled = (float *)net->ws;
    }
    for (long long n0 = 0; n0 < N; n0 += per) {
        const int B = (int)std::min<long long>(per, N - n0);
        int rc = lp_run_layer(net, layer, d_in + (size_t)n0 * h * w * L.cin, nullptr, nullptr, 1, 1, B, h, w, pooled, d_out + (size_t)n0 * out_px * L.cout);
        if (rc) return rc;
    }
    return HIVE_OK;
}

int hive_lpips_forward(hive_lpips *net, const uint8_t *d_ref_u8, const uint8_t *d_est_u8, int N, int H, int W, int variants, double *d_scores,
                       double *d_layer_scores, float *const d_features[5], double *const d_dist[5]) {
    HIVE_ENTER(net ? net->ctx : nullptr);
    if (!net) return hive_fail(nullptr, HIVE_ERR_INVALID, "lpips is NULL");
    hive_ctx *ctx = net->ctx;
    HIVE_REQUIRE(ctx, d_ref_u8 && d_est_u8 && d_scores, "lpips_forward: NULL argument");
    HIVE_REQUIRE(ctx, N >= 1, "lpips_forward: N = %d, need at least one pair", N);
    HIVE_REQUIRE(ctx, H >= LP_MIN_SIDE && W >= LP_MIN_SIDE, "lpips_forward: %d x %d is smaller than 31 x 31, the smallest picture with an output in every layer", H, W);
    HIVE_REQUIRE(ctx, (long long)H * W * 3 < (1ll << 31), "lpips_forward: %d x %d pixels do not fit below 2^31", H, W);
    HIVE_REQUIRE(ctx, variants == 1 || variants == 2, "lpips_forward: variants = %d, need 1 (plain) or 2 (plain and masked)", variants);
    const int sets = variants + 1;
    // the sizes of the five maps and of the pooled inputs
    int fh[5], fw[5];
    long long feat_floats = 0, pooled_floats = 0;
    int max_blocks = 0;
    {
        int h = H, w = W;
        for (int l = 0; l < 5; ++l) {
            LpSizes z;
            HIVE_REQUIRE(ctx, lp_sizes(l, h, w, &z), "lpips_forward: layer %d has no output", l);
            if (LP_LAYERS[l].pool) pooled_floats = std::max(pooled_floats, (long long)z.hp * z.wp * LP_LAYERS[l].cin);
            fh[l] = h = z.ho, fw[l] = w = z.wo;
            feat_floats += (long long)h * w * LP_LAYERS[l].cout;
            max_blocks = std::max(max_blocks, (h * w + LP_THREADS - 1) / LP_THREADS);
        }
    }
    // pairs per chunk: the workspace below its cap, at most 65535 row tiles in the largest launch, variants * nc <= 65535
    const size_t per_pair = (size_t)sets * (feat_floats + pooled_floats) * sizeof(float) + (size_t)variants * max_blocks * sizeof(double);
    long long nc = std::max<long long>(1, (long long)(LP_WS_CAP / per_pair));
    nc = std::min(nc, 65535ll * LP_BM / ((long long)sets * fh[0] * fw[0]));
    nc = std::min<long long>(nc, 65535 / variants);
    HIVE_REQUIRE(ctx, nc >= 1, "lpips_forward: %d x %d is too large for one launch", H, W);
    nc = std::min<long long>(nc, N);
    float *feat[5], *pooled;
    double *partials, *layer_scores;
    auto regions = [&](hive_scratch_layout &lay) {
        for (int l = 0; l < 5; ++l) feat[l] = lay.take<float>((size_t)sets * nc * fh[l] * fw[l] * LP_LAYERS[l].cout);
        pooled = lay.take<float>((size_t)sets * nc * pooled_floats);
        partials = lay.take<double>((size_t)variants * nc * max_blocks);
        layer_scores = lay.take<double>((size_t)5 * variants * N);
    };
    hive_scratch_layout lay;
    regions(lay);
    int rc = hive_reserve_device(ctx, &net->ws, &net->ws_bytes, lay.bytes());
    if (rc) return rc;
    lay = hive_scratch_layout{(char *)net->ws, 0};
    regions(lay);
    if (d_layer_scores) layer_scores = d_layer_scores;
    for (long long n0 = 0; n0 < N; n0 += nc) {
        const int c = (int)std::min<long long>(nc, N - n0);  // (a short last chunk uses the front of every region)
        const uint8_t *ref = d_ref_u8 + (size_t)n0 * H * W * 3, *est = d_est_u8 + (size_t)n0 * H * W * 3;
        int h = H, w = W;
        for (int l = 0; l < 5; ++l) {
            rc = lp_run_layer(net, l, l ? feat[l - 1] : nullptr, ref, est, c, variants, sets * c, h, w, pooled, feat[l]);
            if (rc) return rc;
            h = fh[l], w = fw[l];
            const int hw = h * w, C = LP_LAYERS[l].cout, blocks = (hw + LP_THREADS - 1) / LP_THREADS;
            double *dist = d_dist && d_dist[l] ? d_dist[l] + (size_t)n0 * hw : nullptr;
            hipLaunchKernelGGL(lpips_tail_kernel, dim3((unsigned)blocks, (unsigned)(variants * c)), dim3(LP_THREADS), 0, ctx->stream, feat[l], c, variants, hw, C,
                               net->d_lin[l], partials, dist, (long long)N);
            HIVE_CHECK_HIP(ctx, hipGetLastError());
            double *scores_l = layer_scores + (size_t)l * variants * N;
            if (c == N) {
                rc = hive_similarity_finish(ctx, partials, (int64_t)variants * N, blocks, (double)hw, scores_l);
                if (rc) return rc;
            } else {
                for (int v = 0; v < variants; ++v) {
                    rc = hive_similarity_finish(ctx, partials + (size_t)v * c * blocks, c, blocks, (double)hw, scores_l + (size_t)v * N + n0);
                    if (rc) return rc;
                }
            }
            if (d_features && d_features[l]) {
                const size_t per_picture = (size_t)hw * C;
                for (int s = 0; s < sets; ++s)
                    HIVE_CHECK_HIP(ctx, hipMemcpyAsync(d_features[l] + ((size_t)s * N + n0) * per_picture, feat[l] + (size_t)s * c * per_picture,
                                                       (size_t)c * per_picture * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
    }
    const long long count = (long long)variants * N;
    hipLaunchKernelGGL(lpips_sum_kernel, dim3((unsigned)((count + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS), 0, ctx->stream, layer_scores, count, d_scores);
    HIVE_CHECK_HIP(ctx, hipGetLastError());
    return HIVE_OK;
}

}  // extern "C"
