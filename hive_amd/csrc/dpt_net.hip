// DPT-Hybrid as ONE C-ABI object: hive_dpt_create / hive_dpt_forward / hive_dpt_destroy.
//
// Replaces `dpt.models.DPTDepthModel.forward` of the reference's (absent) third_party/dpt + timm==0.5.4 as HIVE calls it
// (/root/reference/hive/dataset_adaptors.py:1366-1374, 1419) together with the pre- and post-processing around it
// (:1407-1417 `/ 255`, NormalizeImage(0.5, 0.5); :1432-1433 uint16 millimetres; hive/io.py:1032-1039 metres, > max_depth -> 0):
// uint8 frames in HBM -> depth maps in HBM, no PyTorch in between.  Pure orchestration: every layer is one of the library's own
// kernels (csrc/stem.hip, conv.hip, dpt_ops.hip, vit.hip, dpt_head.hip); this file adds the two token-shuffling kernels and the
// activation arena, sized by a plan walk that needs no device (hive_dpt_plan_arena).  The network's structure (module tree of isl-org/DPT `DPT` with the `vitb_rn50_384` backbone):
//   stem (7x7/2 conv, GroupNorm+ReLU, max pool) -> ResNetV2 stages 3 / 4 / 9 bottlenecks (hooks: stage 0 -> layer_1, stage 1 ->
//   layer_2) -> 1x1 patch projection + class token + position embedding -> 12 ViT blocks (hooks 8, 11) -> "project" readout ->
//   1x1 (and 3x3/2) reassemble convs -> layer{1..4}_rn -> RefineNet fusion 4..1 -> depth head -> 1 / (scale x + shift).
#include "hive_internal.hpp"

#include <algorithm>
#include <map>
#include <string>
#include <vector>

typedef unsigned short half_t;  // an element of either 16-bit type (HIVE_BF16 / HIVE_F16): the host side only sizes and offsets buffers

namespace {

// tokens[b][0] = cls + pos[0];  tokens[b][1 + i] = patch[b][i] + pos[1 + i]   (T = __bf16 or _Float16, D % 8 == 0; the adds in float, one rounding)
template <typename T>
__global__ __launch_bounds__(256) void assemble_tokens_kernel(const T *__restrict__ patch, const T *__restrict__ cls, const T *__restrict__ pos,
                                                              T *__restrict__ tokens, int B, int n_patch, int D) {
    const int dv = D / 8;
    const long long total = (long long)B * (n_patch + 1) * dv;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % dv) * 8;
        const long long row = i / dv;
        const int t = (int)(row % (n_patch + 1)), b = (int)(row / (n_patch + 1));
        const T *src = t == 0 ? cls + c : patch + ((size_t)b * n_patch + (t - 1)) * D + c;
        const uint4 ra = *reinterpret_cast<const uint4 *>(src), rp = *reinterpret_cast<const uint4 *>(pos + (size_t)t * D + c);
        const T *a = reinterpret_cast<const T *>(&ra), *p = reinterpret_cast<const T *>(&rp);
        T o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (T)((float)a[j] + (float)p[j]);
        *reinterpret_cast<uint4 *>(tokens + (size_t)row * D + c) = *reinterpret_cast<const uint4 *>(o);
    }
}

// "project" readout input: out[b][i] = concat(tokens[b][1 + i], tokens[b][0])  -> [B * n_patch][2 D]   (16-byte copies: either 16-bit type)
__global__ __launch_bounds__(256) void readout_concat_kernel(const half_t *__restrict__ tokens, half_t *__restrict__ out, int B, int n_patch, int D) {
    const int dv = D / 8;
    const long long total = (long long)B * n_patch * 2 * dv;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % (2 * dv));
        const long long row = i / (2 * dv);
        const int b = (int)(row / n_patch), t = (int)(row % n_patch);
        const half_t *src = c < dv ? tokens + ((size_t)b * (n_patch + 1) + 1 + t) * D + c * 8 : tokens + (size_t)b * (n_patch + 1) * D + (c - dv) * 8;
        *reinterpret_cast<uint4 *>(out + (size_t)row * 2 * D + c * 8) = *reinterpret_cast<const uint4 *>(src);
    }
}

void launch_assemble_tokens(hive_ctx *ctx, int dtype, int blocks, const void *patch, const void *cls, const void *pos, void *tokens, int B, int n_patch, int D) {
    if (dtype == HIVE_BF16)
        hipLaunchKernelGGL(assemble_tokens_kernel<__bf16>, dim3(blocks), dim3(256), 0, ctx->stream, (const __bf16 *)patch, (const __bf16 *)cls, (const __bf16 *)pos,
                           (__bf16 *)tokens, B, n_patch, D);
    else
        hipLaunchKernelGGL(assemble_tokens_kernel<_Float16>, dim3(blocks), dim3(256), 0, ctx->stream, (const _Float16 *)patch, (const _Float16 *)cls,
                           (const _Float16 *)pos, (_Float16 *)tokens, B, n_patch, D);
}

// Activation arena with LIVENESS: the walk releases a map behind its last consumer (everything runs in stream order, so a buffer may be handed out again as
// soon as the kernel that last reads it has been LAUNCHED); alloc takes the first free block that fits, else grows the high-water mark.  Offsets depend on
// the alloc / release sequence alone, so a PLAN walk (no memory: fake addresses, never dereferenced) sizes the arena and the LAUNCH walk over the reserved
// memory repeats its layout.  At 96 frames of 480 x 640 the network's maps total 38 GB; live at any one time: ~10 GB.
struct Arena {
    struct Block {
        size_t off, bytes;
    };
    char *mem = nullptr;                         // null: a plan walk
    size_t limit = 0;                            // launch walk: the bytes the plan reserved
    size_t used = 0;                             // high-water mark
    size_t overrun_end = 0;                      // launch walk: the end of a block beyond `limit` (0: none) -- Net::in_plan refuses to launch on it
    uint64_t layout_hash = 0xcbf29ce484222325ull;  // FNV-1a over the (offset, bytes) of every alloc in order, each as 8 little-endian bytes
    std::vector<Block> free_blocks;              // sorted by offset, coalesced
    std::map<const void *, Block> live;          // what alloc handed out and release has not taken back

    half_t *alloc(size_t elems) {
        const size_t bytes = (elems * sizeof(half_t) + 255) & ~(size_t)255;
        size_t off = used;
        bool found = false;
        for (size_t i = 0; i < free_blocks.size(); ++i)
            if (free_blocks[i].bytes >= bytes) {
                off = free_blocks[i].off;
                if (free_blocks[i].bytes == bytes)
                    free_blocks.erase(free_blocks.begin() + i);
                else
                    free_blocks[i] = Block{off + bytes, free_blocks[i].bytes - bytes};
                found = true;
                break;
            }
        if (!found) {
            if (!free_blocks.empty() && free_blocks.back().off + free_blocks.back().bytes == used) {  // grow the free tail
                off = free_blocks.back().off;
                free_blocks.pop_back();
            }
            used = off + bytes;
        }
        for (uint64_t v : {(uint64_t)off, (uint64_t)bytes})
            for (int i = 0; i < 8; ++i) layout_hash = (layout_hash ^ ((v >> (8 * i)) & 255u)) * 0x100000001b3ull;
        if (mem && off + bytes > limit) overrun_end = off + bytes;
        half_t *p = (half_t *)((mem ? mem : (char *)(uintptr_t)4096) + off);
        live[p] = Block{off, bytes};
        return p;
    }
    void release(const void *p) {
        if (!p) return;
        auto it = live.find(p);
        if (it == live.end()) return;  // not ours (a hook released twice, an external pointer): ignore
        Block b = it->second;
        live.erase(it);
        size_t i = 0;
        while (i < free_blocks.size() && free_blocks[i].off < b.off) ++i;
        free_blocks.insert(free_blocks.begin() + i, b);
        if (i + 1 < free_blocks.size() && free_blocks[i].off + free_blocks[i].bytes == free_blocks[i + 1].off) {
            free_blocks[i].bytes += free_blocks[i + 1].bytes;
            free_blocks.erase(free_blocks.begin() + i + 1);
        }
        if (i > 0 && free_blocks[i - 1].off + free_blocks[i - 1].bytes == free_blocks[i].off) {
            free_blocks[i - 1].bytes += free_blocks[i].bytes;
            free_blocks.erase(free_blocks.begin() + i);
        }
    }
};

}  // namespace

struct hive_dpt {
    hive_ctx *ctx = nullptr;
    hive_dpt_config cfg{};
    std::map<std::string, const void *> w;
    hive_vit *vit = nullptr;
    std::map<std::string, float *> gram_tables;  // per 1 x 1 convolution weight: the tables of hive_gn_gram_prepare (made on first use)
    void *arena = nullptr;                       // the launch walks' memory, grown to the largest plan seen
    size_t arena_bytes = 0;

    const void *get(const std::string &name) const {
        auto it = w.find(name);
        return it == w.end() ? nullptr : it->second;
    }
};

namespace {

struct Map {  // a channels-last activation [N][H][W][C]
    half_t *p;
    int H, W, C;
    float *gn = nullptr;  // GroupNorm statistics of the tensor, per tile of gn_tm rows, left by the convolution that wrote it
    int gn_tm = 0;        // (hive_nhwc_conv_gn); 0: none, the GroupNorm makes its own pass
};

#define DPT_TRY(expr)              \
    do {                           \
        int _rc = (expr);          \
        if (_rc) return _rc;       \
    } while (0)

// One convolution of Net::conv by its named properties; the layer's tensors are prefix + ".weight" and, with `bias`, prefix + ".bias"
struct ConvSpec {
    int cout;
    int k = 1, stride = 1;
    bool same_pad = false;  // timm StdConv2dSame (TensorFlow "SAME", the odd pixel at the bottom / right); else nn.Conv2d(padding = k / 2)
    bool bias = false;
    int relu = 0;
    const half_t *res1 = nullptr, *res2 = nullptr;  // added in the epilogue (before the ReLU)
    Map *relu_copy = nullptr;                       // a second output: relu(out)
    bool gn_stats = false;                          // a ResNetV2 convolution: the GroupNorm behind it gets its statistics from this epilogue (out->gn)
};

// what one call of hive_dpt_forward_frames was given.  Frames are FH x FW; the network runs at H x W (both multiples of 32).  Where the two differ the frames
// enter through the reference's bicubic resize (csrc/resize.hip) and the depth map leaves through its nearest-neighbour resize back to the frame size,
// hand-off included.  (A plan walk reads the four sizes only.)
struct Frames {
    const uint8_t *d_rgb;
    int FH, FW, H, W;
    const void *d_pos;
    float *d_depth;
    float max_depth;
    uint16_t *d_mm;
    float *d_m;
    bool resized() const { return FH != H || FW != W; }
};

int same_out(int i, int s) { return (i + s - 1) / s; }

// One walk over the network.  dry = true is the PLAN walk: the allocation sequence alone (d and the frames' pointers are null and never looked at, ctx
// may be null: it only receives error messages); otherwise the LAUNCH walk over the arena the plan sized.  Every operation allocates first -- from shapes
// alone, never from what a kernel reported, so that both walks make the same sequence -- and has one point where the plan walk leaves it; the launch walk
// passes in_plan() there before it launches anything.
struct Net {
    hive_dpt *d;
    hive_ctx *ctx;
    Arena &a;
    const bool dry;
    const int B, dt;
    const Frames &io;

    int need(const std::string &n, const void **out) const {
        *out = d->get(n);
        if (!*out) return hive_fail(ctx, HIVE_ERR_INVALID, "hive_dpt: tensor '%s' missing from the table", n.c_str());
        return HIVE_OK;
    }
    // no kernel is launched with a pointer whose block ends beyond what the plan reserved
    int in_plan() const {
        if (!a.overrun_end) return HIVE_OK;
        return hive_fail(ctx, HIVE_ERR_STATE, "hive_dpt: the allocation sequence diverged from its plan (a block ends at byte %zu of %zu reserved)", a.overrun_end,
                         a.limit);
    }
    size_t px(const Map &m) const { return (size_t)B * m.H * m.W; }
    void drop(Map &m) {  // the map (and the GroupNorm partial sums riding on it) has no consumer left to launch
        a.release(m.p);
        a.release(m.gn);
        m.p = nullptr;
        m.gn = nullptr;
    }
    int preprocess(half_t *xin) {
        if (io.resized()) return hive_dpt_resize_preprocess(ctx, io.d_rgb, B, io.FH, io.FW, io.H, io.W, 0.5f, 0.5f, dt, xin);
        return hive_dpt_preprocess(ctx, io.d_rgb, (int64_t)B * io.H * io.W * 3, 0.5f, 0.5f, dt, xin);
    }

    int conv(const Map &x, const std::string &prefix, const ConvSpec &s, Map *out) {
        const int k = s.k, stride = s.stride, cout = s.cout;
        int pt, pl, oh, ow;
        if (s.same_pad) {
            oh = same_out(x.H, stride);
            ow = same_out(x.W, stride);
            pt = std::max((oh - 1) * stride + k - x.H, 0) / 2;
            pl = std::max((ow - 1) * stride + k - x.W, 0) / 2;
        } else {
            pt = pl = k / 2;
            oh = (x.H + 2 * pt - k) / stride + 1;
            ow = (x.W + 2 * pl - k) / stride + 1;
        }
        *out = Map{a.alloc((size_t)B * oh * ow * cout), oh, ow, cout};
        if (s.relu_copy) *s.relu_copy = Map{a.alloc((size_t)B * oh * ow * cout), oh, ow, cout};
        const int64_t gn_floats = s.gn_stats ? hive_nhwc_conv_gn_partial_floats((int64_t)B * oh * ow, cout) : 0;
        if (s.gn_stats) out->gn = (float *)a.alloc((size_t)gn_floats * 2);
        if (dry) return HIVE_OK;
        DPT_TRY(in_plan());
        const void *wp, *bp = nullptr;
        DPT_TRY(need(prefix + ".weight", &wp));
        if (s.bias) DPT_TRY(need(prefix + ".bias", &bp));
        half_t *relu_out = s.relu_copy ? s.relu_copy->p : nullptr;
        if (s.gn_stats)
            return hive_nhwc_conv_gn(ctx, x.p, dt, B, x.H, x.W, x.C, cout, k, stride, pt, pl, oh, ow, wp, bp, s.relu, s.res1, s.res2, out->p, relu_out, out->gn, gn_floats,
                                     &out->gn_tm);
        return hive_nhwc_conv(ctx, x.p, dt, B, x.H, x.W, x.C, cout, k, stride, pt, pl, oh, ow, wp, bp, s.relu, s.res1, s.res2, out->p, relu_out);
    }

    // conv + GroupNorm (+ shortcut + ReLU) of a bottleneck's expanding 1 x 1 convolutions as the two-pass operation (its statistics from the input's Gram
    // matrices where hive_gn_gram_preferred says so); small maps take the pair conv, GroupNorm
    int conv_norm(const Map &x, const std::string &conv_prefix, const std::string &norm_prefix, int cout, int stride, const half_t *residual, int relu, Map *out) {
        const int oh = same_out(x.H, stride), ow = same_out(x.W, stride);
        const int64_t scratch_floats = hive_nhwc_conv_gn_partial_floats((int64_t)B * oh * ow, cout) + 2ll * B * 32;
        float *scratch = (float *)a.alloc((size_t)scratch_floats * 2);
        *out = Map{a.alloc((size_t)B * oh * ow * cout), oh, ow, cout};
        const bool eligible = hive_conv_gn_two_pass_eligible(cout, 32, (long long)oh * ow);
        Map t{eligible ? nullptr : a.alloc((size_t)B * oh * ow * cout), oh, ow, cout};  // the pair's intermediate: small maps only
        auto done = [&](int rc) {  // scratch and the pair's intermediate are dead once the launches are queued
            a.release(scratch);
            a.release(t.p);
            return rc;
        };
        if (dry) return done(HIVE_OK);
        DPT_TRY(in_plan());
        const std::string wname = conv_prefix + ".weight";
        const void *wp, *g, *b;
        DPT_TRY(need(wname, &wp));
        DPT_TRY(need(norm_prefix + ".weight", &g));
        DPT_TRY(need(norm_prefix + ".bias", &b));
        int fused = 0;
        if (hive_gn_gram_preferred(x.C, cout, stride, 32, B, oh, ow, ctx->deterministic)) {
            float *&tables = d->gram_tables[wname];
            if (!tables) {
                HIVE_CHECK_HIP(ctx, hipMalloc((void **)&tables, (size_t)hive_gn_gram_table_floats(x.C, 32) * sizeof(float)));
                DPT_TRY(hive_gn_gram_prepare(ctx, wp, dt, x.C, cout, 32, tables));
            }
            DPT_TRY(hive_nhwc_conv_gn_apply_gram(ctx, x.p, dt, B, x.H, x.W, x.C, cout, stride, oh, ow, wp, tables, 32, g, b, d->cfg.gn_eps, residual, relu, out->p, scratch,
                                                 scratch_floats, &fused));
            if (fused) return done(HIVE_OK);
        }
        DPT_TRY(hive_nhwc_conv_gn_apply(ctx, x.p, dt, B, x.H, x.W, x.C, cout, 1, stride, 0, 0, oh, ow, wp, 32, g, b, d->cfg.gn_eps, residual, relu, out->p, scratch,
                                        scratch_floats, &fused));
        if (fused) return done(HIVE_OK);
        if (eligible) return hive_fail(ctx, HIVE_ERR_INVALID, "hive_dpt: conv + GroupNorm of '%s' was not fused", wname.c_str());
        DPT_TRY(hive_nhwc_conv_gn(ctx, x.p, dt, B, x.H, x.W, x.C, cout, 1, stride, 0, 0, oh, ow, wp, nullptr, 0, nullptr, nullptr, t.p, nullptr, scratch, scratch_floats,
                                  &t.gn_tm));
        return done(hive_nhwc_group_norm_stats(ctx, t.p, dt, B, oh * ow, cout, 32, g, b, d->cfg.gn_eps, residual, relu, out->p, scratch, t.gn_tm));
    }

    int group_norm(const Map &x, const std::string &prefix, const half_t *residual, int relu, Map *out) {
        *out = Map{a.alloc(px(x) * x.C), x.H, x.W, x.C};
        if (dry) return HIVE_OK;
        DPT_TRY(in_plan());
        const void *g, *b;
        DPT_TRY(need(prefix + ".weight", &g));
        DPT_TRY(need(prefix + ".bias", &b));
        return hive_nhwc_group_norm_stats(ctx, x.p, dt, B, x.H * x.W, x.C, 32, g, b, d->cfg.gn_eps, residual, relu, out->p, x.gn, x.gn_tm);
    }

    // ConvTranspose2d(C, C, s, s) = 1 x 1 convolution to s s C channels ((dy, dx, co) rows of the re-laid-out weight) + scatter + bias
    int conv_transpose(const Map &x, const std::string &prefix, int s, Map *out) {
        Map tmp{a.alloc(px(x) * s * s * x.C), x.H, x.W, s * s * x.C};
        *out = Map{a.alloc(px(x) * s * s * x.C), s * x.H, s * x.W, x.C};
        if (dry) {
            drop(tmp);
            return HIVE_OK;
        }
        DPT_TRY(in_plan());
        const void *wr, *bias;
        DPT_TRY(need(prefix + ".weight.rows", &wr));
        DPT_TRY(need(prefix + ".bias", &bias));
        DPT_TRY(hive_nhwc_conv(ctx, x.p, dt, B, x.H, x.W, x.C, s * s * x.C, 1, 1, 0, 0, x.H, x.W, wr, nullptr, 0, nullptr, nullptr, tmp.p, nullptr));
        const int rc = hive_nhwc_pixel_shuffle_bias(ctx, tmp.p, bias, dt, B, x.H, x.W, x.C, s, out->p);
        drop(tmp);
        return rc;
    }

    // ---- pre-processing + ResNetV2 stem: 7 x 7 / 2 convolution, GroupNorm + ReLU + MaxPool2dSame(3, 2) -----------------------------------------------
    int stem(Map *feat) {
        const std::string pre = "pretrained.model.patch_embed.backbone.stem.";
        const int H = io.H, W = io.W;
        half_t *xin = a.alloc((size_t)B * H * W * 3);
        Map s0{a.alloc((size_t)B * same_out(H, 2) * same_out(W, 2) * 64), same_out(H, 2), same_out(W, 2), 64};
        const int64_t stem_floats = hive_nhwc_conv_gn_partial_floats((int64_t)B * s0.H * s0.W, 64);
        s0.gn = (float *)a.alloc((size_t)stem_floats * 2);  // the GroupNorm's sums, left by the convolution's epilogue
        if (!dry) {
            DPT_TRY(in_plan());
            DPT_TRY(preprocess(xin));
            const void *sw;
            DPT_TRY(need(pre + "conv.weight", &sw));
            DPT_TRY(hive_resnet_stem_conv_gn(ctx, xin, dt, B, H, W, sw, s0.p, s0.gn, stem_floats, &s0.gn_tm));
        }
        a.release(xin);
        // GroupNorm + ReLU + max pool in one pass: the normalised 64-channel map at half resolution never reaches memory
        *feat = Map{a.alloc((size_t)B * same_out(s0.H, 2) * same_out(s0.W, 2) * 64), same_out(s0.H, 2), same_out(s0.W, 2), 64};
        if (!dry) {
            DPT_TRY(in_plan());
            const void *g, *b;
            DPT_TRY(need(pre + "norm.weight", &g));
            DPT_TRY(need(pre + "norm.bias", &b));
            DPT_TRY(hive_nhwc_group_norm_relu_maxpool(ctx, s0.p, dt, B, s0.H, s0.W, 64, 32, g, b, d->cfg.gn_eps, feat->p, s0.gn_tm ? s0.gn : nullptr, s0.gn_tm));
        }
        drop(s0);
        return HIVE_OK;
    }

    // ---- one ResNetV2 bottleneck (non pre-activation, GroupNorm behind every convolution): *feat is its input, then its output.  first: the stage's
    // first block, with a downsample shortcut; keep_input: the input is a hooked stage output (layer_1, layer_2) and stays
    int bottleneck(const std::string &pre, int cout, int stride, bool first, bool keep_input, Map *feat) {
        const int mid = cout / 4;
        Map in = *feat, shortcut = *feat, t, u, t2, u2;
        if (first) DPT_TRY(conv_norm(in, pre + "downsample.conv", pre + "downsample.norm", cout, stride, nullptr, 0, &shortcut));
        DPT_TRY(conv(in, pre + "conv1", {.cout = mid, .same_pad = true, .gn_stats = true}, &t));
        // norm1 + ReLU applied while conv2 stages its input (csrc/bneck.hip): one kernel, no normalised map.  Needs conv1's sums, which its epilogue leaves
        // for maps of at least one 256-pixel tile: the launch always fuses for these maps (anything else is an error), smaller ones take the pair below
        if (mid == 64 && stride == 1 && (long long)t.H * t.W >= 256) {
            t2 = Map{a.alloc(px(t) * 64), t.H, t.W, 64};
            const int64_t floats = hive_nhwc_conv_gn_partial_floats((int64_t)px(t), 64);
            t2.gn = (float *)a.alloc((size_t)floats * 2);
            if (!dry) {
                DPT_TRY(in_plan());
                const void *g, *b, *w2;
                int fused = 0;
                DPT_TRY(need(pre + "norm1.weight", &g));
                DPT_TRY(need(pre + "norm1.bias", &b));
                DPT_TRY(need(pre + "conv2.weight", &w2));
                DPT_TRY(hive_bneck_gn_conv3x3(ctx, t.p, dt, B, t.H, t.W, 64, t.gn, t.gn_tm, g, b, d->cfg.gn_eps, w2, t2.p, t2.gn, floats, &t2.gn_tm, &fused));
                if (!fused) return hive_fail(ctx, HIVE_ERR_INVALID, "hive_dpt: the 64-channel bottleneck convolution of '%s' was not fused", pre.c_str());
            }
            drop(t);
        } else {
            DPT_TRY(group_norm(t, pre + "norm1", nullptr, 1, &u));
            drop(t);
            DPT_TRY(conv(u, pre + "conv2", {.cout = mid, .k = 3, .stride = stride, .same_pad = true, .gn_stats = true}, &t2));
            drop(u);
        }
        DPT_TRY(group_norm(t2, pre + "norm2", nullptr, 1, &u2));
        drop(t2);
        DPT_TRY(conv_norm(u2, pre + "conv3", pre + "norm3", cout, 1, shortcut.p, 1, feat));  // relu(norm3(conv3(.)) + shortcut)
        drop(u2);
        if (first) drop(shortcut);  // (otherwise the shortcut IS the block's input)
        if (!keep_input) drop(in);
        return HIVE_OK;
    }

    // ---- class token + position embedding, the ViT blocks with their hooks, "project" readout of each hooked block into a map: LAUNCHES ONLY.  The two
    // backbones allocate tokens / tap[] / cat / maps[] themselves, in different orders, and that order is the arena layout.  patch [B][n_patch][D];
    // taps[n_taps]: the hooked blocks, read out by pretrained.act_postprocess{first_stage ..}
    int tokens_vit_readout(const half_t *patch, int n_patch, int D, const int *taps, int n_taps, int first_stage, half_t *tokens, half_t *const *tap, half_t *cat,
                           const Map *maps) {
        const int N = n_patch + 1;
        const void *cls;
        DPT_TRY(need("pretrained.model.cls_token", &cls));
        const int blocks = (int)std::min<long long>(((long long)B * N * D / 8 + 255) / 256, (long long)ctx->num_cus * 16);
        launch_assemble_tokens(ctx, dt, blocks, patch, cls, io.d_pos, tokens, B, n_patch, D);
        HIVE_CHECK_HIP(ctx, hipGetLastError());
        void *tap_out[4];
        for (int r = 0; r < n_taps; ++r) tap_out[r] = tap[r];
        DPT_TRY(hive_vit_forward(d->vit, tokens, B, N, taps, n_taps, tap_out));
        for (int r = 0; r < n_taps; ++r) {
            hipLaunchKernelGGL(readout_concat_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const half_t *)tap[r], cat, B, n_patch, D);
            HIVE_CHECK_HIP(ctx, hipGetLastError());
            const std::string pre = "pretrained.act_postprocess" + std::to_string(first_stage + r) + ".0.project.0.";
            const void *rw, *rb;
            DPT_TRY(need(pre + "weight", &rw));
            DPT_TRY(need(pre + "bias", &rb));  // float32
            DPT_TRY(hive_vit_linear(ctx, cat, dt, rw, (const float *)rb, nullptr, maps[r].p, B * n_patch, D, 2 * D, 1 /* GELU */));
        }
        return HIVE_OK;
    }

    // ---- DPT-Hybrid: ResNetV2 stages 3 / 4 / 9 (stage 0 -> layer_1, stage 1 -> layer_2), then the ViT on the last stage's patches ---------------------
    int hybrid_backbone(Map layer[4]) {
        Map feat;
        DPT_TRY(stem(&feat));
        const int depths[3] = {3, 4, 9}, chans[3] = {256, 512, 1024};
        for (int s = 0; s < 3; ++s) {
            for (int blk = 0; blk < depths[s]; ++blk) {
                const std::string pre = "pretrained.model.patch_embed.backbone.stages." + std::to_string(s) + ".blocks." + std::to_string(blk) + ".";
                // (a later stage's first block reads the hooked output of the stage before it)
                DPT_TRY(bottleneck(pre, chans[s], (blk == 0 && s > 0) ? 2 : 1, blk == 0, blk == 0 && s > 0, &feat));
            }
            if (s < 2) layer[s] = feat;
        }
        return hybrid_reassemble(feat, &layer[2], &layer[3]);
    }

    // 1 x 1 patch projection, tokens, 12 ViT blocks (hooks 8, 11), readout, 1 x 1 (and 3 x 3 / 2) reassemble convolutions
    int hybrid_reassemble(Map feat, Map *layer_3, Map *layer_4) {
        const int gh = feat.H, gw = feat.W, n_patch = gh * gw, N = n_patch + 1, D = 768;
        const std::string pp = "pretrained.act_postprocess";
        Map pe;
        DPT_TRY(conv(feat, "pretrained.model.patch_embed.proj", {.cout = D, .bias = true}, &pe));
        half_t *tokens = a.alloc((size_t)B * N * D), *tap[2] = {a.alloc((size_t)B * N * D), a.alloc((size_t)B * N * D)};
        half_t *cat = a.alloc((size_t)B * n_patch * 2 * D);
        Map maps[2] = {Map{a.alloc((size_t)B * n_patch * D), gh, gw, D}, Map{a.alloc((size_t)B * n_patch * D), gh, gw, D}};
        if (!dry) {
            DPT_TRY(in_plan());
            const int taps[2] = {8, 11};
            DPT_TRY(tokens_vit_readout(pe.p, n_patch, D, taps, 2, 3, tokens, tap, cat, maps));
        }
        drop(feat);  // the last stage's output fed the patch projection only
        drop(pe);
        a.release(tokens);
        a.release(tap[0]);
        a.release(tap[1]);
        a.release(cat);
        Map t4;
        DPT_TRY(conv(maps[0], pp + "3.3", {.cout = D, .bias = true}, layer_3));
        drop(maps[0]);
        DPT_TRY(conv(maps[1], pp + "4.3", {.cout = D, .bias = true}, &t4));
        drop(maps[1]);
        DPT_TRY(conv(t4, pp + "4.4", {.cout = D, .k = 3, .stride = 2, .bias = true}, layer_4));
        drop(t4);
        return HIVE_OK;
    }

    // ---- DPT-Large (timm vit_large_patch16_384 as isl-org/DPT hooks it: blocks 5 / 11 / 17 / 23) ------------------------------------------------------
    // pre-processing -> 16 x 16 / 16 patch embedding (rows + GEMM) -> class token + position embedding -> 24 ViT blocks -> "project"
    // readouts -> reassemble: 1x1 (+ ConvTranspose 4x4/4 | ConvTranspose 2x2/2 | nothing | 3x3/2) to 256 / 512 / 1024 / 1024 channels
    int large_backbone(Map layer[4]) {
        const int H = io.H, W = io.W, D = 1024, gh = H / 16, gw = W / 16, n_patch = gh * gw, N = n_patch + 1;
        half_t *xin = a.alloc((size_t)B * H * W * 3), *cols = a.alloc((size_t)B * n_patch * 768), *pe = a.alloc((size_t)B * n_patch * D);
        half_t *tokens = a.alloc((size_t)B * N * D), *cat = a.alloc((size_t)B * n_patch * 2 * D);
        half_t *tap[4];
        Map maps[4];
        for (int r = 0; r < 4; ++r) {
            tap[r] = a.alloc((size_t)B * N * D);
            maps[r] = Map{a.alloc((size_t)B * n_patch * D), gh, gw, D};
        }
        if (!dry) {
            DPT_TRY(in_plan());
            DPT_TRY(preprocess(xin));
            DPT_TRY(hive_patch_rows(ctx, xin, dt, B, H, W, 3, 16, cols));
            const void *pw, *pb;
            DPT_TRY(need("pretrained.model.patch_embed.proj.weight", &pw));  // [D][16][16][3] = [D][768]
            DPT_TRY(need("pretrained.model.patch_embed.proj.bias.f32", &pb));
            DPT_TRY(hive_vit_linear(ctx, cols, dt, pw, (const float *)pb, nullptr, pe, B * n_patch, D, 768, 0));
            const int taps[4] = {5, 11, 17, 23};
            DPT_TRY(tokens_vit_readout(pe, n_patch, D, taps, 4, 1, tokens, tap, cat, maps));
        }
        a.release(xin);
        a.release(cols);
        a.release(pe);
        a.release(tokens);
        a.release(cat);
        for (int r = 0; r < 4; ++r) a.release(tap[r]);
        const std::string pp = "pretrained.act_postprocess";
        Map t;
        DPT_TRY(conv(maps[0], pp + "1.3", {.cout = 256, .bias = true}, &t));
        drop(maps[0]);
        DPT_TRY(conv_transpose(t, pp + "1.4", 4, &layer[0]));
        drop(t);
        DPT_TRY(conv(maps[1], pp + "2.3", {.cout = 512, .bias = true}, &t));
        drop(maps[1]);
        DPT_TRY(conv_transpose(t, pp + "2.4", 2, &layer[1]));
        drop(t);
        DPT_TRY(conv(maps[2], pp + "3.3", {.cout = 1024, .bias = true}, &layer[2]));
        drop(maps[2]);
        DPT_TRY(conv(maps[3], pp + "4.3", {.cout = 1024, .bias = true}, &t));
        drop(maps[3]);
        DPT_TRY(conv(t, pp + "4.4", {.cout = 1024, .k = 3, .stride = 2, .bias = true}, &layer[3]));
        drop(t);
        return HIVE_OK;
    }

    // RefineNet fusion block n over layer_rn (lrn, and its ReLU) and the coarser block's output (path; none for block 4) -> *out at twice the resolution
    int refinenet(int n, const Map *path, const Map &lrn, const Map &lrn_relu, Map *out) {
        const std::string pre = "scratch.refinenet" + std::to_string(n) + ".";
        Map o = lrn, o_relu = lrn_relu, t;
        if (path) {  // output = path + resConfUnit1(layer_rn): conv2(relu(conv1(relu(x)))) + x + path, and its ReLU for the next unit
            DPT_TRY(conv(lrn_relu, pre + "resConfUnit1.conv1", {.cout = 256, .k = 3, .bias = true, .relu = 1}, &t));
            DPT_TRY(conv(t, pre + "resConfUnit1.conv2", {.cout = 256, .k = 3, .bias = true, .res1 = lrn.p, .res2 = path->p, .relu_copy = &o_relu}, &o));
            drop(t);
        }
        Map u, low, t2;
        DPT_TRY(conv(o_relu, pre + "resConfUnit2.conv1", {.cout = 256, .k = 3, .bias = true, .relu = 1}, &t2));
        DPT_TRY(conv(t2, pre + "resConfUnit2.conv2", {.cout = 256, .k = 3, .bias = true, .res1 = o.p}, &u));
        drop(t2);
        if (o.p != lrn.p) drop(o);  // (with a path, o / o_relu are resConfUnit1's outputs; without, they ARE lrn / lrn_relu, dropped by the caller)
        if (o_relu.p != lrn_relu.p) drop(o_relu);
        // the 1x1 out_conv commutes with the bilinear interpolation: it runs on a quarter of the pixels, its bias is added on load
        DPT_TRY(conv(u, pre + "out_conv", {.cout = 256}, &low));
        drop(u);
        *out = Map{a.alloc(px(low) * 4 * 256), 2 * low.H, 2 * low.W, 256};
        int rc = HIVE_OK;
        if (!dry) {
            DPT_TRY(in_plan());
            const void *ob;
            DPT_TRY(need(pre + "out_conv.bias", &ob));
            rc = hive_nhwc_upsample2x(ctx, low.p, ob, dt, B, low.H, low.W, 256, out->p);
        }
        drop(low);
        return rc;
    }

    // ---- decoder: layerN_rn, four RefineNet fusion blocks, coarse to fine ------------------------------------------------------------------------------
    int decoder(const Map layer[4], Map *path) {
        Map prev{};
        for (int n = 4; n >= 1; --n) {
            Map lrn, lrn_relu;
            DPT_TRY(conv(layer[n - 1], "scratch.layer" + std::to_string(n) + "_rn", {.cout = 256, .k = 3, .relu_copy = &lrn_relu}, &lrn));
            a.release(layer[n - 1].p);  // layer_n fed its layer_rn convolution only
            DPT_TRY(refinenet(n, n == 4 ? nullptr : &prev, lrn, lrn_relu, path));
            drop(lrn);
            drop(lrn_relu);
            if (n != 4) drop(prev);
            prev = *path;
        }
        return HIVE_OK;
    }

    // ---- depth head: conv 256 -> 128 (+ bias, in its epilogue), x2 upsample + conv 128 -> 32 + ReLU + 1x1 + ReLU + inversion ---------------------------
    int head(Map path) {
        const int H = io.H, W = io.W;
        const hive_dpt_config *c = d ? &d->cfg : nullptr;
        Map lo;
        DPT_TRY(conv(path, "scratch.output_conv.0", {.cout = 128, .k = 3, .bias = true}, &lo));
        drop(path);
        float *net_depth = io.resized() ? (float *)a.alloc((size_t)B * H * W * 2) : nullptr;  // f32 depth at the network's size (2 half_t per float)
        if (dry) return HIVE_OK;
        DPT_TRY(in_plan());
        const void *w3;
        DPT_TRY(need("scratch.output_conv.2.weight", &w3));  // [ky][kx][32][128]
        HIVE_REQUIRE(ctx, 2 * lo.H == H && 2 * lo.W == W, "hive_dpt: network size %d x %d must be a multiple of 32", H, W);
        if (!io.resized())
            return hive_dpt_head_fused(ctx, lo.p, nullptr, dt, B, lo.H, lo.W, 128, 32, w3, c->head_b3, c->head_w1, c->head_b1, c->non_negative, c->invert, c->scale, c->shift,
                                       io.d_depth, 1.0f / 1000.0f, io.max_depth, io.d_mm, io.d_m);
        // frames of another size: the head leaves float32 depth at the network's size, the nearest-neighbour resize back to the frame size
        // (dataset_adaptors.py:1421-1426) carries the uint16-mm hand-off
        DPT_TRY(hive_dpt_head_fused(ctx, lo.p, nullptr, dt, B, lo.H, lo.W, 128, 32, w3, c->head_b3, c->head_w1, c->head_b1, c->non_negative, c->invert, c->scale, c->shift,
                                    net_depth, 1.0f / 1000.0f, io.max_depth, nullptr, nullptr));
        return hive_depth_resize_nearest(ctx, net_depth, B, H, W, io.FH, io.FW, 1.0f / 1000.0f, io.max_depth, io.d_depth, io.d_mm, io.d_m);
    }

    int forward(int backbone) {
        Map layer[4], path{};
        DPT_TRY(backbone == 0 ? hybrid_backbone(layer) : large_backbone(layer));
        DPT_TRY(decoder(layer, &path));
        return head(path);
    }
};

// the argument checks shared by the plan and the forward
int check_shapes(hive_ctx *ctx, int B, int frame_h, int frame_w, int H, int W) {
    HIVE_REQUIRE(ctx, B > 0 && frame_h > 0 && frame_w > 0, "hive_dpt_forward: bad frame batch %d x %d x %d", B, frame_h, frame_w);
    HIVE_REQUIRE(ctx, H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0, "hive_dpt_forward: the network's input size must be a multiple of 32 (%d x %d)", H, W);
    return HIVE_OK;
}

// THE plan walk: the arena a forward of these shapes needs, and its layout
int plan_arena(hive_ctx *ctx, int backbone, int B, int frame_h, int frame_w, int H, int W, size_t *bytes, uint64_t *layout_hash) {
    DPT_TRY(check_shapes(ctx, B, frame_h, frame_w, H, W));
    const Frames io{nullptr, frame_h, frame_w, H, W, nullptr, nullptr, 0.0f, nullptr, nullptr};
    Arena plan;
    DPT_TRY((Net{nullptr, ctx, plan, true, B, 0, io}.forward(backbone)));
    *bytes = plan.used;
    if (layout_hash) *layout_hash = plan.layout_hash;
    return HIVE_OK;
}

}  // namespace

extern "C" {

int hive_dpt_create(hive_ctx *ctx, const hive_dpt_config *config, const hive_dpt_tensor *tensors, int n_tensors, hive_dpt **out) {
    HIVE_ENTER(ctx);
    if (!ctx) return hive_fail(nullptr, HIVE_ERR_INVALID, "ctx is NULL");
    HIVE_REQUIRE(ctx, config && tensors && n_tensors > 0 && out, "hive_dpt_create: NULL argument");
    HIVE_REQUIRE(ctx, config->backbone == 0 || config->backbone == 1, "hive_dpt_create: backbone %d (0 = vitb_rn50_384, 1 = vitl16_384)", config->backbone);
    HIVE_REQUIRE(ctx, config->dtype == HIVE_BF16 || config->dtype == HIVE_F16, "hive_dpt_create: dtype %d (HIVE_F16 = %d or HIVE_BF16 = %d)", config->dtype, (int)HIVE_F16,
                 (int)HIVE_BF16);
    const int vit_depth = config->backbone == 0 ? 12 : 24, vit_dim = config->backbone == 0 ? 768 : 1024, vit_heads = vit_dim / 64;
    *out = nullptr;
    hive_dpt *d = new hive_dpt();
    d->ctx = ctx;
    d->cfg = *config;
    for (int i = 0; i < n_tensors; ++i)
        if (tensors[i].name && tensors[i].data) d->w[tensors[i].name] = tensors[i].data;
    // the ViT engine over the table's block weights
    std::vector<hive_vit_block_weights> blocks(vit_depth);
    const char *fields[12] = {"norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                              "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"};
    for (int i = 0; i < vit_depth; ++i) {
        const void **dst = reinterpret_cast<const void **>(&blocks[i]);
        for (int f = 0; f < 12; ++f) {
            const std::string name = "pretrained.model.blocks." + std::to_string(i) + "." + fields[f];
            dst[f] = d->get(name);
            if (!dst[f]) {
                int rc = hive_fail(ctx, HIVE_ERR_INVALID, "hive_dpt_create: tensor '%s' missing from the table", name.c_str());
                delete d;
                return rc;
            }
        }
    }
    int rc = hive_vit_create(ctx, config->dtype, vit_depth, vit_dim, vit_heads, 4 * vit_dim, config->ln_eps, blocks.data(), &d->vit);
    if (rc) {
        hive_dpt_destroy(d);
        return rc;
    }
    *out = d;
    return HIVE_OK;
}

int hive_dpt_plan_arena(int backbone, int B, int frame_h, int frame_w, int net_h, int net_w, int64_t *bytes, uint64_t *layout_hash) {
    if (!bytes) return hive_fail(nullptr, HIVE_ERR_INVALID, "hive_dpt_plan_arena: NULL argument");
    if (backbone != 0 && backbone != 1) return hive_fail(nullptr, HIVE_ERR_INVALID, "hive_dpt_plan_arena: backbone %d (0 = vitb_rn50_384, 1 = vitl16_384)", backbone);
    size_t planned = 0;
    DPT_TRY(plan_arena(nullptr, backbone, B, frame_h, frame_w, net_h, net_w, &planned, layout_hash));
    *bytes = (int64_t)planned;
    return HIVE_OK;
}

int hive_dpt_forward_frames(hive_dpt *d, const uint8_t *d_rgb, int B, int frame_h, int frame_w, int net_h, int net_w, const void *d_pos_embed, float *d_depth,
                            float max_depth, uint16_t *d_out_mm, float *d_out_m) {
    HIVE_ENTER(d ? d->ctx : nullptr);
    if (!d) return hive_fail(nullptr, HIVE_ERR_INVALID, "dpt is NULL");
    hive_ctx *ctx = d->ctx;
    HIVE_REQUIRE(ctx, d_rgb && d_pos_embed && (d_depth || d_out_mm || d_out_m), "hive_dpt_forward: NULL argument");
    // plan the activation arena, reserve it, then launch over it: the launch walk repeats the plan's allocation sequence and is held to it
    size_t planned = 0;
    DPT_TRY(plan_arena(ctx, d->cfg.backbone, B, frame_h, frame_w, net_h, net_w, &planned, nullptr));
    DPT_TRY(hive_reserve_device(ctx, &d->arena, &d->arena_bytes, planned));
    const Frames io{d_rgb, frame_h, frame_w, net_h, net_w, d_pos_embed, d_depth, max_depth, d_out_mm, d_out_m};
    Arena arena;
    arena.mem = (char *)d->arena;
    arena.limit = planned;
    DPT_TRY((Net{d, ctx, arena, false, B, d->cfg.dtype, io}.forward(d->cfg.backbone)));
    if (arena.used != planned)
        return hive_fail(ctx, HIVE_ERR_STATE, "hive_dpt: the allocation sequence diverged from its plan (%zu bytes used, %zu planned)", arena.used, planned);
    return HIVE_OK;
}

int hive_dpt_forward(hive_dpt *d, const uint8_t *d_rgb, int B, int H, int W, const void *d_pos_embed, float *d_depth, float max_depth,
                     uint16_t *d_out_mm, float *d_out_m) {
    return hive_dpt_forward_frames(d, d_rgb, B, H, W, H, W, d_pos_embed, d_depth, max_depth, d_out_mm, d_out_m);
}

int hive_dpt_weights_modified(hive_dpt *d) {
    HIVE_ENTER(d ? d->ctx : nullptr);
    if (!d) return hive_fail(nullptr, HIVE_ERR_INVALID, "dpt is NULL");
    // everything derived from the caller's tensors: the ViT engine's folded LayerNorm weights (rebuilt now, on the context's stream) and the Gram tables of
    // the 1 x 1 convolutions (dropped; rebuilt by the forward that next needs them).  All other weights are read through the caller's pointers at every forward.
    HIVE_CHECK_HIP(d->ctx, hipStreamSynchronize(d->ctx->stream));  // (a forward in flight may still read the tables)
    for (auto &kv : d->gram_tables)
        if (kv.second) (void)hipFree(kv.second);
    d->gram_tables.clear();
    return hive_vit_weights_modified(d->vit);
}

int hive_dpt_arena_bytes(hive_dpt *d, int64_t *bytes) {
    if (!d || !bytes) return hive_fail(d ? d->ctx : nullptr, HIVE_ERR_INVALID, "hive_dpt_arena_bytes: NULL argument");
    *bytes = (int64_t)d->arena_bytes;
    return HIVE_OK;
}

int hive_dpt_destroy(hive_dpt *d) {
    if (!d) return HIVE_OK;
    {
        HIVE_ENTER(d->ctx);
        (void)hipStreamSynchronize(d->ctx->stream);
        if (d->vit) hive_vit_destroy(d->vit);
        if (d->arena) (void)hipFree(d->arena);
        for (auto &kv : d->gram_tables)
            if (kv.second) (void)hipFree(kv.second);
    }
    delete d;
    return HIVE_OK;
}

}  // extern "C"
