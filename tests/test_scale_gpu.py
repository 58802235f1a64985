"""The depth network and its decoder / stem kernels at the benchmark's batch sizes, where activations cross the 32-bit limits: the
headline DPT-Hybrid job (480 x 640, batches of 107), twice that (224 frames: `path_1` past 2^32 elements), and config 4 (DPT-Large on
48 frames of 1080p at a 480 x 864 network size).  No smaller test reaches an element offset past 2^31.

The technique: one input placed at index 0 AND at late indices of ONE batch.  A kernel that computes every pixel with the same
arithmetic must give the copies bit-identical outputs, so any address error past a limit shows up however small it is; and the last
image is compared with a float32 PyTorch reference of that image alone, with the tolerance of the kernel's own small-shape test.
Every test first asserts its premise -- the operand sizes against the limit it is about -- so that shrinking a batch fails loudly
instead of quietly testing nothing.  Deterministic mode (no split-K, no attention key split, no Gram-matrix statistics) throughout.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dpt_weights import seeded_init, seeded_input

pytestmark = pytest.mark.gpu

SCALE, SHIFT = 0.000305, 0.1378
HALF_TIGHT = {torch.bfloat16: 1.0, torch.float16: 0.125}  # float16 carries 3 more significant bits than bfloat16
# 99th percentile of |depth| differences between a frame in a batch and the same frame in another batch (or alone), or a copy of it at an index
# that is not a multiple of 64 of the same batch.  Measured once over the 107 frames of each type (batches of 8) and frame 223 of 224 (alone):
# at most 51.4 mm in bfloat16, 7.6 mm in float16.  Bound: the largest + 40 %.
P99_BATCH_MM = {torch.bfloat16: 72.0, torch.float16: 10.7}
GB = 1e9


@pytest.fixture(params=["bfloat16", "float16"])
def half(request):
    """The 16-bit type of the kernels / network under test."""
    return getattr(torch, request.param)


@pytest.fixture
def det_ctx(gpu_ctx):
    """The default context in deterministic mode for one test; everything the test allocated is released behind it."""
    gpu_ctx.set_deterministic(True)
    torch.cuda.reset_peak_memory_stats()
    try:
        yield gpu_ctx
    finally:
        gpu_ctx.set_deterministic(False)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _ulp(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def _check(out, ref, what):
    """test_conv_gpu.py's bound: two ulps of the largest value elementwise, 0.77 ulp relative Frobenius."""
    u = _ulp(out.dtype)
    err = (out.float() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 2 * u * scale + 0.25 * u, f"{what}: max error {err:.4g} vs scale {scale:.4g}"
    rel = ((out.float() - ref).norm() / ref.norm()).item()
    assert rel < 0.77 * u, f"{what}: relative Frobenius error {rel:.4g}"
    return err, rel


def _premise(what, elements, elem_bytes, limit_name, limit_bytes=None, limit_elements=None):
    nbytes = elements * elem_bytes
    print(f"  premise: {what}: {elements / 1e9:.3f} G elements, {nbytes / GB:.2f} GB; limit {limit_name}")
    if limit_bytes is not None:
        assert nbytes > limit_bytes, f"{what}: {nbytes} bytes do not cross {limit_name}"
    if limit_elements is not None:
        assert elements > limit_elements, f"{what}: {elements} elements do not cross {limit_name}"


def _map(n, h, w, c, dtype, seed, scale=1.0):
    """A channels-last [n, c, h, w] map of distinct random images, drawn on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, h, w, c), generator=g, device="cuda", dtype=dtype)
    if scale != 1.0:
        x.mul_(scale)
    return x.permute(0, 3, 1, 2)  # NHWC memory = channels-last NCHW view


def _plant(x, src, at):
    """Copy image ``src`` of the batch to every index in ``at``."""
    for i in at:
        x[i].copy_(x[src])


def _mm(a, b):
    e = ((a.float() - b.float()).abs() * 1000.0).flatten()
    return float(e.median()), float(torch.quantile(e[::7].cpu(), 0.99))


# ------------------------------------------------------------------------------------------------------------------------------
# A. kernels at the limits


@pytest.mark.parametrize("gather", [False, True], ids=["lds", "gather"])
def test_upsample2x_past_2_31_elements(det_ctx, half, monkeypatch, gather):
    """hive_nhwc_upsample2x with the bias of the producing convolution folded in: [224, 120, 160, 256] -> [224, 240, 320, 256], both the
    LDS-tile kernel and the gather kernel.  A per-pixel kernel: image 0 and its copy at 223 bit-identical, every image bit-identical to the
    same images upsampled in launches of 28 (each below 2^31 bytes), the last image within one rounding of float32 interpolation."""
    from hive_amd.dpt import ops
    if gather:
        monkeypatch.setenv("HIVE_UPSAMPLE_GATHER", "1")
    B, H, W, C = 224, 120, 160, 256
    _premise("upsample output", B * 4 * H * W * C, 2, "2^31 elements / 2^32 bytes", limit_bytes=2 ** 32, limit_elements=2 ** 31)
    x = _map(B, H, W, C, half, seed=21)
    _plant(x, 0, [B - 1])
    b = torch.randn(C, generator=torch.Generator(device="cuda").manual_seed(22), device="cuda").to(half)
    out = ops.upsample2x(x, engine="hip", bias=b)
    torch.cuda.synchronize()
    same = torch.equal(out[0], out[B - 1])
    print(f"  upsample2x ({'gather' if gather else 'lds'}, {half}): copies 0 / {B - 1} bit-identical: {same}")
    assert same, "image 0 and its copy at the end of the batch differ"
    for i in range(0, B, 28):
        part = ops.upsample2x(x[i:i + 28], engine="hip", bias=b)
        assert torch.equal(out[i:i + 28], part), f"images {i}..{i + 27}: the whole batch differs from a launch of 28"
        del part
    xb = (x[B - 1:].float() + b.float().view(1, -1, 1, 1)).to(half).float()  # (x + b rounded to the type first, as the kernel does)
    ref = F.interpolate(xb, scale_factor=2, mode="bilinear", align_corners=True)
    err = (out[B - 1:].float() - ref).abs().max().item()
    print(f"  last image vs float32 interpolate: max error {err:.3g} (bound {_ulp(half) * ref.abs().max().item():.3g})")
    assert err <= _ulp(half) * ref.abs().max().item() + 1e-6
    del x, out, xb, ref


def test_conv3x3_output_conv0_past_2_31_elements(det_ctx, half):
    """hive_nhwc_conv, 3 x 3 from 256 to 128 channels with bias (the head's `output_conv.0`) on [224, 240, 320, 256]: the input is past 2^31
    elements.  Copies 0 / 223 bit-identical; the last image against float32 conv2d to test_conv_gpu.py's bound."""
    from hive_amd.dpt import ops
    B, H, W, Ci, Co = 224, 240, 320, 256, 128
    _premise("conv input", B * H * W * Ci, 2, "2^31 elements / 2^32 bytes", limit_bytes=2 ** 32, limit_elements=2 ** 31)
    _premise("conv output", B * H * W * Co, 2, "2^31 bytes", limit_bytes=2 ** 31)
    g = torch.Generator(device="cpu").manual_seed(31)
    conv = nn.Conv2d(Ci, Co, 3, 1, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * Ci)) ** 0.5)
        conv.bias.copy_(torch.randn(Co, generator=g) * 0.3)
    conv = conv.to(memory_format=torch.channels_last).to(half).cuda()
    x = _map(B, H, W, Ci, half, seed=32)
    _plant(x, 0, [B - 1])
    with torch.no_grad():
        out = ops.conv3x3(x, conv)
        torch.cuda.synchronize()
        same = torch.equal(out[0], out[B - 1])
        print(f"  conv 256 -> 128 ({half}): copies 0 / {B - 1} bit-identical: {same}")
        assert same, "image 0 and its copy at the end of the batch differ"
        ref = F.conv2d(x[B - 1:].float(), conv.weight.float(), conv.bias.float(), 1, 1)
        err, rel = _check(out[B - 1:], ref, "last image")
    print(f"  last image vs float32 conv2d: max error {err:.3g}, relative Frobenius {rel:.3g}")
    del x, out, ref, conv


def test_fused_head_past_2_31_elements(det_ctx, half):
    """hive_dpt_head_fused (bias of output_conv.0 folded in -> x2 upsample -> 3 x 3 128 -> 32 -> ReLU -> 1 x 1 -> ReLU -> inversion ->
    hand-off) on [224, 240, 320, 128], past 2^31 elements.  Copies 0 / 223 bit-identical in depth, mm and m; every image equal to the
    same images in launches of 28; the last image against PyTorch's float32 operators as in test_fused_head_matches_torch."""
    from hive_amd import _lib
    from hive_amd.dpt import ops
    B, H, W, C = 224, 240, 320, 128
    _premise("head input", B * H * W * C, 2, "2^31 elements / 2^32 bytes", limit_bytes=2 ** 32, limit_elements=2 ** 31)
    torch.manual_seed(41)
    x = _map(B, H, W, C, half, seed=42, scale=0.5)
    _plant(x, 0, [B - 1])
    w3 = (torch.randn(32, 128, 3, 3, device="cuda") * 0.05).to(half)
    b3 = torch.randn(32) * 0.1
    w1 = torch.randn(32) * 0.3
    b1, scale, shift = 0.05, 0.01, 0.1
    b0 = torch.randn(128, device="cuda") * 0.2
    w3_dev = w3.permute(2, 3, 0, 1).contiguous()
    b3_np, w1_np = b3.numpy().astype("float32"), w1.numpy().astype("float32")
    ctx = det_ctx

    def head(t):
        n = t.shape[0]
        d = torch.empty((n, 2 * H, 2 * W), dtype=torch.float32, device="cuda")
        mm = torch.empty((n, 2 * H, 2 * W), dtype=torch.int16, device="cuda")
        m = torch.empty((n, 2 * H, 2 * W), dtype=torch.float32, device="cuda")
        ctx.check(ctx.lib.hive_dpt_head_fused(ctx.handle, t.data_ptr(), b0.data_ptr(), _lib.dtype_code(half), n, H, W, C, 32, w3_dev.data_ptr(),
                                              b3_np.ctypes.data, w1_np.ctypes.data, b1, 1, 1, scale, shift, d.data_ptr(), 1.0 / 1000.0, 10.0,
                                              mm.data_ptr(), m.data_ptr()))
        return d, mm, m

    depth, mm, m = head(x)
    torch.cuda.synchronize()
    same = torch.equal(depth[0], depth[B - 1]) and torch.equal(mm[0], mm[B - 1]) and torch.equal(m[0], m[B - 1])
    print(f"  fused head ({half}): copies 0 / {B - 1} bit-identical (depth, mm, m): {same}")
    assert same, "image 0 and its copy at the end of the batch differ"
    for i in range(0, B, 28):
        part = head(x[i:i + 28])
        assert all(torch.equal(a[i:i + 28], p) for a, p in zip((depth, mm, m), part)), f"images {i}..{i + 27}: the whole batch differs from a launch of 28"
        del part
    with torch.no_grad():
        xb = (x[B - 1:].float() + b0.reshape(1, 128, 1, 1)).to(half).contiguous(memory_format=torch.channels_last)
        up = ops.upsample2x(xb, engine="hip").float()
        feat = F.relu(F.conv2d(up, w3.float(), b3.cuda(), padding=1))
        pre = F.relu(F.conv2d(feat, w1.cuda().reshape(1, 32, 1, 1), torch.tensor([b1], device="cuda"))).squeeze(1)
        ref = 1.0 / torch.clamp(scale * pre + shift, min=1e-8)
    got_pre = (1.0 / depth[B - 1:] - shift) / scale
    err = (got_pre - pre).abs().max().item() / (pre.abs().max().item() + 1e-6)
    print(f"  last image vs float32 torch head: pre-inversion relative error {err:.3g} (bound 2e-4)")
    assert err < 2e-4
    assert torch.allclose(depth[B - 1:], ref, rtol=1e-4, atol=1e-6)
    exp_mm = (depth[B - 1:] * 1000.0).clamp(0, 65535).to(torch.int32)
    assert torch.equal(mm[B - 1:].to(torch.int32) & 0xFFFF, exp_mm)
    del x, depth, mm, m, xb, up, feat, pre, ref, got_pre, exp_mm


def test_stem_and_pool_past_2_31_bytes(det_ctx, half):
    """hive_resnet_stem_conv_gn (7 x 7 / 2 'SAME', GroupNorm sums in the epilogue) then hive_nhwc_group_norm_relu_maxpool: [224, 480, 640, 3]
    in, [224, 240, 320, 64] in between (past 2^31 bytes).  Copies 0 / 223 bit-identical in both outputs; the last image against float32
    torch with test_stem_conv_and_maxpool_match_torch's bounds."""
    from hive_amd.dpt import ops
    from hive_amd.dpt.models import GroupNormAct, MaxPool2dSame, StdConv2dSame
    B, H, W = 224, 480, 640
    oh, ow = H // 2, W // 2
    _premise("stem output", B * oh * ow * 64, 2, "2^31 bytes", limit_bytes=2 ** 31)
    g = torch.Generator(device="cpu").manual_seed(51)
    conv = StdConv2dSame(3, 64, 7, stride=2)
    norm = GroupNormAct(64)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        norm.weight.copy_(torch.rand(64, generator=g) + 0.5)
        norm.bias.copy_(torch.randn(64, generator=g) * 0.2)
    conv = conv.to(memory_format=torch.channels_last).to(half).cuda().eval()
    norm = norm.to(half).cuda().eval()
    gd = torch.Generator(device="cuda").manual_seed(52)
    x = (torch.rand((B, H, W, 3), generator=gd, device="cuda") * 2 - 1).to(half).permute(0, 3, 1, 2)
    _plant(x, 0, [B - 1])
    with torch.no_grad():
        conv.engine = "torch"
        wt = conv.standardized_weight()
        conv.engine = "hip"
        out = ops.stem_conv(x, conv, wt)
        stats = getattr(out, "hive_gn_stats", None)
        assert stats is not None, "240 x 320 is whole 8 x 32 tiles: the sums come out of the epilogue"
        pooled = ops.group_norm_relu_maxpool(out, norm, stats=stats)
        torch.cuda.synchronize()
        same = (torch.equal(out[0], out[B - 1]), torch.equal(pooled[0], pooled[B - 1]))
        print(f"  stem ({half}): copies 0 / {B - 1} bit-identical (conv, GroupNorm + ReLU + pool): {same}")
        assert all(same), "image 0 and its copy at the end of the batch differ"
        ph, pw = max((oh - 1) * 2 + 7 - H, 0), max((ow - 1) * 2 + 7 - W, 0)
        last = x[B - 1:].float()
        ref = F.conv2d(F.pad(last, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2)), wt.float(), None, 2, 0)
        err, rel = _check(out[B - 1:], ref, "stem conv, last image")
        ref_n = MaxPool2dSame(3, 2)(F.relu(F.group_norm(out[B - 1:].float(), 32, norm.weight.float(), norm.bias.float(), norm.eps)))
        err_p = (pooled[B - 1:].float() - ref_n).abs().max().item()
    print(f"  last image: conv max error {err:.3g} (relative {rel:.3g}); GroupNorm + ReLU + pool max error {err_p:.3g}")
    assert err_p <= 4 * _ulp(half) * max(ref_n.abs().max().item(), 1.0)
    del x, out, pooled, ref, ref_n, last, stats


# ------------------------------------------------------------------------------------------------------------------------------
# B. the network object at the benchmark's batches


def _model(backbone, half, seed):
    """(float32 PyTorch-formulation model, 16-bit channels-last HIP-engine model) with the same seeded weights."""
    from hive_amd.dpt.models import DPTDepthModel
    ref = DPTDepthModel(path=None, scale=SCALE, shift=SHIFT, invert=True, engine="torch", backbone=backbone).eval()
    seeded_init(ref, seed=seed)
    hip = DPTDepthModel(path=None, scale=SCALE, shift=SHIFT, invert=True, engine="hip", backbone=backbone).eval()
    hip.load_state_dict(ref.state_dict())
    return ref.cuda(), hip.to(memory_format=torch.channels_last).to(half).cuda()


def _frames(n, h, w, seed, plant_at, plant_seed=1000):
    """uint8 [n, h, w, 3] on the device: seeded, distinct frames, with one other frame F copied to every index in ``plant_at``."""
    x = seeded_input(n, h, w, seed=seed)
    f = seeded_input(1, h, w, seed=plant_seed)[0]
    for i in plant_at:
        x[i] = f
    return ((x.cuda() * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _net_in(frames_u8):
    """The float32 network input of uint8 frames: ((x / 255) - 0.5) / 0.5 (dataset_adaptors.py:1407 + NormalizeImage(0.5, 0.5))."""
    return ((frames_u8.float() / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()


def _release(*models):
    for m in models:
        nat = getattr(m, "_native", None)
        if nat is not None:
            nat.close()


@pytest.mark.parametrize("B,half_name,plant_at", [
    (107, "bfloat16", (0, 64, 106)),   # the headline job
    (107, "float16", (0, 64, 106)),    # ... in the reference's type (bench.py value_fp16)
    (224, "bfloat16", (0, 64, 128, 192, 223)),  # path_1 past 2^32 elements
], ids=["b107-bf16", "b107-fp16", "b224-bf16"])
def test_dpt_hybrid_at_the_benchmark_batch(det_ctx, B, half_name, plant_at):
    """hive_dpt_forward_frames (the whole DPT-Hybrid + pre-processing + hand-off as one C-ABI object) at 480 x 640 on B frames with one frame F
    copied to ``plant_at``.  Copies at multiples of 64 bit-identical (every per-image map of 480 x 640 is a multiple of 256 pixels); every frame
    (B = 107) or the last one (B = 224) against the same frames in batches of 8 (or alone); sampled frames against the float32 network; B = 107:
    the native object equals the Python orchestration bit for bit."""
    from hive_amd import depth as depth_mod
    half = getattr(torch, half_name)
    tight = HALF_TIGHT[half]
    H, W = 480, 640
    _premise("path_1 (refinenet1 x2 output)", B * H // 2 * W // 2 * 256, 2, "2^31 bytes", limit_bytes=2 ** 31)
    if B >= 219:
        _premise("path_1 (refinenet1 x2 output)", B * H // 2 * W // 2 * 256, 2, "2^32 elements", limit_elements=2 ** 32)
    ref, hip = _model("vitb_rn50_384", half, seed=1234)
    frames = _frames(B, H, W, seed=B, plant_at=plant_at)
    with torch.no_grad():
        d_big, mm_big, m_big = hip.forward_frames(frames, max_depth=10.0)
    torch.cuda.synchronize()
    arena = hip.native().arena_bytes()
    print(f"  DPT-Hybrid {half} B = {B}: arena_bytes {arena / GB:.2f} GB, peak allocated by torch {torch.cuda.max_memory_allocated() / GB:.2f} GB")
    assert torch.isfinite(d_big).all() and float(d_big.max() - d_big.min()) > 1.0
    p0 = plant_at[0]
    for i in plant_at[1:]:
        same = torch.equal(d_big[p0], d_big[i]) and torch.equal(mm_big[p0], mm_big[i]) and torch.equal(m_big[p0], m_big[i])
        med, p99 = _mm(d_big[i], d_big[p0])
        print(f"  copy at {i} vs {p0}: bit-identical {same}; median {med:.3f} mm, p99 {p99:.3f} mm")
        if i % 64 == 0:
            assert same, f"frame {i} (a multiple of 64) differs from its copy at {p0}"
        else:  # (the per-image maps of the deeper stages are not whole 256-pixel tiles from there: rounding noise, as between batches)
            assert med <= tight * 12.0 and p99 <= P99_BATCH_MM[half], (i, med, p99)
    # the same frames in smaller batches: B = 107 all of them in batches of 8, B = 224 the last frame alone
    chunks = [(i, min(i + 8, B)) for i in range(0, B, 8)] if B < 200 else [(B - 1, B)]
    worst_med, worst_p99 = 0.0, 0.0
    for a, b in chunks:
        with torch.no_grad():
            d_small, _, _ = hip.forward_frames(frames[a:b], max_depth=10.0)
        for j in range(a, b):
            med, p99 = _mm(d_big[j], d_small[j - a])
            worst_med, worst_p99 = max(worst_med, med), max(worst_p99, p99)
        del d_small
    print(f"  batch of {B} vs batches of {chunks[0][1] - chunks[0][0]} ({len(chunks)} calls): worst median {worst_med:.3f} mm, worst p99 {worst_p99:.3f} mm")
    # test_batch_independence_and_determinism's bound (median <= 12 mm in bfloat16, / 8 in float16) and the measured p99 bound
    assert worst_med <= tight * 12.0 and worst_p99 <= P99_BATCH_MM[half], (worst_med, worst_p99)
    # against the float32 network (the per-stage tests' depth bounds)
    idx = [0, B // 2, B - 1]
    with torch.no_grad():
        d_ref = torch.cat([ref(_net_in(frames[i:i + 1])) for i in idx])
    for k, i in enumerate(idx):
        med, p99 = _mm(d_big[i], d_ref[k])
        print(f"  frame {i} vs float32: median {med:.3f} mm, p99 {p99:.3f} mm")
        assert med <= tight * 20.0 and p99 <= tight * 120.0, (i, med, p99)
    del d_ref
    if B < 200:
        # the native object equals the Python orchestration of the same kernels bit for bit
        with torch.no_grad():
            d_py, mm_py, m_py = hip(depth_mod.preprocess_on_device(frames, half), handoff=(10.0,))
        same = torch.equal(d_big, d_py) and torch.equal(mm_big, mm_py) and torch.equal(m_big, m_py)
        print(f"  network object vs Python orchestration, {B} frames: bit-identical {same}")
        assert same, f"depth differs by up to {float((d_big - d_py).abs().max()) * 1000:.3f} mm"
        del d_py, mm_py, m_py
    print(f"  peak allocated by torch {torch.cuda.max_memory_allocated() / GB:.2f} GB")
    _release(hip)
    del ref, hip, frames, d_big, mm_big, m_big


def test_dpt_large_config4_batch(det_ctx):
    """BASELINE config 4 as bench.py's config4_leg runs it: 48 frames of 1080 x 1920 through DPT-Large at the reference's 480 x 864 network size --
    bicubic resize in, network, nearest resize back with the mm hand-off, one C-ABI call.  `path_1` (240 x 432 x 256 per frame) is past 2^31 bytes.
    Frame 47, a copy of frame 0, bit-identical to it; against itself run alone and against the float32 network on the same resized input."""
    from hive_amd import depth as depth_mod
    B, H, W = 48, 1080, 1920
    net = depth_mod.network_size(H, W)
    assert net == (480, 864)
    _premise("path_1 (refinenet1 x2 output)", B * net[0] // 2 * net[1] // 2 * 256, 2, "2^31 bytes", limit_bytes=2 ** 31)
    ref, hip = _model("vitl16_384", torch.bfloat16, seed=1234)
    frames = _frames(B, H, W, seed=48, plant_at=(0, B - 1))
    with torch.no_grad():
        d_big, mm_big, m_big = hip.forward_frames(frames, max_depth=10.0, net_size=net)
    torch.cuda.synchronize()
    arena = hip.native().arena_bytes()
    print(f"  DPT-Large B = {B} at {net}: arena_bytes {arena / GB:.2f} GB, peak allocated by torch {torch.cuda.max_memory_allocated() / GB:.2f} GB")
    assert d_big.shape == (B, H, W) and torch.isfinite(d_big).all() and float(d_big.max() - d_big.min()) > 0.5
    same = torch.equal(d_big[0], d_big[B - 1])
    c_med, c_p99 = _mm(d_big[B - 1], d_big[0])
    print(f"  copies 0 / {B - 1}: bit-identical {same}; median {c_med:.3f} mm, p99 {c_p99:.3f} mm")
    with torch.no_grad():
        d_one, _, _ = hip.forward_frames(frames[B - 1:], max_depth=10.0, net_size=net)
        x32 = depth_mod.resize_preprocess_on_device(frames[B - 1:], net, torch.float32)
        d32 = F.interpolate(ref(x32).unsqueeze(1), size=(H, W), mode="nearest").squeeze(1)
    a_med, a_p99 = _mm(d_big[B - 1], d_one[0])
    r_med, r_p99 = _mm(d_big[B - 1], d32[0])
    print(f"  frame {B - 1} vs alone: bit-identical {torch.equal(d_big[B - 1], d_one[0])}, median {a_med:.3f} mm, p99 {a_p99:.3f} mm; "
          f"vs float32: median {r_med:.3f} mm, p99 {r_p99:.3f} mm")
    assert a_med <= 20.0 and r_med <= 20.0, (a_med, r_med)
    # The 30 x 54 stage's per-image offsets are not whole 256-pixel tiles, yet the copies came out bit-identical when measured (deterministic mode):
    # no kernel on this path rounds a pixel differently by where its image sits in the batch.  Held to that.
    assert same, f"copies 0 / {B - 1} differ: median {c_med:.3f} mm, p99 {c_p99:.3f} mm"
    print(f"  peak allocated by torch {torch.cuda.max_memory_allocated() / GB:.2f} GB")
    _release(hip)
    del ref, hip, frames, d_big, mm_big, m_big, d_one, x32, d32
