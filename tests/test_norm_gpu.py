"""The normalisation and element-wise kernels through the C ABI, pinned to one ulp: hive_vit_layernorm, hive_nhwc_group_norm (its own statistics and
tile partials), hive_nhwc_group_norm_relu_maxpool, hive_nhwc_bias_act, hive_dpt_preprocess, hive_dpt_head_tail, hive_depth_mm_to_m.

The operands are the small integers of tests/norm_reference.py: every statistic is exact in float32 in any order, so each output must lie in
[round_T(ref - rho), round_T(ref + rho)] with ref the float64 definition and rho a COUNTED number of float32 roundings (derived beside each reference
there; tests/test_norm_reference_cpu.py checks references, generators and radii without a GPU).  At least 3/4 of the intervals of every case are a
single value: there the assertion is bit for bit, elsewhere one ulp of the element type.  Every group and every row has its own mean and spread, one
in eight is constant (var = 0), so a neighbour's statistics, a lost pixel, a wrong divisor or a missing eps leave the interval.  The element-wise entry
points are compared with ``torch.equal`` against the stated roundings applied in order to dyadic operands.

Outputs are written into poisoned buffers with a guard region behind them: an element the kernel skipped and one it wrote past the end both fail."""
import numpy as np
import pytest
import torch

import norm_reference as R

pytestmark = pytest.mark.gpu

POISON = 0x7FC5  # a NaN in both element types
GUARD = 2048     # elements behind every output


@pytest.fixture(params=["bfloat16", "float16"])
def half(request):
    """The 16-bit element type of the kernels under test."""
    return getattr(torch, request.param)


def _fmt(half):
    return str(half).split(".")[1]


def _code(dtype):
    from hive_amd import _lib
    return _lib.dtype_code(dtype)


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_references():
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _cached(key, make):
    """Operands and references are computed once and shared (never modified)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _dev(a, dtype):
    """Values that are exact in ``dtype`` (asserted by the generators), on the device."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device="cuda", dtype=dtype)


def _host(t):
    return t.double().cpu().numpy()


def _p(t):
    return None if t is None else t.data_ptr()


def _poisoned(elements, dtype):
    """(raw int16 buffer of elements + GUARD poisoned values, its view in dtype)."""
    buf = torch.full((elements + GUARD,), POISON, dtype=torch.int16, device="cuda")
    return buf, buf.view(dtype)


def _guard_intact(buf, elements):
    return bool((buf[elements:] == POISON).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_vit_layernorm

@pytest.mark.parametrize("M,D", R.LN_CASES)
def test_layernorm_interval(gpu_ctx, half, M, D):
    fmt = _fmt(half)
    x, gamma, beta = _cached(("ln", M, D), lambda: R.ln_operands(M, D))
    lo, hi, ref = _cached(("ln", M, D, fmt), lambda: R.ln_interval(x, gamma, beta, R.LN_EPS, fmt))
    rows = M + 5  # a padded buffer: the rows beyond M hold values in x and must stay untouched in out
    xd = torch.zeros(rows, D, dtype=half, device="cuda")
    xd[:M] = _dev(x, half)
    xd[M:] = 3
    g, b = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    buf, out = _poisoned(rows * D, half)
    gpu_ctx.check(gpu_ctx.lib.hive_vit_layernorm(gpu_ctx.handle, xd.data_ptr(), _code(half), g.data_ptr(), b.data_ptr(), out.data_ptr(), M, D, R.LN_EPS))
    torch.cuda.synchronize()
    assert _guard_intact(buf, M * D), "rows beyond M were written"
    share = R.check_interval(_host(out[:M * D]).reshape(M, D), lo, hi, f"layernorm M={M} D={D} {fmt}", ref)
    assert share >= 0.75
    if M >= 3:  # the constant row: beta exactly
        assert np.array_equal(_host(out[(M // 2) * D:(M // 2 + 1) * D]), R.round_to(beta.astype(np.float64), fmt))


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_nhwc_group_norm

def _gn_case(N, HW, C, G, fmt, half):
    def make():
        x, gamma, beta, res = R.gn_operands(N, HW, C, G, fmt)
        return x, gamma, beta, res, _dev(x, half), _dev(gamma, half), _dev(beta, half), _dev(res, half)
    return _cached(("gn", N, HW, C, G, fmt), make)


def _group_norm(ctx, half, xd, gd, bd, rd, N, HW, C, G, eps, relu, partial=None, TM=0):
    buf, out = _poisoned(N * HW * C, half)
    if partial is None:
        rc = ctx.lib.hive_nhwc_group_norm(ctx.handle, xd.data_ptr(), _code(half), N, HW, C, G, gd.data_ptr(), bd.data_ptr(), eps, _p(rd), int(relu), out.data_ptr())
    else:
        rc = ctx.lib.hive_nhwc_group_norm_stats(ctx.handle, xd.data_ptr(), _code(half), N, HW, C, G, gd.data_ptr(), bd.data_ptr(), eps, _p(rd), int(relu),
                                                out.data_ptr(), partial.data_ptr(), TM)
    ctx.check(rc)
    torch.cuda.synchronize()
    assert _guard_intact(buf, N * HW * C), "group norm wrote behind its output"
    return buf[:N * HW * C]


@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("N,HW,C,G", R.GN_CASES)
def test_group_norm_interval(gpu_ctx, half, N, HW, C, G, relu, res):
    fmt = _fmt(half)
    x, gamma, beta, r, xd, gd, bd, rd = _gn_case(N, HW, C, G, fmt, half)
    eps = R.gn_eps(HW, C // G)
    lo, hi, ref = R.gn_interval(x, gamma, beta, G, eps, fmt, r if res else None, relu)
    bits = _group_norm(gpu_ctx, half, xd, gd, bd, rd if res else None, N, HW, C, G, eps, relu)
    share = R.check_interval(_host(bits.view(half)).reshape(N, HW, C), lo, hi, f"group norm {(N, HW, C, G)} relu={relu} residual={res} {fmt}", ref)
    assert share >= 0.75
    assert torch.equal(bits, _group_norm(gpu_ctx, half, xd, gd, bd, rd if res else None, N, HW, C, G, eps, relu)), "two calls differ"


@pytest.mark.parametrize("relu,res", [(False, False), (True, True)])
@pytest.mark.parametrize("N,HW,C,G,TM", R.GN_TILE_CASES)
def test_group_norm_from_tile_partials(gpu_ctx, half, N, HW, C, G, TM, relu, res):
    """Statistics from [tile][h][sum, sq][C] partials computed here from the same integers: the sums are exact, so the output equals the own-statistics
    path bit for bit, and lies in the float64 interval."""
    fmt = _fmt(half)
    x, gamma, beta, r, xd, gd, bd, rd = _gn_case(N, HW, C, G, fmt, half)
    eps = R.gn_eps(HW, C // G)
    partial = torch.from_numpy(R.gn_tile_partials(x, TM)).cuda()
    lo, hi, ref = R.gn_interval(x, gamma, beta, G, eps, fmt, r if res else None, relu)
    bits = _group_norm(gpu_ctx, half, xd, gd, bd, rd if res else None, N, HW, C, G, eps, relu, partial, TM)
    R.check_interval(_host(bits.view(half)).reshape(N, HW, C), lo, hi, f"group norm from tiles {(N, HW, C, G, TM)} relu={relu} residual={res} {fmt}", ref)
    assert torch.equal(bits, _group_norm(gpu_ctx, half, xd, gd, bd, rd if res else None, N, HW, C, G, eps, relu)), "tile partials and own statistics differ"


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_nhwc_group_norm_relu_maxpool

@pytest.mark.parametrize("tiles", [False, True])
@pytest.mark.parametrize("H,W,C", R.POOL_CASES)
def test_group_norm_relu_maxpool(gpu_ctx, half, H, W, C, tiles):
    fmt, N, HW, G = _fmt(half), 2, H * W, R.pool_groups(H, W, C)
    x, gamma, beta, _, xd, gd, bd, _ = _gn_case(N, HW, C, G, fmt, half)
    eps = R.gn_eps(HW, C // G)
    lo, hi, ref = R.gn_pool_interval(x, gamma, beta, G, eps, fmt, H, W)
    Ho, Wo, _, _ = R.same_pool_geometry(H, W)
    TM = R.pool_tile_rows(HW) if tiles else 0
    partial = torch.from_numpy(R.gn_tile_partials(x, TM)).cuda() if tiles else None
    n_out = N * Ho * Wo * C
    buf, out = _poisoned(n_out, half)
    gpu_ctx.check(gpu_ctx.lib.hive_nhwc_group_norm_relu_maxpool(gpu_ctx.handle, xd.data_ptr(), _code(half), N, H, W, C, G, gd.data_ptr(), bd.data_ptr(), eps,
                                                                out.data_ptr(), _p(partial), TM))
    torch.cuda.synchronize()
    assert _guard_intact(buf, n_out), "the pooling wrote behind its output"
    share = R.check_interval(_host(out[:n_out]).reshape(N, Ho * Wo, C), lo, hi, f"group norm + relu + max pool {(H, W, C)} tiles={tiles} {fmt}", ref)
    assert share >= 0.75
    # and bit for bit what gn_apply followed by the pooling kernel gives on the same statistics
    normed = _group_norm(gpu_ctx, half, xd, gd, bd, None, N, HW, C, G, eps, True, partial, TM).view(half)
    buf2, out2 = _poisoned(n_out, half)
    gpu_ctx.check(gpu_ctx.lib.hive_nhwc_maxpool3x3s2(gpu_ctx.handle, normed.data_ptr(), _code(half), N, H, W, C, out2.data_ptr()))
    torch.cuda.synchronize()
    assert _guard_intact(buf2, n_out) and torch.equal(buf[:n_out], buf2[:n_out]), "fused and separate pooling differ"


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_nhwc_bias_act

def _bias_act(ctx, half, xd, bd, r1, r2, n_px, C, relu, out_relu):
    n = n_px * C
    buf, out = _poisoned(n, half)
    buf_r, out_r = _poisoned(n, half)
    ctx.check(ctx.lib.hive_nhwc_bias_act(ctx.handle, xd.data_ptr(), _code(half), n_px, C, bd.data_ptr(), int(relu), _p(r1), _p(r2), out.data_ptr(),
                                         out_r.data_ptr() if out_relu else None))
    torch.cuda.synchronize()
    assert _guard_intact(buf, n) and _guard_intact(buf_r, n if out_relu else 0), "bias_act wrote where it must not"
    return out[:n], out_r[:n]


# n_px x C / 8 vectors: one below, equal to and one above a multiple of 256 (C = 256: 32 vectors a pixel, the nearest counts)
@pytest.mark.parametrize("n_px,C", [(255, 8), (256, 8), (257, 8), (511, 8), (7, 256), (8, 256), (9, 256)])
def test_bias_act_every_combination(gpu_ctx, half, n_px, C):
    """x + bias is rounded to T, + residual, rounded to T before + residual2, ReLU, rounded to T; out_relu = relu(out) (the kernel's comment)."""
    fmt = _fmt(half)
    rng = np.random.default_rng([n_px, C])
    x, bias, r1, r2 = R.dyadic(rng, (n_px, C), fmt), R.dyadic(rng, (C,), fmt), R.dyadic(rng, (n_px, C), fmt), R.dyadic(rng, (n_px, C), fmt)
    xd, bd, r1d, r2d = _dev(x, half), _dev(bias, half), _dev(r1, half), _dev(r2, half)
    for mask in range(16):
        res, res2, relu, out_relu = bool(mask & 1), bool(mask & 2), bool(mask & 4), bool(mask & 8)
        want, want_relu = R.bias_act_reference(x, bias, fmt, r1 if res else None, r2 if res2 else None, relu)
        out, out_r = _bias_act(gpu_ctx, half, xd, bd, r1d if res else None, r2d if res2 else None, n_px, C, relu, out_relu)
        what = f"bias_act {(n_px, C)} residual={res} residual2={res2} relu={relu} {fmt}"
        assert torch.equal(out, _dev(want, half).reshape(-1)), what
        if out_relu:
            assert torch.equal(out_r, _dev(want_relu, half).reshape(-1)), what + " out_relu"


def test_bias_act_grid_stride(gpu_ctx, half):
    """More vectors than the launch has threads (256 x 32 x CUs): the first threads make a second trip.  The reference is the same sequence of roundings with
    torch's element-wise float32 operations (float32 sums of these dyadic operands are exact; float32 -> T is one rounding)."""
    C = 256
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_px = cus * 32 * 256 // (C // 8) + 37
    gen = torch.Generator(device="cuda").manual_seed(11)

    def draw(shape):
        k = torch.randint(-1024, 1025, shape, generator=gen, device="cuda").float()
        return (k * torch.exp2(-torch.randint(0, 5, shape, generator=gen, device="cuda").float())).to(half)
    x, bias, r1 = draw((n_px, C)), draw((C,)), draw((n_px, C))
    want = torch.relu((x.float() + bias.float()).to(half).float() + r1.float()).to(half)
    out, out_r = _bias_act(gpu_ctx, half, x, bias, r1, None, n_px, C, True, True)
    assert torch.equal(out, want.reshape(-1)) and torch.equal(out_r, want.reshape(-1))


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_dpt_preprocess

@pytest.mark.parametrize("mean,std", [(0.5, 0.5), (0.485, 0.229)])
@pytest.mark.parametrize("n", [4, 1023, 1024, 1027, 4099])
def test_preprocess_is_the_float64_table(gpu_ctx, half, n, mean, std):
    """All 256 byte values (97 i + 13 mod 256 visits each from n = 256 on); n not a multiple of 4 ends in the scalar tail."""
    fmt = _fmt(half)
    rgb = ((np.arange(n) * 97 + 13) % 256).astype(np.uint8)
    assert n < 256 or len(np.unique(rgb)) == 256
    want = R.preprocess_table(mean, std, fmt)[rgb]
    buf, out = _poisoned(n, half)
    gpu_ctx.check(gpu_ctx.lib.hive_dpt_preprocess(gpu_ctx.handle, torch.from_numpy(rgb).cuda().data_ptr(), n, mean, std, _code(half), out.data_ptr()))
    torch.cuda.synchronize()
    assert _guard_intact(buf, n), "preprocess wrote behind its output"
    assert torch.equal(out[:n], _dev(want, half))


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_dpt_head_tail, hive_depth_mm_to_m

DEPTH_SCALE, MAX_DEPTH = 0.001, 10.0


def _head_tail(ctx, half, feat_d, n_px, C, pre_bias, pre_relu, w, bias, non_negative, invert, scale, shift, outputs=(True, True, True)):
    guard = 64
    depth = torch.full((n_px + guard,), float("nan"), device="cuda") if outputs[0] else None
    mm = torch.full((n_px + guard,), 0x5A5A, dtype=torch.int16, device="cuda") if outputs[1] else None
    m = torch.full((n_px + guard,), float("nan"), device="cuda") if outputs[2] else None
    ctx.check(ctx.lib.hive_dpt_head_tail(ctx.handle, feat_d.data_ptr(), _code(half), n_px, C, None if pre_bias is None else pre_bias.ctypes.data, int(pre_relu),
                                         w.ctypes.data, float(bias), int(non_negative), int(invert), scale, shift, _p(depth), DEPTH_SCALE, MAX_DEPTH, _p(mm), _p(m)))
    torch.cuda.synchronize()
    assert depth is None or bool(torch.isnan(depth[n_px:]).all())
    assert mm is None or bool((mm[n_px:] == 0x5A5A).all())
    assert m is None or bool(torch.isnan(m[n_px:]).all())
    return (None if depth is None else depth[:n_px].cpu().numpy(), None if mm is None else mm[:n_px].cpu().numpy().view(np.uint16),
            None if m is None else m[:n_px].cpu().numpy())


@pytest.mark.parametrize("n_px", [1, 256, 257])
@pytest.mark.parametrize("C", [8, 32, 64])
def test_head_tail_every_option(gpu_ctx, half, C, n_px):
    """Integer features, weights and biases: the dot product is exact in any order.  scale = 2^-4: scale * acc is exact, fused or not.  All three outputs
    against numpy float32, step by step, with and without pre-bias, pre-ReLU, non_negative and invert."""
    rng = np.random.default_rng([C, n_px])
    feat = rng.integers(-4, 5, size=(n_px, C)).astype(np.float64)
    pre_bias, w = rng.integers(-2, 3, size=C).astype(np.float32), rng.integers(-3, 4, size=C).astype(np.float32)
    feat_d = _dev(feat, half)
    for mask in range(16):
        pb, pre_relu, non_negative, invert = pre_bias if mask & 1 else None, bool(mask & 2), bool(mask & 4), bool(mask & 8)
        want = R.head_tail_reference(feat, pb, pre_relu, w, 5.0, non_negative, invert, 0.0625, 0.75, DEPTH_SCALE, MAX_DEPTH)
        got = _head_tail(gpu_ctx, half, feat_d, n_px, C, pb, pre_relu, w, 5.0, non_negative, invert, 0.0625, 0.75)
        for name, a, b in zip(("depth", "millimetres", "metres"), got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), f"head_tail C={C} n_px={n_px} options {mask:04b}: {name}"
    # any subset of the outputs
    want = R.head_tail_reference(feat, pre_bias, True, w, 5.0, True, True, 0.0625, 0.75, DEPTH_SCALE, MAX_DEPTH)
    for outputs in ((True, False, False), (False, True, False), (False, False, True)):
        got = _head_tail(gpu_ctx, half, feat_d, n_px, C, pre_bias, True, w, 5.0, True, True, 0.0625, 0.75, outputs)
        for on, a, b in zip(outputs, got, want):
            assert (a is None) if not on else np.array_equal(a, b)


def test_head_tail_zero_accumulator_and_zero_shift(gpu_ctx, half):
    """depth = 1 / 1e-8f, the millimetres saturate at 65535, the metres are cut to 0 by max_depth."""
    feat = np.zeros((3, 8))
    feat[1], feat[2] = 2, -1
    w = np.ones(8, dtype=np.float32)
    want = R.head_tail_reference(feat, None, False, w, 0.0, True, True, 0.5, 0.0, DEPTH_SCALE, MAX_DEPTH)
    assert want[0][0] == np.float32(1) / np.float32(1e-8) and want[1][0] == 65535 and want[2][0] == 0 and want[1][1] == 125
    got = _head_tail(gpu_ctx, half, _dev(feat, half), 3, 8, None, False, w, 0.0, True, True, 0.5, 0.0)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n", [1, 256, 257])
def test_depth_mm_to_m(gpu_ctx, n):
    special = np.array([65535, 0, 1, 9999, 10000, 10001, 5000, 10002, 32768], dtype=np.uint16)  # 0, 1, the largest, either side of max_depth = 10 m
    mm = np.resize(special, n)
    mm[len(special):] = (np.arange(n)[len(special):] * 257) % 20000
    want = R.depth_mm_to_m_reference(mm, DEPTH_SCALE, MAX_DEPTH)
    assert n == 1 or ((want == 0).sum() >= 2 and (want > 0).any())
    out = torch.full((n + 64,), float("nan"), device="cuda")
    gpu_ctx.check(gpu_ctx.lib.hive_depth_mm_to_m(gpu_ctx.handle, torch.from_numpy(mm.view(np.int16)).cuda().data_ptr(), n, DEPTH_SCALE, MAX_DEPTH, out.data_ptr()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all()) and np.array_equal(out[:n].cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------------------------------------
# bad arguments

def test_bad_arguments_are_rejected_and_the_context_stays_usable(gpu_ctx, half):
    lib, h, code = gpu_ctx.lib, gpu_ctx.handle, _code(half)
    t = torch.zeros(4096, dtype=half, device="cuda")
    f = torch.zeros(4096, device="cuda")
    u8 = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    u16 = torch.zeros(4096, dtype=torch.int16, device="cuda")
    w = np.ones(64, dtype=np.float32)
    p, wp = t.data_ptr(), w.ctypes.data
    bad = {
        "bias_act: NULL x": lambda: lib.hive_nhwc_bias_act(h, None, code, 4, 8, p, 0, None, None, p, None),
        "bias_act: NULL bias": lambda: lib.hive_nhwc_bias_act(h, p, code, 4, 8, None, 0, None, None, p, None),
        "bias_act: NULL out": lambda: lib.hive_nhwc_bias_act(h, p, code, 4, 8, p, 0, None, None, None, None),
        "bias_act: C = 12": lambda: lib.hive_nhwc_bias_act(h, p, code, 4, 12, p, 0, None, None, p, None),
        "bias_act: C = 0": lambda: lib.hive_nhwc_bias_act(h, p, code, 4, 0, p, 0, None, None, p, None),
        "bias_act: n_px = 0": lambda: lib.hive_nhwc_bias_act(h, p, code, 0, 8, p, 0, None, None, p, None),
        "bias_act: dtype": lambda: lib.hive_nhwc_bias_act(h, p, 99, 4, 8, p, 0, None, None, p, None),
        "preprocess: std = 0": lambda: lib.hive_dpt_preprocess(h, u8.data_ptr(), 16, 0.5, 0.0, code, p),
        "preprocess: n = 0": lambda: lib.hive_dpt_preprocess(h, u8.data_ptr(), 0, 0.5, 0.5, code, p),
        "preprocess: NULL input": lambda: lib.hive_dpt_preprocess(h, None, 16, 0.5, 0.5, code, p),
        "preprocess: unaligned input": lambda: lib.hive_dpt_preprocess(h, u8.data_ptr() + 1, 16, 0.5, 0.5, code, p),
        "preprocess: unaligned output": lambda: lib.hive_dpt_preprocess(h, u8.data_ptr(), 16, 0.5, 0.5, code, p + 2),
        "preprocess: dtype": lambda: lib.hive_dpt_preprocess(h, u8.data_ptr(), 16, 0.5, 0.5, 99, p),
        "head_tail: C = 72": lambda: lib.hive_dpt_head_tail(h, p, code, 4, 72, None, 0, wp, 0.0, 1, 1, 1.0, 0.0, f.data_ptr(), 0.001, 10.0, None, None),
        "head_tail: C = 12": lambda: lib.hive_dpt_head_tail(h, p, code, 4, 12, None, 0, wp, 0.0, 1, 1, 1.0, 0.0, f.data_ptr(), 0.001, 10.0, None, None),
        "head_tail: C = 0": lambda: lib.hive_dpt_head_tail(h, p, code, 4, 0, None, 0, wp, 0.0, 1, 1, 1.0, 0.0, f.data_ptr(), 0.001, 10.0, None, None),
        "head_tail: n_px = 0": lambda: lib.hive_dpt_head_tail(h, p, code, 0, 8, None, 0, wp, 0.0, 1, 1, 1.0, 0.0, f.data_ptr(), 0.001, 10.0, None, None),
        "head_tail: no output": lambda: lib.hive_dpt_head_tail(h, p, code, 4, 8, None, 0, wp, 0.0, 1, 1, 1.0, 0.0, None, 0.001, 10.0, None, None),
        "head_tail: NULL weight": lambda: lib.hive_dpt_head_tail(h, p, code, 4, 8, None, 0, None, 0.0, 1, 1, 1.0, 0.0, f.data_ptr(), 0.001, 10.0, None, None),
        "head_tail: NULL features": lambda: lib.hive_dpt_head_tail(h, None, code, 4, 8, None, 0, wp, 0.0, 1, 1, 1.0, 0.0, f.data_ptr(), 0.001, 10.0, None, None),
        "head_tail: dtype": lambda: lib.hive_dpt_head_tail(h, p, 99, 4, 8, None, 0, wp, 0.0, 1, 1, 1.0, 0.0, f.data_ptr(), 0.001, 10.0, None, None),
        "depth_mm_to_m: n = 0": lambda: lib.hive_depth_mm_to_m(h, u16.data_ptr(), 0, 0.001, 10.0, f.data_ptr()),
        "depth_mm_to_m: NULL input": lambda: lib.hive_depth_mm_to_m(h, None, 4, 0.001, 10.0, f.data_ptr()),
        "depth_mm_to_m: NULL output": lambda: lib.hive_depth_mm_to_m(h, u16.data_ptr(), 4, 0.001, 10.0, None),
        "layernorm: D = 128": lambda: lib.hive_vit_layernorm(h, p, code, f.data_ptr(), f.data_ptr(), p, 4, 128, 1e-6),
        "layernorm: D = 1280": lambda: lib.hive_vit_layernorm(h, p, code, f.data_ptr(), f.data_ptr(), p, 1, 1280, 1e-6),
        "group_norm: C = 24": lambda: lib.hive_nhwc_group_norm(h, p, code, 1, 4, 24, 3, p, p, 1e-5, None, 0, p),
        "group_norm: C % G": lambda: lib.hive_nhwc_group_norm(h, p, code, 1, 4, 32, 3, p, p, 1e-5, None, 0, p),
        "group_norm: tiles longer than a sample": lambda: lib.hive_nhwc_group_norm_stats(h, p, code, 1, 4, 32, 4, p, p, 1e-5, None, 0, p, f.data_ptr(), 8),
        "group_norm_relu_maxpool: in place": lambda: lib.hive_nhwc_group_norm_relu_maxpool(h, p, code, 1, 2, 2, 32, 4, p, p, 1e-5, p, None, 0),
    }
    for what, call in bad.items():
        assert call() != 0, f"{what}: accepted"
        assert lib.hive_last_error(h), f"{what}: no message"
    torch.cuda.synchronize()
    assert not bool(t.any()) and not bool(f.any()), "a rejected call wrote"
    # the context is still usable
    mm = torch.tensor([1000, 20000], dtype=torch.int16, device="cuda")
    out = torch.zeros(2, device="cuda")
    gpu_ctx.check(lib.hive_depth_mm_to_m(h, mm.data_ptr(), 2, 0.001, 10.0, out.data_ptr()))
    assert out.cpu().tolist() == [float(np.float32(0.001) * np.float32(1000)), 0.0]
