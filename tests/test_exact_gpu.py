"""Exact-integer tests of the MFMA kernels (csrc/vit.hip, conv.hip, stem.hip, gram.hip, mfma_pipe.hpp) through the C ABI and ``hive_amd.dpt.ops``.

The kernels accumulate in float32 and round once, so for the integer operands of tests/exact_reference.py (every sum of absolute terms below 2^24:
asserted by the generators) the output is fully determined -- the exact integer result rounded once to the element type -- whatever the summation
order, the split-K partition or the tile shape.  Every comparison below is ``torch.equal`` against that value, for bfloat16 and float16 alike; the two
exceptions (the GELU epilogue, the counting case of attention) state their bound.  The references are index arithmetic and float64 matmuls written in
the test tree (tests/test_exact_reference_cpu.py checks them against nested loops); nothing comes from ``hive_amd.dpt.models``.

The same holds for the persistent kernels of csrc/bneck.hip (hive_bneck_gn_conv3x3: the test supplies the GroupNorm sums, so mean and rstd are small integers of its own
choosing per image and group) and csrc/dpt_head.hip (hive_dpt_head_fused: integer inputs whose upsampled values lie on a 2^-10 grid), both through more than two trips of
their tile loops, and for hive_nhwc_upsample2x, whose un-contracted float32 arithmetic exact_reference.upsample2x_f32 restates operation by operation.

The shapes are the smallest that reach each kernel, ring depth, split and tail by the launch rules of launch_gemm / qkv_t / attention_t / launch_conv_t on
the MI355X's 256 CUs; where a case's path depends on the CU count the rule (restated in exact_reference.gemm_path / conv_path) is asserted to select it on
this device, and the context's launch counters are asserted to have moved accordingly.  A device where it does not fails -- nothing is skipped."""
import pytest
import torch
import torch.nn as nn

import exact_reference as E

pytestmark = pytest.mark.gpu

POISON = 0x7FC5  # a NaN in both element types: an element the kernel did not write fails torch.equal, a written guard element shows as other bits
GUARD = 4096     # elements behind the buffer


@pytest.fixture(params=["bfloat16", "float16"])
def half(request):
    """The 16-bit element type of the kernels under test."""
    return getattr(torch, request.param)


def _code(dtype):
    from hive_amd import _lib
    return _lib.dtype_code(dtype)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _set_env(monkeypatch, env):
    for name in ("HIVE_GEMM_TILE", "HIVE_GEMM_RING", "HIVE_SPLITK", "HIVE_CONV_DEEP", "HIVE_QKV_MERGE", "HIVE_ATT_KSPLIT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_references():
    """The shared references (about 1 GB of float64 on the device) go back to the allocator when this module is done."""
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _cached(key, make):
    """References and operands are computed once and shared by the element types and epilogues (never modified)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _poisoned(elements, dtype):
    buf = torch.full((elements,), POISON, dtype=torch.int16, device="cuda")
    return buf, buf.view(dtype)


def _untouched(buf, start):
    return bool((buf[start:] == POISON).all())


def _dev(t, dtype):
    return t.to(device="cuda", dtype=dtype)


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_vit_linear

def _gemm_case(M, N, K):
    def make():
        A, W, bias, res, _ = E.gemm_operands(M, N, K)
        A, W, bias, res = A.cuda(), W.cuda(), bias.cuda(), res.cuda()
        return A, W, bias, res, E.gemm_exact(A, W, bias), E.gemm_exact(A, W, bias, res)
    return _cached(("gemm", M, N, K), make)


def _linear(ctx, half, A, W, bias, residual, M, N, K, epi, in_place=False):
    """One launch into a poisoned buffer with rows beyond M and a guard region behind; asserts that only the M rows were written."""
    rows = (M + 255) // 256 * 256 + 128
    buf, C = _poisoned(rows * N + GUARD, half)
    if in_place:
        C[:M * N] = residual.reshape(-1)
    res_ptr = None if epi != 2 else (C.data_ptr() if in_place else residual.data_ptr())
    ctx.check(ctx.lib.hive_vit_linear(ctx.handle, A.data_ptr(), _code(half), W.data_ptr(), bias.data_ptr(), res_ptr, C.data_ptr(), M, N, K, epi))
    torch.cuda.synchronize()
    assert _untouched(buf, M * N), "rows beyond M or the guard region were written"
    return C[:M * N].view(M, N)


def _assert_gemm_path(ctx, M, N, K, env, before, launches):
    """The launch rule selects the intended kernel on this device, and the counters moved as that rule says."""
    path = E.gemm_path(M, N, K, _cus(), env)
    assert path == E.gemm_path(M, N, K, 256, env), f"{_cus()} CUs: the rule selects {path}, the case was chosen for {E.gemm_path(M, N, K, 256, env)}"
    after = ctx.launch_stats()
    split, deep = (path[1] > 1, path[2]) if path[0] == "tile128" else (False, False)
    assert after[0] - before[0] == (launches if split else 0), f"split-K launches {after[0] - before[0]}, path {path}"
    assert after[1] - before[1] == (launches if deep else 0), f"deep-ring launches {after[1] - before[1]}, path {path}"
    return path


@pytest.mark.parametrize("M,N,K,env", E.LINEAR_CASES, ids=lambda v: "-".join(f"{k[5:]}={x}" for k, x in v.items()) or "policy" if isinstance(v, dict) else str(v))
def test_linear_exact(gpu_ctx, half, monkeypatch, M, N, K, env):
    """Epilogues 0 (bias) and 2 (bias + residual), and 2 in place as the model runs it (x += proj(...)): bit for bit."""
    A64, W64, bias64, res64, exact0, exact2 = _gemm_case(M, N, K)
    A, W, res, bias = A64.to(half), W64.to(half), res64.to(half), bias64.float()
    _set_env(monkeypatch, env)
    before = gpu_ctx.launch_stats()
    out0 = _linear(gpu_ctx, half, A, W, bias, None, M, N, K, 0)
    out2 = _linear(gpu_ctx, half, A, W, bias, res, M, N, K, 2)
    out2i = _linear(gpu_ctx, half, A, W, bias, res, M, N, K, 2, in_place=True)
    path = _assert_gemm_path(gpu_ctx, M, N, K, env, before, 3)
    if (M, N, K) == (9800, 2048, 64):
        assert path[0] == "tile256" and path[1] > _cus() // 8 * 8 and M % 256, "more tiles than persistent workgroups, ragged last row tile"
    assert torch.equal(out0, E.round_once(exact0, half)), f"epilogue 0: {int((out0 != E.round_once(exact0, half)).sum())} elements differ"
    want2 = E.round_once(exact2, half)
    assert torch.equal(out2, want2), f"epilogue 2: {int((out2 != want2).sum())} elements differ"
    assert torch.equal(out2i, want2), f"epilogue 2 in place: {int((out2i != want2).sum())} elements differ"


@pytest.mark.parametrize("M,N,K,env", E.GELU_CASES, ids=lambda v: "-".join(f"{k[5:]}={x}" for k, x in v.items()) or "policy" if isinstance(v, dict) else str(v))
def test_linear_gelu_bound(gpu_ctx, half, monkeypatch, M, N, K, env):
    """Epilogue 1 cannot be bit-exact: against float64 erf-GELU of the exact pre-activation (all in -8..8), within half a unit in the last place of the
    element type at that value (the one rounding) plus 6e-7, the absolute error the kernel states for its GELU (vit.hip gelu_exact2, tools/fit_gelu.py)."""
    def make():
        A, W, bias, _ = E.gelu_operands(M, N, K)
        A, W, bias = A.cuda(), W.cuda(), bias.cuda()
        return A, W, bias, E.gelu64(E.gemm_exact(A, W, bias))
    A64, W64, bias64, want = _cached(("gelu", M, N, K), make)
    A, W, bias = A64.to(half), W64.to(half), bias64.float()
    assert torch.equal(A.double(), A64) and torch.equal(W.double(), W64) and torch.equal(bias.double(), bias64), "operands must be exact in the element type"
    _set_env(monkeypatch, env)
    before = gpu_ctx.launch_stats()
    out = _linear(gpu_ctx, half, A, W, bias, None, M, N, K, 1)
    _assert_gemm_path(gpu_ctx, M, N, K, env, before, 1)
    err = (out.double() - want).abs()
    bound = 0.5 * E.ulp(want, half) + 6e-7
    worst = (err - bound).max().item()
    print(f"gelu {M} x {N} x {K} {half}: max error {err.max().item():.3e}, max (error - bound) {worst:.3e}")
    assert torch.isfinite(out).all() and bool((err <= bound).all()), f"{int((err > bound).sum())} elements outside the bound, worst by {worst:.3e}"


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_vit_qkv

def _qkv_exact(ctx, half, monkeypatch, B, N, D, H, modes):
    """hive_vit_qkv under each HIVE_QKV_MERGE mode against the exact q | k and v^T; the launch counters against qkv_t's rule restated here."""
    def make():
        x, W, bias, Np, _ = E.qkv_operands(B, N, D)
        x, W, bias = x.cuda(), W.cuda(), bias.cuda()
        exact = E.gemm_exact(x.reshape(B * Np, D), W, bias)
        return x, W, bias, Np, exact
    x64, W64, bias64, Np, exact = _cached(("qkv", B, N, D), make)
    x, W, bias = x64.to(half), W64.to(half), bias64.float()
    want_qk = torch.cat([E.q_expected(exact[:, :D], half).cuda(), E.round_once(exact[:, D:2 * D], half)], dim=1)
    want_vT = E.vt_store(E.round_once(exact[:, 2 * D:], half), B, Np, H)
    M, cus = B * Np, _cus()
    tiles_all = -(-M // 128) * (3 * D // 128)
    forms = {}
    for mode in modes:
        _set_env(monkeypatch, {} if mode is None else {"HIVE_QKV_MERGE": mode})
        qk_buf, qk = _poisoned(M * 2 * D + GUARD, half)
        vT_buf, vT = _poisoned(M * D + GUARD, half)
        before = ctx.launch_stats()
        ctx.check(ctx.lib.hive_vit_qkv(ctx.handle, x.data_ptr(), _code(half), W.data_ptr(), bias.data_ptr(), qk.data_ptr(), vT.data_ptr(), B, Np, D, H))
        torch.cuda.synchronize()
        after = ctx.launch_stats()
        merged = mode != "0" and tiles_all <= ((2 * cus) // 8 * 8 if mode == "2" else cus)
        if merged:  # one launch of gemm_kernel<EPI_QKV_ALL>: the four-stage ring where the tiles fit the CUs, else the two-stage one; never split
            forms[mode] = "merged, deep ring" if tiles_all <= cus else "merged, two-stage ring"
            assert after[1] - before[1] == int(tiles_all <= cus) and after[0] == before[0], f"HIVE_QKV_MERGE={mode}: counters {before} -> {after}"
        else:  # two launches through launch_gemm: q | k (N = 2 D) and v^T (N = D)
            forms[mode] = "two launches"
            paths = [E.gemm_path(M, 2 * D, D, cus, {}), E.gemm_path(M, D, D, cus, {})]
            assert after[1] - before[1] == sum(int(p[0] == "tile128" and p[2]) for p in paths), f"HIVE_QKV_MERGE={mode}: counters {before} -> {after}"
            assert after[0] - before[0] == sum(int(p[0] == "tile128" and p[1] > 1) for p in paths), f"HIVE_QKV_MERGE={mode}: counters {before} -> {after}"
        assert _untouched(qk_buf, M * 2 * D) and _untouched(vT_buf, M * D), f"HIVE_QKV_MERGE={mode}: guard region written"
        got_qk, got_vT = qk[:M * 2 * D].view(M, 2 * D), vT[:M * D].view(B, H, 64, Np)
        assert torch.equal(got_qk[:, :D], want_qk[:, :D]), f"HIVE_QKV_MERGE={mode}: q, {int((got_qk[:, :D] != want_qk[:, :D]).sum())} elements differ"
        assert torch.equal(got_qk[:, D:], want_qk[:, D:]), f"HIVE_QKV_MERGE={mode}: k, {int((got_qk[:, D:] != want_qk[:, D:]).sum())} elements differ"
        assert torch.equal(got_vT, want_vT), f"HIVE_QKV_MERGE={mode}: v^T, {int((got_vT != want_vT).sum())} elements differ"
    return forms


@pytest.mark.parametrize("B,N,D,H", E.QKV_CASES)
def test_qkv_exact(gpu_ctx, half, monkeypatch, B, N, D, H):
    """q | k and v^T bit for bit -- q as float32(exact) * float32(head_dim^-0.5 log2 e) rounded once, v^T in its stored token order -- for the merged
    launch (one workgroup per CU, four-stage ring) and the two launches (HIVE_QKV_MERGE=0).  HIVE_QKV_MERGE=2 runs too, but at these shapes (all tiles fit
    the CUs: asserted) it is the same merged launch as the default; the form it adds is test_qkv_exact_two_workgroups_per_cu's."""
    forms = _qkv_exact(gpu_ctx, half, monkeypatch, B, N, D, H, (None, "0", "2"))
    assert forms == {None: "merged, deep ring", "0": "two launches", "2": "merged, deep ring"}, f"{_cus()} CUs: {forms}"


def test_qkv_exact_two_workgroups_per_cu(gpu_ctx, half, monkeypatch):
    """More tiles than CUs, at most two workgroups per CU (2 x 1201 tokens: 19 x 18 = 342 tiles): HIVE_QKV_MERGE=2 merges q | k and v^T into one launch of
    gemm_kernel<EPI_QKV_ALL> on the TWO-stage ring, the default runs two launches; both bit for bit."""
    B, N, D, H = E.QKV_TWO_PER_CU_CASE
    forms = _qkv_exact(gpu_ctx, half, monkeypatch, B, N, D, H, (None, "2"))
    assert forms == {None: "two launches", "2": "merged, two-stage ring"}, f"{_cus()} CUs: {forms}"


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_vit_attention

def _attention_form(Np, ksplit):
    """attention_t splits the keys two ways (attention_kernel<T, 2>) only from four key tiles on: of the issue's shapes 1201 and 577 tokens reach it under
    HIVE_ATT_KSPLIT=1; 77, 64 and 130 tokens (2, 1 and 3 tiles) run attention_kernel<T, 1> under either setting."""
    return 2 if ksplit == "1" and Np // 64 >= 4 else 1


def _attention(ctx, half, qk, vT, B, N, Np, D, H):
    buf, out = _poisoned(B * Np * D + GUARD, half)
    ctx.check(ctx.lib.hive_vit_attention(ctx.handle, qk.data_ptr(), _code(half), vT.data_ptr(), out.data_ptr(), B, N, Np, D, H))
    torch.cuda.synchronize()
    assert _untouched(buf, B * Np * D), "guard region written"
    return out[:B * Np * D].view(B, Np, D)[:, :N]


@pytest.mark.parametrize("ksplit", ["0", "1"])
@pytest.mark.parametrize("B,N,D,H", E.ATTENTION_CASES)
def test_attention_selection_exact(gpu_ctx, half, monkeypatch, B, N, D, H, ksplit):
    """Every (head, query) selects one key (score 0, every other key <= -256: weight exactly 0, l = 1): the output is that key's v bit for bit, for
    every real query, head and channel.  Padded key rows repeat real keys' codes (a broken mask doubles l), head 0's targets run backwards (the maximum
    rises at the last key tile: the rescale branch), and with the keys split two ways targets fall in both halves."""
    Np = (N + 63) // 64 * 64
    qk64, v64, want64, perm = _cached(("att-sel", B, N, H), lambda: E.attention_selection(B, N, H))
    n_tiles = Np // 64
    if n_tiles >= 4:
        first_half = (n_tiles + 1) // 2 * 64
        for b in range(B):
            for h in range(H):
                assert bool((perm[b, h] < first_half).any()) and bool((perm[b, h] >= first_half).any()), "targets must fall in both key halves"
    late = perm[:, 0, :32]
    assert bool((late >= max(0, N - 64)).all()), "head 0: the first queries' targets sit in the last key tile"
    qk, vT = _dev(qk64, half), _dev(E.vt_store(v64, B, Np, H), half)
    assert torch.equal(qk.cpu().long(), qk64), "operands must be exact in the element type"
    assert _attention_form(Np, ksplit) == (2 if ksplit == "1" and N in (1201, 577) else 1), "the split kernel at 1201 and 577 tokens only"
    _set_env(monkeypatch, {"HIVE_ATT_KSPLIT": ksplit})
    out = _attention(gpu_ctx, half, qk, vT, B, N, Np, D, H)
    want = _dev(want64, half)
    assert torch.equal(out, want), f"{int((out != want).sum())} of {want.numel()} elements differ"


@pytest.mark.parametrize("ksplit", ["0", "1"])
@pytest.mark.parametrize("B,N,D,H", E.ATTENTION_CASES)
def test_attention_counting(gpu_ctx, half, monkeypatch, B, N, D, H, ksplit):
    """q' = 0: every real key weighs 1, l = N, and with v[j][c] = 127 [j = c mod D] the output is 127 count_c / N -- a key counted twice or dropped moves a
    column by a factor of at least 1.5.  Bound: one unit in the last place of the element type (the float32 1 / l, the multiply and the final rounding)."""
    Np = (N + 63) // 64 * 64
    qk64, v64, want = _cached(("att-count", B, N, H), lambda: E.attention_counting(B, N, H))
    qk, vT = _dev(qk64, half), _dev(E.vt_store(v64, B, Np, H), half)
    assert _attention_form(Np, ksplit) == (2 if ksplit == "1" and N in (1201, 577) else 1), "the split kernel at 1201 and 577 tokens only"
    _set_env(monkeypatch, {"HIVE_ATT_KSPLIT": ksplit})
    out = _attention(gpu_ctx, half, qk, vT, B, N, Np, D, H).double()
    want = want.cuda().expand(B, N, D)
    err = (out - want).abs()
    bound = E.ulp(want, half) * (want != 0)
    print(f"attention counting {B} x {N} {half} ksplit {ksplit}: max error {err.max().item():.3e} (in ulp: {(err / E.ulp(want, half)).max().item():.3f})")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements beyond one ulp, max {err.max().item():.3e}"


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_nhwc_conv3x3 / hive_nhwc_conv

def _nchw(t_nhwc, dtype):
    """[n][h][w][c] on any device -> the channels-last [n, c, h, w] CUDA tensor the ops take."""
    return t_nhwc.to(device="cuda", dtype=dtype).permute(0, 3, 1, 2)


def _conv_module(cin, cout, k, s, padding, wt64, bias64, half):
    conv = nn.Conv2d(cin, cout, k, s, 0 if padding == "same" else padding, bias=True)
    with torch.no_grad():
        conv.weight.copy_(wt64.double())
        conv.bias.copy_(bias64.double())
    return conv.to(memory_format=torch.channels_last).to(half).cuda()


def _conv_case(case, r=4, p_zero=None):
    def make():
        n, cin, cout, k, s, h, w, padding = case[:8]
        pt, pl, oh, ow = E.conv_geometry(k, s, h, w, padding)
        x, wt, bias, r1, r2, _ = E.case_conv_operands(case, r=r, p_zero=p_zero)
        xd, wd = x.cuda(), wt.cuda()
        plain = E.conv_exact(xd, wd, s, pt, pl, oh, ow)
        return x, wt, bias, r1, r2, plain
    return _cached(("conv", r) + tuple(case[:8]), make)


def _run_conv(x, conv, wt, k, s, padding, **kw):
    from hive_amd.dpt import ops
    if k == 3 and s == 1 and padding == 1 and conv.out_channels % 128 == 0:
        return ops.conv3x3(x, conv, **kw)  # hive_nhwc_conv3x3
    return ops.conv2d(x, conv, weight=wt, same_pad=padding == "same", **kw)  # hive_nhwc_conv


def _assert_conv_path(ctx, case, before, launches):
    n, cin, cout, k, s, h, w, padding, env, expected = case
    _, _, oh, ow = E.conv_geometry(k, s, h, w, padding)
    path = E.conv_path(n * oh * ow, cin, cout, k, _cus(), env)
    if expected is not None:
        assert path == expected, f"{_cus()} CUs: the rule selects {path}, the case was chosen for {expected}"
    after = ctx.launch_stats()
    assert after[1] - before[1] == (launches if path[0] == "deep" else 0), f"deep-ring launches {after[1] - before[1]}, path {path}"
    assert after[0] - before[0] == (launches if path[0] == "deep" and path[1] > 1 else 0), f"split-K launches {after[0] - before[0]}, path {path}"


def _case_id(v):
    if isinstance(v, dict):
        return "-".join(f"{k[5:]}={x}" for k, x in v.items()) or "policy"
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("case", E.CONV_CASES, ids=lambda c: "-".join(_case_id(v) for v in c[:9]))
def test_conv_exact(gpu_ctx, half, monkeypatch, case):
    """Every case with a plain epilogue, bias + ReLU, and bias + two shortcuts with the ReLU copy: bit for bit, and out_relu == relu(out)."""
    n, cin, cout, k, s, h, w, padding, env, _ = case
    x64, wt64, bias64, r1_64, r2_64, plain = _conv_case(case)
    conv = _conv_module(cin, cout, k, s, padding, wt64, bias64, half)
    x, wt = _nchw(x64, half), conv.weight
    assert wt.is_contiguous(memory_format=torch.channels_last) and torch.equal(x.permute(0, 2, 3, 1).cpu().long(), x64)
    r1, r2 = _nchw(r1_64, half), _nchw(r2_64, half)
    biased = plain + bias64.cuda().double()
    _set_env(monkeypatch, env)
    before = gpu_ctx.launch_stats()
    got_plain = _run_conv(x, conv, wt, k, s, padding, with_bias=False)
    got_relu = _run_conv(x, conv, wt, k, s, padding, relu=True)
    got_sum, got_sum_relu = _run_conv(x, conv, wt, k, s, padding, residual=r1, residual2=r2, also_relu=True)
    torch.cuda.synchronize()
    _assert_conv_path(gpu_ctx, case, before, 3)

    def same(got, exact, what):
        want = E.round_once(exact, half).permute(0, 3, 1, 2)
        assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} elements differ"

    same(got_plain, plain, "plain")
    same(got_relu, biased.clamp_min(0.0), "bias + ReLU")
    total = biased + r1_64.cuda().double() + r2_64.cuda().double()
    same(got_sum, total, "bias + two shortcuts")
    same(got_sum_relu, total.clamp_min(0.0), "ReLU copy")
    assert torch.equal(got_sum_relu, torch.relu(got_sum)), "out_relu must be relu(out)"


def _tile_part_sums(rows, hw, tile_rows):
    """Integer sums and sums of squares of the stored rows [M][C] per (tile, image half): [tiles][2][2][C] float64, the partial layout of the epilogue
    (as tests/test_conv_gpu.py decodes it: per tile, the rows of the image the tile starts in, then those of the next image)."""
    m, c = rows.shape
    r = torch.arange(m, device=rows.device)
    tile = r // tile_rows
    part = r // hw - (tile * tile_rows) // hw
    assert int(part.max()) <= 1
    n_tiles = (m + tile_rows - 1) // tile_rows
    out = torch.zeros(n_tiles * 2, 2, c, dtype=torch.float64, device=rows.device)
    out[:, 0].index_add_(0, tile * 2 + part, rows)
    out[:, 1].index_add_(0, tile * 2 + part, rows * rows)
    return out.view(n_tiles, 2, 2, c)


@pytest.mark.parametrize("case", E.CONV_STATS_CASES, ids=lambda c: "-".join(_case_id(v) for v in c[:9]))
def test_conv_group_norm_sums_exact(gpu_ctx, half, monkeypatch, case):
    """GroupNorm statistics from the epilogue (conv_kernel with 128- and 256-row tiles, conv_deep_kernel): the stored outputs bit for bit, and the partial
    sums and sums of squares equal to the integer sums of the stored outputs exactly (operands in -2..2: every sum of squares below 2^24, asserted)."""
    from hive_amd.dpt import ops
    n, cin, cout, k, s, h, w, padding, env, path_expected, tile_rows_expected = case
    x64, wt64, bias64, _, _, plain = _conv_case(case, r=2, p_zero=0.1)
    conv = _conv_module(cin, cout, k, s, padding, wt64, bias64, half)
    x = _nchw(x64, half)
    _set_env(monkeypatch, env)
    before = gpu_ctx.launch_stats()
    out = ops.conv2d(x, conv, weight=conv.weight, same_pad=padding == "same", gn_stats=True)
    partial, tile_rows = out.hive_gn_stats
    torch.cuda.synchronize()
    _assert_conv_path(gpu_ctx, case[:9] + (path_expected,), before, 1)  # the rule reaches the intended kernel on this device, and the deep-ring counter says so
    assert tile_rows == tile_rows_expected, f"statistics over {tile_rows}-row tiles, the case was chosen for {tile_rows_expected} ({_cus()} CUs)"
    want = E.round_once(plain + bias64.cuda().double(), half).permute(0, 3, 1, 2)
    assert torch.equal(out, want), f"{int((out != want).sum())} elements differ"
    rows = out.permute(0, 2, 3, 1).reshape(-1, cout).double()
    sums = _tile_part_sums(rows, out.shape[2] * out.shape[3], tile_rows)
    assert float(sums[:, :, 1].max()) < E.LIMIT and float(sums[:, :, 0].abs().max()) < E.LIMIT
    got = partial[: sums.shape[0] * 4 * cout].view(sums.shape[0], 2, 2, cout).double()
    assert torch.equal(got, sums), f"{int((got != sums).sum())} partial sums differ, max by {(got - sums).abs().max().item()}"


# ------------------------------------------------------------------------------------------------------------------------------------
# stem, patch embedding, transposed convolution

@pytest.mark.parametrize("n,h,w", E.STEM_CASES)
def test_stem_conv_exact(gpu_ctx, half, n, h, w):
    """The 7 x 7 / 2 "SAME" convolution of the 3-channel frame (csrc/stem.hip) with integer weights, and the GroupNorm sums its epilogue leaves."""
    from hive_amd.dpt import ops
    x64, wt64, _ = E.stem_operands(n, h, w)
    (oh, pt), (ow, pl) = E.same_geometry(h, 7, 2), E.same_geometry(w, 7, 2)
    want = E.round_once(E.conv_exact(x64.cuda(), wt64.cuda(), 2, pt, pl, oh, ow), half).permute(0, 3, 1, 2)
    conv = nn.Conv2d(3, 64, 7, 2, bias=False)
    weight = wt64.to(device="cuda", dtype=half)
    out = ops.stem_conv(_nchw(x64, half), conv, weight)
    assert out.shape == want.shape and torch.equal(out, want), f"{int((out != want).sum())} of {want.numel()} elements differ"
    stats = getattr(out, "hive_gn_stats", None)
    assert (stats is not None) == (oh % 8 == 0 and ow % 32 == 0)
    if stats is not None:  # 8 x 32 tiles in row-major order, `run` consecutive tiles of one image per row of the partials
        partial, tile_rows = stats
        run = tile_rows // 256
        n_runs = (oh // 8) * (ow // 32) // run
        tiles = out.permute(0, 2, 3, 1).double().view(n, oh // 8, 8, ow // 32, 32, 64).permute(0, 1, 3, 2, 4, 5).reshape(n, n_runs, run * 256, 64)
        got = partial[: n * n_runs * 4 * 64].view(n, n_runs, 2, 2, 64).double()
        assert float((tiles ** 2).sum(2).max()) < E.LIMIT
        assert torch.equal(got[:, :, 0, 0], tiles.sum(2)) and torch.equal(got[:, :, 0, 1], (tiles ** 2).sum(2)) and float(got[:, :, 1].abs().max()) == 0.0


@pytest.mark.parametrize("n,h,w,D", E.PATCH_CASES)
def test_patch_embed_exact(gpu_ctx, half, n, h, w, D):
    """16 x 16 patches to rows (hive_patch_rows) and the GEMM: bit for bit."""
    from hive_amd.dpt import ops
    x64, wt64, bias64, _, _, _ = E.conv_operands(n, 3, D, 16, h, w, h // 16, w // 16)
    pe = nn.Conv2d(3, D, 16, 16)
    with torch.no_grad():
        pe.weight.copy_(wt64.double())
        pe.bias.copy_(bias64.double())
    pe = pe.to(memory_format=torch.channels_last).to(half).cuda()
    x = _nchw(x64, half)
    assert ops.patch_embed_eligible(x, pe)
    tok = ops.patch_embed(x, pe)
    want = E.round_once(E.patch_embed_exact(x64.cuda(), wt64.cuda(), bias64.cuda()), half)
    assert tok.shape == want.shape and torch.equal(tok, want), f"{int((tok != want).sum())} of {want.numel()} elements differ"


@pytest.mark.parametrize("n,cin,cout,s,h,w", E.CONV_TRANSPOSE_CASES)
def test_conv_transpose_exact(gpu_ctx, half, n, cin, cout, s, h, w):
    """ConvTranspose2d with kernel == stride 4 and 2: the 1 x 1 convolution to (dy, dx, co) channels (its result exact in the element type: the
    generator asserts |sum| <= 256) and the pixel shuffle with bias, bit for bit."""
    from hive_amd.dpt import ops
    x64, wt64, bias64, _ = E.conv_transpose_operands(n, cin, cout, s, h, w)
    ct = nn.ConvTranspose2d(cin, cout, s, s, 0, bias=True)
    with torch.no_grad():
        ct.weight.copy_(wt64.double())
        ct.bias.copy_(bias64.double())
    ct = ct.to(half).cuda()
    x = _nchw(x64, half)
    assert ops.conv_transpose_eligible(x, ct)
    out = ops.conv_transpose(x, ct)
    parts = E.conv_transpose_parts(x64.cuda(), wt64.cuda())
    assert torch.equal(E.round_once(parts, half).double(), parts), "the intermediate must be exact in the element type"
    want = E.round_once(E.pixel_shuffle(parts, bias64.cuda()), half).permute(0, 3, 1, 2)
    assert out.shape == want.shape and torch.equal(out, want), f"{int((out != want).sum())} of {want.numel()} elements differ"


# ------------------------------------------------------------------------------------------------------------------------------------
# Gram matrices

@pytest.mark.parametrize("n,cin,cout,stride,h,w", E.GRAM_CASES)
def test_gram_parts_exact(gpu_ctx, half, n, cin, cout, stride, h, w):
    """hive_gn_gram_stats with d_S_out / d_s_out: the parts, summed over ``parts``, equal the integer X^T X and sum x per image exactly."""
    from hive_amd import _lib
    oh, ow = (h + stride - 1) // stride, (w + stride - 1) // stride
    x64, _ = E.gram_operands(n, cin, h, w, oh, ow)
    g = torch.Generator(device="cpu").manual_seed(cin + cout)
    wt = E.draw(g, (cout, cin, 1, 1), 4).to(device="cuda", dtype=half).contiguous(memory_format=torch.channels_last)
    x = _nchw(x64, half)
    ctx, lib, G = gpu_ctx, gpu_ctx.lib, 32
    tables = torch.empty(int(lib.hive_gn_gram_table_floats(cin, G)), dtype=torch.float32, device="cuda")
    ctx.check(lib.hive_gn_gram_prepare(ctx.handle, wt.data_ptr(), _lib.dtype_code(half), cin, cout, G, tables.data_ptr()))
    parts = int(lib.hive_gn_gram_parts(ctx.handle, n, cin, oh, ow))
    assert parts >= 1
    S = torch.full((n, parts, cin, cin), float("nan"), dtype=torch.float32, device="cuda")
    s = torch.full((n, parts, cin), float("nan"), dtype=torch.float32, device="cuda")
    stats = torch.empty(n, G, 2, dtype=torch.float32, device="cuda")
    ctx.check(lib.hive_gn_gram_stats(ctx.handle, x.data_ptr(), _lib.dtype_code(half), n, h, w, cin, cout, stride, oh, ow, G, tables.data_ptr(), 1e-5,
                                     stats.data_ptr(), S.data_ptr(), s.data_ptr()))
    torch.cuda.synchronize()
    S_want, s_want = E.gram_exact(x64.cuda(), stride)
    assert torch.equal(S.double().sum(1), S_want), f"X^T X: max difference {(S.double().sum(1) - S_want).abs().max().item()}"
    assert torch.equal(s.double().sum(1), s_want), f"sum x: max difference {(s.double().sum(1) - s_want).abs().max().item()}"


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_bneck_gn_conv3x3 (csrc/bneck.hip) through the C ABI: the test supplies the GroupNorm sums, so the statistics are its own

SENTINEL = -123456.0  # float buffers the kernel may not write


def _bneck_case(case):
    """The operands (CPU, int64 / float64) and the exact convolution float64 [n][h][w][64] on the device, computed 16 images at a time."""
    def make():
        n = E.bneck_batch(case, _cus())
        t, partial, tile_rows, gamma, beta, wt, a, b, _ = E.bneck_operands(n, *case[1:])
        exact = E.conv3x3_exact(E.bneck_normalised(t.cuda(), a, b), wt)
        return n, t, partial, tile_rows, gamma, beta, wt, exact
    return _cached(("bneck",) + tuple(case), make)


def _bneck(ctx, half, t, partial, tile_rows, gamma, beta, w, n, h, wd, C=64, eps=E.BNECK_EPS):
    """One call into a poisoned output and a sentinel-filled buffer for the sums, both with a guard region behind.  -> (out buffer (int16 view), out, sums, tile rows, fused)"""
    import ctypes
    tiles = n * E.bneck_tiles(h, wd)[0]
    buf, out = _poisoned(n * h * wd * 64 + GUARD, half)
    sums = torch.full((tiles * 4 * 64 + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    rows, fused = ctypes.c_int(-1), ctypes.c_int(-1)
    ctx.check(ctx.lib.hive_bneck_gn_conv3x3(ctx.handle, t.data_ptr(), _code(half), n, h, wd, C, None if partial is None else partial.data_ptr(), tile_rows,
                                            gamma.data_ptr(), beta.data_ptr(), eps, w.data_ptr(), out.data_ptr(), sums.data_ptr(), tiles * 4 * 64,
                                            ctypes.byref(rows), ctypes.byref(fused)))
    torch.cuda.synchronize()
    return buf, out, sums, rows.value, fused.value


@pytest.mark.parametrize("case", E.BNECK_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_bneck_exact(gpu_ctx, half, case):
    """conv2(relu(norm1(t))) bit for bit: round_once of the integer convolution of u = relu(t a + b) with zero padding, for statistics that differ from image to
    image (so a neighbouring image's a, b -- or a normalised zero in the padding -- gives other integers), through more than two trips of the tile loop.  Where the
    kernel leaves GroupNorm sums, row ``tile`` holds exactly the integer sum and sum of squares of THAT tile's stored outputs; where not, it writes none."""
    n, t64, partial64, tile_rows, gamma64, beta64, wt64, exact = _bneck_case(case)
    h, w = case[1:3]
    cus, (per, _) = _cus(), E.bneck_tiles(h, w)
    tiles = n * per
    if case[0] is None:  # the premise, on this device: grid = min(tiles, CUs)
        print(f"  premise: {tiles} tiles on {cus} workgroups: {tiles - 2 * cus} of them make three trips, the rest two; trips {cus // per} images apart")
        assert 2 * cus < tiles < 3 * cus and cus % per == 0 and (cus // per) % 5 != 0, "three and two trips, consecutive trips in images with other statistics"
    t, gamma, beta = _dev(t64, half), _dev(gamma64, half), _dev(beta64, half)
    wgt = _dev(wt64.permute(0, 2, 3, 1).contiguous(), half)  # [co][(ky, kx, ci)]
    partial = partial64.to(device="cuda", dtype=torch.float32)
    buf, out, sums, rows, fused = _bneck(gpu_ctx, half, t, partial, tile_rows, gamma, beta, wgt, n, h, w)
    assert fused == 1
    assert _untouched(buf, n * h * w * 64), "the guard region behind the output was written"
    got, want = out[:n * h * w * 64].view(n, h, w, 64), E.round_once(exact, half)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} outputs differ, first in image {int((got != want).reshape(n, -1).any(1).nonzero()[0])}"
    if E.bneck_has_sums(h, w):
        assert rows == h * w // per
        stored = E.bneck_tile_sums(want.double(), h, w)  # [tiles][2][64]
        assert float(stored[:, 1].max()) < E.LIMIT and float(stored[:, 0].abs().max()) < E.LIMIT, "a tile's sum is not exact in float32"
        left = sums[:tiles * 4 * 64].view(tiles, 2, 2, 64).double()
        assert torch.equal(left[:, 0], stored), f"{int((left[:, 0] != stored).sum())} sums differ, first in tile {int((left[:, 0] != stored).reshape(tiles, -1).any(1).nonzero()[0])}"
        assert float(left[:, 1].abs().max()) == 0.0, "the h = 1 half must be zero"
        assert bool((sums[tiles * 4 * 64:] == SENTINEL).all()), "the guard region behind the sums was written"
    else:
        assert rows == 0 and bool((sums == SENTINEL).all()), "no sums are left here: the buffer must stay untouched"


def test_bneck_not_eligible_writes_nothing(gpu_ctx, half):
    """C != 64, no input sums, or no tile rows: *fused == 0, *gn_tile_rows == 0, and neither the output nor the sums are touched."""
    case = E.BNECK_CASES[2]
    n, t64, partial64, tile_rows, gamma64, beta64, wt64, _ = _bneck_case(case)
    h, w = case[1:3]
    t, gamma, beta, wgt = _dev(t64, half), _dev(gamma64, half), _dev(beta64, half), _dev(wt64.permute(0, 2, 3, 1).contiguous(), half)
    partial = partial64.to(device="cuda", dtype=torch.float32)
    for what, kw in (("C = 32", dict(partial=partial, tile_rows=tile_rows, C=32)), ("NULL d_in_partial", dict(partial=None, tile_rows=tile_rows)),
                     ("in_tile_rows = 0", dict(partial=partial, tile_rows=0)), ("in_tile_rows = -1", dict(partial=partial, tile_rows=-1))):
        buf, _, sums, rows, fused = _bneck(gpu_ctx, half, t, kw["partial"], kw["tile_rows"], gamma, beta, wgt, n, h, w, C=kw.get("C", 64))
        assert fused == 0 and rows == 0, what
        assert _untouched(buf, 0) and bool((sums == SENTINEL).all()), f"{what}: a buffer was written"


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_nhwc_upsample2x (csrc/dpt_ops.hip): both forms against the float32 restatement

@pytest.mark.parametrize("N,C,H,W", E.UPSAMPLE_CASES)
def test_upsample2x_bit_exact(gpu_ctx, half, monkeypatch, N, C, H, W):
    """The LDS-tile form (C <= 512) and the gather form (HIVE_UPSAMPLE_GATHER, and C = 1024 by the rule), with and without the folded bias: equal to
    exact_reference.upsample2x_f32 bit for bit -- small values, exact zeros and values next to the largest finite one included."""
    x, bias = E.upsample_operands(N, C, H, W, half)
    xd, bd = x.cuda(), bias.cuda()
    n_out = N * 4 * H * W * C
    for with_bias in (False, True):
        want = _cached(("up", N, C, H, W, half, with_bias), lambda: E.upsample2x_f32(x, bias if with_bias else None).cuda())
        for gather in (False, True):
            if gather:
                monkeypatch.setenv("HIVE_UPSAMPLE_GATHER", "1")
            else:
                monkeypatch.delenv("HIVE_UPSAMPLE_GATHER", raising=False)
            buf, out = _poisoned(n_out + GUARD, half)
            gpu_ctx.check(gpu_ctx.lib.hive_nhwc_upsample2x(gpu_ctx.handle, xd.data_ptr(), bd.data_ptr() if with_bias else None, _code(half), N, H, W, C, out.data_ptr()))
            torch.cuda.synchronize()
            assert _untouched(buf, n_out), "guard region written"
            got = out[:n_out].view(N, 2 * H, 2 * W, C)
            what = f"{'gather' if gather or C > 512 else 'LDS tile'} form, {'with' if with_bias else 'no'} bias"
            assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {n_out} elements differ"


# ------------------------------------------------------------------------------------------------------------------------------------
# hive_dpt_head_fused (csrc/dpt_head.hip)

def _head_case(case):
    def make():
        N = E.head_batch(case, _cus())
        return (N,) + E.head_operands(N, case[1], case[2])
    return _cached(("head",) + tuple(case[:3]), make)


def _head(ctx, half, x, b0, w3, b3, w1, b1, N, H, W, non_negative, invert, outputs=(True, True, True)):
    """One call; the outputs not requested are passed as NULL and stay sentinel-filled, a guard region behind each stays untouched.  -> (depth, mm, m) numpy"""
    n_px = N * 4 * H * W
    depth = torch.full((n_px + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    mm = torch.full((n_px + GUARD,), 0x5A5A, dtype=torch.int16, device="cuda")
    m = torch.full((n_px + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    ptr = [b.data_ptr() if on else None for b, on in zip((depth, mm, m), outputs)]
    ctx.check(ctx.lib.hive_dpt_head_fused(ctx.handle, x.data_ptr(), None if b0 is None else b0.data_ptr(), _code(half), N, H, W, 128, 32, w3.data_ptr(), b3.ctypes.data,
                                          w1.ctypes.data, float(b1), int(non_negative), int(invert), E.HEAD_SCALE, E.HEAD_SHIFT, ptr[0], E.HEAD_DEPTH_SCALE,
                                          E.HEAD_MAX_DEPTH, ptr[1], ptr[2]))
    torch.cuda.synchronize()
    for buf, on, fill in ((depth, outputs[0], SENTINEL), (mm, outputs[1], 0x5A5A), (m, outputs[2], SENTINEL)):
        assert bool((buf[n_px if on else 0:] == fill).all()), "an output that was not requested, or a guard region, was written"
    return depth[:n_px].cpu().numpy(), mm[:n_px].cpu().numpy().view("uint16"), m[:n_px].cpu().numpy()


@pytest.mark.parametrize("case", E.HEAD_CASES, ids=lambda c: "x".join(str(v) for v in c[:3]))
def test_head_fused_exact(gpu_ctx, half, case):
    """depth, millimetres and metres bit for bit: the restated upsampling of x + b0 (not the product's kernel), exact 3 x 3 sums with zero padding, exact 1 x 1
    sums, then the epilogue as norm_reference.head_tail_reference states it -- with b0 and with NULL (as the network calls it), non_negative and invert on and
    off, every output on its own, and through two and three trips of the tile loop (the LDS-DMA prefetch of the next tile's patch)."""
    import numpy as np
    N, x64, b0_64, w3_64, b3_64, w1_64, b1 = _head_case(case)
    H, W = case[1:3]
    cus, tiles = _cus(), N * E.head_tiles(H, W)
    if case[0] is None:  # the premise, on this device: grid = min(tiles, 2 CUs)
        print(f"  premise: {tiles} tiles on {2 * cus} workgroups: {tiles - 4 * cus} of them make three trips, the rest two")
        assert 4 * cus < tiles < 6 * cus
    x, w3 = _dev(x64, half), _dev(w3_64.permute(2, 3, 0, 1).contiguous(), half)  # [tap][oc][ic]
    b0 = b0_64.to(device="cuda", dtype=torch.float32)
    b3, w1 = b3_64.numpy().astype(np.float32), w1_64.numpy().astype(np.float32)
    variants = E.head_variants(case)
    for with_b0 in sorted({v[0] for v in variants}):
        feat = _cached(("head-sums", half, with_b0) + tuple(case[:3]), lambda: E.head_sums(x64, b0_64 if with_b0 else None, w3_64, half, device="cuda"))
        for _, nn, inv in [v for v in variants if v[0] == with_b0]:
            want = E.head_expected(feat, b3_64, w1_64, b1[with_b0], nn, inv)
            got = _head(gpu_ctx, half, x, b0 if with_b0 else None, w3, b3, w1, b1[with_b0], N, H, W, nn, inv)
            for name, a, b in zip(("depth", "millimetres", "metres"), got, want):
                assert a.dtype == b.dtype and np.array_equal(a, b), f"b0 {with_b0}, non_negative {nn}, invert {inv}: {int((a != b).sum())} of {a.size} {name} differ"
            if case[3] == E.HEAD_GRID and (with_b0, nn, inv) == (True, 1, 1):  # any one output alone
                for k in range(3):
                    outputs = tuple(j == k for j in range(3))
                    alone = _head(gpu_ctx, half, x, b0, w3, b3, w1, b1[True], N, H, W, nn, inv, outputs)
                    assert np.array_equal(alone[k], want[k]), f"output {k} alone"
