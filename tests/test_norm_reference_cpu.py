"""tests/norm_reference.py checked on the CPU: the roundings against numpy's and torch's own, the float64 references against nested loops at tiny sizes,
every generator's conditions (exact operands, sums below 2^24, 3/4 of the intervals single-valued) at every shape tests/test_norm_gpu.py uses, a float32
step-by-step restatement of each kernel's arithmetic inside the interval (contracted and un-contracted), and three float64 mutations outside it: the last
pixel left out of the sums, a ``cnt - 1`` divisor, ``eps`` omitted."""
import math

import numpy as np
import pytest
import torch

import norm_reference as R

FMTS = list(R.FORMATS)


# ------------------------------------------------------------------------------------------------------------------------------------
# roundings

@pytest.mark.parametrize("fmt", FMTS)
def test_round_to_is_the_formats_own_rounding(fmt):
    """From float32 values torch's conversion is a single rounding; from float64, numpy's float16 cast is.  Ties, subnormals, overflow included."""
    rng = np.random.default_rng(1)
    p, emin, fmax = R.FORMATS[fmt]
    with np.errstate(over="ignore"):
        v = np.concatenate([rng.standard_normal(20000) * np.exp2(rng.integers(-30, 17, size=20000)),
                            (np.arange(-4096, 4097) + 0.5) * 2.0 ** -p, (np.arange(-4096, 4097) + 0.5) * 2.0 ** (emin - p),  # ties, normal and subnormal
                            [0.0, -0.0, fmax, fmax * (1 + 2.0 ** -(p + 2)), fmax * (1 + 2.0 ** -p), -fmax * 2]]).astype(np.float32)
    want = torch.from_numpy(v).to(getattr(torch, fmt)).double().numpy()
    assert np.array_equal(R.round_to(v.astype(np.float64), fmt), want)
    if fmt == "float16":
        v64 = v.astype(np.float64) * (1 + 2.0 ** -40)  # not float32 values
        with np.errstate(over="ignore"):
            assert np.array_equal(R.round_to(v64, fmt), v64.astype(np.float16).astype(np.float64))
    # float64 -> T in ONE rounding: just above a tie of T, below the float32 resolution -- a conversion through float32 lands on the tie and rounds to even
    x = 1.0 + 2.0 ** -p + 2.0 ** -40
    assert R.round_to(x, fmt) == 1.0 + 2.0 ** (1 - p) and R.round_to(float(np.float32(x)), fmt) == 1.0


# ------------------------------------------------------------------------------------------------------------------------------------
# references against nested loops

def _loop_group_norm(x, gamma, beta, G, eps):
    N, HW, C = x.shape
    cpg = C // G
    y = np.zeros((N, HW, C))
    for n in range(N):
        for g in range(G):
            vals = [int(x[n, p, g * cpg + c]) for p in range(HW) for c in range(cpg)]
            mean = math.fsum(vals) / len(vals)
            var = math.fsum((v - mean) ** 2 for v in vals) / len(vals)
            for p in range(HW):
                for c in range(g * cpg, (g + 1) * cpg):
                    y[n, p, c] = (int(x[n, p, c]) - mean) / math.sqrt(var + eps) * gamma[c] + beta[c]
    return y


@pytest.mark.parametrize("N,HW,C,G", [(2, 3, 8, 2), (1, 5, 16, 16), (2, 1, 8, 1), (3, 4, 8, 8)])
def test_group_norm_reference_against_nested_loops(N, HW, C, G):
    x, gamma, beta, _ = R.gn_operands(N, HW, C, G, "float16")
    eps = float(np.float32(1e-5))
    y, rho = R.gn_values(x, gamma, beta, G, 1e-5)
    want = _loop_group_norm(x, gamma, beta, G, eps)
    assert np.allclose(y, want, rtol=1e-12, atol=1e-9)  # (a constant group: the two orders of (x - mean) a + beta differ by 1e-16 * 316 * 96)
    assert (rho > 0).all() and (rho >= R.K_GROUP_NORM * R.U * np.abs(beta)[None, None, :]).all()


def test_layer_norm_reference_against_nested_loops():
    x, gamma, beta = R.ln_operands(5, 256)
    y, _ = R.ln_values(x, gamma, beta, 1e-6)
    eps = float(np.float32(1e-6))
    for i in range(5):
        row = [int(v) for v in x[i]]
        mean = math.fsum(row) / 256
        var = math.fsum((v - mean) ** 2 for v in row) / 256
        want = [(v - mean) / math.sqrt(var + eps) * float(gamma[j]) + float(beta[j]) for j, v in enumerate(row)]
        assert np.allclose(y[i], want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (7, 5), (8, 32), (9, 13), (3, 4)])
def test_pool_reference_against_nested_loops(H, W):
    rng = np.random.default_rng(H * 100 + W)
    v = rng.standard_normal((2, H * W, 3))
    Ho, Wo, pt, pl = R.same_pool_geometry(H, W)
    assert (Ho, Wo) == (math.ceil(H / 2), math.ceil(W / 2))
    total = max((Ho - 1) * 2 + 3 - H, 0)
    assert pt == total // 2 and total - pt in (pt, pt + 1)
    want = np.full((2, Ho * Wo, 3), -np.inf)
    for n in range(2):
        for oy in range(Ho):
            for ox in range(Wo):
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = 2 * oy + ky - pt, 2 * ox + kx - pl
                        if 0 <= iy < H and 0 <= ix < W:
                            want[n, oy * Wo + ox] = np.maximum(want[n, oy * Wo + ox], v[n, iy * W + ix])
    assert np.array_equal(R.pool_max(v, H, W), want)


@pytest.mark.parametrize("N,HW,TM", [(3, 7, 5), (2, 6, 6), (3, 5, 4), (2, 4, 1), (1, 9, 4)])
def test_tile_partials_against_nested_loops(N, HW, TM):
    rng = np.random.default_rng(N * 100 + HW)
    x = rng.integers(-9, 10, size=(N, HW, 8))
    tiles = (N * HW + TM - 1) // TM
    want = np.zeros((tiles, 2, 2, 8))
    for r in range(N * HW):
        t, n = r // TM, r // HW
        h = 0 if (t * TM) // HW == n else 1
        want[t, h, 0] += x[n, r % HW]
        want[t, h, 1] += x[n, r % HW] ** 2
    got = R.gn_tile_partials(x, TM)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # summed over the tiles they are the samples' totals
    assert np.array_equal(got[:, :, 0].sum(axis=(0, 1)), x.sum(axis=(0, 1)))


def test_the_tile_cases_straddle_or_not_as_stated():
    straddling = {case: R.gn_straddling_tiles(case[0], case[1], case[4]) for case in R.GN_TILE_CASES}
    assert straddling[(3, 300, 64, 32, 256)] == 2 and straddling[(2, 37, 64, 32, 37)] == 0 and straddling[(3, 131, 256, 32, 128)] == 2


def test_bias_act_reference_against_nested_loops():
    rng = np.random.default_rng(3)
    for fmt in FMTS:
        x, b = R.dyadic(rng, (5, 8), fmt), R.dyadic(rng, (8,), fmt)
        r1, r2 = R.dyadic(rng, (5, 8), fmt), R.dyadic(rng, (5, 8), fmt)
        out, out_relu = R.bias_act_reference(x, b, fmt, r1, r2, relu=False)
        inexact = 0
        for i in range(5):
            for j in range(8):
                f = float(R.round_to(x[i, j] + b[j], fmt)) + r1[i, j]
                inexact += f != float(R.round_to(f, fmt))
                f = float(R.round_to(f, fmt)) + r2[i, j]
                assert out[i, j] == float(R.round_to(f, fmt)) and out_relu[i, j] == max(out[i, j], 0.0)
        assert inexact > 0  # the intermediate rounding matters for these operands


# ------------------------------------------------------------------------------------------------------------------------------------
# float32 restatements of the kernels

def _fma32(a, b, c):
    """fma in float32 for float32-valued float64 arrays: a b is exact in float64; the sum is rounded to float64 first (a double rounding in rare ties)."""
    return R.f32(a * b + c)


def _gn_kernel(x, gamma, beta, G, eps, fmt, residual, relu, contract):
    """gn_partial / gn_finalize / gn_apply step by step (csrc/dpt_ops.hip): exact sums, mean and rstd in float64 rounded once, the rest in float32."""
    N, HW, C = x.shape
    cpg = C // G
    xg = x.reshape(N, HW, G, cpg)
    s, q, cnt = xg.sum(axis=(1, 3)).astype(np.float64), (xg * xg).sum(axis=(1, 3)).astype(np.float64), float(HW * cpg)
    mean = s / cnt
    var = np.maximum(q / cnt - mean * mean, 0.0)
    mean32 = np.repeat(R.f32(mean), cpg, axis=1)[:, None, :]
    rstd32 = np.repeat(R.f32(1.0 / np.sqrt(var + float(np.float32(eps)))), cpg, axis=1)[:, None, :]
    xf = x.astype(np.float64)
    a = R.f32(rstd32 * gamma[None, None, :])
    if contract:
        y = _fma32(xf, a, _fma32(-mean32, a, beta[None, None, :]))
    else:
        y = R.f32(R.f32(xf * a) + R.f32(beta[None, None, :] - R.f32(mean32 * a)))
    if residual is not None:
        y = R.f32(R.round_to(y, fmt) + residual)
    if relu:
        y = np.maximum(y, 0.0)
    return y


def _ln_kernel(x, gamma, beta, eps, contract, rsqrt_ulps):
    """layernorm_kernel step by step (csrc/vit.hip); the reciprocal square root correctly rounded, or one float32 step above / below it."""
    D = x.shape[1]
    mean = x.sum(axis=1, keepdims=True) // D
    d = (x - mean).astype(np.float64)
    v = R.f32(R.f32((d * d).sum(axis=1, keepdims=True) / D) + float(np.float32(eps)))
    r = (1.0 / np.sqrt(v)).astype(np.float32)
    if rsqrt_ulps:
        r = np.nextafter(r, np.float32(np.inf * rsqrt_ulps))
    t = R.f32(d * r.astype(np.float64))
    g, b = gamma.astype(np.float64)[None, :], beta.astype(np.float64)[None, :]
    return _fma32(t, g, b) if contract else R.f32(R.f32(t * g) + b)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N,HW,C,G", R.GN_CASES)
def test_group_norm_conditions_and_restatement(fmt, N, HW, C, G):
    """The generator's assertions and the 3/4 condition at every GPU shape and option; the float32 restatement inside the interval in both forms."""
    x, gamma, beta, res = R.gn_operands(N, HW, C, G, fmt)
    eps = R.gn_eps(HW, C // G)
    mean, var = R.gn_statistics(x, G)
    const = np.array([R.gn_is_constant(i) for i in range(N * G)]).reshape(N, G)
    if HW * (C // G) > 1:
        assert (var[const] == 0).all() and (var[~const] > 0).all()
    else:
        assert (var == 0).all()
    # a neighbour's statistics are far away: the offsets of groups g and g ^ 1, and of samples n and n + 1, differ by 5 at least
    off = np.array([R.gn_offset(i) for i in range(N * G)]).reshape(N, G)
    assert G == 1 or (np.abs(off[:, 0::2] - off[:, 1::2]) >= 5).all()
    assert N == 1 or (np.abs(np.diff(off, axis=0)) >= 1).all()
    for residual in (None, res):
        for relu in (False, True):
            lo, hi, _ = R.gn_interval(x, gamma, beta, G, eps, fmt, residual, relu)
            for contract in (False, True):
                out = R.round_to(_gn_kernel(x, gamma, beta, G, eps, fmt, residual, relu, contract), fmt)
                R.check_interval(out, lo, hi, f"restatement residual={residual is not None} relu={relu} contract={contract}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("H,W,C", R.POOL_CASES)
def test_pool_conditions_and_restatement(fmt, H, W, C):
    G = R.pool_groups(H, W, C)
    x, gamma, beta, _ = R.gn_operands(2, H * W, C, G, fmt)
    eps = R.gn_eps(H * W, C // G)
    lo, hi, _ = R.gn_pool_interval(x, gamma, beta, G, eps, fmt, H, W)
    y = _gn_kernel(x, gamma, beta, G, eps, fmt, None, True, False)
    R.check_interval(R.round_to(R.pool_max(y, H, W), fmt), lo, hi, "restatement")
    partial = R.gn_tile_partials(x, R.pool_tile_rows(H * W))  # asserts exactness
    assert np.array_equal(partial[:, :, 1].astype(np.int64).sum(axis=(0, 1)), (x * x).sum(axis=(0, 1)))


@pytest.mark.parametrize("N,HW,C,G,TM", R.GN_TILE_CASES)
def test_tile_partials_are_exact_at_the_gpu_shapes(N, HW, C, G, TM):
    x = R.gn_operands(N, HW, C, G, "bfloat16")[0]
    partial = R.gn_tile_partials(x, TM)
    assert np.array_equal(partial[:, :, 0].astype(np.int64).sum(axis=(0, 1)), x.sum(axis=(0, 1)))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,D", R.LN_CASES)
def test_layer_norm_conditions_and_restatement(fmt, M, D):
    x, gamma, beta = R.ln_operands(M, D)
    lo, hi, _ = R.ln_interval(x, gamma, beta, R.LN_EPS, fmt)
    if M >= 3:
        assert np.ptp(x[M // 2]) == 0 and np.count_nonzero(x[M - 1]) == 1
    for contract in (False, True):
        for ulps in (-1, 0, 1):
            out = R.round_to(_ln_kernel(x, gamma, beta, R.LN_EPS, contract, ulps), fmt)
            R.check_interval(out, lo, hi, f"restatement contract={contract} rsqrt {ulps:+d} ulp")


# ------------------------------------------------------------------------------------------------------------------------------------
# mutations

def _gn_mutant(x, gamma, beta, G, eps, kind):
    N, HW, C = x.shape
    cpg = C // G
    xg = x.reshape(N, HW, G, cpg).astype(np.float64)
    used = xg[:, :-1] if kind == "last pixel left out" else xg
    cnt = float(HW * cpg) - (1.0 if kind == "cnt - 1" else 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = used.sum(axis=(1, 3)) / cnt
        var = np.maximum((used * used).sum(axis=(1, 3)) / cnt - mean * mean, 0.0)
    return R.gn_values(x, gamma, beta, G, 0.0 if kind == "eps omitted" else eps, mean, var)[0]


@pytest.mark.parametrize("kind", ["last pixel left out", "cnt - 1", "eps omitted"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N,HW,C,G", R.GN_CASES)
def test_group_norm_mutations_leave_the_interval(fmt, N, HW, C, G, kind):
    x, gamma, beta, _ = R.gn_operands(N, HW, C, G, fmt)
    eps = R.gn_eps(HW, C // G)
    lo, hi, _ = R.gn_interval(x, gamma, beta, G, eps, fmt)
    bad = R.outside(R.round_to(_gn_mutant(x, gamma, beta, G, eps, kind), fmt), lo, hi)
    print(f"{kind} {fmt} {(N, HW, C, G)}: {bad.mean():.1%} of the elements rejected")
    if kind == "eps omitted" and not any(R.gn_is_constant(i) for i in range(N * G)) and HW * (C // G) > 1:
        return  # no group with var = 0: eps changes rstd by 1e-5 / (2 var), below a float32 rounding of the terms -- nothing to see, in any check
    assert bad.any()
    if kind != "eps omitted":
        assert bad.mean() >= (0.02 if HW * (C // G) > 8000 else 0.1)  # a statistic moved by 1 / cnt of its spread: it shows in a good share of the elements


@pytest.mark.parametrize("kind", ["last element left out", "D - 1", "eps omitted"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,D", R.LN_CASES)
def test_layer_norm_mutations_leave_the_interval(fmt, M, D, kind):
    x, gamma, beta = R.ln_operands(M, D)
    lo, hi, _ = R.ln_interval(x, gamma, beta, R.LN_EPS, fmt)
    xf = x.astype(np.float64)
    used = xf[:, :-1] if kind == "last element left out" else xf
    cnt = D - 1.0 if kind == "D - 1" else float(D)
    mean = used.sum(axis=1, keepdims=True) / cnt
    var = np.maximum((used * used).sum(axis=1, keepdims=True) / cnt - mean * mean, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = (xf - mean) / np.sqrt(var + (0.0 if kind == "eps omitted" else float(np.float32(R.LN_EPS)))) * gamma[None, :] + beta[None, :]
    bad = R.outside(R.round_to(y, fmt), lo, hi)
    print(f"{kind} {fmt} {(M, D)}: {bad.mean():.1%} of the elements rejected")
    if kind == "eps omitted" and M < 3:
        return  # no constant row: eps = 1e-6 beside var >= 1/2 is below a float32 rounding
    assert bad.any()


# ------------------------------------------------------------------------------------------------------------------------------------
# element-wise references

def test_preprocess_table_is_the_float64_formula():
    for fmt in FMTS:
        tab = R.preprocess_table(0.5, 0.5, fmt)
        assert tab[0] == -1.0 and tab[255] == 1.0 and (np.diff(tab) >= 0).all() and len(np.unique(tab)) > 100
        R.assert_exact(tab, fmt, "table")


def test_head_tail_reference_edge_cases():
    """Accumulator 0 and shift 0: depth 1 / 1e-8f, millimetres saturate at 65535, metres are cut to 0 by max_depth."""
    feat, w = np.zeros((2, 8)), np.ones(8, dtype=np.float32)
    feat[1] = 2
    depth, mm, m = R.head_tail_reference(feat, None, 0, w, 0.0, 1, 1, 0.5, 0.0, 0.001, 10.0)
    assert depth[0] == np.float32(1) / np.float32(1e-8) and mm[0] == 65535 and m[0] == 0
    assert depth[1] == np.float32(0.125) and mm[1] == 125 and m[1] == np.float32(0.001) * np.float32(125)
    assert np.array_equal(R.depth_mm_to_m_reference(np.array([0, 1, 65535], dtype=np.uint16), 0.001, 10.0),
                          np.array([0, np.float32(0.001), 0], dtype=np.float32))
