"""Operands, float64 references and derived intervals for the normalisation and element-wise kernels (csrc/vit.hip layernorm_kernel, csrc/dpt_ops.hip
gn_partial / gn_finalize / gn_finalize_tiles / gn_apply / gn_relu_maxpool / bias_act).

The operands are small integers held in bfloat16 / float16.  Every sum and every sum of squares a statistics kernel forms in float32 is then an integer
below 2^24 -- exact in any order, for any slab count, tile size and reduction tree -- so the mean and the variance are fixed up to one division and only
a handful of float32 roundings separate them from the stored value.  The check per element:

  ref   the operation in float64 from its definition, ``eps`` taken as the float32 value;
  rho   k * 2^-24 * (|x a| + |mean a| + |beta|) with a = rstd * gamma: k float32 roundings (each at most 2^-24 relative) on the longest path from the
        exact sums to the value, COUNTED in the kernel's source next to each reference below, never fitted.  (1 + 2^-16) on top covers the second-order
        terms (k^2 2^-48) and the float64 arithmetic of the reference and of gn_finalize (2^-53 per step): five orders of magnitude below one rounding;
  lo, hi  round_T(ref - rho), round_T(ref + rho), ONE rounding from float64 (``round_to``; torch's float64 -> 16-bit conversions go through float32).

``lo <= out <= hi`` is asserted for every element.  Where lo == hi that is bit for bit; every reference asserts that this holds for at least 3/4 of its
elements (``assert_sharp``), so no case passes on wide intervals.  A step that rounds to T in the middle (GroupNorm + residual) carries the interval
through: rounding, adding a constant, ReLU and max are monotonic.

Nothing is imported from the product tree.  Everything is numpy float64 / int64 on the CPU."""
import numpy as np

U = 2.0 ** -24                 # one float32 rounding, relative
SLACK = 1.0 + 2.0 ** -16       # second-order terms and the float64 steps (see above)
LIMIT = 2 ** 24                # integers below it are exact in float32
FORMATS = {"bfloat16": (8, -125, 3.3895313892515355e38), "float16": (11, -13, 65504.0)}  # significand bits, frexp exponent of the least normal, largest finite

# gn_apply_kernel / gn_relu_maxpool_kernel (dpt_ops.hip is built with -ffp-contract=off: one form).  gn_finalize forms mean and rstd in float64 from
# the exact sums and rounds each ONCE to float32 (IEEE division and sqrt in float64: below SLACK).  Then, all in float32:
#   a = rstd * gamma          mean path: [mean -> f32] 1                x path: [rstd -> f32] 1      beta path:
#   t = mean * a                         [rstd -> f32, a] 2, t 1                a 1, u 1, y 1                    b 1, y 1
#   b = beta - t                         b 1
#   y = x * a + b  (u = x * a)           y 1                   = 6                        = 4                      = 2
K_GROUP_NORM = 6
# layernorm_kernel (vit.hip allows contraction).  sum x is an integer, mean = sum / D an integer (the rows are built so), d = x - mean and sum d^2 are
# exact (a one-pass sum x^2 would be too).  Then: var = ssq / D 1, var + eps 1, rsqrtf 2 (one ulp = two half-ulps), d * rstd 1, * gamma 1, + beta 1 = 7 on
# the d a term; the contracted form fma(d rstd, gamma, beta) has one rounding fewer.  beta itself sees 1.
K_LAYER_NORM = 7


# ------------------------------------------------------------------------------------------------------------------------------------
# number formats

def round_to(x, fmt):
    """float64 -> the nearest value of ``fmt`` (ties to even, gradual underflow, overflow to infinity), returned as float64: one rounding."""
    p, emin, fmax = FORMATS[fmt]
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        _, e = np.frexp(x)  # x = m 2^e with 0.5 <= |m| < 1
        q = np.ldexp(1.0, np.maximum(e, emin) - p)  # the spacing of fmt at x
        r = np.rint(x / q) * q  # x / q is exact; rint rounds halves to even multiples
        r = np.where(np.abs(r) > fmax, np.copysign(np.inf, r), r)
    return np.where(np.isfinite(x), r, x)


def assert_exact(x, fmt, what):
    assert np.array_equal(round_to(x, fmt), np.asarray(x, dtype=np.float64)), f"{what}: not exact in {fmt}"


def f32(x):
    """float64 -> float32 -> float64: one float32 rounding."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------------------
# intervals

def outside(out, lo, hi):
    """Elements of ``out`` (float64 view of the kernel's output) not in [lo, hi]; a NaN is outside."""
    out = np.asarray(out, dtype=np.float64)
    return ~((lo <= out) & (out <= hi))


def single_valued(lo, hi):
    return float(np.mean(lo == hi))


def assert_sharp(lo, hi, what):
    """The condition against a vacuous pass: at least 3/4 of the elements admit exactly one value."""
    share = single_valued(lo, hi)
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all(), f"{what}: malformed interval"
    assert share >= 0.75, f"{what}: only {share:.3f} of the elements are single-valued"
    return share


def check_interval(out, lo, hi, what, ref=None):
    """Assert lo <= out <= hi everywhere; the message names the worst element.  Returns the share of single-valued elements."""
    out = np.asarray(out, dtype=np.float64)
    assert out.shape == lo.shape == hi.shape, f"{what}: shape {out.shape} vs {lo.shape}"
    bad = outside(out, lo, hi)
    share = single_valued(lo, hi)
    if bad.any():
        with np.errstate(invalid="ignore"):
            dist = np.where(bad, np.maximum(lo - out, out - hi), 0.0)
        dist = np.where(np.isnan(dist), np.inf, dist)
        i = np.unravel_index(int(np.argmax(dist)), out.shape)
        r = "" if ref is None else f" ref {ref[i]!r}"
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements ({bad.mean():.3%}) outside their interval; worst at {i}: out {out[i]!r}, "
                             f"interval [{lo[i]!r}, {hi[i]!r}]{r}; {share:.3f} of the intervals are single values")
    return share


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_norm_gpu.py (tests/test_norm_reference_cpu.py checks every generator condition at each of them)

LN_EPS = 1e-6
LN_CASES = [(M, D) for D in (256, 512, 768, 1024) for M in (1, 4, 5, 131)]  # all four CH instantiations; fewer than, equal to, just past a workgroup's four rows
# (N, HW, C, G).  With VC = C / 8 channel vectors and PP = 256 / VC pixel lanes, slabs = min(64, HW / (4 PP) + 1):
GN_CASES = [(2, 37, 64, 32), (3, 131, 256, 32), (1, 9, 2048, 32), (2, 300, 8, 8), (1, 1, 32, 32), (2, 5, 16, 16),
            (1, 252, 2048, 32), (1, 253, 2048, 32),  # PP = 1: 64 slabs of 4 pixels, one trip of the four-loads loop each; at HW = 252 the last slab is empty
            (1, 325, 2048, 32),                      # 64 slabs of 6 pixels: the four-loads loop leaves a remainder of two; slabs 55.. are empty
            (2, 1025, 8, 1)]                         # VC = 1, PP = 256: two slabs of 513 pixels, threads with two and with three pixels
GN_TILE_CASES = [(3, 300, 64, 32, 256), (2, 37, 64, 32, 37), (3, 131, 256, 32, 128), (2, 300, 8, 8, 256)]  # (N, HW, C, G, TM): straddling; TM = HW; TM just below HW
POOL_CASES = [(H, W, C) for (H, W) in ((1, 1), (2, 2), (7, 5), (8, 32), (9, 13)) for C in (8, 64)]  # N = 2


def gn_eps(HW, cpg):
    """GroupNorm's eps: 1e-5 as the network's.  A group of ONE element has var = 0 always; at 1e-5 the kernel's own float32 error there (an ulp of
    316 |x| gamma, cancelled down to beta) spans several steps of T, so no check could be sharp.  eps = 0.25 makes 1 / sqrt(eps) = 2 exactly: the case
    still exercises the clamp, the indexing and that eps is added at all (without it: a division by zero)."""
    return 0.25 if HW * cpg == 1 else 1e-5


def pool_groups(H, W, C):
    """Groups of a pooling case: 32 for 64 channels as the network, 2 for 8; a 1 x 1 map gets groups of 8 channels (a group of two values is constant too often)."""
    return {8: 2, 64: 32}[C] if H * W > 1 else C // 8


def pool_tile_rows(HW):
    """Tile rows of the pooling cases' partials: two thirds of a map, so that the second tile straddles the two samples (1 for a 1 x 1 map)."""
    return max(1, 2 * HW // 3)


# ------------------------------------------------------------------------------------------------------------------------------------
# GroupNorm

SPREADS = (1, 2, 4, 8, 3)


def gn_constant(HW, cpg):
    """The value of the constant groups: the largest multiple of 8 up to 96 whose sum of squares over a group stays below 2^24."""
    c = 96
    while c > 8 and c * c * HW * cpg >= LIMIT:
        c -= 8
    return c


def gn_is_constant(i):
    return i % 8 == 5


def gn_offset(i):
    """The mean of (sample, group) pair i = n G + g: -12..12, 7 apart (mod 25) between neighbouring groups, non-zero apart between samples for G in 1..32."""
    return (i * 7 + 3) % 25 - 12


def gn_operands(N, HW, C, G, fmt, seed=0):
    """x [N][HW][C] int64, gamma [C], beta [C], residual [N][HW][C] (float64, exact in fmt).  Pair i = n G + g holds gn_offset(i) + U(-r..r) with r
    cycling through SPREADS (its first two values are offset + r and offset - r: never constant by accident); one pair in eight is constant."""
    assert C % G == 0
    cpg = C // G
    rng = np.random.default_rng([seed, N, HW, C, G])
    x = np.empty((N, HW, G, cpg), dtype=np.int64)
    const = gn_constant(HW, cpg)
    for n in range(N):
        for g in range(G):
            i = n * G + g
            m, r = gn_offset(i), SPREADS[i % 5]
            blk = m + rng.integers(-r, r + 1, size=HW * cpg)
            if blk.size >= 2:
                blk[0], blk[1] = m + r, m - r
            if gn_is_constant(i):
                blk[:] = const
            x[n, :, g, :] = blk.reshape(HW, cpg)
    x = x.reshape(N, HW, C)
    gamma = rng.integers(4, 17, size=C) / 8.0 * (rng.integers(0, 2, size=C) * 2 - 1)
    beta = rng.integers(-16, 17, size=C) / 16.0
    residual = rng.integers(-64, 65, size=(N, HW, C)) / 8.0
    for name, v in (("x", x), ("gamma", gamma), ("beta", beta), ("residual", residual)):
        assert_exact(v, fmt, f"group norm {name}")
    # exactness of the statistics: a channel's sums over a whole sample bound every slab's, tile's, thread's and tree node's partial sum
    assert int(np.abs(x).sum(axis=1).max()) < LIMIT and int((x * x).sum(axis=1).max()) < LIMIT, "a per-channel sum reaches 2^24"
    assert int((x * x).reshape(N, HW, G, cpg).sum(axis=(1, 3)).max()) < LIMIT, "a group's sum of squares reaches 2^24"
    return x, gamma, beta, residual


def gn_statistics(x, G):
    """(mean, var) [N][G] in float64 from the definition (two passes)."""
    N, HW, C = x.shape
    xg = x.reshape(N, HW, G, C // G).astype(np.float64)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    return mean, var


def gn_values(x, gamma, beta, G, eps, mean=None, var=None):
    """The normalised values before any rounding and their radius: (y, rho), float64 [N][HW][C].  K_GROUP_NORM roundings."""
    N, HW, C = x.shape
    cpg = C // G
    if mean is None:
        mean, var = gn_statistics(x, G)
    eps = float(np.float32(eps))
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = 1.0 / np.sqrt(var + eps)
        a = np.repeat(rstd, cpg, axis=1)[:, None, :] * gamma[None, None, :]
        mu = np.repeat(mean, cpg, axis=1)[:, None, :]
        xf = x.astype(np.float64)
        y = (xf - mu) * a + beta[None, None, :]
        rho = K_GROUP_NORM * U * SLACK * (np.abs(xf * a) + np.abs(mu * a) + np.abs(beta)[None, None, :])
    return y, rho


def gn_interval(x, gamma, beta, G, eps, fmt, residual=None, relu=False, what="group norm"):
    """[lo, hi] of hive_nhwc_group_norm's output: round_T(y -+ rho); with a residual r the kernel forms float32(z + r) from the rounded z in [lo, hi] and
    rounds again: both roundings are monotonic, so the ends are round_T(float32(lo + r)) and round_T(float32(hi + r)), with lo + r exact in float64
    (asserted) -- the float32 rounding of the sum is applied, as the kernel applies it, instead of widening by it (a sum that is a tie of T would
    otherwise always admit two values).  ReLU last (it commutes with the rounding).  Returns (lo, hi, ref)."""
    y, rho = gn_values(x, gamma, beta, G, eps)
    lo, hi = round_to(y - rho, fmt), round_to(y + rho, fmt)
    ref = y
    if residual is not None:
        slo, shi = lo + residual, hi + residual  # exact in float64
        assert np.array_equal(slo - residual, lo) and np.array_equal(shi - residual, hi), "z + r is not exact in float64"
        lo, hi = round_to(f32(slo), fmt), round_to(f32(shi), fmt)
        ref = round_to(y, fmt) + residual
    if relu:
        lo, hi, ref = np.maximum(lo, 0.0), np.maximum(hi, 0.0), np.maximum(ref, 0.0)
    assert_sharp(lo, hi, what)
    return lo, hi, ref


def same_pool_geometry(H, W):
    """3 x 3 / 2 window, TensorFlow "SAME" padding: ceil(i / 2) outputs, the odd padding pixel at the bottom / right."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    return Ho, Wo, max((Ho - 1) * 2 + 3 - H, 0) // 2, max((Wo - 1) * 2 + 3 - W, 0) // 2


def pool_max(v, H, W):
    """[N][H W][C] -> [N][Ho Wo][C]: the window maximum, padded positions never winning."""
    N, _, C = v.shape
    Ho, Wo, pt, pl = same_pool_geometry(H, W)
    pad = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf)
    pad[:, pt:pt + H, pl:pl + W] = v.reshape(N, H, W, C)
    out = np.full((N, Ho, Wo, C), -np.inf)
    for ky in range(3):
        for kx in range(3):
            out = np.maximum(out, pad[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2])
    return out.reshape(N, Ho * Wo, C)


def gn_pool_interval(x, gamma, beta, G, eps, fmt, H, W, what="group norm + relu + max pool"):
    """[lo, hi] of hive_nhwc_group_norm_relu_maxpool: the window maximum of the float64 values, ReLU, one rounding; the interval is the window's."""
    y, rho = gn_values(x, gamma, beta, G, eps)
    lo = round_to(np.maximum(pool_max(y - rho, H, W), 0.0), fmt)
    hi = round_to(np.maximum(pool_max(y + rho, H, W), 0.0), fmt)
    assert_sharp(lo, hi, what)
    return lo, hi, np.maximum(pool_max(y, H, W), 0.0)


def gn_tile_partials(x, TM):
    """What a convolution's epilogue leaves for gn_finalize_tiles_kernel: float32 [tile][h][sum, sq][C] over tiles of TM rows of the [N HW][C] matrix,
    h = 0 for the rows of the image the tile's first row lies in, h = 1 for the rows past that image's end (TM <= HW: two images at most)."""
    N, HW, C = x.shape
    assert 0 < TM <= HW
    rows = x.reshape(N * HW, C)
    tiles = (N * HW + TM - 1) // TM
    partial = np.zeros((tiles, 2, 2, C), dtype=np.int64)
    for t in range(tiles):
        r0, r1 = t * TM, min((t + 1) * TM, N * HW)
        split = min(r1, (r0 // HW + 1) * HW)
        for h, part in enumerate((rows[r0:split], rows[split:r1])):
            partial[t, h, 0], partial[t, h, 1] = part.sum(axis=0), (part * part).sum(axis=0)
    assert int(np.abs(partial).max()) < LIMIT
    return partial.astype(np.float32)


def gn_straddling_tiles(N, HW, TM):
    """How many tiles hold rows of two images."""
    return sum(1 for t in range((N * HW + TM - 1) // TM) if min((t + 1) * TM, N * HW) > (t * TM // HW + 1) * HW)


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm

LN_SPREADS = (1, 2, 4, 8, 16, 3)


def ln_operands(M, D, seed=0):
    """x [M][D] int64, gamma [D], beta [D] float32 multiples of 1/8.  Row i: offset (5 + 37 i) mod 65 - 32 plus U(-s..s), s cycling through LN_SPREADS, then
    lowered by one at its first entries so that the row sum is a multiple of D (an integer mean).  For M >= 3 row M // 2 is constant (0 for M < 16, else 64:
    var = 0, rstd = 1 / sqrt(eps)); for M >= 2 row M - 1 holds a single non-zero entry, D, at column (7 M) mod D."""
    rng = np.random.default_rng([seed, M, D])
    x = np.empty((M, D), dtype=np.int64)
    for i in range(M):
        off, s = (5 + 37 * i) % 65 - 32, LN_SPREADS[i % 6]
        row = off + rng.integers(-s, s + 1, size=D)
        row[:int(row.sum() % D)] -= 1
        assert row.max() > row.min()
        x[i] = row
    if M >= 3:
        x[M // 2] = 0 if M < 16 else 64
    if M >= 2:
        x[M - 1] = 0
        x[M - 1, (7 * M) % D] = D
    gamma = (rng.integers(4, 17, size=D) / 8.0 * (rng.integers(0, 2, size=D) * 2 - 1)).astype(np.float32)
    beta = (rng.integers(-16, 17, size=D) / 8.0).astype(np.float32)
    assert (x.sum(axis=1) % D == 0).all(), "a row's mean is not an integer"
    mean = x.sum(axis=1) // D
    assert int((x * x).sum(axis=1).max()) < LIMIT and int(((x - mean[:, None]) ** 2).sum(axis=1).max()) < LIMIT, "a row's sum of squares reaches 2^24"
    for fmt in FORMATS:
        assert_exact(x, fmt, "layer norm x")
    return x, gamma, beta


def ln_values(x, gamma, beta, eps):
    """(y, rho) of LayerNorm over the last dimension, float64 from the definition.  K_LAYER_NORM roundings."""
    xf, g, b = x.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64)
    mean = xf.mean(axis=1, keepdims=True)
    var = ((xf - mean) ** 2).mean(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = g[None, :] / np.sqrt(var + float(np.float32(eps)))
        y = (xf - mean) * a + b[None, :]
        rho = K_LAYER_NORM * U * SLACK * (np.abs(xf * a) + np.abs(mean * a) + np.abs(b)[None, :])
    return y, rho


def ln_interval(x, gamma, beta, eps, fmt, what="layer norm"):
    y, rho = ln_values(x, gamma, beta, eps)
    lo, hi = round_to(y - rho, fmt), round_to(y + rho, fmt)
    assert_sharp(lo, hi, what)
    return lo, hi, y


# ------------------------------------------------------------------------------------------------------------------------------------
# element-wise entry points: the stated roundings in order, on dyadic operands (every float32 sum below is exact, so float64 forms it too)

def dyadic(rng, shape, fmt):
    """k 2^-e, |k| <= 1024, e in 0..4, rounded to fmt: sums of a few of them are multiples of 2^-4 below 2^13, exact in float32, but not in fmt."""
    v = rng.integers(-1024, 1025, size=shape) * np.ldexp(1.0, -rng.integers(0, 5, size=shape))
    return round_to(v, fmt)


def bias_act_reference(x, bias, fmt, residual=None, residual2=None, relu=False):
    """hive_nhwc_bias_act on [n_px][C]: x + bias rounded to T; + residual; rounded to T before + residual2; ReLU; rounded to T.
    Returns (out, out_relu) with out_relu = relu(out)."""
    f = round_to(x + bias[None, :], fmt)
    if residual is not None:
        f = f + residual
    if residual2 is not None:
        f = round_to(f, fmt) + residual2
    if relu:
        f = np.maximum(f, 0.0)
    assert np.array_equal(f32(f), f), "a float32 sum is not exact: the operands are not dyadic enough"
    out = round_to(f, fmt)
    return out, np.maximum(out, 0.0)


def preprocess_table(mean, std, fmt):
    """((v / 255 - mean) / std) in float64 for the float32 values of mean and std, rounded to float32, then to T."""
    mean, std = float(np.float32(mean)), float(np.float32(std))
    return round_to(f32((np.arange(256, dtype=np.float64) / 255.0 - mean) / std), fmt)


def head_tail_reference(feat, pre_bias, pre_relu, weight, bias, non_negative, invert, scale, shift, depth_scale, max_depth):
    """hive_dpt_head_tail in numpy float32, step by step (integer operands: the dot product is exact in any order; scale a power of two: scale * acc is
    exact, so the multiply-add is the same fused or not).  Returns (depth f32, mm u16, metres f32)."""
    one = np.float32
    x = feat.astype(np.float32) + (np.zeros_like(weight) if pre_bias is None else pre_bias.astype(np.float32))[None, :]
    if pre_relu:
        x = np.maximum(x, one(0))
    acc = (x.astype(np.float64) @ weight.astype(np.float64) + float(bias))
    assert float((np.abs(x).astype(np.float64) @ np.abs(weight).astype(np.float64)).max()) + abs(float(bias)) < LIMIT
    assert np.array_equal(acc, np.rint(acc)), "the accumulator is not an integer"
    acc = acc.astype(np.float32)
    if non_negative:
        acc = np.maximum(acc, one(0))
    depth = acc
    if invert:
        t = one(scale) * acc
        assert np.array_equal(t.astype(np.float64), float(one(scale)) * acc.astype(np.float64)), "scale * acc is not exact"
        depth = one(1) / np.maximum(t + one(shift), one(1e-8))
    mm = np.minimum(np.maximum(depth * one(1000), one(0)), one(65535)).astype(np.int32).astype(np.uint16)
    m = one(depth_scale) * mm.astype(np.float32)
    m = np.where(m > one(max_depth), one(0), m).astype(np.float32)
    return depth.astype(np.float32), mm, m


def depth_mm_to_m_reference(mm, depth_scale, max_depth):
    m = np.float32(depth_scale) * mm.astype(np.float32)
    return np.where(m > np.float32(max_depth), np.float32(0), m).astype(np.float32)
