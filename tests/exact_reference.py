"""Integer operands and exact references for the MFMA kernels (csrc/vit.hip, conv.hip, stem.hip, gram.hip, mfma_pipe.hpp).

The kernels accumulate in float32 and round once.  Products of small integers held in bfloat16 / float16 are exact, and sums of them are exact in
float32 below 2^24 in ANY order, for any split-K partition and any tile shape.  For integer operands a kernel's output is therefore fully determined:
the exact integer result, rounded once (to nearest even) to the element type -- a single misplaced, dropped or duplicated term fails ``torch.equal``.

Everything here is index arithmetic followed by an int64 (numpy) or float64 (torch) matmul, written from the operations' definitions: nothing is
imported from the product tree, and no convolution / attention operator or 16/32-bit matmul of a library is called.  The float64 forms run on
whatever device their operands live on; for these integers they are exact (every partial sum is an integer far below 2^53).

The generators return the operands as int64 (or float64 where they are scaled by a power of two) CPU tensors together with ``bound``, an upper
bound of max over outputs of sum |a| |w| + |bias| + |residuals| (max |a| times the largest absolute row sum of the weights, plus the largest
bias and residuals -- never below the true maximum).  ``bound < 2^24`` is asserted: it is the condition for exactness, not a tolerance.  They
also assert coverage: at least 80 % of the activations are non-zero, and every K position has a non-zero weight in some output channel.

The last three sections do the same for the bottleneck convolution (csrc/bneck.hip), the x2 bilinear upsampling (csrc/dpt_ops.hip) and the fused depth head
(csrc/dpt_head.hip), each with its own conditions stated at its head; the epilogue of the head is norm_reference.head_tail_reference (the test tree's)."""
import math

import numpy as np
import torch

import norm_reference as R

LIMIT = 2 ** 24
Q_SCALE = np.float32(0.125) * np.float32(1.4426950408889634)  # head_dim^-0.5 * log2(e) as the kernel holds it: a float32 (0.125 f is exact)


# ------------------------------------------------------------------------------------------------------------------------------------
# operands

def draw(gen, shape, r, p_zero=None):
    """int64 values in -r..r: a uniform magnitude 1..r, a uniform sign, and zero with probability ``p_zero`` (default: 1 / (2 r + 1), i.e. uniform on -r..r)."""
    p_zero = 1.0 / (2 * r + 1) if p_zero is None else p_zero
    mag = torch.randint(1, r + 1, shape, generator=gen, dtype=torch.int64)
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64) * 2 - 1
    keep = (torch.rand(shape, generator=gen, dtype=torch.float64) >= p_zero).to(torch.int64)
    return mag * sign * keep


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(int(seed))


def check_conditions(act, wmat, bound):
    """The two coverage conditions and the exactness condition.  ``wmat``: [outputs][K]."""
    assert bound < LIMIT, f"bound {bound} is not below 2^24: float32 accumulation would not be exact"
    frac = float((act != 0).double().mean())
    assert frac >= 0.8, f"only {frac:.3f} of the activations are non-zero"
    assert bool((wmat != 0).any(dim=0).all()), "a K position has no non-zero weight in any output channel"


def upper_bound(act, wmat, *others):
    """max |a| * max_n sum_k |w[n][k]| + sum of max |other|: an upper bound of every output's sum of absolute terms."""
    b = int(act.abs().max()) * int(wmat.abs().sum(dim=1).max())
    for o in others:
        if o is not None:
            b += int(math.ceil(float(o.abs().max())))
    return b


def gemm_operands(M, N, K, seed=0, r=4):
    """A [M][K], W [N][K] in -r..r, bias [N] in -8..8, residual [M][N] in -64..64 (all exact in both element types), and the bound."""
    g = _gen(seed * 7919 + M * 31 + N * 17 + K)
    A, W = draw(g, (M, K), r), draw(g, (N, K), r)
    bias, res = draw(g, (N,), 8), draw(g, (M, N), 64)
    bound = upper_bound(A, W, bias, res)
    check_conditions(A, W, bound)
    return A, W, bias, res, bound


def gelu_operands(M, N, K, seed=0):
    """Operands for the GELU epilogue: integers in -4..4 times powers of two (float64 tensors, exact in both element types), scaled so that the
    pre-activations A W^T + bias have a spread of about 1.6; asserts that every one of them lies in -8..8 (the interesting part of the curve).
    bias: multiples of 1/8 in -1..1.  ``bound`` is that of the integer sums (before the power-of-two scale)."""
    g = _gen(seed * 104729 + M * 31 + N * 17 + K)
    A, W = draw(g, (M, K), 4), draw(g, (N, K), 4)
    spread = math.sqrt(K) * (60.0 / 9.0)  # var of uniform -4..4 is 60 / 9; of a product of two, its square
    e = max(0, int(math.ceil(math.log2(spread / 1.6))))
    ea = e // 2
    check_conditions(A, W, upper_bound(A, W) + 2 ** e)
    A64, W64 = A.double() * 2.0 ** -ea, W.double() * 2.0 ** -(e - ea)
    bias = draw(g, (N,), 8).double() / 8.0
    pre = A64 @ W64.t() + bias
    assert float(pre.abs().max()) <= 8.0, f"pre-activation {float(pre.abs().max())} outside -8..8"
    return A64, W64, bias, upper_bound(A, W) + 2 ** e  # (a bias of 1.0 is 2^e integer units)


def qkv_operands(B, N, D, seed=0):
    """x [B][Np][D] (rows N..Np-1 zero, as the model pads), W [3 D][D], bias [3 D]; Np = N rounded up to 64."""
    Np = (N + 63) // 64 * 64
    g = _gen(seed * 15485863 + B * 131 + N * 17 + D)
    x = torch.zeros(B, Np, D, dtype=torch.int64)
    x[:, :N] = draw(g, (B, N, D), 4)
    W, bias = draw(g, (3 * D, D), 4), draw(g, (3 * D,), 8)
    bound = upper_bound(x, W, bias)
    check_conditions(x[:, :N], W, bound)
    return x, W, bias, Np, bound


def ring_border(x_nhwc, base=5):
    """Give the map a distinct non-zero border ring, so that a halo tap read where a zero belongs -- or a border pixel read one place off -- shows: magnitude
    base + (y + 2 x) mod 3 (above every interior value; it changes from a pixel to its row and column neighbours), sign (-1)^(c + x) (it changes
    along a row, along a diagonal and from channel to channel)."""
    n, h, w, c = x_nhwc.shape
    yy, xx, cc = torch.arange(h)[:, None, None], torch.arange(w)[None, :, None], torch.arange(c)[None, None, :]
    ring = (base + (yy + 2 * xx) % 3) * (1 - 2 * ((cc + xx) % 2))
    on = ((yy == 0) | (yy == h - 1) | (xx == 0) | (xx == w - 1)).expand(h, w, c)
    x_nhwc[:, on] = ring.expand(h, w, c)[on]
    return x_nhwc


def conv_operands(n, cin, cout, k, h, w, oh, ow, seed=0, r=4, p_zero=None, bias_r=8, res_r=64):
    """x [n][h][w][cin] with a border ring, weight [cout][cin][k][k], bias [cout], two residuals [n][oh][ow][cout], and the bound."""
    g = _gen(seed * 32452843 + n * 1009 + cin * 131 + cout * 17 + k * 7 + h * 3 + w)
    x = draw(g, (n, h, w, cin), r, p_zero)
    if h >= 3 and w >= 3:
        ring_border(x, base=r + 1)
    wt = draw(g, (cout, cin, k, k), r, p_zero)
    bias = draw(g, (cout,), bias_r)
    r1, r2 = draw(g, (n, oh, ow, cout), res_r), draw(g, (n, oh, ow, cout), res_r)
    wm = weight_matrix(wt)
    bound = upper_bound(x, wm, bias, r1, r2)
    check_conditions(x, wm, bound)
    return x, wt, bias, r1, r2, bound


def conv_transpose_operands(n, cin, cout, s, h, w, seed=0):
    """ConvTranspose2d with kernel == stride: x [n][h][w][cin] in -2..2 (90 % non-zero), weight [cin][cout][s][s] in -1..1, bias in -8..8.  The kernels
    store the 1 x 1 convolution's result in the element type before the bias is added, so that intermediate has to be exact in bfloat16 as well:
    asserts sum |a| |w| <= 256 (integers up to 256 are bfloat16 values)."""
    g = _gen(seed * 49979687 + n * 1009 + cin * 131 + cout * 17 + s * 7 + h * 3 + w)
    x = draw(g, (n, h, w, cin), 2, 0.1)
    wt = draw(g, (cin, cout, s, s), 1, 0.1)
    bias = draw(g, (cout,), 8)
    wm = wt.permute(2, 3, 1, 0).reshape(s * s * cout, cin)
    inner = upper_bound(x, wm)
    assert inner <= 256, f"the 1 x 1 convolution's result may reach {inner}: not exact in bfloat16"
    check_conditions(x, wm, inner + 8)
    return x, wt, bias, inner + 8


def gram_operands(n, cin, h, w, oh, ow, seed=0):
    """x [n][h][w][cin] in -4..4; the bound of the Gram sums is 16 oh ow."""
    g = _gen(seed * 67867967 + n * 1009 + cin * 131 + h * 3 + w)
    x = draw(g, (n, h, w, cin), 4)
    bound = 16 * oh * ow
    assert bound < LIMIT and float((x != 0).double().mean()) >= 0.8
    return x, bound


# ------------------------------------------------------------------------------------------------------------------------------------
# rounding

def round_once(exact, dtype):
    """The float64 value cast to the element type by torch: round to nearest even, once.  (torch goes through float32; asserted to be exact there.)"""
    exact = exact.double()
    assert torch.equal(exact.float().double(), exact), "the exact result is not a float32 value: the cast would round twice"
    return exact.to(dtype)


def ulp(value, dtype):
    """Unit in the last place of ``dtype`` at ``value`` (float64 tensor): 2^(floor(log2 |v|) - m), the exponent clamped at the smallest normal one."""
    m, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    a = value.double().abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a))))
    e = torch.where(a > 0, e, torch.full_like(a, emin)).clamp_min(emin)
    return torch.pow(torch.full_like(a, 2.0), e - m)


def gelu64(x):
    """erf-GELU in float64."""
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


# ------------------------------------------------------------------------------------------------------------------------------------
# GEMM

def gemm_exact(A, W, bias=None, residual=None):
    """A W^T + bias (+ residual) in float64, on the operands' device."""
    out = A.double() @ W.double().t()
    if bias is not None:
        out = out + bias.double()
    if residual is not None:
        out = out + residual.double()
    return out


def gemm_exact_int(A, W, bias=None, residual=None):
    """The same in numpy int64."""
    out = np.asarray(A, dtype=np.int64) @ np.asarray(W, dtype=np.int64).T
    if bias is not None:
        out = out + np.asarray(bias, dtype=np.int64)
    if residual is not None:
        out = out + np.asarray(residual, dtype=np.int64)
    return out


def q_expected(exact_q, dtype):
    """q leaves the GEMM as (x Wq + b) * head_dim^-0.5 * log2(e), rounded once: the float32 of the exact sum times the float32 constant, one float32
    multiply (on the host), then one rounding to the element type."""
    e32 = exact_q.detach().cpu().double().numpy().astype(np.float32)
    assert np.array_equal(e32.astype(np.float64), exact_q.detach().cpu().double().numpy())
    prod = (e32 * Q_SCALE).astype(np.float32)
    return torch.from_numpy(prod).to(dtype)


def vt_slot(Np):
    """Column of the stored v^T that holds token t: bits 2 and 3 of the token index exchanged (token quads 4..7 and 8..11 of every 16 swapped)."""
    tok = torch.arange(Np)
    return (tok & ~12) | ((tok & 4) << 1) | ((tok & 8) >> 1)


def vt_store(v, B, Np, H):
    """v [B Np][H 64] (token-major) -> the stored v^T [B][H][64][Np]: stored[b][h][c][slot(t)] = v[b Np + t][64 h + c]."""
    logical = v.reshape(B, Np, H, 64).permute(0, 2, 3, 1)
    stored = torch.empty_like(logical.contiguous())
    stored[..., vt_slot(Np).to(v.device)] = logical
    return stored


# ------------------------------------------------------------------------------------------------------------------------------------
# convolution

def same_geometry(i, k, s):
    """timm / TensorFlow "SAME": output ceil(i / s), total padding max((o - 1) s + k - i, 0), the odd pixel at the bottom / right.  -> (o, pad_before)"""
    o = -(-i // s)
    total = max((o - 1) * s + k - i, 0)
    return o, total // 2


def symmetric_geometry(i, k, s, p):
    """nn.Conv2d's symmetric padding p.  -> (o, pad_before)"""
    return (i + 2 * p - k) // s + 1, p


def im2col(x, k, s, pt, pl, oh, ow):
    """x [n][h][w][c] -> [n oh ow][k k c]: row (n, oy, ox), column (ky, kx, c) holds x[n][oy s - pt + ky][ox s - pl + kx][c], zero outside the map."""
    n, h, w, c = x.shape
    dev = x.device
    iy = torch.arange(oh, device=dev)[:, None] * s - pt + torch.arange(k, device=dev)[None, :]   # [oh][k]
    ix = torch.arange(ow, device=dev)[:, None] * s - pl + torch.arange(k, device=dev)[None, :]   # [ow][k]
    oky, okx = (iy >= 0) & (iy < h), (ix >= 0) & (ix < w)
    iyc, ixc = iy.clamp(0, h - 1), ix.clamp(0, w - 1)
    cols = x[:, iyc[:, None, :, None], ixc[None, :, None, :], :]                                   # [n][oh][ow][k][k][c]
    inside = (oky[:, None, :, None] & okx[None, :, None, :]).to(x.dtype)                           # [oh][ow][k][k]
    cols = cols * inside[None, :, :, :, :, None]
    return cols.reshape(n * oh * ow, k * k * c)


def weight_matrix(wt):
    """weight [cout][cin][k][k] -> [cout][(ky, kx, cin)], the K order of ``im2col``."""
    cout = wt.shape[0]
    return wt.permute(0, 2, 3, 1).reshape(cout, -1)


def conv_exact(x, wt, s, pt, pl, oh, ow, bias=None, residuals=()):
    """Convolution of x [n][h][w][cin] with weight [cout][cin][k][k] (+ bias + residuals [n][oh][ow][cout]) in float64 -> [n][oh][ow][cout]."""
    k = wt.shape[2]
    out = gemm_exact(im2col(x.double(), k, s, pt, pl, oh, ow), weight_matrix(wt), bias).reshape(x.shape[0], oh, ow, wt.shape[0])
    for r in residuals:
        out = out + r.double()
    return out


def conv_exact_int(x, wt, s, pt, pl, oh, ow, bias=None, residuals=()):
    """The same with a numpy int64 matmul."""
    k = wt.shape[2]
    out = gemm_exact_int(im2col(x.long(), k, s, pt, pl, oh, ow).numpy(), weight_matrix(wt).numpy(), None if bias is None else bias.numpy())
    out = out.reshape(x.shape[0], oh, ow, wt.shape[0])
    for r in residuals:
        out = out + r.numpy().astype(np.int64)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# other layouts

def patch_rows(x, P):
    """x [n][h][w][c] -> [n (h / P) (w / P)][(dy, dx, c)]: the P x P patches as rows."""
    n, h, w, c = x.shape
    return x.reshape(n, h // P, P, w // P, P, c).permute(0, 1, 3, 2, 4, 5).reshape(n * (h // P) * (w // P), P * P * c)


def patch_embed_exact(x, wt, bias):
    """Conv2d(c, D, P, P) as patches x weights: -> [n][tokens][D] in float64.  weight [D][c][P][P]."""
    P = wt.shape[2]
    rows = patch_rows(x.double(), P)
    return gemm_exact(rows, weight_matrix(wt), bias).reshape(x.shape[0], -1, wt.shape[0])


def conv_transpose_parts(x, wt):
    """ConvTranspose2d with kernel == stride s, first half: the 1 x 1 convolution to (dy, dx, co) channels.  x [n][h][w][cin], weight [cin][cout][s][s]
    -> [n][h][w][s][s][cout] in float64."""
    cin, cout, s, _ = wt.shape
    n, h, w, _ = x.shape
    wm = wt.permute(2, 3, 1, 0).reshape(s * s * cout, cin)
    return gemm_exact(x.reshape(-1, cin), wm).reshape(n, h, w, s, s, cout)


def pixel_shuffle(t, bias=None):
    """[n][h][w][s][s][c] -> [n][h s][w s][c] (+ bias per channel): out[n][y s + dy][x s + dx][c] = t[n][y][x][dy][dx][c]."""
    n, h, w, s, _, c = t.shape
    out = t.permute(0, 1, 3, 2, 4, 5).reshape(n, h * s, w * s, c)
    return out if bias is None else out + bias.double()


def gram_exact(x, stride):
    """sum_p x_p x_p^T [n][c][c] and sum_p x_p [n][c] over the pixels a 1 x 1 convolution of this stride reads, in float64."""
    xs = x[:, ::stride, ::stride, :].double()
    xs = xs.reshape(xs.shape[0], -1, xs.shape[3])
    return xs.transpose(1, 2) @ xs, xs.sum(1)


# ------------------------------------------------------------------------------------------------------------------------------------
# attention cases (the kernel takes q | k and v^T as inputs)

def _bits(idx, nb):
    return (idx[..., None] >> torch.arange(nb)) & 1


def attention_perms(B, N, H, seed=0):
    """A target key per (image, head, query): head 0 reversed (the running maximum rises at the last key tile for the first queries), head 1 the
    identity, the others seeded random permutations; all differ."""
    g = _gen(seed * 86028121 + B * 131 + N * 17 + H)
    perm = torch.empty(B, H, N, dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            if h == 0:
                perm[b, h] = torch.arange(N - 1, -1, -1).roll(-b)
            elif h == 1:
                perm[b, h] = torch.arange(N).roll(-b)
            else:
                perm[b, h] = torch.randperm(N, generator=g)
    return perm


def attention_selection(B, N, H, seed=0):
    """Selection case.  Key j carries its index's bits and their complements in 2 nb of the head's 64 dimensions (a per-head choice of dimensions);
    query i carries -256 times the opposite pattern of its target t: q'.k = -256 * (Hamming distance of j and t): 0 for the target, <= -256 for every
    other key.  exp2 of the others is exactly 0 in float32, l = 1, and the output is v[target] bit for bit.  The padded key rows N..Np-1 hold copies
    of real keys' codes (and their own non-zero v): a broken key mask gives l = 2.  The other dimensions of k are random, those of q zero.
    -> qk [B Np][2 D], v [B Np][D] (token-major, before ``vt_store``), expected [B][N][D], perm [B][H][N]; all int64."""
    Np, D = (N + 63) // 64 * 64, H * 64
    nb = max(1, int(math.ceil(math.log2(Np))))
    assert 2 * nb <= 64
    g = _gen(seed * 9999991 + B * 131 + N * 17 + H)
    perm = attention_perms(B, N, H, seed)
    key_code = torch.arange(Np)
    pad = torch.arange(N, Np)
    key_code[N:] = (pad * 7 + 3) % N                     # a real key's code on every padded row
    kb = _bits(key_code, nb)                             # [Np][nb]
    q = torch.zeros(B, Np, H, 64, dtype=torch.int64)
    k = draw(g, (B, Np, H, 64), 4)
    for h in range(H):
        dims = torch.randperm(64, generator=g)[:2 * nb]
        k[:, :, h, dims[:nb]] = kb
        k[:, :, h, dims[nb:]] = 1 - kb
        for b in range(B):
            tb = _bits(perm[b, h], nb)                   # [N][nb]
            q[b, :N, h, dims[:nb]] = -256 * (1 - tb)
            q[b, :N, h, dims[nb:]] = -256 * tb
    v = torch.randint(-128, 128, (B, Np, H, 64), generator=g, dtype=torch.int64)
    v[:, N:][v[:, N:] == 0] = 5
    expected = torch.empty(B, N, H, 64, dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            expected[b, :, h] = v[b, perm[b, h], h]
    qk = torch.cat([q.reshape(B * Np, D), k.reshape(B * Np, D)], dim=1)
    return qk, v.reshape(B * Np, D), expected.reshape(B, N, D), perm


def attention_scores(qk, B, Np, H):
    """q'.k for every (image, head, query, key) in int64: [B][H][Np][Np]."""
    D = H * 64
    q = qk[:, :D].reshape(B, Np, H, 64).permute(0, 2, 1, 3)
    k = qk[:, D:].reshape(B, Np, H, 64).permute(0, 2, 1, 3)
    return torch.from_numpy(np.matmul(q.numpy(), k.numpy().transpose(0, 1, 3, 2)))


def attention_counting(B, N, H, seed=0):
    """Counting case.  q' = 0: every real key has weight 1 and l = N.  v[j][c] = 127 where j = c (mod H 64), else 0 -- on the padded rows too, so that
    a padded key that is counted shows.  The exact output is 127 count_c / N with count_c = #{j < N: j = c (mod D)}, the same for every query.
    -> qk [B Np][2 D] int64, v [B Np][D] int64, expected [D] float64."""
    Np, D = (N + 63) // 64 * 64, H * 64
    g = _gen(seed * 7777777 + B * 131 + N * 17 + H)
    k = draw(g, (B * Np, D), 4)
    qk = torch.cat([torch.zeros(B * Np, D, dtype=torch.int64), k], dim=1)
    j = torch.arange(Np)
    v1 = torch.zeros(Np, D, dtype=torch.int64)
    v1[j, j % D] = 127
    v = v1.repeat(B, 1)
    count = torch.bincount(torch.arange(N) % D, minlength=D).double()
    return qk, v, 127.0 * count / N


# ------------------------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_exact_gpu.py (tests/test_exact_reference_cpu.py checks every generator's conditions at each of them)

# (M, N, K, switches): hive_vit_linear, epilogues 0 / 2 / 2 in place
LINEAR_CASES = [
    (129, 128, 64, {"HIVE_GEMM_TILE": "128", "HIVE_GEMM_RING": "2"}),    # one K-step: the ring is shorter than its depth; the last row tile holds one row
    (129, 128, 64, {"HIVE_GEMM_TILE": "128", "HIVE_GEMM_RING": "4"}),
    (200, 256, 704, {"HIVE_SPLITK": "0"}),                               # 11 K-steps: an odd number, and ways that do not divide it
    (200, 256, 704, {}),
    (200, 256, 704, {"HIVE_SPLITK": "5"}),
    (200, 256, 704, {"HIVE_SPLITK": "7"}),
    (200, 256, 704, {"HIVE_SPLITK": "5", "HIVE_GEMM_RING": "2"}),
    (200, 256, 704, {"HIVE_SPLITK": "0", "HIVE_GEMM_RING": "2"}),
    (1216, 768, 3072, {}),                                               # batch-1 fc2 under the launch policy: split four ways on the deep ring at 256 CUs
    (257, 256, 128, {"HIVE_GEMM_TILE": "256"}),                          # the 256-tile kernel forced; the last row tile holds one row
    (9800, 2048, 64, {}),                                                # the 256-tile kernel by the rule: 39 x 8 = 312 tiles on 256 persistent workgroups, ragged last row tile
]
GELU_CASES = [(129, 128, 64, {"HIVE_GEMM_TILE": "128", "HIVE_GEMM_RING": "2"}), (200, 256, 704, {}), (200, 256, 704, {"HIVE_SPLITK": "5"}),
              (257, 256, 128, {"HIVE_GEMM_TILE": "256"}), (1216, 768, 3072, {})]
QKV_CASES = [(1, 1201, 768, 12), (2, 77, 768, 12), (3, 130, 768, 12), (1, 577, 1024, 16)]                       # (B, N, D, H)
QKV_TWO_PER_CU_CASE = (2, 1201, 768, 12)  # 19 x 18 = 342 tiles: more than the CUs, at most two workgroups per CU -- merged on the two-stage ring under HIVE_QKV_MERGE=2 only
ATTENTION_CASES = [(1, 1201, 768, 12), (2, 77, 768, 12), (1, 64, 768, 12), (3, 130, 768, 12), (1, 577, 1024, 16)]

# (n, cin, cout, k, stride, h, w, padding, switches, expected path at 256 CUs or None).  padding: "same" (timm) or the symmetric amount.
CONV_CASES = [
    (1, 64, 256, 3, 1, 255, 257, 1, {}, ("tile", 256, 256)),             # M = 65,535: 256 tiles of 256 rows, the last one ragged
    (1, 64, 128, 3, 1, 255, 257, 1, {}, ("tile", 256, 128)),
    (1, 64, 64, 3, 1, 255, 257, 1, {}, ("tile", 256, 64)),
    (1, 256, 256, 3, 1, 33, 41, 1, {"HIVE_CONV_DEEP": "0"}, ("tile", 128, 256)),   # tiles end mid-row
    (1, 256, 128, 3, 1, 33, 41, 1, {"HIVE_CONV_DEEP": "0"}, ("tile", 128, 128)),
    (1, 256, 256, 3, 1, 33, 41, 1, {}, ("deep", 4)),
    (3, 256, 256, 3, 1, 7, 9, 1, {"HIVE_CONV_DEEP": "0"}, ("tile", 128, 256)),     # every pixel near a border
    (3, 256, 256, 3, 1, 7, 9, 1, {}, ("deep", 4)),
    (1, 256, 256, 3, 1, 15, 20, 1, {"HIVE_SPLITK": "0"}, ("deep", 1)),
    (1, 256, 256, 3, 1, 15, 20, 1, {}, ("deep", 4)),
    (1, 256, 256, 3, 1, 15, 20, 1, {"HIVE_SPLITK": "2"}, ("deep", 2)),
    (1, 256, 256, 3, 1, 15, 20, 1, {"HIVE_SPLITK": "5"}, ("deep", 5)),
    (1, 256, 256, 3, 1, 15, 20, 1, {"HIVE_SPLITK": "7"}, ("deep", 7)),
    (1, 64, 256, 3, 1, 16, 16, 1, {"HIVE_SPLITK": "0"}, ("deep", 1)),
    (1, 64, 256, 3, 1, 16, 16, 1, {}, ("deep", 1)),
    (1, 64, 256, 3, 1, 16, 16, 1, {"HIVE_SPLITK": "2"}, ("deep", 2)),
    (1, 64, 256, 3, 1, 16, 16, 1, {"HIVE_SPLITK": "5"}, ("deep", 5)),
    (1, 64, 256, 3, 1, 16, 16, 1, {"HIVE_SPLITK": "7"}, ("deep", 7)),
    (2, 128, 128, 3, 2, 24, 32, "same", {}, None),                       # stride 2 "SAME", even input: pad 0 top / left, 1 bottom / right
    (2, 128, 128, 3, 2, 24, 32, "same", {"HIVE_CONV_DEEP": "0"}, None),
    (2, 128, 128, 3, 2, 23, 31, "same", {}, None),                       # odd input: pad 1 / 1
    (2, 128, 128, 3, 2, 23, 31, "same", {"HIVE_CONV_DEEP": "0"}, None),
    (2, 64, 128, 3, 2, 15, 20, 1, {}, None),                             # stride 2, symmetric padding 1
    (2, 64, 128, 3, 2, 15, 20, 1, {"HIVE_CONV_DEEP": "0"}, None),
    (2, 64, 64, 3, 1, 24, 32, "same", {}, ("tile", 256, 64)),
    (2, 64, 256, 1, 1, 24, 32, "same", {}, None),                        # 1 x 1
    (2, 64, 256, 1, 1, 24, 32, "same", {"HIVE_CONV_DEEP": "0"}, None),
    (2, 64, 64, 1, 1, 24, 32, "same", {}, ("tile", 256, 64)),
    (2, 256, 128, 1, 2, 24, 32, "same", {}, None),                       # 1 x 1 stride 2
    (2, 256, 128, 1, 2, 23, 31, "same", {"HIVE_CONV_DEEP": "0"}, None),
]
# (n, cin, cout, k, stride, h, w, padding, switches, expected path at 256 CUs, expected tile rows of the statistics): operands in -2..2
CONV_STATS_CASES = [
    (2, 64, 128, 3, 1, 24, 32, 1, {"HIVE_CONV_DEEP": "0"}, ("tile", 128, 128), 128),   # conv_kernel, 128-row tiles (tiles straddle the two images)
    (2, 64, 64, 1, 1, 40, 56, "same", {}, ("tile", 256, 64), 256),                    # conv_kernel, 256-row tiles
    (2, 64, 128, 3, 1, 24, 32, 1, {}, ("deep", 1), 128),                              # conv_deep_kernel (12 tiles of 128 rows <= CUs; 9 K-steps: no split)
]
STEM_CASES = [(1, 96, 128), (1, 61, 77), (2, 64, 64)]                     # (n, h, w)
PATCH_CASES = [(2, 96, 160, 256), (1, 48, 80, 128)]                       # (n, h, w, D): 16 x 16 patches of a 3-channel frame
CONV_TRANSPOSE_CASES = [(2, 64, 64, 4, 6, 10), (1, 128, 64, 2, 7, 5)]     # (n, cin, cout, s, h, w)
GRAM_CASES = [(2, 64, 256, 1, 20, 24), (2, 128, 512, 1, 37, 45), (1, 256, 1024, 1, 30, 40), (2, 256, 512, 2, 47, 61), (1, 64, 256, 2, 24, 32)]  # (n, cin, cout, stride, h, w)


def conv_geometry(k, s, h, w, padding):
    """(pad_top, pad_left, oh, ow) of a case."""
    if padding == "same":
        (oh, pt), (ow, pl) = same_geometry(h, k, s), same_geometry(w, k, s)
    else:
        (oh, pt), (ow, pl) = symmetric_geometry(h, k, s, padding), symmetric_geometry(w, k, s, padding)
    return pt, pl, oh, ow


def case_conv_operands(case, r=4, p_zero=None):
    n, cin, cout, k, s, h, w, padding = case[:8]
    pt, pl, oh, ow = conv_geometry(k, s, h, w, padding)
    return conv_operands(n, cin, cout, k, h, w, oh, ow, r=r, p_zero=p_zero)


def stem_operands(n, h, w):
    """The 7 x 7 / 2 "SAME" stem: a 3-channel frame in -4..4, weights in -2..2 (so that the GroupNorm sums of squares stay below 2^24)."""
    (oh, _), (ow, _) = same_geometry(h, 7, 2), same_geometry(w, 7, 2)
    g = _gen(1299709 + n * 1009 + h * 3 + w)
    x = ring_border(draw(g, (n, h, w, 3), 4), base=5)
    wt = draw(g, (64, 3, 7, 7), 2, 0.1)
    wm = weight_matrix(wt)
    bound = upper_bound(x, wm)
    check_conditions(x, wm, bound)
    return x, wt, bound


# the launch rules of vit.hip launch_gemm / conv.hip launch_conv_t, restated: the GPU tests assert that a case reaches the path it was chosen for
def splitk_ways(tiles, kt, cus):
    return 1 if tiles <= 0 or kt < 32 else max(1, min(4, cus // tiles))


def gemm_path(M, N, K, cus, env):
    """("tile256", tiles) or ("tile128", split_k, deep) for hive_vit_linear on ``cus`` CUs under the switches ``env``."""
    force = env.get("HIVE_GEMM_TILE")
    tiles256 = -(-M // 256) * (N // 256)
    rounds = -(-tiles256 // cus)
    fills = tiles256 * 5 >= rounds * cus * 3
    if N % 256 == 0 and ((force and force[0] == "2") or (not force and fills)):
        return ("tile256", tiles256)
    tiles = -(-M // 128) * (N // 128)
    sk = env.get("HIVE_SPLITK")
    split = max(1, min(int(sk), K // 64)) if sk is not None else splitk_ways(tiles, K // 64, cus)
    if tiles > 4096:
        split = 1
    ring = env.get("HIVE_GEMM_RING")
    deep = ring[0] == "4" if ring else tiles * split <= cus
    return ("tile128", split, deep)


def conv_path(M, cin, cout, k, cus, env):
    """("deep", split_k) or ("tile", tm, tn) for hive_nhwc_conv on ``cus`` CUs under the switches ``env``."""
    tn = 256 if cout % 256 == 0 else (128 if cout % 128 == 0 else 64)
    tm = 256
    if tn >= 128:
        per = cout // tn
        t256, t128 = -(-M // 256) * per, -(-M // 128) * per
        r256, r128 = -(-t256 // cus), -(-t128 // cus)
        if t256 < cus or r128 * 128 * 100 < r256 * 256 * 85:
            tm = 128
    tiles128 = -(-M // 128) * (cout // 128)
    if env.get("HIVE_CONV_DEEP", "1")[0] != "0" and cout % 128 == 0 and tiles128 <= cus and tiles128 <= 4096:
        kt = k * k * (cin // 64)
        sk = env.get("HIVE_SPLITK")
        split = max(1, min(int(sk), kt)) if sk is not None else splitk_ways(tiles128, kt, cus)
        return ("deep", max(1, min(split, cus // tiles128)))
    return ("tile", tm, tn)


# ------------------------------------------------------------------------------------------------------------------------------------
# the bottleneck convolution (csrc/bneck.hip): GroupNorm + ReLU applied while the 3 x 3 convolution stages its input
#
# The test hands the kernel the sums of the GroupNorm in front itself, so the statistics are what it chooses: an integer mean m in -2..2 and a variance v in
# {0, 0.75} per (image, group).  With eps = 0.25, gn_finalize_tiles_kernel (double: mean = s / cnt, var = q / cnt - mean^2, rstd = (float)(1 / sqrt(var + eps)))
# gives mean = m and rstd = 2 or 1 exactly.  gamma = +-1 and an integer beta make a = rstd gamma and b = beta - m a small integers, and
# u = relu(t a + b) an integer of at most 16: the convolution's input, product by product exact, padded with zeros of u (not with relu(b)).

BNECK_EPS = 0.25
BNECK_TH, BNECK_TW = 16, 32   # the kernel's output tile
# (n or None, h, w, keep, rows): n None = chosen by the CU count so that 2 cus < tiles < 3 cus (``bneck_batch``); keep = the share of non-zero weights (0.25
# where the kernel leaves GroupNorm sums: the sums of squares of a tile stay below 2^24); rows = "image" (one row of input partials per image) or
# "straddle" (rows of 2/3 of an image: most hold the pieces of two images)
BNECK_CASES = [
    (2, 24, 32, 0.25, "image"),       # sums; the last tile row is ragged (8 of 16 rows)
    (3, 37, 45, 0.5, "straddle"),     # ragged both ways, no sums
    (2, 16, 32, 0.25, "image"),       # exactly one tile per image; sums
    (1, 1, 1, 0.5, "image"),
    (1, 3, 70, 0.5, "image"),         # three tiles in a row, the last one 6 columns wide
    (None, 17, 33, 0.5, "image"),     # 4 mostly empty tiles per image, more than two trips of the tile loop, no sums
    (None, 24, 32, 0.25, "image"),    # the same with sums
]


def bneck_tiles(h, w):
    """(tiles per image, tiles along x)."""
    tx, ty = -(-w // BNECK_TW), -(-h // BNECK_TH)
    return tx * ty, tx


def bneck_has_sums(h, w):
    """launch_bneck's rule: the kernel leaves GroupNorm sums where the width is whole tiles and the tiles per image divide the pixels."""
    return w % BNECK_TW == 0 and (h * w) % bneck_tiles(h, w)[0] == 0


def bneck_batch(case, cus):
    """The case's batch on a device of ``cus`` CUs (grid = min(tiles, cus)); for the multi-trip cases the premise is asserted: 2 cus < tiles < 3 cus, so
    some workgroups make three trips and the rest two, and a workgroup's consecutive trips (cus tiles apart) lie in different images."""
    n, h, w = case[:3]
    if n is not None:
        return n
    per = bneck_tiles(h, w)[0]
    n = (5 * cus // 2) // per
    assert 2 * cus < n * per < 3 * cus and cus >= per, f"{cus} CUs: {n * per} tiles do not lie between two and three trips"
    return n


def bneck_statistics(n):
    """m [n][32] int64 in -2..2 and v [n][32] float64 in {0, 0.75}, by formula from the pair index i = 32 img + g as norm_reference.gn_offset: m changes between
    neighbouring groups and between ANY two images whose distance is no multiple of 5; v changes between two consecutive images in two cases of three."""
    img, g = torch.arange(n)[:, None], torch.arange(32)[None, :]
    i = img * 32 + g
    m = (i * 7 + 3) % 5 - 2
    v = ((img + g + img // 3) % 2).double() * 0.75
    return m, v


def bneck_partials(m, v, hw, tile_rows):
    """The input partials float64 [tiles][2][2][64] in the layout of norm_reference.gn_tile_partials (tiles of ``tile_rows`` rows of the [n hw][64] matrix; h = 0:
    the rows of the image the tile starts in, h = 1: those of the next one): a piece of r rows of image i holds sum = r m and sq = r (m^2 + v) in both
    channels of a group -- over an image hw m and hw (m^2 + v): mean m, variance v.  All are multiples of 1/4 below 2^24: exact floats."""
    n = m.shape[0]
    mc, vc = m.double().repeat_interleave(2, dim=1), v.repeat_interleave(2, dim=1)  # per channel
    assert 0 < tile_rows <= hw
    tiles = -(-n * hw // tile_rows)
    partial = torch.zeros(tiles, 2, 2, 64, dtype=torch.float64)
    for t in range(tiles):
        r0, r1 = t * tile_rows, min((t + 1) * tile_rows, n * hw)
        split = min(r1, (r0 // hw + 1) * hw)
        for h_, (img, r) in enumerate(((r0 // hw, split - r0), (r0 // hw + 1, r1 - split))):
            if r > 0:
                partial[t, h_, 0], partial[t, h_, 1] = r * mc[img], r * (mc[img] ** 2 + vc[img])
    assert torch.equal(partial.float().double(), partial) and float(partial.abs().max()) < LIMIT
    return partial


def bneck_finalize(partial, n, hw, tile_rows, eps=BNECK_EPS):
    """gn_finalize_tiles_kernel restated (float64, C = 64, G = 32): (mean, rstd) [n][32] as it stores them, in float32."""
    mean, rstd = np.empty((n, 32), dtype=np.float32), np.empty((n, 32), dtype=np.float32)
    p = partial.numpy()
    for img in range(n):
        t0, t1 = img * hw // tile_rows, (img * hw + hw - 1) // tile_rows
        s, q = np.zeros(64), np.zeros(64)
        for t in range(t0, t1 + 1):
            h_ = 0 if t * tile_rows // hw == img else 1
            s, q = s + p[t, h_, 0], q + p[t, h_, 1]
        s, q, cnt = s.reshape(32, 2).sum(1), q.reshape(32, 2).sum(1), float(hw * 2)
        mu = s / cnt
        var = np.maximum(q / cnt - mu * mu, 0.0)
        mean[img], rstd[img] = mu.astype(np.float32), (1.0 / np.sqrt(var + float(np.float32(eps)))).astype(np.float32)
    return mean, rstd


def bneck_operands(n, h, w, keep, rows, seed=0):
    """t [n][h][w][64] in -2..2 with a border ring of 3..5, the input partials [tiles][2][2][64] (float64) and their tile rows, gamma [64] +-1, beta [64] in
    -2..2, weight [64][64][3][3] in {-1, 0, 1}, a and b [n][64] (int64: y = t a + b), and the bound.  Asserts every condition named above."""
    hw = h * w
    g = _gen(seed * 22801763 + n * 1009 + h * 3 + w)
    m, v = bneck_statistics(n)
    tile_rows = hw if rows == "image" else max(1, 2 * hw // 3)
    partial = bneck_partials(m, v, hw, tile_rows)
    mean, rstd = bneck_finalize(partial, n, hw, tile_rows)
    want_rstd = torch.where(v == 0, 2.0, 1.0)
    assert np.array_equal(mean.astype(np.float64), m.double().numpy()) and np.array_equal(rstd.astype(np.float64), want_rstd.numpy()), "mean, rstd are not m and 2 / 1"
    if n > 1:  # a neighbouring image's statistics are wrong ones
        assert bool((m[1:] != m[:-1]).all()) and float((want_rstd[1:] != want_rstd[:-1]).double().mean()) > 0.5, "consecutive images share statistics"
        assert bool((m[:, 1:] != m[:, :-1]).all())
    gamma = torch.randint(0, 2, (64,), generator=g, dtype=torch.int64) * 2 - 1
    beta = torch.tensor([-2, -1, 0, 0, 1, 1, 1, 2, 2, 2])[torch.randint(0, 10, (64,), generator=g)]  # (more often positive: b > 0 for more than 40 % of the pairs)
    a = want_rstd.long().repeat_interleave(2, dim=1) * gamma[None, :]
    b = beta[None, :] - m.repeat_interleave(2, dim=1) * a
    t = draw(g, (n, h, w, 64), 2)
    if h >= 3 and w >= 3:
        ring_border(t, base=3)
    wt = draw(g, (64, 64, 3, 3), 1, 1.0 - keep)
    u = bneck_normalised(t, a, b)
    assert 0 <= int(u.min()) and int(u.max()) <= 16
    frac = float((u != 0).double().mean())
    assert frac >= 0.4, f"only {frac:.3f} of the normalised input is non-zero"
    shown = float((b > 0).double().mean())
    assert shown >= 0.4, f"relu(b) != 0 for only {shown:.3f} of the (image, channel) pairs: a normalised zero in the padding would not show"
    wm = weight_matrix(wt)
    assert bool((wm != 0).any(dim=0).all()), "a K position has no non-zero weight in any output channel"
    bound = upper_bound(u, wm)
    assert bound < LIMIT
    return t, partial, tile_rows, gamma, beta, wt, a, b, bound


def bneck_normalised(t, a, b):
    """u = relu(t a + b): the tensor the convolution reads (the same dtype and device as t; a, b [n][64])."""
    return (t * a[:, None, None, :].to(t.device, t.dtype) + b[:, None, None, :].to(t.device, t.dtype)).clamp_min(0)


def conv3x3_exact(x, wt, chunk=16):
    """3 x 3 convolution, stride 1, one pixel of zeros all round, in float64 on x's device, ``chunk`` images at a time (the im2col matrix stays small)."""
    n, h, w, _ = x.shape
    wd = wt.to(x.device)
    return torch.cat([conv_exact(x[i:i + chunk].double(), wd, 1, 1, 1, h, w) for i in range(0, n, chunk)])


def bneck_tile_sums(y, h, w):
    """Sum and sum of squares of y [n][h][w][64] (float64) over the pixels of every 16 x 32 tile, tiles numbered as the kernel numbers them: [tiles][2][64]."""
    n = y.shape[0]
    per, tx = bneck_tiles(h, w)
    yy, xx = torch.arange(h, device=y.device)[:, None], torch.arange(w, device=y.device)[None, :]
    tile = ((yy // BNECK_TH) * tx + xx // BNECK_TW).reshape(-1)
    idx = (torch.arange(n, device=y.device)[:, None] * per + tile[None, :]).reshape(-1)
    rows = y.reshape(n * h * w, 64)
    out = torch.zeros(n * per, 2, 64, dtype=torch.float64, device=y.device)
    out[:, 0].index_add_(0, idx, rows)
    out[:, 1].index_add_(0, idx, rows * rows)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# bilinear x2 upsampling, align_corners=True (csrc/dpt_ops.hip upsample2x_kernel / upsample2x_lds_kernel, and phase (b) of csrc/dpt_head.hip): both files
# are built without contraction, so the result is a fixed sequence of float32 operations -- restated here in numpy float32, one rounded operation per step

UPSAMPLE_CASES = [(1, 8, 1, 1), (1, 8, 1, 9), (1, 16, 9, 1), (2, 32, 7, 5), (1, 128, 24, 32), (2, 256, 15, 20), (1, 1024, 6, 5)]  # (N, C, H, W); C = 1024: the gather form by the rule


def upsample_axis(size):
    """Per output index 0 .. 2 size - 1: (i0, i1, l0, l1) -- s = f32(size - 1) / f32(2 size - 1), f = s * f32(o), i0 = int(f), i1 = min(i0 + 1, size - 1),
    l1 = f - f32(i0), l0 = 1 - l1, every operation in float32."""
    one = np.float32
    out = 2 * size
    s = one(size - 1) / one(out - 1) if out > 1 else one(0)
    f = s * np.arange(out).astype(np.float32)
    i0 = f.astype(np.int32)
    i1 = np.minimum(i0 + 1, size - 1)
    l1 = f - i0.astype(np.float32)
    l0 = one(1) - l1
    assert f.dtype == l0.dtype == l1.dtype == np.float32 and int(i0.min()) >= 0 and int(i1.max()) <= size - 1
    return i0, i1, l0, l1


def upsample2x_blend_f32(v):
    """v float32 [N][H][W][C] -> float32 [N][2 H][2 W][C]: y = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11), before the rounding to the element type."""
    assert v.dtype == np.float32
    y0, y1, h0, h1 = upsample_axis(v.shape[1])
    x0, x1, w0, w1 = upsample_axis(v.shape[2])
    w0, w1, h0, h1 = w0[None, None, :, None], w1[None, None, :, None], h0[None, :, None, None], h1[None, :, None, None]
    r0, r1 = v[:, y0], v[:, y1]
    top = w0 * r0[:, :, x0] + w1 * r0[:, :, x1]
    bot = w0 * r1[:, :, x0] + w1 * r1[:, :, x1]
    out = h0 * top + h1 * bot
    assert out.dtype == np.float32
    return out


def upsample2x_f32(x, bias=None):
    """x [N][H][W][C] of a 16-bit type (CPU) -> [N][2 H][2 W][C] of that type: the optional bias [C] first, (T)(x + b) with the sum in float32; the blend
    in float32; one rounding to the element type."""
    dtype = x.dtype
    assert dtype in (torch.bfloat16, torch.float16)
    v = x.float()
    if bias is not None:
        v = (v + bias.float()[None, None, None, :]).to(dtype).float()
    assert bool(torch.isfinite(v).all())
    return torch.from_numpy(upsample2x_blend_f32(v.numpy())).to(dtype)


def upsample_operands(N, C, H, W, dtype, seed=0):
    """x [N][H][W][C] and bias [C] of the element type: normal values x 2^(-6..6) (at least 2^-10 in magnitude), one in sixteen an exact zero, one in sixteen within a few steps of the largest
    finite value (either sign); the bias in -4..4 in steps of 1/8 (x + bias stays finite: half a step of the largest values is 16 in float16)."""
    g = _gen(seed * 2750159 + N * 1009 + C * 131 + H * 3 + W)
    shape = (N, H, W, C)
    x = torch.randn(shape, generator=g, dtype=torch.float32) * torch.exp2(torch.randint(-6, 7, shape, generator=g).float())
    x = torch.where(x.abs() < 2.0 ** -10, torch.copysign(torch.full_like(x, 2.0 ** -10), x), x)  # (no subnormal inputs)
    kind = torch.randint(0, 16, shape, generator=g)
    big = torch.finfo(dtype).max * (1.0 - torch.randint(0, 8, shape, generator=g).float() * torch.finfo(dtype).eps) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    x = torch.where(kind == 0, torch.zeros_like(x), torch.where(kind == 1, big, x)).to(dtype)
    bias = (torch.randint(-32, 33, (C,), generator=g).float() / 8.0).to(dtype)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite((x.float() + bias.float()).to(dtype)).all())
    if x.numel() >= 256:
        assert bool((x == 0).any()) and bool((x.float().abs() > 0.99 * torch.finfo(dtype).max).any())
    tiny = torch.finfo(dtype).tiny
    assert bool(((x == 0) | (x.float().abs() >= tiny)).all()), "a subnormal input"
    return x, bias


# ------------------------------------------------------------------------------------------------------------------------------------
# the fused depth head (csrc/dpt_head.hip): x2 upsampling -> conv 3 x 3 (128 -> 32) + bias -> ReLU -> conv 1 x 1 + bias -> ReLU -> inversion -> hand-off
#
# x in 1..5 and b0 in 0..3: every upsampled value lies in [1, 8], a multiple of 2^-10 (float16) or 2^-7 (bfloat16).  w3 in -1..1 and an integer b3 in -8..8: a
# 3 x 3 sum has sum |terms| <= 1152 * 8 + 8 = 9224 < 2^14, i.e. below 2^24 in units of 2^-10: exact in float32 in any order, the four-wave exchange included.
# The same holds for the 1 x 1 sums while sum |feat w1| + |b1| < 2^14 (asserted per pixel).  From there the epilogue is norm_reference.head_tail_reference.

HEAD_UNIT = 2.0 ** -10
HEAD_SCALE, HEAD_SHIFT, HEAD_DEPTH_SCALE, HEAD_MAX_DEPTH = 2.0 ** -8, 0.1378, 0.001, 10.0
HEAD_TH, HEAD_TW = 8, 16      # the kernel's output tile
HEAD_GRID = "grid"            # every (b0, non_negative, invert), and each output on its own
# (N or None, H, W, variants): N None = chosen by the CU count so that 4 cus < tiles < 6 cus (the grid is 2 cus: ``head_batch``); variants = HEAD_GRID or a
# list of (b0 given, non_negative, invert)
HEAD_CASES = [
    (1, 2, 2, [(False, 1, 1)]),                   # the 10 x 18 patch is larger than the 4 x 4 output on all sides
    (1, 2, 40, HEAD_GRID),                        # 5 tiles in a row, half of each below the map
    (2, 13, 21, [(True, 1, 0)]),                  # ragged both ways
    (1, 48, 64, [(False, 1, 1)]),                 # 96 whole tiles, as the network calls it (no b0)
    (None, 5, 9, [(True, 1, 1), (False, 1, 1)]),  # 4 ragged tiles per image; two and three trips of the tile loop: the LDS-DMA prefetch of the next tile's patch
]


def head_tiles(H, W):
    return -(-2 * H // HEAD_TH) * -(-2 * W // HEAD_TW)


def head_batch(case, cus):
    N, H, W = case[:3]
    if N is not None:
        return N
    per = head_tiles(H, W)
    N = (5 * cus) // per
    assert 4 * cus < N * per < 6 * cus, f"{cus} CUs: {N * per} tiles do not lie between two and three trips of a grid of {2 * cus}"
    return N


def head_variants(case):
    if case[3] != HEAD_GRID:
        return list(case[3])
    return [(b0, nn, inv) for b0 in (False, True) for nn in (0, 1) for inv in (0, 1)]


def head_sums(x, b0, w3, dtype, device="cpu"):
    """The exact 3 x 3 sums float64 [N][2 H][2 W][32] (on ``device``) over the restated upsampling of x + b0 in the element type, zero padding.  Asserts that
    the upsampled values lie in [1, 8] and are multiples of 2^-10."""
    up = upsample2x_f32(x.to(dtype), None if b0 is None else b0.to(dtype)).double()
    assert float(up.min()) >= 1.0 and float(up.max()) <= 8.0 and torch.equal(torch.round(up / HEAD_UNIT) * HEAD_UNIT, up)
    return conv3x3_exact(up.to(device), w3, chunk=8)


def head_pre(feat, b3, w1, b1):
    """The 1 x 1 sums before the last ReLU, float64 [pixels], and the largest sum |relu(feat + b3) w1| + |b1| of a pixel."""
    f = (feat.reshape(-1, 32) + b3.double().to(feat.device)).clamp_min(0.0)
    w = w1.double().to(feat.device)
    return f @ w + float(b1), float((f @ w.abs()).max()) + abs(float(b1))


def head_operands(N, H, W, seed=0):
    """x [N][H][W][128] in 1..5, b0 [128] in 0..3, w3 [32][128][3][3] in -1..1, b3 [32] in -8..8, w1 [32] in -2..2 (all int64), and the integers b1 = (without b0,
    with b0): minus the median of the 1 x 1 sums of the float16 form (every form's share of clipped pixels is asserted by ``head_expected``)."""
    g = _gen(seed * 39916801 + N * 1009 + H * 3 + W)
    x = torch.randint(1, 6, (N, H, W, 128), generator=g, dtype=torch.int64)
    b0 = torch.randint(0, 4, (128,), generator=g, dtype=torch.int64)
    w3, b3, w1 = draw(g, (32, 128, 3, 3), 1), draw(g, (32,), 8), draw(g, (32,), 2)
    assert bool((weight_matrix(w3) != 0).any(dim=0).all()) and int((w1 != 0).sum()) >= 16
    if N > 1:
        assert bool((x[1:] != x[:-1]).reshape(N - 1, -1).any(dim=1).all()), "two consecutive images are equal"
    b1 = tuple(-int(torch.round(head_pre(head_sums(x, b, w3, torch.float16), b3, w1, 0)[0].median())) for b in (None, b0))
    return x, b0, w3, b3, w1, b1


def head_expected(feat, b3, w1, b1, non_negative, invert):
    """(depth float32, millimetres uint16, metres float32) [pixels] from the exact 3 x 3 sums: norm_reference.head_tail_reference on them in units of 2^-10 (its
    operands are integers then; scale / 2^10 times the integer accumulator is the product scale * acc, exactly).  Without the inversion the depth is the
    accumulator itself: scaled back exactly, and handed off in millimetres as the epilogue states it.  Asserts the exactness condition of the 1 x 1
    sums and that the last ReLU clips between 10 % and 90 % of the pixels."""
    pre, worst = head_pre(feat, b3, w1, b1)
    assert worst < 2 ** 14, f"sum |feat w1| + |b1| reaches {worst}"
    clipped = float((pre < 0).double().mean())
    assert 0.1 <= clipped <= 0.9, f"the last ReLU clips {clipped:.3f} of the pixels"
    one = np.float32
    units = (feat.reshape(-1, 32) / HEAD_UNIT).cpu().numpy()
    args = (units, b3.double().numpy() / HEAD_UNIT, True, w1.numpy().astype(np.float32), float(b1) / HEAD_UNIT, non_negative)
    if invert:
        return R.head_tail_reference(*args, True, HEAD_SCALE * HEAD_UNIT, HEAD_SHIFT, HEAD_DEPTH_SCALE, HEAD_MAX_DEPTH)
    acc = R.head_tail_reference(*args, False, 1.0, 0.0, HEAD_DEPTH_SCALE, HEAD_MAX_DEPTH)[0]
    depth = acc * one(HEAD_UNIT)
    assert np.array_equal(depth.astype(np.float64), pre.clamp_min(0.0).cpu().numpy() if non_negative else pre.cpu().numpy())
    mm = np.minimum(np.maximum(depth * one(1000), one(0)), one(65535)).astype(np.int32).astype(np.uint16)
    return depth, mm, R.depth_mm_to_m_reference(mm, HEAD_DEPTH_SCALE, HEAD_MAX_DEPTH)
