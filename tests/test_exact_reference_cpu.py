"""tests/exact_reference.py checked on the CPU: every reference against a direct nested-loop numpy version of the operation's definition at tiny
shapes, the float64-matmul forms against the int64 forms, and every generator's exactness (bound < 2^24) and coverage conditions at every shape
tests/test_exact_gpu.py uses."""
import math

import numpy as np
import pytest
import torch

import exact_reference as E


def _loop_conv(x, wt, s, pt, pl, oh, ow):
    """out[n][oy][ox][co] = sum_{ky, kx, c} x[n][oy s - pt + ky][ox s - pl + kx][c] w[co][c][ky][kx], taps outside the map skipped."""
    x, wt = x.numpy().astype(np.int64), wt.numpy().astype(np.int64)
    n, h, w, _ = x.shape
    cout, _, k, _ = wt.shape
    out = np.zeros((n, oh, ow, cout), dtype=np.int64)
    for b in range(n):
        for oy in range(oh):
            for ox in range(ow):
                for co in range(cout):
                    acc = 0
                    for ky in range(k):
                        for kx in range(k):
                            iy, ix = oy * s - pt + ky, ox * s - pl + kx
                            if 0 <= iy < h and 0 <= ix < w:
                                acc += int(np.dot(x[b, iy, ix], wt[co, :, ky, kx]))
                    out[b, oy, ox, co] = acc
    return out


@pytest.mark.parametrize("k,s,h,w,padding", [
    (3, 1, 5, 7, 1), (3, 2, 6, 8, "same"), (3, 2, 7, 5, "same"), (3, 2, 6, 8, 1), (3, 2, 7, 5, 1), (1, 1, 4, 5, "same"), (1, 2, 6, 4, "same"), (1, 2, 5, 7, "same"),
    (7, 2, 12, 10, "same"), (7, 2, 9, 11, "same"), (3, 1, 2, 2, 1),
])
def test_convolution_reference_against_nested_loops(k, s, h, w, padding):
    pt, pl, oh, ow = E.conv_geometry(k, s, h, w, padding)
    if padding == "same":  # ceil(i / s) outputs; the odd padding pixel at the bottom / right
        assert (oh, ow) == (math.ceil(h / s), math.ceil(w / s))
        total = max((oh - 1) * s + k - h, 0)
        assert pt == total // 2 and total - pt in (pt, pt + 1)
    g = torch.Generator().manual_seed(k * 100 + h)
    x, wt = E.draw(g, (2, h, w, 3), 4), E.draw(g, (4, 3, k, k), 4)
    bias, r1, r2 = E.draw(g, (4,), 8), E.draw(g, (2, oh, ow, 4), 64), E.draw(g, (2, oh, ow, 4), 64)
    want = _loop_conv(x, wt, s, pt, pl, oh, ow)
    assert np.array_equal(E.conv_exact_int(x, wt, s, pt, pl, oh, ow), want)
    got = E.conv_exact(x, wt, s, pt, pl, oh, ow)
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), want.astype(np.float64))
    full = want + bias.numpy() + r1.numpy() + r2.numpy()
    assert np.array_equal(E.conv_exact_int(x, wt, s, pt, pl, oh, ow, bias, (r1, r2)), full)
    assert np.array_equal(E.conv_exact(x, wt, s, pt, pl, oh, ow, bias, (r1, r2)).numpy(), full.astype(np.float64))


def test_same_padding_even_and_odd_inputs():
    assert E.same_geometry(24, 3, 2) == (12, 0) and E.same_geometry(23, 3, 2) == (12, 1)    # even: 0 top / left, 1 bottom / right; odd: 1 / 1
    assert E.same_geometry(32, 3, 1) == (32, 1) and E.same_geometry(24, 1, 2) == (12, 0)
    assert E.same_geometry(96, 7, 2) == (48, 2) and E.same_geometry(61, 7, 2) == (31, 3)
    assert E.symmetric_geometry(15, 3, 2, 1) == (8, 1) and E.symmetric_geometry(20, 3, 2, 1) == (10, 1)


def test_border_ring_is_distinct_and_nonzero():
    x = E.ring_border(torch.zeros(2, 5, 6, 4, dtype=torch.int64), base=5)
    assert int(x[:, 1:-1, 1:-1].abs().max()) == 0, "the interior is left alone"
    ring = x.clone()
    ring[:, 1:-1, 1:-1] = 5
    assert int(ring.abs().min()) >= 5 and int(ring.abs().max()) <= 7
    # a border pixel differs from its neighbours along the ring (a tap read one column or one row off shows), in every channel
    for row in (0, 4):
        assert bool((x[:, row, 1:] != x[:, row, :-1]).all())
    for col in (0, 5):
        assert bool((x[:, 1:, col] != x[:, :-1, col]).all())
    assert bool((x[:, 0, 1] != x[:, 1, 0]).all()) and bool((x[:, 4, 4] != x[:, 3, 5]).all())


def test_gemm_reference_against_nested_loops_and_int64():
    A, W, bias, res, bound = E.gemm_operands(5, 128, 64)
    a, w_, b, r = A.numpy(), W.numpy(), bias.numpy(), res.numpy()
    want = np.zeros((5, 128), dtype=np.int64)
    for i in range(5):
        for j in range(128):
            acc = 0
            for k in range(64):
                acc += int(a[i, k]) * int(w_[j, k])
            want[i, j] = acc + int(b[j]) + int(r[i, j])
    assert np.array_equal(E.gemm_exact_int(A, W, bias, res), want)
    assert np.array_equal(E.gemm_exact(A, W, bias, res).numpy(), want.astype(np.float64))
    assert int(np.abs(want).max()) <= bound
    # a larger shape: the float64 matmul against the int64 one
    A, W, bias, res, _ = E.gemm_operands(200, 256, 704)
    assert np.array_equal(E.gemm_exact(A, W, bias, res).numpy(), E.gemm_exact_int(A, W, bias, res).astype(np.float64))


def test_round_once_is_round_to_nearest_even():
    v = torch.tensor([255.0, 256.0, 257.0, 258.0, 259.0, 261.0, 263.0, -257.0, 2049.0, 2051.0, 4099.0], dtype=torch.float64)
    assert E.round_once(v, torch.bfloat16).tolist() == [255.0, 256.0, 256.0, 258.0, 260.0, 260.0, 264.0, -256.0, 2048.0, 2048.0, 4096.0]  # steps of 2, 16, 32
    assert E.round_once(v, torch.float16).tolist() == [255.0, 256.0, 257.0, 258.0, 259.0, 261.0, 263.0, -257.0, 2048.0, 2052.0, 4100.0]   # steps of 2, 4
    with pytest.raises(AssertionError):
        E.round_once(torch.tensor([2.0 ** 24 + 1.0], dtype=torch.float64), torch.bfloat16)
    assert E.ulp(torch.tensor([1.0, 1.5, 2.0, 0.1057, 0.0]), torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -11, 2.0 ** -133]
    assert E.ulp(torch.tensor([1.0, 3.9, 1e-6]), torch.float16).tolist() == [2.0 ** -10, 2.0 ** -9, 2.0 ** -24]


def test_q_scale_is_one_float32_multiply():
    exact = torch.tensor([[3.0, -1001.0, 12288.0]], dtype=torch.float64)
    c = np.float32(0.125) * np.float32(1.4426950408889634)
    assert E.Q_SCALE.dtype == np.float32 and E.Q_SCALE == c
    for dtype in (torch.bfloat16, torch.float16):
        want = [float(torch.tensor(float(np.float32(np.float32(v) * c))).to(dtype)) for v in exact[0].tolist()]
        assert E.q_expected(exact, dtype).float()[0].tolist() == want


def test_vt_token_order():
    """Bits 2 and 3 of the token index exchanged: quads 4..7 and 8..11 of every 16 swap; an involution; vt_store puts token t's values in column slot(t)."""
    slot = E.vt_slot(64)
    for t in range(64):
        q, r = (t % 16) // 4, t % 4
        want = t - t % 16 + {0: 0, 1: 2, 2: 1, 3: 3}[q] * 4 + r
        assert int(slot[t]) == want
    assert torch.equal(slot[slot], torch.arange(64))
    B, Np, H = 2, 64, 3
    v = torch.arange(B * Np * H * 64).reshape(B * Np, H * 64)
    stored = E.vt_store(v, B, Np, H)
    assert stored.shape == (B, H, 64, Np)
    for b in range(B):
        for h in range(H):
            for c in (0, 17, 63):
                for t in range(Np):
                    assert int(stored[b, h, c, int(slot[t])]) == int(v[b * Np + t, h * 64 + c])


def test_patch_rows_and_patch_embedding_against_nested_loops():
    g = torch.Generator().manual_seed(5)
    P, n, h, w, c, D = 4, 2, 8, 12, 3, 5
    x, wt, bias = E.draw(g, (n, h, w, c), 4), E.draw(g, (D, c, P, P), 4), E.draw(g, (D,), 8)
    want = np.zeros((n, (h // P) * (w // P), D), dtype=np.int64)
    xn, wn = x.numpy(), wt.numpy()
    for b in range(n):
        for py in range(h // P):
            for px in range(w // P):
                for d in range(D):
                    acc = int(bias[d])
                    for dy in range(P):
                        for dx in range(P):
                            for ch in range(c):
                                acc += int(xn[b, py * P + dy, px * P + dx, ch]) * int(wn[d, ch, dy, dx])
                    want[b, py * (w // P) + px, d] = acc
    assert np.array_equal(E.patch_embed_exact(x, wt, bias).numpy(), want.astype(np.float64))
    rows = E.patch_rows(x, P)
    assert rows.shape == (n * 6, P * P * c) and int(rows[1 * 6 + 1 * 3 + 2, (2 * P + 3) * c + 1]) == int(x[1, 1 * P + 2, 2 * P + 3, 1])


@pytest.mark.parametrize("s,h,w", [(2, 3, 4), (4, 2, 3)])
def test_transposed_convolution_and_pixel_shuffle_against_nested_loops(s, h, w):
    g = torch.Generator().manual_seed(s)
    n, cin, cout = 2, 6, 8
    x, wt, bias = E.draw(g, (n, h, w, cin), 2), E.draw(g, (cin, cout, s, s), 1, 0.1), E.draw(g, (cout,), 8)
    want = np.zeros((n, h * s, w * s, cout), dtype=np.int64)
    xn, wn = x.numpy(), wt.numpy()
    for b in range(n):
        for y in range(h):
            for xx in range(w):
                for dy in range(s):
                    for dx in range(s):
                        for co in range(cout):
                            want[b, y * s + dy, xx * s + dx, co] = int(np.dot(xn[b, y, xx], wn[:, co, dy, dx])) + int(bias[co])
    got = E.pixel_shuffle(E.conv_transpose_parts(x, wt), bias)
    assert np.array_equal(got.numpy(), want.astype(np.float64))


def test_gram_reference_against_nested_loops():
    g = torch.Generator().manual_seed(9)
    x = E.draw(g, (2, 5, 7, 6), 4)
    for stride in (1, 2):
        S = np.zeros((2, 6, 6), dtype=np.int64)
        s_ = np.zeros((2, 6), dtype=np.int64)
        for b in range(2):
            for y in range(0, 5, stride):
                for xx in range(0, 7, stride):
                    p = x[b, y, xx].numpy()
                    S[b] += np.outer(p, p)
                    s_[b] += p
        got_S, got_s = E.gram_exact(x, stride)
        assert np.array_equal(got_S.numpy(), S.astype(np.float64)) and np.array_equal(got_s.numpy(), s_.astype(np.float64))


@pytest.mark.parametrize("B,N,H", [(1, 64, 2), (2, 77, 3), (1, 300, 2)])
def test_attention_cases_by_explicit_softmax(B, N, H):
    """The selection case: the target scores 0, every other key (the padded copies excepted) <= -256, and an explicit softmax (float32 exp2: 2^-256 is exactly 0) over
    the REAL keys has l = 1 and returns v[target] exactly; the padded rows repeat real keys' codes and would be counted by a kernel that does not mask them.  The counting case: 127 count_c / N by a loop."""
    Np, D = (N + 63) // 64 * 64, H * 64
    qk, v, want, perm = E.attention_selection(B, N, H)
    assert int(qk.abs().max()) <= 256 and int(v.abs().max()) <= 128
    scores = E.attention_scores(qk, B, Np, H)
    vv = v.reshape(B, Np, H, 64)
    for b in range(B):
        for h in range(H):
            assert sorted(perm[b, h].tolist()) == list(range(N))
            s = scores[b, h, :N, :N]
            assert bool((s.gather(1, perm[b, h][:, None]) == 0).all())
            off = s.clone()
            off.scatter_(1, perm[b, h][:, None], -256)
            assert int(off.max()) <= -256
            p = torch.exp2(s.float()).double()  # exp2(-256) is exactly 0 in float32
            assert bool((p.sum(1) == 1).all())
            out = (p @ vv[b, :N, h].double()) / p.sum(1, keepdim=True)
            assert torch.equal(out, want[b, :, h * 64:(h + 1) * 64].double())
            if Np > N:  # every padded row repeats a real key's code and carries non-zero values
                assert bool((scores[b, h, :N, N:] == 0).any(0).all()) and bool((vv[b, N:, h] != 0).all())
    assert len({tuple(perm[0, h].tolist()) for h in range(H)}) == H, "a different permutation per head"
    qk, v, want = E.attention_counting(B, N, H)
    assert int(qk[:, :D].abs().max()) == 0
    count = [0] * D
    for j in range(N):
        count[j % D] += 1
    assert want.tolist() == [127.0 * c / N for c in count]
    vv = v.reshape(B, Np, D)
    for j in range(Np):
        assert int(vv[B - 1, j, j % D]) == 127 and int(vv[B - 1, j].sum()) == 127


def test_launch_rules_select_the_intended_paths_at_256_cus():
    for M, N, K, env in E.LINEAR_CASES:
        path = E.gemm_path(M, N, K, 256, env)
        if env.get("HIVE_GEMM_TILE") == "256" or (M, N, K) == (9800, 2048, 64):
            assert path[0] == "tile256"
        else:
            assert path[0] == "tile128"
    assert E.gemm_path(1216, 768, 3072, 256, {}) == ("tile128", 4, True)
    assert E.gemm_path(9800, 2048, 64, 256, {}) == ("tile256", 312)
    reached = set()
    for n, cin, cout, k, s, h, w, padding, env, expected in E.CONV_CASES:
        _, _, oh, ow = E.conv_geometry(k, s, h, w, padding)
        path = E.conv_path(n * oh * ow, cin, cout, k, 256, env)
        assert expected is None or path == expected
        reached.add(path if path[0] == "tile" else ("deep", min(path[1], 2)))
    for n, cin, cout, k, s, h, w, padding, env, expected, tile_rows in E.CONV_STATS_CASES:
        _, _, oh, ow = E.conv_geometry(k, s, h, w, padding)
        assert E.conv_path(n * oh * ow, cin, cout, k, 256, env) == expected and tile_rows == (128 if expected[0] == "deep" else expected[1]) <= oh * ow
    assert {c[9][0] for c in E.CONV_STATS_CASES} == {"tile", "deep"}
    B, N, D, H = E.QKV_TWO_PER_CU_CASE
    assert 256 < -(-B * ((N + 63) // 64 * 64) // 128) * (3 * D // 128) <= 512
    assert all(-(-B * ((N + 63) // 64 * 64) // 128) * (3 * D // 128) <= 256 for B, N, D, H in E.QKV_CASES)
    assert {("tile", 256, 256), ("tile", 256, 128), ("tile", 256, 64), ("tile", 128, 256), ("tile", 128, 128), ("deep", 1), ("deep", 2)} <= reached


# every generator's conditions (asserted inside it) at every shape of the GPU file
@pytest.mark.parametrize("M,N,K", sorted({c[:3] for c in E.LINEAR_CASES}))
def test_gemm_operands_meet_their_conditions(M, N, K):
    A, W, bias, res, bound = E.gemm_operands(M, N, K)
    assert bound < E.LIMIT and int(A.abs().max()) <= 4 and int(W.abs().max()) <= 4
    for t in (A, W, bias, res):  # exact in both element types
        assert torch.equal(t.to(torch.bfloat16).long(), t) and torch.equal(t.to(torch.float16).long(), t)


@pytest.mark.parametrize("M,N,K", sorted({c[:3] for c in E.GELU_CASES}))
def test_gelu_operands_meet_their_conditions(M, N, K):
    A, W, bias, bound = E.gelu_operands(M, N, K)
    assert bound < E.LIMIT
    for t in (A, W, bias):
        assert torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)
    pre = A @ W.t() + bias
    assert float(pre.abs().max()) <= 8.0 and float(pre.std()) > 0.8, "inside -8..8 and spread over the curve"
    assert torch.equal(pre.float().double(), pre), "the pre-activation is a float32 value"


@pytest.mark.parametrize("B,N,D,H", E.QKV_CASES + [E.QKV_TWO_PER_CU_CASE])
def test_qkv_operands_meet_their_conditions(B, N, D, H):
    x, W, bias, Np, bound = E.qkv_operands(B, N, D)
    assert bound < E.LIMIT and Np % 64 == 0 and 0 <= Np - N < 64 and D == H * 64 and int(x[:, N:].abs().max() if Np > N else 0) == 0


@pytest.mark.parametrize("case", sorted({c[:8] for c in E.CONV_CASES}, key=str), ids=str)
def test_conv_operands_meet_their_conditions(case):
    x, wt, bias, r1, r2, bound = E.case_conv_operands(case)
    assert bound < E.LIMIT
    if x.shape[1] >= 3 and x.shape[2] >= 3:  # the border ring: non-zero, and larger than any interior value
        assert int(x[:, 0].abs().min()) >= 5 and int(x[:, :, -1].abs().min()) >= 5 and int(x.abs().max()) == 7 and int(x[:, 1:-1, 1:-1].abs().max()) <= 4


@pytest.mark.parametrize("case", sorted({c[:8] for c in E.CONV_STATS_CASES}, key=str), ids=str)
def test_conv_statistics_operands_meet_their_conditions(case):
    x, wt, bias, r1, r2, bound = E.case_conv_operands(case, r=2, p_zero=0.1)
    # a tile part holds at most 256 rows: its sum of squares stays below 2^24 while the outputs' mean square stays below 2^16 (the GPU test asserts the sums themselves)
    n, cin, cout, k, s, h, w, padding = case
    pt, pl, oh, ow = E.conv_geometry(k, s, h, w, padding)
    out = E.conv_exact(x, wt, s, pt, pl, oh, ow, bias)
    assert bound < E.LIMIT and float((out ** 2).mean()) < 2.0 ** 16 / 4


def test_other_operands_meet_their_conditions():
    for n, h, w in E.STEM_CASES:
        assert E.stem_operands(n, h, w)[2] < E.LIMIT
    for n, h, w, D in E.PATCH_CASES:
        assert E.conv_operands(n, 3, D, 16, h, w, h // 16, w // 16)[5] < E.LIMIT
    for n, cin, cout, s, h, w in E.CONV_TRANSPOSE_CASES:
        x, wt, bias, bound = E.conv_transpose_operands(n, cin, cout, s, h, w)
        parts = E.conv_transpose_parts(x, wt)
        assert float(parts.abs().max()) <= 256 and torch.equal(parts.to(torch.bfloat16).double(), parts)
    for n, cin, cout, stride, h, w in E.GRAM_CASES:
        oh, ow = (h + stride - 1) // stride, (w + stride - 1) // stride
        assert E.gram_operands(n, cin, h, w, oh, ow)[1] < E.LIMIT


# ------------------------------------------------------------------------------------------------------------------------------------
# bottleneck convolution, x2 upsampling, fused depth head

import norm_reference as R

HALVES = [torch.bfloat16, torch.float16]


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return torch.equal(a, b) if torch.is_tensor(a) else a == b


def test_bneck_partials_are_in_the_layout_of_gn_tile_partials():
    """With v = 0 the rows equal norm_reference.gn_tile_partials of a tensor that holds m in every pixel of an (image, group); with v they finalise to (m, 2 | 1)."""
    for n, hw, tile_rows in ((3, 300, 200), (2, 37, 37), (3, 131, 128), (4, 768, 512)):
        m, v = E.bneck_statistics(n)
        x = m.repeat_interleave(2, dim=1)[:, None, :].expand(n, hw, 64).numpy()
        got = E.bneck_partials(m, torch.zeros_like(v), hw, tile_rows)
        assert np.array_equal(got.numpy(), R.gn_tile_partials(x, tile_rows).astype(np.float64))
        assert tile_rows == hw or R.gn_straddling_tiles(n, hw, tile_rows) >= 1
        mean, rstd = E.bneck_finalize(E.bneck_partials(m, v, hw, tile_rows), n, hw, tile_rows)
        assert np.array_equal(mean, m.numpy().astype(np.float32)) and np.array_equal(rstd, np.where(v.numpy() == 0, 2.0, 1.0).astype(np.float32))
        assert set(np.unique(rstd)) == {1.0, 2.0} and set(np.unique(mean)) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    for d in (1, 2, 3, 4, 64, 128):  # two images this far apart never share a group's mean (bneck_batch: a workgroup's consecutive trips at 256 CUs are 64 / 128 images apart)
        m, _ = E.bneck_statistics(d + 7)
        assert bool((m[d:] != m[:-d]).all())


@pytest.mark.parametrize("case", E.BNECK_CASES, ids=str)
def test_bneck_operands_meet_their_conditions(case):
    """The generator's own assertions at every case (256 CUs), determinism, the premise of the multi-trip cases, and from the reference: where the kernel leaves sums
    every tile / channel sum of squares of the stored outputs is below 2^24 in both element types."""
    n = E.bneck_batch(case, 256)
    h, w, keep, rows = case[1:]
    ops = E.bneck_operands(n, h, w, keep, rows)
    assert _same(ops, E.bneck_operands(n, h, w, keep, rows)), "the generator is not deterministic"
    t, partial, tile_rows, gamma, beta, wt, a, b, bound = ops
    per, _ = E.bneck_tiles(h, w)
    assert (keep == 0.25) == E.bneck_has_sums(h, w) and bound < E.LIMIT
    assert (tile_rows == h * w) == (rows == "image") and (rows == "image" or R.gn_straddling_tiles(n, h * w, tile_rows) >= 1)
    if case[0] is None:
        assert 2 * 256 < n * per < 3 * 256
    for tt in (t, gamma, beta, wt):
        assert torch.equal(tt.to(torch.bfloat16).long(), tt) and torch.equal(tt.to(torch.float16).long(), tt)
    if h >= 3 and w >= 3:
        assert int(t[:, 0].abs().min()) >= 3 and int(t[:, :, -1].abs().min()) >= 3 and int(t[:, 1:-1, 1:-1].abs().max()) <= 2
    u = E.bneck_normalised(t, a, b)
    y = E.conv3x3_exact(u, wt)
    assert float(y.abs().max()) <= bound
    if E.bneck_has_sums(h, w):
        for dtype in HALVES:
            sums = E.bneck_tile_sums(E.round_once(y, dtype).double(), h, w)
            assert sums.shape == (n * per, 2, 64) and float(sums[:, 1].max()) < E.LIMIT and float(sums[:, 0].abs().max()) < E.LIMIT


def test_bneck_cases_round_in_bfloat16_and_tile_sums_against_a_loop():
    """At least one case with half of the weights kept has |y| above 256 (the single rounding to bfloat16 is exercised); bneck_tile_sums against slices."""
    above, changed = 0, 0
    for case in [c for c in E.BNECK_CASES if c[3] == 0.5]:
        n = E.bneck_batch(case, 256)
        t, _, _, _, _, wt, a, b, _ = E.bneck_operands(n, *case[1:])
        y = E.conv3x3_exact(E.bneck_normalised(t, a, b), wt)
        above += int(float(y.abs().max()) > 256)
        changed += int(not torch.equal(E.round_once(y, torch.bfloat16).double(), y))
    assert above >= 1 and changed >= 1, f"{above} cases above 256, {changed} with an output that bfloat16 rounds"
    n, h, w = 2, 24, 64
    z = torch.arange(n * h * w * 64, dtype=torch.float64).reshape(n, h, w, 64) % 13 - 6
    got = E.bneck_tile_sums(z, h, w)
    assert E.bneck_tiles(h, w) == (4, 2)
    for img in range(n):
        for ty in range(2):
            for tx in range(2):
                blk = z[img, ty * 16:ty * 16 + 16, tx * 32:tx * 32 + 32].reshape(-1, 64)
                assert torch.equal(got[img * 4 + ty * 2 + tx, 0], blk.sum(0)) and torch.equal(got[img * 4 + ty * 2 + tx, 1], (blk * blk).sum(0))


@pytest.mark.parametrize("N,C,H,W", [(1, 8, 1, 1), (1, 8, 1, 9), (1, 8, 9, 1), (2, 8, 7, 5), (1, 8, 24, 32), (1, 8, 15, 20)])
def test_upsample2x_restatement_against_interpolate_in_float64(N, C, H, W):
    """The float32 restatement against F.interpolate(align_corners=True) of the same values in float64.  Bound: the source coordinate f = s * o carries two
    float32 roundings (s, the product), at most 2^-23 (size - 1) per axis, and moves the blend by at most that times the difference of two neighbours
    (<= 2 max |v|); the blend itself is five rounded operations deep (w0 = 1 - w1, the products, two sums, the outer product and sum: 8 roundings of values
    of at most max |v|).  The integer parts agree wherever f is not within that error of an integer -- the blend is continuous there."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(H * 100 + W)
    v = torch.randn((N, H, W, C), generator=g, dtype=torch.float32)
    got = E.upsample2x_blend_f32(v.numpy()).astype(np.float64)
    ref = F.interpolate(v.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
    vmax = float(v.abs().max())
    bound = (2.0 ** -23 * (H + W) * 2 + 8 * 2.0 ** -24) * vmax
    assert got.shape == ref.shape == (N, 2 * H, 2 * W, C) and float(np.abs(got - ref).max()) <= bound
    # the corners are copied (align_corners), and both element types round the same blend once
    assert np.array_equal(got[:, 0, 0], v.numpy()[:, 0, 0].astype(np.float64))
    for dtype in HALVES:
        x = v.to(dtype)
        assert torch.equal(E.upsample2x_f32(x), torch.from_numpy(E.upsample2x_blend_f32(x.float().numpy())).to(dtype))
        bias = torch.full((C,), 0.375, dtype=dtype)
        assert torch.equal(E.upsample2x_f32(x, bias), E.upsample2x_f32((x.float() + 0.375).to(dtype)))


def test_upsample2x_is_exact_on_a_constant_map():
    for dtype in HALVES:
        for c in (1.0, -3.140625, 0.0, 65504.0 if dtype == torch.float16 else 3.3895313892515355e38, 2.0 ** -10):
            x = torch.full((1, 7, 5, 8), c, dtype=dtype)
            assert torch.equal(E.upsample2x_f32(x), torch.full((1, 14, 10, 8), c, dtype=dtype))
    for size in (1, 2, 5, 24, 240, 320):  # the weights: l0 + l1 = 1 up to one rounding, sources inside the map, the last output on the last source
        i0, i1, l0, l1 = E.upsample_axis(size)
        assert float(l1.min()) >= 0 and float(l1.max()) < 1 and i0[0] == 0 and l1[0] == 0 and int(i1[-1]) == size - 1
        assert bool((np.diff(i0) >= 0).all()) and bool((np.diff(i0) <= 1).all())


@pytest.mark.parametrize("N,C,H,W", E.UPSAMPLE_CASES)
def test_upsample_operands_meet_their_conditions(N, C, H, W):
    for dtype in HALVES:
        x, bias = E.upsample_operands(N, C, H, W, dtype)
        assert _same((x, bias), E.upsample_operands(N, C, H, W, dtype)) and x.dtype == bias.dtype == dtype
        for b in (None, bias):
            assert bool(torch.isfinite(E.upsample2x_f32(x, b)).all())
    assert (C > 512) == (C == 1024), "C = 1024 only takes the gather form by the launch rule"


@pytest.mark.parametrize("case", E.HEAD_CASES, ids=lambda c: str(c[:3]))
def test_head_operands_meet_their_conditions(case):
    """head_sums / head_expected assert theirs (upsampled values in [1, 8] on the 2^-10 grid, sum |feat w1| + |b1| < 2^14 per pixel, the last ReLU clips 10 - 90 %)
    for every variant and element type; here also: determinism, the sums' bound, the premise of the multi-trip case at 256 CUs and that the outputs vary."""
    N = E.head_batch(case, 256)
    H, W = case[1:3]
    ops = E.head_operands(N, H, W)
    assert _same(ops, E.head_operands(N, H, W)), "the generator is not deterministic"
    x, b0, w3, b3, w1, b1 = ops
    if case[0] is None:
        assert 4 * 256 < N * E.head_tiles(H, W) < 6 * 256
    assert 1 <= int(x.min()) and int(x.max()) <= 5 and 0 <= int(b0.min()) and int(b0.max()) <= 3 and int(w3.abs().max()) == 1 and int(b3.abs().max()) <= 8
    variants = E.head_variants(case)
    assert len(variants) == (8 if case[3] == E.HEAD_GRID else len(case[3]))
    for dtype in HALVES:
        for with_b0 in sorted({v[0] for v in variants}):
            feat = E.head_sums(x, b0 if with_b0 else None, w3, dtype)
            assert float(feat.abs().max()) <= 9224 - 8 and torch.equal(torch.round(feat / E.HEAD_UNIT) * E.HEAD_UNIT, feat)
            for _, nn, inv in [v for v in variants if v[0] == with_b0]:
                depth, mm, m = E.head_expected(feat, b3, w1, b1[with_b0], nn, inv)
                assert depth.dtype == np.float32 and mm.dtype == np.uint16 and m.dtype == np.float32 and depth.shape == (N * 4 * H * W,)
                assert len(np.unique(depth)) > depth.size // 8 and np.isfinite(depth).all()


def test_head_variants_cover_every_option():
    seen = {v for case in E.HEAD_CASES for v in E.head_variants(case)}
    assert seen == {(b0, nn, inv) for b0 in (False, True) for nn in (0, 1) for inv in (0, 1)}
    assert sum(1 for c in E.HEAD_CASES if c[3] == E.HEAD_GRID) == 1
