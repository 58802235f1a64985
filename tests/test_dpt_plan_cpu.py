"""CPU-only checks of the DPT network object's host rules (no device, no context): the arena plan every forward sizes itself by
(``hive_dpt_plan_arena``, csrc/dpt_net.hip) against the layouts recorded from the one-function orchestration it replaced, and the
rule that chooses the Gram-matrix GroupNorm statistics (``hive_gn_gram_preferred``, csrc/conv.hip) at its edges."""
import ctypes

import pytest

from hive_amd import _lib
from hive_amd.dpt.native import plan_arena

HYBRID, LARGE = 0, 1

# (backbone, B, frame h, frame w, net h, net w) -> (bytes, FNV-1a over the (offset, bytes) of every allocation in order).  Recorded from the dry walk of
# `run_forward` at commit 516d56e ("Geometry tests at ragged tiles and both rounding modes; bbox mode fix"), the last one with the orchestration as one
# function, with the same hash added to its `alloc`.  Between them: a map under 256 pixels (the pair instead of the fused two-pass), the 64-channel
# bottleneck branch, both backbones, the `net_depth` buffer of the resized path, the benchmark batch.
RECORDED = {
    (HYBRID, 1, 96, 160, 96, 160): (4210944, 0x3b31d130d171e2c4),
    (LARGE, 1, 96, 160, 96, 160): (4085760, 0x9282a264038050c6),
    (HYBRID, 2, 96, 160, 96, 160): (8421888, 0x15bfcb0367487b12),
    (LARGE, 2, 96, 160, 96, 160): (8171520, 0xc0bebb1a597e1a3b),
    (HYBRID, 3, 480, 640, 480, 640): (252523264, 0xfa1ef27179a5429d),
    (HYBRID, 107, 480, 640, 480, 640): (9006521088, 0x98808d24e7ddee01),
    (LARGE, 1, 480, 864, 480, 864): (110315520, 0xcd5baad25babae08),
    (HYBRID, 1, 72, 100, 96, 128): (3371264, 0xd8c02d4931cd0934),
    (HYBRID, 1, 1080, 1920, 352, 640): (61731072, 0xa85554f369291cd6),
}


@pytest.mark.parametrize("case", sorted(RECORDED), ids=lambda c: "-".join(map(str, c)))
def test_arena_plan_is_the_recorded_layout(case):
    backbone, b, fh, fw, nh, nw = case
    assert plan_arena(backbone, b, fh, fw, net_size=(nh, nw)) == RECORDED[case]


def test_arena_plan_refuses_what_the_forward_refuses():
    lib = _lib.load()
    n = ctypes.c_int64(0)
    plan = lambda *a: lib.hive_dpt_plan_arena(*a, ctypes.byref(n), None)
    assert plan(HYBRID, 1, 96, 160, 96, 160) == _lib.OK and n.value == RECORDED[(HYBRID, 1, 96, 160, 96, 160)][0]  # (the hash is optional)
    for bad in ((HYBRID, 1, 90, 160, 90, 160), (LARGE, 1, 96, 150, 96, 150), (HYBRID, 1, 96, 160, 0, 160), (HYBRID, 0, 96, 160, 96, 160),
                (HYBRID, 1, 0, 160, 96, 160), (2, 1, 96, 160, 96, 160), (-1, 1, 96, 160, 96, 160)):
        assert plan(*bad) == _lib.ERR_INVALID, bad
    assert lib.hive_dpt_plan_arena(HYBRID, 1, 96, 160, 96, 160, None, None) == _lib.ERR_INVALID
    with pytest.raises(_lib.HiveError, match="multiple of 32"):
        plan_arena(HYBRID, 1, 480, 640, net_size=(90, 160))


# N, H_out, W_out whose product is the pixel count named; with C_out = 256 the output has 256 times as many elements
PX_149_999_872, PX_150_000_128 = (11, 1, 53267), (2, 1, 292969)  # 585 937 and 585 938 pixels
PX_249_999_872, PX_250_000_128 = (2, 589, 829), (27, 7, 5167)    # 976 562 and 976 563 pixels


def _preferred(c_in, c_out, stride, g, shape, deterministic=0):
    return _lib.load().hive_gn_gram_preferred(c_in, c_out, stride, g, *shape, deterministic)


def test_gram_rule_at_its_edges(monkeypatch):
    """The rule as it stood in the network object and in ops.py: C_in 64 / 128 from 150 000 000 output elements, C_in 256 with stride 2 from 250 000 000.
    An eligible output has C_out % 256 == 0 channels, and neither threshold is a multiple of 256 (150 000 000 = 2^7 3 5^8, 250 000 000 = 2^7 5^9), so the
    counts 149 999 999 / 150 000 000 / 249 999 999 / 250 000 000 themselves cannot occur: the table stands at the nearest counts that can, the multiples of
    256 on either side of each threshold (128 below it, 128 above) -- no reachable count lies between them."""
    monkeypatch.delenv("HIVE_GN_GRAM", raising=False)
    for n, h, w in (PX_149_999_872, PX_150_000_128, PX_249_999_872, PX_250_000_128):
        assert h * w >= 256
    assert [256 * n * h * w for n, h, w in (PX_149_999_872, PX_150_000_128, PX_249_999_872, PX_250_000_128)] == [149_999_872, 150_000_128, 249_999_872, 250_000_128]
    for c_in in (64, 128):
        for stride in (1, 2):
            assert _preferred(c_in, 256, stride, 32, PX_149_999_872) == 0
            assert _preferred(c_in, 256, stride, 32, PX_150_000_128) == 1
    assert _preferred(256, 256, 2, 32, PX_249_999_872) == 0
    assert _preferred(256, 256, 2, 32, PX_250_000_128) == 1
    assert _preferred(256, 256, 2, 32, PX_150_000_128) == 0, "C_in 256 keeps the two-pass form up to its own, higher threshold"
    big = (107, 480, 640)  # far past both thresholds
    for c_out in (256, 512, 1024):
        assert _preferred(256, c_out, 1, 32, big) == 0
        for stride in (1, 2):
            assert _preferred(512, c_out, stride, 32, big) == 0
    # at the network's own shapes: 33 frames of 480 x 640 are past the 64 -> 256 threshold of stage 0, 30 are not
    assert _preferred(64, 256, 1, 32, (33, 120, 160)) == 1 and _preferred(64, 256, 1, 32, (30, 120, 160)) == 0


@pytest.mark.parametrize("c_in,stride,shape", [(64, 1, PX_150_000_128), (128, 2, PX_150_000_128), (256, 2, PX_250_000_128)])
def test_gram_rule_switches(monkeypatch, c_in, stride, shape):
    monkeypatch.delenv("HIVE_GN_GRAM", raising=False)
    assert _preferred(c_in, 256, stride, 32, shape) == 1
    assert _preferred(c_in, 256, stride, 32, shape, deterministic=1) == 0
    for g in (16, 64, 8, 0):
        assert _preferred(c_in, 256, stride, g, shape) == 0, g
    n, h, w = shape
    for c_out in (128, 384, 640):  # not whole 256-channel tiles (with as many pixels and more, so that the element count is no reason)
        assert _preferred(c_in, c_out, stride, 32, (4 * n, h, w)) == 0, c_out
    assert _preferred(c_in, 256, stride, 32, (n * h * w, 15, 17)) == 0, "a 255-pixel map: below one tile"
    assert _preferred(c_in, 256, stride, 32, (n * h * w, 16, 16)) == 1
    monkeypatch.setenv("HIVE_GN_GRAM", "0")  # read at every call
    assert _preferred(c_in, 256, stride, 32, shape) == 0
    monkeypatch.setenv("HIVE_GN_GRAM", "1")
    assert _preferred(c_in, 256, stride, 32, shape) == 1
