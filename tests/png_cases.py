"""The seeded pictures both PNG test files run (tests/test_png_cpu.py against zlib and Pillow, tests/test_png_gpu.py against the restatement), and the
restatement's result of every case, computed once per process.  Sizes are chosen per kind so that the FILTERED stream (H * (1 + W * bytes per pixel)) hits
the segment constant S = 8192 where the case says so."""
import functools

import numpy as np

import png_restatement as R

KINDS = ("gray8", "gray16", "rgb8")
BPP = {"gray8": 1, "gray16": 2, "rgb8": 3}
S = R.SEGMENT

# (H, W) per kind whose stream H * (1 + W * bpp) is S - 1, S and S + 1 bytes, and one whose rows straddle the segment ends:
#   gray8   8191 = 1 * (1 + 8190),     8192 = 2 * (1 + 4095),     8193 = 3 * (1 + 2730)
#   gray16  8191 = 1 * (1 + 2 * 4095), 8193 = 3 * (1 + 2 * 1365); 1 + 2 W is odd, so no picture has a stream of 8192: 8190 = 2 * (1 + 2 * 2047) stands in
#   rgb8    8191 = 1 * (1 + 3 * 2730), 8192 = 2 * (1 + 3 * 1365), 8193 = 3 * (1 + 3 * 910)
BOUNDARY = {
    "gray8": {"S-1": (1, 8190), "S": (2, 4095), "S+1": (3, 2730), "straddle": (5, 3001)},
    "gray16": {"S-1": (1, 4095), "S": (2, 2047), "S+1": (3, 1365), "straddle": (5, 1501)},
    "rgb8": {"S-1": (1, 2730), "S": (2, 1365), "S+1": (3, 910), "straddle": (5, 1001)},
}
# two identical halves of one row, noise between them: pixels from the first half's start to the second's -> bytes 40 000 / 32 768 / 32 769 (gray8),
# 40 000 / 32 768 / 32 770 (gray16: a pixel is two bytes) and 40 200 / 32 766 / 32 769 (rgb8: three): at or just inside the window, and just past it
HALF_GAPS = {"gray8": (40000, 32768, 32769), "gray16": (20000, 16384, 16385), "rgb8": (13400, 10922, 10923)}
CONTENTS = ("1x1", "1x7", "7x1", "S-1", "S", "S+1", "straddle", "flat", "halves_far", "halves_32768", "halves_32769", "noise", "skewed", "ramp_noise", "ramp",
            "mask")
ONLY = {"all_bytes": ("gray8",), "depth_480x640": ("gray16",)}
SIZE_RECORD = (("ramp_noise", "gray16"), ("ramp", "rgb8"), ("mask", "gray8"), ("depth_480x640", "gray16"))
# gray8, 1025 x 2047, pixel (x // 5 + 3 y) % 256: a stream of 1025 * 2048 = 2 099 200 bytes, 257 segments and 1025 sort tiles, so the picture-level scans take a
# second chunk of 256.  The restatement needs seconds for it: its file is recorded here (tests/test_png_cpu.py checks the record against the restatement, the
# GPU test checks the GPU's file against the record and reads it back)
LONG_SHAPE = (1025, 2047)
LONG_RECORD = {"length": 25126, "sha256": "73d73adee4592c651b28ba84099316e66cadebead15ff3b56b945e4a61950c82"}


@functools.lru_cache(maxsize=None)
def long_picture():
    yy, xx = np.mgrid[0:LONG_SHAPE[0], 0:LONG_SHAPE[1]]
    a = ((xx // 5 + 3 * yy) % 256).astype(np.uint8)
    a.setflags(write=False)
    return a


def _as_kind(values, kind):
    """An int array [H][W] (or [H][W][3] for rgb8) of byte values as a picture of the kind; gray16 spreads a byte over both halves of the sample."""
    values = np.asarray(values)
    if kind == "gray16":
        return (values.astype(np.uint16) * 257).astype(np.uint16)
    return values.astype(np.uint8)


def _shape(kind, height, width):
    return (height, width, 3) if kind == "rgb8" else (height, width)


def _noise(rng, kind, height, width):
    if kind == "gray16":
        return rng.integers(0, 65536, (height, width), dtype=np.uint16)
    return rng.integers(0, 256, _shape(kind, height, width), dtype=np.uint8)


def _ramp_noise(rng, height, width):
    """A smooth 16-bit ramp with 3 bits of noise: a depth map in millimetres."""
    yy, xx = np.mgrid[0:height, 0:width]
    smooth = 1500 + 3 * xx + 2 * yy + (200 * np.sin(xx / 37.0) * np.cos(yy / 23.0)).astype(np.int64)
    return (smooth + rng.integers(0, 8, (height, width))).astype(np.uint16)


def _halves(rng, kind, gap):
    """One row of noise in which the 1200 bytes that start ``gap`` pixels in repeat the row's first 1200 bytes.  One row has one filter, so the halves are
    equal in the filtered stream too (but for the first pixel under a filter that looks left)."""
    half = 1200 // BPP[kind]
    row = _noise(rng, kind, 1, gap + half)
    row[0, gap:gap + half] = row[0, :half]
    return row


FIBONACCI = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987)  # with the end-of-block symbol's 1 in front and 1597 behind: a chain of 17 leaves


@functools.lru_cache(maxsize=None)
def skewed_row():
    """The raw bytes of a one-row picture whose SECOND segment is coded with the counts 1 (end of block), 1, 2, 3, 5 .. 987, 1597: the Huffman tree of these
    is a chain 16 deep, so the 15-bit limit binds.  A picture of skewed pixel values alone does not get there: the matcher turns the frequent values into
    matches.  So the segment is BUILT of tokens.  8191 noise bytes (values 32 .. 255; with the row's filter byte they fill the first segment) are the
    dictionary.  The second segment is 1597 units of one or two literals (15 values below 32 with the Fibonacci counts, 2582 in all) and a copy of three
    dictionary bytes: the copy's source is the oldest one still within 4096 bytes (a match of three bytes may not be further), the byte behind the source
    differs from the byte behind the copy (so the match is exactly three bytes: length symbol 257, 1597 times), and the three bytes that start at each
    literal have never occurred before (so it stays a literal).  15 564 bytes: whole pixels of 1, 2 and 3 bytes.  tests/test_png_cpu.py checks the counts
    and the depth on the restatement's tokens."""
    rng = np.random.default_rng(0)
    literals = rng.permutation(np.repeat(np.arange(15)[::-1], FIBONACCI))   # value 0 the most frequent: the filter None has the smallest sum
    units = rng.permutation(np.array([2] * (len(literals) - 1597) + [1] * (2 * 1597 - len(literals))))
    stream = [0] + [int(v) for v in rng.integers(32, 256, 8191)]            # index = position in the filtered stream (filter None)
    latest = {}                                                             # triple -> (where its latest copy starts, the byte behind that copy)
    for q in range(S - 4096, S - 3, 3):
        latest[tuple(stream[q:q + 3])] = (q, stream[q + 3])
    seen = {tuple(stream[q:q + 3]) for q in range(len(stream) - 2)}         # every three bytes in a row so far
    at = 0
    for n in units:
        front = tuple(int(v) for v in literals[at:at + n])
        at += n
        behind = int(literals[at]) if at < len(literals) else -1
        for t in sorted(latest, key=lambda t: latest[t][0]):
            where, follows = latest[t]
            fresh = [(front + t)[j:j + 3] for j in range(n)]                # the three bytes that start at each literal
            if len(stream) + n - where <= 4096 and follows != behind and not any(f in seen for f in fresh) and len(set(fresh)) == n:
                break
        else:
            raise RuntimeError("no dictionary triple left")
        latest[t] = (len(stream) + n, behind)
        stream.extend(front + t)
        seen.update(tuple(stream[q:q + 3]) for q in range(len(stream) - n - 5, len(stream) - 2))
    return np.array(stream[1:], np.uint8)


@functools.lru_cache(maxsize=None)
def picture(content, kind):
    """The picture of a case, the same in every process (read-only)."""
    rng = np.random.default_rng(7 * (CONTENTS + tuple(ONLY)).index(content) + KINDS.index(kind))
    bpp = BPP[kind]
    if content in ("1x1", "1x7", "7x1"):
        h, w = int(content[0]), int(content[2])
        a = _noise(rng, kind, h, w)
    elif content in BOUNDARY[kind]:
        h, w = BOUNDARY[kind][content]
        yy, xx = np.mgrid[0:h, 0:w]
        base = (xx // 5 + 3 * yy) % 256     # stretches of equal bytes, so matches run into the segment's end
        a = _as_kind(np.stack([base, base, base], axis=2) if kind == "rgb8" else base, kind)
    elif content == "flat":                 # a few segments of one value
        h, w = 40, 3 * S // (40 * bpp)
        a = _as_kind(np.full(_shape(kind, h, w), 77), kind)
    elif content == "halves_far":
        a = _halves(rng, kind, HALF_GAPS[kind][0])
    elif content == "halves_32768":
        a = _halves(rng, kind, HALF_GAPS[kind][1])
    elif content == "halves_32769":
        a = _halves(rng, kind, HALF_GAPS[kind][2])
    elif content == "noise":
        a = _noise(rng, kind, 37, 3 * S // (37 * bpp) + 5)
    elif content == "all_bytes":            # every byte value, near-equal counts
        a = rng.permutation(np.arange(256 * 40) % 256).astype(np.uint8).reshape(80, 128)
    elif content == "skewed":               # one row: a noise segment, then the segment skewed_row() builds, as pixels of the kind
        row = skewed_row()
        a = {"gray8": row.reshape(1, -1), "rgb8": row.reshape(1, -1, 3),
             "gray16": (row.reshape(-1, 2)[:, 0].astype(np.uint16) << 8 | row.reshape(-1, 2)[:, 1]).reshape(1, -1)}[kind]
    elif content == "ramp_noise":
        a = _ramp_noise(rng, 48, 64)
        a = a if kind == "gray16" else _as_kind(np.stack([a & 255] * 3, axis=2) if kind == "rgb8" else a & 255, kind)
    elif content == "depth_480x640":
        a = _ramp_noise(rng, 480, 640)
    elif content == "ramp":                 # (3x, 5y, x + y) mod 256
        yy, xx = np.mgrid[0:96, 0:128]
        rgb = np.stack([3 * xx, 5 * yy, xx + yy], axis=2) % 256
        a = _as_kind(rgb if kind == "rgb8" else rgb[:, :, 0] + rgb[:, :, 1] & 255, kind) if kind != "gray16" else (300 * xx + 5 * yy).astype(np.uint16)
    elif content == "mask":                 # object ids 0 .. 3 in blobs
        yy, xx = np.mgrid[0:96, 0:128]
        ids = ((xx // 24 + yy // 32) % 4) * (((xx - 64) ** 2 + (yy - 48) ** 2) < 60 ** 2)
        a = np.stack([ids] * 3, axis=2).astype(np.uint8) if kind == "rgb8" else ids.astype(np.uint16 if kind == "gray16" else np.uint8)
    else:
        raise ValueError(content)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def cases(with_large=True):
    """(content, kind) of every case."""
    out = [(c, k) for c in CONTENTS for k in KINDS] + [(c, k) for c, kinds in ONLY.items() for k in kinds]
    return out if with_large else [case for case in out if case[0] != "depth_480x640"]


@functools.lru_cache(maxsize=None)
def restated(content, kind):
    """(file, report) of the restatement for one case."""
    return R.encode_counted(picture(content, kind))
