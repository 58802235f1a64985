"""Baseline JPEG as csrc/jpeg.hip writes it, restated in numpy with integer arithmetic only: the rules of include/hive_mi355x.h (hive_jpeg_encode), which are
libjpeg's (Annex K tables, the JFIF 16-bit fixed-point colour conversion, the "slow" integer DCT of Loeffler, Ligtenberg and Moschytz, one interleaved scan with
a restart interval of one MCU row) and give, byte for byte, the file Pillow writes with ``quality=q, subsampling=s, optimize=False, restart_marker_rows=1``
(tests/test_jpeg_cpu.py compares whole files).

``encode(rgb, quality, subsampling)`` -> the file's bytes; ``encode_counted`` also returns the counters the coverage test reads.
"""
import numpy as np

SUBSAMPLINGS = ("4:4:4", "4:2:0")

LUMINANCE_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                        18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                       np.int64)
CHROMINANCE_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                         + [99] * 32, np.int64)
# natural (row-major) index of the k-th coefficient in zigzag order
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHR_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUM_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
AC_CHR_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHR_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
HUFFMAN = ((0x00, DC_LUM_BITS, DC_VALS), (0x10, AC_LUM_BITS, AC_LUM_VALS), (0x01, DC_CHR_BITS, DC_VALS), (0x11, AC_CHR_BITS, AC_CHR_VALS))


def quant_tables(quality):
    """(luminance, chrominance) tables of 64 in natural order: libjpeg's quality scaling of the Annex K tables, clipped to 1 .. 255 (baseline)."""
    if not 1 <= quality <= 100:
        raise ValueError(f"quality {quality} outside 1 .. 100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (LUMINANCE_Q, CHROMINANCE_Q))


def huffman_codes(bits, vals):
    """symbol -> (code, length) of a table given as the counts per length 1 .. 16 and the symbols in code order (Annex C)."""
    codes, code, at = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[at]] = (code, length)
            code += 1
            at += 1
        code <<= 1
    return codes


def header(height, width, quality, subsampling, mcus_per_row):
    """Everything in front of the entropy-coded scan, as Pillow writes it."""
    be16 = lambda v: bytes([v >> 8, v & 255])
    out = b"\xFF\xD8" + b"\xFF\xE0" + be16(16) + b"JFIF\0" + bytes([1, 1, 0]) + be16(1) + be16(1) + bytes([0, 0])
    for index, table in enumerate(quant_tables(quality)):
        out += b"\xFF\xDB" + be16(67) + bytes([index]) + bytes(int(v) for v in table[ZIGZAG])
    luma = 0x22 if subsampling == "4:2:0" else 0x11
    out += b"\xFF\xC0" + be16(17) + bytes([8]) + be16(height) + be16(width) + bytes([3, 1, luma, 0, 2, 0x11, 1, 3, 0x11, 1])
    for ident, bits, vals in HUFFMAN:
        out += b"\xFF\xC4" + be16(19 + len(vals)) + bytes([ident]) + bytes(bits) + bytes(vals)
    out += b"\xFF\xDD" + be16(4) + be16(mcus_per_row)
    return out + b"\xFF\xDA" + be16(12) + bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


HEADER_BYTES = len(header(1, 1, 90, "4:2:0", 1))


def color_convert(rgb):
    """(Y, Cb, Cr) int64 planes: the JFIF conversion in 16-bit fixed point."""
    r, g, b = (rgb[:, :, k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, height, width):
    """Replicate the last column up to ``width`` and the last row up to ``height``."""
    h, w = plane.shape
    return np.pad(plane, ((0, height - h), (0, width - w)), mode="edge")


def downsample_420(plane, padded_h, padded_w):
    """(padded_h / 2, padded_w / 2): columns replicated at full resolution, rows replicated up to an EVEN height only, the 2 x 2 mean with the bias 1, 2, 1, 2 ..
    along the output row, then the last down-sampled row replicated up to the padded height."""
    h = plane.shape[0]
    full = _pad(plane, h + (h & 1), padded_w)
    total = full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2]
    bias = 1 + (np.arange(total.shape[1]) & 1)
    return _pad((total + bias) >> 2, padded_h // 2, padded_w // 2)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first):
    """The 8-point butterfly along the last axis (CONST_BITS 13, PASS1_BITS 2): the first pass scales up by 4, the second removes it."""
    d = [d[..., k] for k in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = 11 if first else 15
    out = [None] * 8
    out[0] = (tmp10 + tmp11) << 2 if first else _descale(tmp10 + tmp11, 2)
    out[4] = (tmp10 - tmp11) << 2 if first else _descale(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * 4433
    out[2] = _descale(z1 + tmp13 * 6270, n)
    out[6] = _descale(z1 - tmp12 * 15137, n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    out[7] = _descale(tmp4 + z1 + z3, n)
    out[5] = _descale(tmp5 + z2 + z4, n)
    out[3] = _descale(tmp6 + z2 + z3, n)
    out[1] = _descale(tmp7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def quantised_blocks(plane, table):
    """(rows, cols, 64) quantised coefficients in ZIGZAG order of a plane whose sides are multiples of 8."""
    h, w = plane.shape
    blocks = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)  # (by, bx, row, column)
    rows = _dct_pass(blocks, True)
    coefficients = _dct_pass(rows.swapaxes(-1, -2), False).swapaxes(-1, -2).reshape(h // 8, w // 8, 64)
    divisor = table << 3
    q = np.sign(coefficients) * ((np.abs(coefficients) + (divisor >> 1)) // divisor)
    return q[:, :, ZIGZAG]


class _Bits:
    def __init__(self):
        self.value, self.count = 0, 0

    def put(self, code, length):
        self.value = (self.value << length) | code
        self.count += length

    def flush(self):
        """The bytes of the interval: padded with 1-bits to a whole byte, a 0x00 stuffed behind every 0xFF; and the number stuffed."""
        pad = -self.count % 8
        raw = ((self.value << pad) | ((1 << pad) - 1)).to_bytes((self.count + pad) // 8, "big")
        return raw.replace(b"\xFF", b"\xFF\x00"), raw.count(b"\xFF")


def _category(v):
    return int(abs(v)).bit_length()


def _value_bits(v, size):
    return (v if v >= 0 else v - 1) & ((1 << size) - 1)


def encode_block(bits, block, predictor, dc_codes, ac_codes, counters):
    diff = int(block[0]) - predictor
    size = _category(diff)
    counters["max_dc_category"] = max(counters["max_dc_category"], size)
    bits.put(*dc_codes[size])
    bits.put(_value_bits(diff, size), size)
    nonzero = np.flatnonzero(block[1:]) + 1
    last = 0
    for k in nonzero:
        run = int(k) - last - 1
        while run >= 16:
            bits.put(*ac_codes[0xF0])
            counters["zrl"] += 1
            run -= 16
        v = int(block[k])
        size = _category(v)
        bits.put(*ac_codes[run << 4 | size])
        bits.put(_value_bits(v, size), size)
        last = int(k)
    if last < 63:
        bits.put(*ac_codes[0x00])
        counters["eob_only_blocks"] += len(nonzero) == 0
    return int(block[0])


def encode_counted(rgb, quality, subsampling):
    """(the file, counters) of an (H, W, 3) uint8 picture."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"an (H, W, 3) uint8 picture, got {rgb.dtype} {rgb.shape}")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling {subsampling!r} is not one of {SUBSAMPLINGS}")
    H, W = rgb.shape[:2]
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"{H} x {W}: sides of 1 .. 65535")
    luma_q, chroma_q = quant_tables(quality)
    sub = subsampling == "4:2:0"
    mcu = 16 if sub else 8
    mcus_x, mcus_y = -(-W // mcu), -(-H // mcu)
    y, cb, cr = color_convert(rgb)
    blocks_w, blocks_h = -(-W // 8), -(-H // 8)  # real luminance blocks; the rest of the MCU grid is dummy blocks
    luma = np.zeros((mcus_y * mcu // 8, mcus_x * mcu // 8, 64), np.int64)
    luma[:blocks_h, :blocks_w] = quantised_blocks(_pad(y, blocks_h * 8, blocks_w * 8), luma_q)
    if sub:
        chroma = [quantised_blocks(downsample_420(c, mcus_y * 16, mcus_x * 16), chroma_q) for c in (cb, cr)]
    else:
        chroma = [quantised_blocks(_pad(c, mcus_y * 8, mcus_x * 8), chroma_q) for c in (cb, cr)]
    counters = {"stuffed_ff": 0, "zrl": 0, "eob_only_blocks": 0, "right_dummy_blocks": 0, "bottom_dummy_blocks": 0, "max_dc_category": 0, "intervals": mcus_y,
                "chroma_rows_replicated_after_downsampling": max(0, mcus_y * 8 - (H + 1) // 2) if sub else 0}
    tables = [(huffman_codes(HUFFMAN[0][1], HUFFMAN[0][2]), huffman_codes(HUFFMAN[1][1], HUFFMAN[1][2])),
              (huffman_codes(HUFFMAN[2][1], HUFFMAN[2][2]), huffman_codes(HUFFMAN[3][1], HUFFMAN[3][2]))]
    out = [header(H, W, quality, subsampling, mcus_x)]
    for my in range(mcus_y):
        bits, predictors = _Bits(), [0, 0, 0]
        for mx in range(mcus_x):
            if sub:
                members = []
                for dy in range(2):
                    for dx in range(2):
                        by, bx = 2 * my + dy, 2 * mx + dx
                        block = luma[by, bx]
                        if by >= blocks_h:  # a dummy row: zero AC, the DC of the block before it in the MCU (Y01)
                            block = np.zeros(64, np.int64)
                            block[0] = members[1][0]
                            counters["bottom_dummy_blocks"] += 1
                        elif bx >= blocks_w:  # past the right edge: zero AC, the DC of the block to its left
                            block = np.zeros(64, np.int64)
                            block[0] = members[-1][0]
                            counters["right_dummy_blocks"] += 1
                        members.append(block)
            else:
                members = [luma[my, mx]]
            for block in members:
                predictors[0] = encode_block(bits, block, predictors[0], *tables[0], counters)
            for c in range(2):
                predictors[1 + c] = encode_block(bits, chroma[c][my, mx], predictors[1 + c], *tables[1], counters)
        data, stuffed = bits.flush()
        counters["stuffed_ff"] += stuffed
        out.append(data + (bytes([0xFF, 0xD0 + my % 8]) if my + 1 < mcus_y else b"\xFF\xD9"))
    return b"".join(out), counters


def encode(rgb, quality, subsampling):
    return encode_counted(rgb, quality, subsampling)[0]
