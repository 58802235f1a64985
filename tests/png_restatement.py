"""PNG as csrc/png.hip writes it, restated in numpy from the PNG specification (filters, chunks, CRC-32), RFC 1950 (zlib, Adler-32) and RFC 1951 (deflate)
and the rules stated above ``hive_png_encode`` in include/hive_mi355x.h -- not from the kernel.  ``encode`` returns the whole file, ``encode_counted`` the file
and what the tests look at: the filtered stream, the filter of every row, every token of the parse and how every segment was coded.  zlib is not used here:
tests/test_png_cpu.py decodes these files with zlib and Pillow.
"""
import numpy as np

SEGMENT = 8192          # bytes of the filtered stream per deflate block
WINDOW = 32768
MAX_MATCH, MIN_MATCH = 258, 3
FAR = 4096              # a match of three bytes further away than this is not taken
FIXED_BYTES = 8 + 25 + 12 + 2 + 4 + 12   # signature, IHDR, the IDAT frame, the zlib header, the Adler-32, IEND

LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def kind_of(picture):
    a = np.asarray(picture)
    if a.dtype == np.uint8 and a.ndim == 2:
        return "gray8"
    if a.dtype == np.uint16 and a.ndim == 2:
        return "gray16"
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3:
        return "rgb8"
    raise ValueError(f"{a.dtype} {a.shape}")


def raw_rows(picture):
    """(rows [H][rowbytes] uint8 as PNG orders the samples, bytes per pixel)."""
    a, kind = np.asarray(picture), kind_of(picture)
    if kind == "gray16":
        return np.stack([a >> 8, a & 255], axis=2).astype(np.uint8).reshape(a.shape[0], -1), 2
    return np.ascontiguousarray(a).reshape(a.shape[0], -1), (3 if kind == "rgb8" else 1)


def filter_rows(rows, bpp):
    """The filtered stream (H * (1 + rowbytes) bytes) and the filter type of every row: all five filters against the RAW previous row (zero above the first),
    the smallest sum of |signed byte| wins, ties to the lowest type."""
    height, rowbytes = rows.shape
    out = np.zeros((height, rowbytes + 1), np.uint8)
    types = np.zeros(height, np.int64)
    zero = np.zeros(rowbytes, np.int64)
    for y in range(height):
        x = rows[y].astype(np.int64)
        b = rows[y - 1].astype(np.int64) if y else zero
        a = np.concatenate([np.zeros(bpp, np.int64), x[:-bpp]]) if rowbytes > bpp else np.zeros(rowbytes, np.int64)
        c = np.concatenate([np.zeros(bpp, np.int64), b[:-bpp]]) if rowbytes > bpp else np.zeros(rowbytes, np.int64)
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        candidates = [(x - pred) & 255 for pred in (zero, a, b, (a + b) >> 1, paeth)]
        sums = [int(np.where(f < 128, f, 256 - f).sum()) for f in candidates]
        types[y] = int(np.argmin(sums))  # the first of equal sums
        out[y, 0] = types[y]
        out[y, 1:] = candidates[types[y]]
    return out.reshape(-1), types


def previous_equal(stream):
    """prev[p] = the nearest q < p with stream[q:q + 3] == stream[p:p + 3] (both inside the stream), or -1: from a stable sort by the three bytes."""
    n = len(stream)
    prev = np.full(n, -1, np.int64)
    if n < 4:
        return prev
    s = stream.astype(np.int64)
    key = s[:-2] << 16 | s[1:-1] << 8 | s[2:]
    order = np.argsort(key, kind="stable")
    same = key[order[1:]] == key[order[:-1]]
    prev[order[1:][same]] = order[:-1][same]
    return prev


def match_lengths(stream, distance):
    """For every position p the number of bytes, at most 258 and not past the end of p's segment, that equal the bytes ``distance[p]`` before them (0 where the
    distance is not 1 .. min(p, 32768)).  Three bytes further away than FAR count as no match."""
    n = len(stream)
    p = np.arange(n)
    room = np.minimum(np.minimum((p // SEGMENT + 1) * SEGMENT, n) - p, MAX_MATCH)
    alive = (distance >= 1) & (distance <= p) & (distance <= WINDOW)
    length = np.zeros(n, np.int64)
    src = p - np.where(alive, distance, 0)
    for k in range(MAX_MATCH):
        alive = alive & (k < room)
        idx = np.flatnonzero(alive)
        if not len(idx):
            break
        ok = stream[idx + k] == stream[src[idx] + k]
        alive[idx[~ok]] = False
        length[idx[ok]] += 1
    length[(length == MIN_MATCH) & (distance > FAR)] = 0
    length[length < MIN_MATCH] = 0
    return length


def best_matches(stream, bpp, rowbytes):
    """(length, distance) per position: the longest of the three candidates (one pixel left, one row up, the nearest equal three bytes), ties to the smaller
    distance; length 0 where none reaches three bytes."""
    n = len(stream)
    p = np.arange(n)
    prev = previous_equal(stream)
    candidates = [np.full(n, bpp, np.int64), np.full(n, rowbytes + 1, np.int64), np.where(prev >= 0, p - prev, 0)]
    best_len, best_dist = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for d in candidates:
        length = match_lengths(stream, d)
        better = (length > best_len) | ((length == best_len) & (length > 0) & (d < best_dist))
        best_len, best_dist = np.where(better, length, best_len), np.where(better, d, best_dist)
    return best_len, best_dist


def code_lengths(counts, limit):
    """Huffman code lengths of at most ``limit`` bits.  Fewer than two used symbols: the lowest unused symbols get a count of 1 until two are used.  The tree:
    leaves in order of (count, symbol); always join the two smallest of (next leaf, next joined node), a leaf before a node of the same count; a joined node
    queues behind the earlier ones.  Deeper than the limit: every used count becomes (count + 1) >> 1, and again."""
    counts = [int(c) for c in counts]
    k = 0
    while sum(c > 0 for c in counts) < 2:
        if counts[k] == 0:
            counts[k] = 1
        k += 1
    while True:
        leaves = sorted((c, s) for s, c in enumerate(counts) if c)
        m = len(leaves)
        weight = [c for c, _ in leaves]
        parent = [0] * (2 * m - 1)
        li, ni = 0, m
        for new in range(m, 2 * m - 1):
            total = 0
            for _ in range(2):
                if li < m and (ni >= new or weight[li] <= weight[ni]):  # ni == new: no joined node waits
                    pick, li = li, li + 1
                else:
                    pick, ni = ni, ni + 1
                parent[pick] = new
                total += weight[pick]
            weight.append(total)
        lengths = [0] * len(counts)
        for leaf, (_, s) in enumerate(leaves):
            node, depth = leaf, 0
            while node != 2 * m - 2:
                node, depth = parent[node], depth + 1
            lengths[s] = depth
        if max(lengths) <= limit:
            return lengths
        counts = [(c + 1) >> 1 if c else 0 for c in counts]


def unlimited_depth(counts):
    """The deepest leaf of the Huffman tree of ``counts`` with no limit (for the test that the skewed case needs the limit)."""
    return max(code_lengths(counts, 10 ** 9))


def canonical_codes(lengths):
    """RFC 1951 3.2.2: codes of one length count up in symbol order."""
    bl_count = [0] * 17
    for n in lengths:
        bl_count[n] += 1
    bl_count[0] = 0
    next_code, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    codes = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            codes[s] = next_code[n]
            next_code[n] += 1
    return codes


class BitWriter:
    """Bits from the least significant bit of every byte up (RFC 1951 3.1.1)."""

    def __init__(self):
        self.bits = []

    def put(self, value, n):          # a number: least significant bit first
        self.bits.extend((value >> i) & 1 for i in range(n))

    def put_code(self, code, n):      # a Huffman code: most significant bit first
        self.bits.extend((code >> i) & 1 for i in range(n - 1, -1, -1))

    def to_bytes(self):
        bits = self.bits + [0] * (-len(self.bits) % 8)
        return np.packbits(np.array(bits, np.uint8).reshape(-1, 8), axis=1, bitorder="little").reshape(-1).tobytes() if bits else b""


def symbol_of(value, base):
    return max(s for s, b in enumerate(base) if b <= value)


def parse_segment(stream, start, end, best_len, best_dist):
    """Greedy from the segment's start: [(position, length, distance)], length 0 for a literal."""
    tokens, p = [], start
    while p < end:
        if best_len[p]:
            tokens.append((p, int(best_len[p]), int(best_dist[p])))
            p += int(best_len[p])
        else:
            tokens.append((p, 0, 0))
            p += 1
    return tokens


def dynamic_block(stream, tokens, final):
    """The BTYPE 2 block of these tokens as a BitWriter.  No repeat symbols 16 / 17 / 18: every code length is sent as itself."""
    lit_counts, dist_counts = [0] * 286, [0] * 30
    lit_counts[256] = 1
    for p, length, distance in tokens:
        if length:
            lit_counts[257 + symbol_of(length, LENGTH_BASE)] += 1
            dist_counts[symbol_of(distance, DIST_BASE)] += 1
        else:
            lit_counts[int(stream[p])] += 1
    lit_len, dist_len = code_lengths(lit_counts, 15), code_lengths(dist_counts, 15)
    lit_code, dist_code = canonical_codes(lit_len), canonical_codes(dist_len)
    hlit = max(257, max(s for s, n in enumerate(lit_len) if n) + 1)
    hdist = max(1, max(s for s, n in enumerate(dist_len) if n) + 1)
    sequence = lit_len[:hlit] + dist_len[:hdist]
    cl_counts = [0] * 19
    for n in sequence:
        cl_counts[n] += 1
    cl_len = code_lengths(cl_counts, 7)
    cl_code = canonical_codes(cl_len)
    hclen = max(4, max(i for i, s in enumerate(CL_ORDER) if cl_len[s]) + 1)
    w = BitWriter()
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.put(cl_len[s], 3)
    for n in sequence:
        w.put_code(cl_code[n], cl_len[n])
    for p, length, distance in tokens:
        if length:
            s = symbol_of(length, LENGTH_BASE)
            w.put_code(lit_code[257 + s], lit_len[257 + s])
            w.put(length - LENGTH_BASE[s], LENGTH_EXTRA[s])
            d = symbol_of(distance, DIST_BASE)
            w.put_code(dist_code[d], dist_len[d])
            w.put(distance - DIST_BASE[d], DIST_EXTRA[d])
        else:
            w.put_code(lit_code[int(stream[p])], lit_len[int(stream[p])])
    w.put_code(lit_code[256], lit_len[256])
    return w


def deflate(stream, bpp, rowbytes):
    """(the deflate bytes, [(tokens, "dynamic" | "stored")] per segment).  A segment is a dynamic block, behind which an empty stored block (000, zeros up to
    the byte, 00 00 FF FF) brings the stream back to a byte -- the last segment's block carries BFINAL and is only padded -- or, where that is not smaller than
    5 + its bytes, one stored block."""
    best_len, best_dist = best_matches(stream, bpp, rowbytes)
    out, report = [], []
    n = len(stream)
    for start in range(0, n, SEGMENT):
        end = min(start + SEGMENT, n)
        final = end == n
        tokens = parse_segment(stream, start, end, best_len, best_dist)
        w = dynamic_block(stream, tokens, final)
        if not final:
            w.put(0, 3)
        coded = w.to_bytes() + (b"" if final else b"\x00\x00\xff\xff")
        length = end - start
        if len(coded) < length + 5:
            out.append(coded)
            report.append((tokens, "dynamic"))
        else:
            out.append(bytes([1 if final else 0, length & 255, length >> 8, ~length & 255, (~length >> 8) & 255]) + stream[start:end].tobytes())
            report.append((tokens, "stored"))
    return b"".join(out), report


_CRC_TABLE = None


def crc32(data, crc=0):
    """The PNG specification's sample CRC: polynomial 0xEDB88320, bit by bit through a table of 256."""
    global _CRC_TABLE
    if _CRC_TABLE is None:
        _CRC_TABLE = []
        for n in range(256):
            c = n
            for _ in range(8):
                c = 0xEDB88320 ^ (c >> 1) if c & 1 else c >> 1
            _CRC_TABLE.append(c)
    c = crc ^ 0xFFFFFFFF
    for b in data:
        c = _CRC_TABLE[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def adler32(stream):
    """RFC 1950: s1 = 1 + the sum of the bytes, s2 = the sum of every s1, both mod 65521."""
    s1, s2 = 1, 0
    for i in range(0, len(stream), 4096):
        d = stream[i:i + 4096].astype(np.int64)
        s2 = (s2 + len(d) * s1 + int((d * np.arange(len(d), 0, -1)).sum())) % 65521  # byte k of the piece is in len - k of its running sums
        s1 = (s1 + int(d.sum())) % 65521
    return s2 << 16 | s1


def chunk(kind, data):
    body = kind + data
    return len(data).to_bytes(4, "big") + body + crc32(body).to_bytes(4, "big")


def encode_counted(picture):
    """(file, report): report has ``stream`` (the filtered bytes), ``filters``, ``segments`` ([(tokens, how)]), ``idat`` (the zlib stream)."""
    a = np.asarray(picture)
    kind = kind_of(a)
    rows, bpp = raw_rows(a)
    stream, filters = filter_rows(rows, bpp)
    body, segments = deflate(stream, bpp, rows.shape[1])
    idat = b"\x78\x01" + body + adler32(stream).to_bytes(4, "big")
    ihdr = a.shape[0:2][1].to_bytes(4, "big") + a.shape[0].to_bytes(4, "big") + bytes([16 if kind == "gray16" else 8, 2 if kind == "rgb8" else 0, 0, 0, 0])
    data = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")
    return data, {"stream": stream, "filters": filters, "segments": segments, "idat": idat}


def encode(picture):
    return encode_counted(picture)[0]


def stored_bound(picture):
    """Bytes of the all-stored file: what ``hive_png_layout`` reserves, before rounding up to a multiple of 4."""
    rows, _ = raw_rows(picture)
    n = rows.shape[0] * (1 + rows.shape[1])
    return FIXED_BYTES + n + 5 * ((n + SEGMENT - 1) // SEGMENT)
