"""The PNG rules on the CPU: every file of the numpy restatement (tests/png_restatement.py, what csrc/png.hip must reproduce byte for byte) is a PNG that
Pillow and zlib read back exactly; the stored bound holds; the window, the code-length limit and the size record are what the case list says they are.
No GPU: tests/test_png_gpu.py compares the device's bytes with these files."""
import io
import os
import struct
import warnings
import zlib

import numpy as np
import pytest

import png_cases as C
import png_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"gray8": "L", "gray16": "I;16", "rgb8": "RGB"}
# ours / Pillow's compress_level=1 file, measured (profiles/png_probe.json) and rounded up to the next 0.05: a later rule change that compresses worse trips it
LEVEL1_PINS = {("ramp_noise", "gray16"): 1.00, ("ramp", "rgb8"): 1.40, ("mask", "gray8"): 1.00, ("depth_480x640", "gray16"): 1.05}


def _chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(data):
        (length,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + length]
        (crc,) = struct.unpack(">I", data[at + 8 + length:at + 12 + length])
        out.append((kind, body, crc))
        at += 12 + length
    assert at == len(data)
    return out


def _stored_bound(picture):
    """The formula of hive_png_layout, restated: 63 bytes of frame, the filtered stream, 5 bytes per segment of 8192."""
    a = np.asarray(picture)
    rowbytes = a.shape[1] * (a.itemsize if a.ndim == 2 else 3)
    stream = a.shape[0] * (1 + rowbytes)
    return 8 + 25 + 12 + 2 + 4 + 12 + stream + 5 * -(-stream // 8192)


def _pillow(picture, level):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(np.asarray(picture)).save(out, "PNG", compress_level=level)
    return out.getvalue()


def _histogram(report, segment):
    tokens, _ = report["segments"][segment]
    lit, dist = [0] * 286, [0] * 30
    lit[256] = 1
    for p, length, distance in tokens:
        if length:
            lit[257 + R.symbol_of(length, R.LENGTH_BASE)] += 1
            dist[R.symbol_of(distance, R.DIST_BASE)] += 1
        else:
            lit[int(report["stream"][p])] += 1
    return lit, dist


@pytest.mark.parametrize("content,kind", C.cases())
def test_the_restatement_writes_a_png_that_reads_back(content, kind):
    from PIL import Image
    picture = C.picture(content, kind)
    data, report = C.restated(content, kind)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        image = Image.open(io.BytesIO(data))
        image.load()
    assert image.format == "PNG" and image.mode == MODES[kind] and image.size == (picture.shape[1], picture.shape[0])
    back = np.array(image)
    assert back.shape == picture.shape and np.array_equal(back.astype(picture.dtype), picture)
    chunks = _chunks(data)
    assert [k for k, _, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    for k, body, crc in chunks:
        assert crc == zlib.crc32(k + body), k
    idat = chunks[1][1]
    assert idat[:2] == b"\x78\x01" and idat == report["idat"]
    assert zlib.decompress(idat) == report["stream"].tobytes(), "the deflate stream and its Adler-32"
    assert len(report["stream"]) == picture.shape[0] * (1 + picture[0].nbytes)
    assert len(report["segments"]) == -(-len(report["stream"]) // C.S)
    bound = _stored_bound(picture)
    assert bound == R.stored_bound(picture) and len(data) <= bound, (len(data), bound)
    for tokens, _ in report["segments"]:
        for p, length, distance in tokens:
            assert length == 0 or (3 <= length <= 258 and 1 <= distance <= min(p, 32768) and p % C.S + length <= C.S), (p, length, distance)


def test_the_layout_is_the_stored_bound():
    """hive_png_layout (host only) gives the restated formula rounded up to a multiple of 4, and refuses what it cannot take."""
    from hive_amd import _lib, png
    cases = C.cases()
    offsets, total = png.layout([(C.picture(*case).shape[:2], case[1]) for case in cases])
    want = [(_stored_bound(C.picture(*case)) + 3) // 4 * 4 for case in cases]
    assert list(np.diff(np.append(offsets, total))) == want and offsets[0] == 0
    with pytest.raises(_lib.HiveError, match="sides of 1 .. 65535"):
        png.layout([((0, 5), "gray8")])
    table = (_lib.PngImage * 1)()
    table[0].height = table[0].width = 4
    table[0].kind = 3
    offsets, total = np.zeros(1, np.int64), _lib.c_int64(0)
    with pytest.raises(_lib.HiveError, match="unknown kind 3"):
        _lib.check(_lib.load().hive_png_layout(table, 1, _lib.ptr(offsets), total))


def test_the_header_declares_what_the_library_exports():
    header = open(os.path.join(ROOT, "include", "hive_mi355x.h")).read()
    from hive_amd import _lib
    lib = _lib.load()
    for name in ("hive_png_layout", "hive_png_encode"):
        assert f"int {name}(" in header and hasattr(lib, name) and name in _lib.SIGNATURES
    for word in ("S = 8192", "repeat symbols 16, 17, 18", "EMPTY stored block", "not pinned against Pillow's filter heuristic", "(count + 1) >> 1"):
        assert word in header, word
    assert [name for name, _ in _lib.PngImage._fields_] == ["pixels", "height", "width", "pitch", "kind"]


@pytest.mark.parametrize("kind", C.KINDS)
def test_noise_is_stored_and_never_larger_than_the_bound(kind):
    for content in ("noise", "halves_far", "halves_32769") + (("all_bytes",) if kind == "gray8" else ()):
        data, report = C.restated(content, kind)
        assert len(data) <= _stored_bound(C.picture(content, kind))
        assert [how for _, how in report["segments"]].count("stored") >= len(report["segments"]) - 1, content


def test_every_compressible_case_is_smaller_than_its_rows():
    for content, kind in C.cases():
        if content in ("S-1", "S", "S+1", "straddle", "flat", "skewed", "ramp_noise", "ramp", "mask", "depth_480x640"):
            data, report = C.restated(content, kind)
            assert len(data) < len(report["stream"]), (content, kind)


@pytest.mark.parametrize("kind", C.KINDS)
def test_the_window_ends_at_32768(kind):
    """Two equal halves of one row: at most 32 768 bytes apart the second is coded as matches into the first; further apart it is not, and no match anywhere
    reaches past the window."""
    far = {"halves_32768": [], "halves_far": [], "halves_32769": []}
    for content, matches in far.items():
        _, report = C.restated(content, kind)
        matches.extend((p, length, distance) for tokens, _ in report["segments"] for p, length, distance in tokens if distance > 30000)
    gap = C.HALF_GAPS[kind][1] * C.BPP[kind]
    assert gap <= 32768 < C.HALF_GAPS[kind][2] * C.BPP[kind]
    inside = far["halves_32768"]
    assert inside and all(d == gap for _, _, d in inside) and sum(length for _, length, _ in inside) >= 1100, "the second half is matches at the gap"
    assert not far["halves_far"] and not far["halves_32769"]
    assert len(C.restated("halves_32768", kind)[0]) < len(C.restated("halves_32769", kind)[0]) - 1000


@pytest.mark.parametrize("kind", C.KINDS)
def test_a_flat_picture_is_runs_cut_at_258_and_at_the_segment_end(kind):
    _, report = C.restated("flat", kind)
    lengths = [length for tokens, _ in report["segments"] for _, length, _ in tokens if length]
    assert max(lengths) == 258 and lengths.count(258) > 50
    for tokens, how in report["segments"][:-1]:
        p, length, _ = tokens[-1]
        assert how == "dynamic" and length and p % C.S + length == C.S, "the last match of a segment ends with it"
    # one or two distance codes in use: the table sent is still complete (zlib inflates it above) and follows the rule for a single code
    for segment in range(len(report["segments"])):
        lit, dist = _histogram(report, segment)
        lengths = R.code_lengths(dist, 15)
        assert sum(2.0 ** -n for n in lengths if n) == 1.0
        if sum(c > 0 for c in dist) == 1:
            assert sorted(n for n in lengths if n) == [1, 1] and lengths[0] == 1


def test_a_single_or_missing_distance_code_gets_a_complete_table():
    assert R.code_lengths([0] * 30, 15) == [1, 1] + [0] * 28
    assert R.code_lengths([7] + [0] * 29, 15) == [1, 1] + [0] * 28
    assert R.code_lengths([0, 0, 0, 9] + [0] * 26, 15) == [1, 0, 0, 1] + [0] * 26


@pytest.mark.parametrize("kind", C.KINDS)
def test_the_skewed_case_needs_the_length_limit(kind):
    """The second segment's symbols have the counts 1, 1, 2, 3, 5 .. 987, 1597: without a limit the deepest code would be 16 bits."""
    _, report = C.restated("skewed", kind)
    assert list(report["filters"]) == [0] and len(report["segments"]) == 2
    lit, dist = _histogram(report, 1)
    assert sorted(c for c in lit if c) == sorted((1,) + C.FIBONACCI + (1597,)) and lit[257] == 1597 and lit[256] == 1
    assert R.unlimited_depth(lit) == 16 > 15
    limited = R.code_lengths(lit, 15)
    assert max(limited) <= 15 and sum(2.0 ** -n for n in limited if n) == 1.0


def test_the_filter_rule_equals_pillows_choice_on_smooth_pictures():
    """Stated, not pinned in general: on the ramp and the flat picture Pillow (libpng's heuristic) picks the same filter row for row; on noisy rows it may not."""
    for content, kind in (("ramp", "gray16"), ("ramp", "rgb8"), ("flat", "gray8")):
        picture = C.picture(content, kind)
        _, report = C.restated(content, kind)
        theirs = zlib.decompress(b"".join(body for k, body, _ in _chunks(_pillow(picture, 6)) if k == b"IDAT"))
        step = 1 + picture[0].nbytes
        assert list(theirs[::step]) == list(report["filters"]), (content, kind)


@pytest.mark.parametrize("content,kind", C.SIZE_RECORD)
def test_the_size_record(content, kind):
    """Ours against Pillow's level 1 (the pin) and level 6 (printed): the design goal is zlib's fast setting."""
    picture = C.picture(content, kind)
    ours, level1, level6 = len(C.restated(content, kind)[0]), len(_pillow(picture, 1)), len(_pillow(picture, 6))
    print(f"{content} {kind}: {ours} bytes, x{ours / level1:.3f} of level 1 ({level1}), x{ours / level6:.3f} of level 6 ({level6})")
    assert ours <= LEVEL1_PINS[(content, kind)] * level1, (ours, level1, level6)


def test_the_long_record_is_the_restatements_file():
    """The slow one (seconds): 257 segments and 1025 sort tiles.  The file recorded for the GPU test is the restatement's, and Pillow reads the input back."""
    import hashlib
    picture = C.long_picture()
    stream = picture.shape[0] * (1 + picture.shape[1])
    assert -(-stream // C.S) == 257 and -(-stream // 2048) == 1025
    data = R.encode(picture)
    assert {"length": len(data), "sha256": hashlib.sha256(data).hexdigest()} == C.LONG_RECORD
    from PIL import Image
    image = Image.open(io.BytesIO(data))
    assert image.mode == "L" and np.array_equal(np.array(image), picture)


def test_png_encoder_names_are_checked_without_a_gpu():
    from hive_amd import png
    from hive_amd.options import PipelineOptions
    png.check_encoder("host")
    png.check_encoder("gpu")
    with pytest.raises(ValueError, match="png_encoder 'zlib'"):
        png.check_encoder("zlib")
    assert PipelineOptions().png_encoder == "host" and PipelineOptions(png_encoder="gpu").copy().png_encoder == "gpu"
    with pytest.raises(ValueError, match="uint8 or uint16"):
        png.kind_of(0, np.zeros((4, 4), np.float32))
    assert [png.kind_of(0, C.picture("1x7", kind)) for kind in C.KINDS] == list(C.KINDS)
