"""Baseline JPEG, the parts that need no GPU: the numpy restatement (tests/jpeg_restatement.py) against the files Pillow writes, whole files; that the case list
reaches every corner of the rule; ``hive_jpeg_layout`` (host only) and the new C ABI symbols; ``read_glb`` on a JPEG-textured file and ``write_glb``'s argument
checks."""
import ctypes
import io
import json
import os
import re

import numpy as np
import pytest

import gltf_restatement as G
import jpeg_cases as C
import jpeg_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pillow_has_jpeg():
    from PIL import features
    return features.check("jpg")


needs_pillow_jpeg = pytest.mark.skipif(not _pillow_has_jpeg(), reason="this Pillow was built without libjpeg")


def _pillow_file(picture, quality, subsampling):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(np.asarray(picture)).save(out, format="JPEG", quality=quality, subsampling=C.PILLOW_SUBSAMPLING[subsampling], optimize=False, restart_marker_rows=1)
    return out.getvalue()


@needs_pillow_jpeg
@pytest.mark.parametrize("subsampling", C.SUBSAMPLINGS)
@pytest.mark.parametrize("quality", C.QUALITIES)
def test_restatement_equals_pillows_file(quality, subsampling):
    """The WHOLE file, header and scan, for every size and content of the list (no header field differs from Pillow's)."""
    for height, width, content in C.cases():
        mine = C.restated(height, width, content, quality, subsampling)[0]
        theirs = _pillow_file(C.picture(height, width, content), quality, subsampling)
        assert mine == theirs, (height, width, content, quality, subsampling, len(mine), len(theirs))
        assert mine[:2] == b"\xFF\xD8" and mine[-2:] == b"\xFF\xD9" and len(mine) > R.HEADER_BYTES == 629


@needs_pillow_jpeg
@pytest.mark.parametrize("case", C.LONG)
def test_restatement_equals_pillows_file_past_256_intervals(case):
    mine, counters = C.restated(*case)
    assert counters["intervals"] == 257
    assert mine == _pillow_file(C.picture(*case[:3]), *case[3:])


def test_case_list_reaches_every_corner_of_the_rule():
    total = {}
    for subsampling in C.SUBSAMPLINGS:
        for quality in C.QUALITIES:
            for case in C.cases():
                for key, value in C.restated(*case, quality, subsampling)[1].items():
                    total[key] = max(total.get(key, 0), value) if key in ("max_dc_category", "intervals") else total.get(key, 0) + value
    assert total["stuffed_ff"] > 0 and total["zrl"] > 0 and total["eob_only_blocks"] > 0
    assert total["right_dummy_blocks"] > 0 and total["bottom_dummy_blocks"] > 0
    assert total["intervals"] > 8, "the RST index wraps"
    # the largest DC difference 8-bit samples can give: a block of 0 (DC -1024 at quality 100) beside a block of 255 (DC 1016): 2040, category 11
    assert total["max_dc_category"] == 11 and C.restated(16, 16, "blocks", 100, "4:4:4")[1]["max_dc_category"] == 11
    # the chroma bottom rule: H mod 16 = 8 leaves four chroma rows to fill AFTER down-sampling
    for height, width in ((72, 104), (24, 40)):
        assert height % 16 == 8 and C.restated(height, width, "noise", 90, "4:2:0")[1]["chroma_rows_replicated_after_downsampling"] == 4
        assert C.restated(height, width, "noise", 90, "4:4:4")[1]["chroma_rows_replicated_after_downsampling"] == 0
    # a dummy block of each kind in one picture: 9 x 17 has two block rows and three block columns of luminance in 1 x 2 MCUs of 4:2:0 -- no dummy row, one dummy
    # column; 37 x 61: five block rows in three MCU rows (a dummy row), eight block columns in four MCUs (none)
    assert C.restated(9, 17, "flat", 90, "4:2:0")[1]["right_dummy_blocks"] == 2 and C.restated(9, 17, "flat", 90, "4:2:0")[1]["bottom_dummy_blocks"] == 0
    assert C.restated(37, 61, "flat", 90, "4:2:0")[1]["bottom_dummy_blocks"] == 8 and C.restated(37, 61, "flat", 90, "4:2:0")[1]["right_dummy_blocks"] == 0
    assert C.restated(57, 131, "flat", 90, "4:2:0")[1]["right_dummy_blocks"] == 8, "17 block columns in nine MCUs, four MCU rows"
    assert C.restated(40, 24, "flat", 90, "4:2:0")[1]["right_dummy_blocks"] == 5 and C.restated(40, 24, "flat", 90, "4:2:0")[1]["bottom_dummy_blocks"] == 4, \
        "five block rows beside a dummy column, a dummy row of four (its corner block counts as one of the row)"
    assert C.restated(1040, 16, "flat", 90, "4:2:0")[1]["intervals"] == 65 and C.restated(1040, 16, "flat", 90, "4:4:4")[1]["intervals"] == 130


def test_restatement_rejects_bad_arguments():
    picture = np.zeros((8, 8, 3), np.uint8)
    for bad in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            R.encode(picture, bad, "4:2:0")
    with pytest.raises(ValueError, match="subsampling"):
        R.encode(picture, 90, "4:2:2")
    with pytest.raises(ValueError, match="uint8"):
        R.encode(picture.astype(np.float32), 90, "4:2:0")


def test_symbols_are_declared_exported_and_bound():
    from hive_amd import _lib
    header = open(os.path.join(ROOT, "include", "hive_mi355x.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hive_jpeg_layout", "hive_jpeg_encode"):
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert "typedef struct hive_jpeg_image" in header and "22 + 63 * 26 = 1660 bits" in header, "the bound's derivation stands above the declaration"
    assert int(re.search(r"#define HIVE_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == _lib.load().hive_abi_version(), "additions only"
    assert ctypes.sizeof(_lib.JpegImage) == 24
    assert "hive_jpeg_encode" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _layout(shapes, subsampling_code):
    from hive_amd import _lib
    table = (_lib.JpegImage * len(shapes))()
    for row, (height, width) in zip(table, shapes):
        row.data, row.height, row.width, row.pitch = None, height, width, 3 * width  # host only: the pointer is not looked at
    offsets, total = (ctypes.c_int64 * len(shapes))(), ctypes.c_int64(-1)
    rc = _lib.load().hive_jpeg_layout(table, len(shapes), subsampling_code, offsets, total)
    return rc, list(offsets), total.value


@pytest.mark.parametrize("subsampling", C.SUBSAMPLINGS)
def test_layout_bounds_every_file(subsampling):
    """Host only, no device: the bound of every picture is the stated formula and at least the restatement's file at every quality and content."""
    from hive_amd import _lib, jpeg
    shapes = list(C.SIZES) + [C.LARGE]
    rc, offsets, total = _layout(shapes, _lib.JPEG_SUBSAMPLING[subsampling])
    assert rc == 0 and offsets[0] == 0 and all(o % 4 == 0 for o in offsets) and total % 4 == 0
    bounds = np.diff(offsets + [total])
    mcu = 16 if subsampling == "4:2:0" else 8
    for (height, width), bound in zip(shapes, bounds):
        mcus_x, mcus_y = -(-width // mcu), -(-height // mcu)
        blocks = mcus_x * mcus_y * (6 if subsampling == "4:2:0" else 3)
        assert bound == -(-(629 + 416 * blocks + 2 * mcus_y) // 4) * 4
    for (height, width, content) in C.cases():
        bound = bounds[shapes.index((height, width))]
        for quality in C.QUALITIES:
            assert len(C.restated(height, width, content, quality, subsampling)[0]) <= bound
    got_offsets, got_total = jpeg.layout(shapes, subsampling)
    assert list(got_offsets) == offsets and got_total == total
    assert _layout([(65535, 65535)], _lib.JPEG_SUBSAMPLING[subsampling])[0] == 0, "the largest picture of the format has a bound (in int64)"


def test_layout_rejects_and_names_the_picture():
    from hive_amd import _lib
    lib = _lib.load()
    for shapes, code, word in (([(8, 8), (0, 8)], 2, b"picture 1 is 0 x 8"), ([(8, 0)], 0, b"picture 0 is 8 x 0"), ([(8, 8), (8, 8), (65536, 8)], 2, b"picture 2 is 65536 x 8"),
                               ([(8, 65536)], 0, b"picture 0 is 8 x 65536"), ([(8, 8)], 1, b"unknown subsampling 1"), ([(8, 8)], 7, b"unknown subsampling 7")):
        rc, _, _ = _layout(shapes, code)
        assert rc == _lib.ERR_INVALID and word in lib.hive_last_error(None), lib.hive_last_error(None)
    assert lib.hive_jpeg_layout(None, 0, 2, (ctypes.c_int64 * 1)(), ctypes.c_int64(0)) == _lib.ERR_INVALID


def test_python_arguments_are_checked_before_any_launch():
    """Every refusal is a ValueError raised on the host: none of these calls reaches a device (this test runs without one)."""
    from hive_amd import jpeg
    good = np.zeros((8, 8, 3), np.uint8)
    for picture, word in ((good.astype(np.float32), "uint8"), (good[:, :, :2], r"\(H, W, 3\)"), (good[:, :, 0], r"\(H, W, 3\)"), (np.zeros((0, 8, 3), np.uint8), "0 x 8")):
        with pytest.raises(ValueError, match=word):
            jpeg.encode(picture)
    for quality in (0, 101, 90.5, "90", True):
        with pytest.raises(ValueError, match="quality"):
            jpeg.encode(good, quality=quality)
    with pytest.raises(ValueError, match="subsampling"):
        jpeg.encode(good, subsampling="4:2:2")
    with pytest.raises(ValueError, match="no pictures"):
        jpeg.encode([])


def _jpeg_blob(mime="image/jpeg", shift=0, damage=False):
    """A GLB of one textured and one coloured mesh assembled on the host whose image is the restatement's JPEG of a 24 x 40 picture."""
    rng = np.random.default_rng(21)
    textured = {"vertices": rng.normal(size=(7, 3)), "faces": rng.integers(0, 7, (5, 3)), "uv": rng.random((7, 2))}
    coloured = {"vertices": rng.normal(size=(4, 3)).astype(np.float32), "faces": np.array([[0, 1, 2], [2, 1, 3]], np.int32), "colors": rng.integers(0, 256, (4, 3), np.uint8)}
    data = C.restated(24, 40, "gradient_noise", 90, "4:2:0")[0]
    if damage:
        data = b"\xFF\xD8\x00" + data[3:]
    blob, doc, binary = G.assemble([textured, coloured], ["000003", "000000"], textures=[data])
    doc = json.loads(json.dumps(doc))
    doc["images"][0]["mimeType"] = mime
    if shift:
        view = doc["bufferViews"][doc["images"][0]["bufferView"]]
        view["byteOffset"] += shift
        view["byteLength"] -= shift
    return G.container(doc, binary), data


@needs_pillow_jpeg
def test_read_glb_reads_a_jpeg_texture(tmp_path):
    from PIL import Image
    from hive_amd import gltf
    blob, data = _jpeg_blob()
    path = tmp_path / "scene.glb"
    path.write_bytes(blob)
    scene = gltf.read_glb(str(path))
    assert list(scene.geometry) == ["000003", "000000"]
    texture = scene.meshes()[0]["texture"]
    assert texture.shape == (24, 40, 3) and np.array_equal(texture, np.array(Image.open(io.BytesIO(data)).convert("RGB")))


def test_read_glb_rejects_bad_jpeg_views(tmp_path):
    from hive_amd import gltf

    def refuses(data, word):
        path = tmp_path / "bad.glb"
        path.write_bytes(data)
        with pytest.raises(gltf.GltfError, match=word):
            gltf.read_glb(str(path))
    refuses(_jpeg_blob(damage=True)[0], "does not start FF D8 FF")
    refuses(_jpeg_blob(shift=2)[0], "4-byte aligned")
    refuses(_jpeg_blob(mime="image/webp")[0], "a PNG or a JPEG")


def test_write_glb_rejects_unknown_formats_and_qualities(tmp_path):
    from hive_amd import gltf
    from hive_amd.mesh import Mesh
    scene = gltf.Scene()
    scene.add_geometry(Mesh(np.eye(3), np.array([[0, 1, 2]], np.int32), np.zeros((3, 3), np.uint8)), node_name="000000")
    path = str(tmp_path / "never.glb")
    with pytest.raises(ValueError, match="texture_format 'webp'"):
        gltf.write_glb(path, scene, texture_format="webp")
    for quality in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            gltf.write_glb(path, scene, texture_format="jpeg", jpeg_quality=quality)
    with pytest.raises(ValueError, match="subsampling"):
        gltf.write_glb(path, scene, texture_format="jpeg", jpeg_subsampling="4:1:1")
    assert not os.path.exists(path)


def test_pipeline_options_carry_the_texture_format():
    import argparse
    from hive_amd.options import PipelineOptions
    assert PipelineOptions().texture_format == "png" and PipelineOptions().jpeg_quality == 90
    parser = argparse.ArgumentParser()
    PipelineOptions.add_args(parser)
    options = PipelineOptions.from_args(parser.parse_args(["--texture_format", "jpeg", "--jpeg_quality", "75"]))
    assert options.texture_format == "jpeg" and options.jpeg_quality == 75 and options.export_gltf is False
    assert PipelineOptions.from_args(parser.parse_args([])).texture_format == "png"
    with pytest.raises(SystemExit):
        parser.parse_args(["--texture_format", "webp"])
