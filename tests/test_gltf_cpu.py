"""glTF export, the parts that need no GPU: the new C ABI symbols, ``hive_gltf_layout`` (host only) against the numpy restatement, ``read_glb``'s strictness on
blobs the restatement assembles, the centring rule on a worked example, the player's metadata and ``align_scene``."""
import ctypes
import io
import json
import os
import re
import struct

import numpy as np
import pytest

import gltf_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    from hive_amd import _lib
    header = open(os.path.join(ROOT, "include", "hive_mi355x.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hive_gltf_layout", "hive_gltf_pack"):
        assert re.search(rf"^int {name}\(", header, flags=re.M), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert "typedef struct hive_gltf_mesh" in header and "typedef struct hive_gltf_view" in header
    # additions only: the ABI number stays (tests/test_pairs_cpu.py pins it); a library without the two symbols fails to load by name
    assert int(re.search(r"#define HIVE_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    assert _lib.load().hive_abi_version() == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.GltfMesh) == 64 and ctypes.sizeof(_lib.GltfView) == 16
    stubs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "hive_gltf_layout" in stubs and "hive_gltf_pack" in stubs


def _layout(shapes, quantize):
    """hive_gltf_layout of meshes given as (V, F, has uv, colour channels or 0); the pointers are placeholders (the call only tests them against NULL)."""
    from hive_amd import _lib
    lib = _lib.load()
    table = (_lib.GltfMesh * len(shapes))()
    for row, (V, F, uv, channels) in zip(table, shapes):
        row.vertices, row.faces, row.n_vertices, row.n_faces = 16, 16, V, F
        row.uv = 16 if uv else None
        row.colors, row.color_channels = (16 if channels else None), channels
        row.vertex_dtype, row.face_dtype = _lib.GLTF_F64, _lib.GLTF_I64
    views = (_lib.GltfView * (4 * len(shapes)))()
    total = ctypes.c_int64(-1)
    rc = lib.hive_gltf_layout(table, len(shapes), quantize, views, total)
    return rc, [[(v.offset, v.length) for v in views[4 * k:4 * k + 4]] for k in range(len(shapes))], total.value


def _stand_in(V, F, uv, channels):
    mesh = {"vertices": np.zeros((V, 3)), "faces": np.zeros((F, 3), np.int64)}
    if uv:
        mesh["uv"] = np.zeros((V, 2))
    if channels:
        mesh["colors"] = np.zeros((V, channels), np.uint8)
    return mesh


@pytest.mark.parametrize("quantize", [0, 1])
def test_layout_equals_restatement(quantize):
    sizes = (1, 3, 65535, 65536)
    shapes = []
    for V in sizes:  # odd and even face counts: 3 F uint16 indices end off a 4-byte boundary when F is odd
        shapes += [(V, 1, False, 0), (V, 5, True, 0), (V, 2, False, 3), (V, 7, False, 4), (V, 3, True, 4)]
    rc, views, total = _layout(shapes, quantize)
    assert rc == 0
    want_views, want_total = R.layout([_stand_in(*s) for s in shapes], quantize)
    assert views == want_views and total == want_total
    assert total % 4 == 0 and all(offset % 4 == 0 for row in views for offset, length in row if length)
    for (V, F, uv, channels), row in zip(shapes, views):
        assert row[R.INDICES][1] == 3 * F * (2 if quantize and V <= 65535 else 4), "uint16 indices up to 65535 vertices when quantised"
        assert (row[R.TEXCOORD][1] > 0) == uv and (row[R.COLOR][1] > 0) == bool(channels)
    # a mesh alone: the same lengths, offsets from 0
    for shape, row in zip(shapes, views):
        rc, alone, _ = _layout([shape], quantize)
        assert rc == 0 and [length for _, length in alone[0]] == [length for _, length in row] and alone[0][0][0] == 0


def test_layout_rejects_and_names_the_mesh():
    from hive_amd import _lib
    lib = _lib.load()
    for shapes, word in (([(4, 2, False, 3), (4, 0, False, 3)], b"mesh 1 has n_faces == 0"), ([(0, 2, False, 3)], b"mesh 0 has 0 vertices"),
                         ([(4, 2, False, 3), (4, 2, False, 3), (4, 2, False, 2)], b"mesh 2: 2 colour channels")):
        rc, _, _ = _layout(shapes, 0)
        assert rc == _lib.ERR_INVALID and word in lib.hive_last_error(None), lib.hive_last_error(None)


def _png(texture):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(texture).save(out, format="PNG")
    return out.getvalue()


def _two_meshes():
    rng = np.random.default_rng(21)
    textured = {"vertices": rng.normal(size=(7, 3)), "faces": rng.integers(0, 7, (5, 3)), "uv": rng.random((7, 2))}
    coloured = {"vertices": rng.normal(size=(4, 3)).astype(np.float32), "faces": np.array([[0, 1, 2], [2, 1, 3]], np.int32), "colors": rng.integers(0, 256, (4, 3), np.uint8)}
    texture = rng.integers(0, 256, (6, 9, 3), np.uint8)
    return textured, coloured, texture


@pytest.mark.parametrize("quantize", [False, True])
def test_read_glb_accepts_the_restatements_blob(tmp_path, quantize):
    from hive_amd import gltf
    from hive_amd.mesh import Mesh
    textured, coloured, texture = _two_meshes()
    matrix = np.array([[-1.0, 0, 0, 0.5], [0, -1.0, 0, 2.0], [0, 0, 1.0, -3.0], [0, 0, 0, 1.0]])
    lut = np.arange(255, -1, -1).astype(np.uint8)
    blob, doc, binary = R.assemble([textured, coloured], ["000003", "000000"], quantize=quantize, lut=lut, matrix=matrix, textures=[_png(texture)],
                                   camera=dict(resolution=(64, 48), focal=(50.0, 52.0)))
    R.check_container(blob)
    path = tmp_path / "scene.glb"
    path.write_bytes(blob)
    scene = gltf.read_glb(str(path))
    assert list(scene.geometry) == ["000003", "000000"] and np.array_equal(scene.transform, matrix)
    assert scene.camera == {"resolution": (64, 48), "focal": (50.0, 52.0)}
    a, b = scene.meshes()
    assert isinstance(a, dict) and isinstance(b, Mesh)
    assert np.array_equal(a["faces"], textured["faces"]) and a["faces"].dtype == np.int64 and np.array_equal(b.faces, coloured["faces"])
    assert np.array_equal(a["texture"], texture)
    assert np.array_equal(b.visual.vertex_colors, np.hstack([lut[coloured["colors"]], np.full((4, 1), 255, np.uint8)]))
    c = R.texcoords(textured["uv"])
    if quantize:
        for got, mesh in ((a["vertices"], textured), (b.vertices, coloured)):
            q, lo, s = R.quantise_positions(mesh["vertices"])
            assert np.array_equal(got, q.astype(np.float64) * s + lo)
            assert np.all(np.abs(got - mesh["vertices"].astype(np.float64)) <= s / 2 + 4 * np.spacing(np.abs(np.stack(R.bounds_of(mesh["vertices"]))).max(axis=0)))
        stored = np.rint(np.clip(c, 0, 1) * 65535.0) / 65535.0
    else:
        assert np.array_equal(a["vertices"], textured["vertices"].astype(np.float32).astype(np.float64))
        assert np.array_equal(b.vertices, coloured["vertices"].astype(np.float64))
        stored = c.astype(np.float32).astype(np.float64)
    assert np.array_equal(a["uv"], np.stack([stored[:, 0], 1.0 - stored[:, 1]], axis=1)), "uv back in the atlas's bottom-left convention"
    # under the root transform
    moved = scene.meshes(apply_transform=True)[1]
    assert np.array_equal(moved.vertices, b.vertices @ matrix[:3, :3].T + matrix[:3, 3])


def _rebuild(doc, binary):
    return R.container(doc, binary)


def test_read_glb_rejects_damaged_blobs(tmp_path):
    from hive_amd import gltf
    textured, coloured, texture = _two_meshes()
    blob, doc, binary = R.assemble([textured, coloured], ["a", "b"], textures=[_png(texture)])

    def refuses(data, word):
        path = tmp_path / "bad.glb"
        path.write_bytes(data)
        with pytest.raises(gltf.GltfError, match=word):
            gltf.read_glb(str(path))
    good = tmp_path / "good.glb"
    good.write_bytes(blob)
    gltf.read_glb(str(good))
    # a truncated BIN chunk: the file ends 8 bytes early (the header still states the full length), and one whose header was corrected but whose chunk is short
    refuses(blob[:-8], "the header says")
    short = bytearray(blob[:-8])
    struct.pack_into("<I", short, 8, len(short))
    refuses(bytes(short), "passes the end of the file")
    json_len = struct.unpack_from("<I", blob, 12)[0]
    struct.pack_into("<I", short, 20 + json_len, struct.unpack_from("<I", blob, 20 + json_len)[0] - 8)
    refuses(bytes(short), "buffer 0 has")
    # an accessor past its view
    past = json.loads(json.dumps(doc))
    past["accessors"][0]["count"] += 1
    refuses(_rebuild(past, binary), "accessor 0 ends at byte")
    # a view past the buffer
    past = json.loads(json.dumps(doc))
    past["bufferViews"][0]["byteLength"] = len(binary) + 4
    refuses(_rebuild(past, binary), "the buffer has")
    # an index outside the vertices
    past = json.loads(json.dumps(doc))
    index_view = past["bufferViews"][past["accessors"][past["meshes"][1]["primitives"][0]["indices"]]["bufferView"]]
    broken = bytearray(binary)
    struct.pack_into("<I", broken, index_view["byteOffset"], 4)
    refuses(_rebuild(past, bytes(broken)), "outside")
    # an unknown required extension
    past = json.loads(json.dumps(doc))
    past["extensionsUsed"] = past["extensionsRequired"] = ["KHR_draco_mesh_compression"]
    refuses(_rebuild(past, binary), "KHR_draco_mesh_compression")
    # magic, alignment
    refuses(b"glTG" + blob[4:], "magic")
    past = json.loads(json.dumps(doc))
    past["bufferViews"][1]["byteOffset"] += 2
    refuses(_rebuild(past, binary), "4-byte boundary")


def _pipeline(**options):
    from hive_amd.options import PipelineOptions, StorageOptions
    from hive_amd.pipeline import Pipeline
    return Pipeline(options=PipelineOptions(**options), storage_options=StorageOptions("in", "out"))


def _host_scene(*vertex_sets):
    from hive_amd import gltf
    from hive_amd.mesh import Mesh
    scene = gltf.Scene(camera=dict(resolution=(64, 48), focal=(50.0, 50.0)))
    for k, vertices in enumerate(vertex_sets):
        scene.add_geometry(Mesh(np.asarray(vertices, np.float64), np.array([[0, 1, 2]], np.int32), np.zeros((len(vertices), 3), np.uint8)), node_name=f"{k:06d}")
    return scene


def test_centring_of_a_worked_example():
    """Two meshes by hand.  bg spans x [-1, 3], y [0.1, 2.1], z [1, 5]; fg spans x [0, 0.5], y [-0.3, 1], z [2, 2.5].  After the turn diag(-1, -1, 1, 1) the joint
    bounds are x [-3, 1], y [-2.1, 0.3], z [1, 5]: centroid x = -1, so the offset is (1, 2.1, -1), and 2.1 is not a float32: the stored offset is float32(2.1)."""
    bg = _host_scene([[-1, 0.1, 1], [3, 2.1, 5], [0, 1, 2]])
    fg = _host_scene([[0, -0.3, 2], [0.5, 1, 2.5], [0.2, 0, 2.2]])
    pipe = _pipeline()
    fg2, bg2 = pipe._center_scenes(None, fg, bg)
    want = np.array([[-1.0, 0, 0, 1.0], [0, -1.0, 0, float(np.float32(2.1))], [0, 0, 1.0, -1.0], [0, 0, 0, 1.0]])
    assert np.array_equal(fg2.transform, want) and np.array_equal(bg2.transform, want)
    assert want[1, 3] != 2.1, "the offset is rounded to float32"
    turn, translation = R.centring(fg.bounds, bg.bounds)
    assert np.array_equal(translation @ turn, want)
    assert np.array_equal(turn[:3, :3], np.diag([-1.0, -1.0, 1.0])) and not np.any(turn[:3, :3][~np.eye(3, dtype=bool)]), "the turn is exact: no 1.2e-16"
    assert np.array_equal(fg.transform, np.eye(4)) and np.array_equal(bg.transform, np.eye(4)), "the scenes handed in are not changed"
    joint = pipe._get_scene_bounds(fg2, bg2)
    assert abs(joint[0, 0] + joint[1, 0]) < 1e-12 and abs(joint[0, 1]) < 1e-6 and joint[0, 2] == 0.0
    # an empty foreground scene contributes no bounds: the offset comes from the background alone
    empty = _host_scene()
    assert empty.is_empty and empty.bounds is None
    fg3, bg3 = pipe._center_scenes(None, empty, bg)
    turn, translation = R.centring(None, bg.bounds)
    assert np.array_equal(bg3.transform, translation @ turn) and np.array_equal(fg3.transform, bg3.transform)
    assert np.array_equal(bg3.transform[:3, 3], np.array([1.0, np.float32(2.1), -1.0]))
    # a foreground mesh that widens the bounds moves the centre
    wide = _host_scene([[-9, 0.5, 2], [0, 1, 2.5], [0, 0.6, 2.2]])
    _, bg4 = pipe._center_scenes(None, wide, bg)
    assert bg4.transform[0, 3] == -3.0  # x [-9, 3] -> [-3, 9] after the turn, centroid 3


def test_scene_container():
    from hive_amd import gltf
    scene = _host_scene([[0, 0, 0], [1, 2, 3], [1, 0, 0]])
    with pytest.raises(ValueError):
        scene.add_geometry(scene.geometry["000000"], node_name="000000")
    assert not scene.is_empty and np.array_equal(scene.bounds, [[0, 0, 0], [1, 2, 3]])
    other = scene.copy()
    other.apply_transform(np.diag([2.0, 1.0, 1.0, 1.0]))
    other.apply_transform(np.array([[1.0, 0, 0, 5], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))
    assert np.array_equal(other.bounds, [[5, 0, 0], [7, 2, 3]]), "apply_transform left-multiplies"
    assert np.array_equal(scene.transform, np.eye(4)) and other.camera == scene.camera
    assert gltf.camera_json(scene.camera)["perspective"]["aspectRatio"] == 64 / 48


def test_metadata_keys_and_align_scene():
    from types import SimpleNamespace
    pipe = _pipeline(num_frames=7)
    dataset = SimpleNamespace(fps=30.0, frame_height=480, frame_width=640, camera_matrix=np.array([[525.0, 0, 320], [0, 525.0, 240], [0, 0, 1]]),
                              base_path="/data/some_video")
    metadata = pipe._get_webxr_metadata(dataset)
    assert list(metadata) == ["fps", "fov_y", "num_frames", "use_vertex_colour_for_bg", "add_ground_plane", "add_sky_box"]
    assert metadata == dict(fps=30.0, fov_y=49, num_frames=7, use_vertex_colour_for_bg=True, add_ground_plane=False, add_sky_box=False)
    json.dumps(metadata)
    assert pipe._get_dataset_name(dataset) == "some_video"
    scene = pipe._create_empty_scene(dataset)
    assert scene.is_empty and scene.camera == {"resolution": (640, 480), "focal": (525.0, 525.0)}
    with pytest.raises(NotImplementedError, match="align_scene"):
        _pipeline(align_scene=True)._center_scenes(None, _host_scene(), _host_scene([[0, 0, 0], [1, 1, 1], [1, 0, 0]]))
    from hive_amd.options import PipelineOptions
    assert PipelineOptions().export_gltf is False
