"""numpy restatements of the glTF export's rules (include/hive_mi355x.h, the glTF section; hive_amd/pipeline.py ``_center_scenes``) and an independent
structural check of a GLB container, both written from the glTF 2.0 specification and KHR_mesh_quantization -- not from hive_amd/gltf.py.

A mesh here is a dict of numpy arrays: ``vertices`` (V, 3) float32 / float64, ``faces`` (F, 3) int32 / int64 and either ``uv`` (V, 2) float64 or ``colors``
(V, 3 or 4) uint8."""
import json
import struct

import numpy as np

POSITION, TEXCOORD, COLOR, INDICES = range(4)


def view_bytes(mesh, quantize):
    V, F = len(mesh["vertices"]), len(mesh["faces"])
    short = quantize and V <= 65535
    return [V * (8 if quantize else 12), (V * (4 if quantize else 8)) if mesh.get("uv") is not None else 0, V * 4 if mesh.get("colors") is not None else 0,
            F * 3 * (2 if short else 4)]


def layout(meshes, quantize):
    """views[n][4] = (offset, length) in the order POSITION, TEXCOORD_0, COLOR_0, indices (absent: (0, 0)) and the buffer's length: every view at the next
    multiple of 4, the buffer's end on a multiple of 4."""
    at, views = 0, []
    for mesh in meshes:
        row = []
        for size in view_bytes(mesh, quantize):
            if size == 0:
                row.append((0, 0))
                continue
            at = (at + 3) // 4 * 4
            row.append((at, size))
            at += size
        views.append(row)
    return views, (at + 3) // 4 * 4


def bounds_of(vertices):
    v = np.asarray(vertices).astype(np.float64)
    return v.min(axis=0), v.max(axis=0)


def step_of(lo, hi):
    return np.where(hi == lo, 1.0, (hi - lo) / 65535.0)


def quantise_positions(vertices):
    """(q uint16 (V, 3), lo, s): q = min(65535, rint((x - lo) / s)), rint half to even, float64 with one rounding per operation."""
    x = np.asarray(vertices).astype(np.float64)
    lo, hi = bounds_of(x)
    s = step_of(lo, hi)
    return np.minimum(65535.0, np.rint((x - lo) / s)).astype(np.uint16), lo, s


def texcoords(uv):
    uv = np.asarray(uv, np.float64)
    return np.stack([uv[:, 0], 1.0 - uv[:, 1]], axis=1)  # top-left origin, the subtraction in float64


def pack(meshes, quantize, lut=None):
    """(the buffer's bytes, bounds (n, 2, 3) float64) by the pack rules."""
    views, total = layout(meshes, quantize)
    out = np.zeros(total, np.uint8)

    def put(view, array):
        data = np.frombuffer(np.ascontiguousarray(array).tobytes(), np.uint8)
        assert len(data) == view[1], (len(data), view)
        out[view[0]:view[0] + view[1]] = data
    bounds = []
    for mesh, row in zip(meshes, views):
        x = np.asarray(mesh["vertices"])
        V = len(x)
        lo, hi = bounds_of(x)
        bounds.append([lo, hi])
        if quantize:
            q = np.zeros((V, 4), "<u2")
            q[:, :3] = quantise_positions(x)[0]
            put(row[POSITION], q)
        else:
            put(row[POSITION], x.astype("<f4"))
        if mesh.get("uv") is not None:
            c = texcoords(mesh["uv"])
            put(row[TEXCOORD], np.rint(np.clip(c, 0.0, 1.0) * 65535.0).astype("<u2") if quantize else c.astype("<f4"))
        if mesh.get("colors") is not None:
            c = np.asarray(mesh["colors"], np.uint8)
            rgba = np.full((V, 4), 255, np.uint8)
            rgba[:, :c.shape[1]] = c
            if lut is not None:
                rgba[:, :3] = np.asarray(lut, np.uint8)[rgba[:, :3]]
            put(row[COLOR], rgba)
        f = np.asarray(mesh["faces"]).astype(np.int64)
        assert f.min() >= 0 and f.max() < V
        put(row[INDICES], f.astype("<u2" if quantize and V <= 65535 else "<u4"))
    return out.tobytes(), np.array(bounds)


def centring(fg_bounds, bg_bounds):
    """(turn, translation) of ``_center_scenes`` (/root/reference/hive/pipeline.py:999-1029) from the bounds (2, 3) of the two scenes BEFORE the turn (fg_bounds
    None: no foreground): the turn about z by 180 degrees is exactly diag(-1, -1, 1, 1); the offset (-centroid_x, -min_y, -min_z) of the joint bounds after the
    turn is rounded to float32."""
    turn = np.diag([-1.0, -1.0, 1.0, 1.0])

    def turned(b):  # x and y change sign, so their minima and maxima change places
        b = np.asarray(b, np.float64)
        return np.array([[-b[1, 0], -b[1, 1], b[0, 2]], [-b[0, 0], -b[0, 1], b[1, 2]]])
    joint = turned(bg_bounds)
    if fg_bounds is not None:
        fg = turned(fg_bounds)
        joint = np.array([np.minimum(fg[0], joint[0]), np.maximum(fg[1], joint[1])])
    centroid = joint.mean(axis=0)
    translation = np.eye(4)
    translation[:3, 3] = np.array([-centroid[0], -joint[0, 1], -joint[0, 2]]).astype(np.float32)
    return turn, translation


# ---------------------------------------------------------------------------------------------------------------- the container
MAGIC, JSON_CHUNK, BIN_CHUNK = 0x46546C67, 0x4E4F534A, 0x004E4942
COMPONENT_BYTES = {5120: 1, 5121: 1, 5122: 2, 5123: 2, 5125: 4, 5126: 4}
TYPE_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT2": 4, "MAT3": 9, "MAT4": 16}


def container(doc, binary):
    """A GLB blob: the 12-byte header, the JSON chunk padded with spaces, the BIN chunk padded with zeros."""
    text = json.dumps(doc).encode()
    text += b" " * (-len(text) % 4)
    binary = binary + b"\0" * (-len(binary) % 4)
    body = struct.pack("<II", len(text), JSON_CHUNK) + text
    if binary:
        body += struct.pack("<II", len(binary), BIN_CHUNK) + binary
    return struct.pack("<III", MAGIC, 2, 12 + len(body)) + body


def check_container(blob):
    """Structural check of a GLB blob against the specification; returns (document, binary buffer).  Asserts: header, chunk order / lengths / padding, every
    buffer view inside the buffer and on a 4-byte boundary, every accessor inside its view with its component's alignment, POSITION min / max present and equal
    to the stored values' (integers when quantised), index values inside the vertex count, node / mesh / material / texture / image references resolving,
    extensionsRequired a subset of extensionsUsed."""
    magic, version, length = struct.unpack_from("<III", blob, 0)
    assert magic == MAGIC and version == 2 and length == len(blob) and length % 4 == 0
    n, kind = struct.unpack_from("<II", blob, 12)
    assert kind == JSON_CHUNK and n % 4 == 0
    text = blob[20:20 + n]
    doc = json.loads(text.decode())
    assert text.rstrip(b" ") == text.rstrip(), "the JSON chunk is padded with spaces only"
    at, binary = 20 + n, b""
    if at < length:
        m, kind = struct.unpack_from("<II", blob, at)
        assert kind == BIN_CHUNK and m % 4 == 0 and at + 8 + m == length
        binary = blob[at + 8:]
    assert doc["asset"]["version"] == "2.0"
    assert set(doc.get("extensionsRequired", [])) <= set(doc.get("extensionsUsed", []))
    if "buffers" in doc:
        assert len(doc["buffers"]) == 1 and "uri" not in doc["buffers"][0]
        size = doc["buffers"][0]["byteLength"]
        assert size <= len(binary) < size + 4 and not any(binary[size:])
    for view in doc.get("bufferViews", []):
        assert view["buffer"] == 0 and view.get("byteOffset", 0) % 4 == 0 and view.get("byteOffset", 0) + view["byteLength"] <= doc["buffers"][0]["byteLength"]
        if "byteStride" in view:
            assert view["byteStride"] % 4 == 0 and 4 <= view["byteStride"] <= 252

    def values(index):
        a = doc["accessors"][index]
        view = doc["bufferViews"][a["bufferView"]]
        size, width = COMPONENT_BYTES[a["componentType"]], TYPE_WIDTH[a["type"]]
        start = view.get("byteOffset", 0) + a.get("byteOffset", 0)
        stride = view.get("byteStride", size * width)
        assert start % size == 0 and a["count"] >= 1
        assert a.get("byteOffset", 0) + stride * (a["count"] - 1) + size * width <= view["byteLength"], "the accessor passes its view"
        dtype = {5121: "u1", 5123: "<u2", 5125: "<u4", 5126: "<f4"}[a["componentType"]]
        rows = [np.frombuffer(binary, dtype, width, start + k * stride) for k in range(a["count"])] if stride != size * width else \
            np.frombuffer(binary, dtype, width * a["count"], start).reshape(a["count"], width)
        return np.array(rows), a
    assert doc["scene"] == 0 and len(doc["scenes"]) == 1
    for root in doc["scenes"][0]["nodes"]:
        assert 0 <= root < len(doc["nodes"])
    for node in doc["nodes"]:
        for child in node.get("children", []):
            assert 0 <= child < len(doc["nodes"])
        if "matrix" in node:
            assert len(node["matrix"]) == 16 and not ({"translation", "rotation", "scale"} & set(node))
        if "camera" in node:
            assert 0 <= node["camera"] < len(doc["cameras"])
        if "mesh" in node:
            assert 0 <= node["mesh"] < len(doc["meshes"])
    quantised = "KHR_mesh_quantization" in doc.get("extensionsUsed", [])
    for mesh in doc.get("meshes", []):
        for primitive in mesh["primitives"]:
            assert "NORMAL" not in primitive["attributes"]
            position, a = values(primitive["attributes"]["POSITION"])
            assert a["type"] == "VEC3" and (a["componentType"] == 5126 or (quantised and a["componentType"] == 5123 and not a.get("normalized", False)))
            assert np.array_equal(np.array(a["min"], position.dtype), position.min(axis=0)) and np.array_equal(np.array(a["max"], position.dtype), position.max(axis=0))
            if a["componentType"] == 5123:
                assert all(isinstance(v, int) for v in a["min"] + a["max"])
            for name in ("TEXCOORD_0", "COLOR_0"):
                if name in primitive["attributes"]:
                    other, b = values(primitive["attributes"][name])
                    assert b["count"] == a["count"]
                    if b["componentType"] != 5126:
                        assert b.get("normalized") is True
            idx, b = values(primitive["indices"])
            assert b["type"] == "SCALAR" and b["componentType"] in (5123, 5125) and b["count"] % 3 == 0 and int(idx.max()) < a["count"]
            assert doc["bufferViews"][b["bufferView"]].get("target", 34963) == 34963
            if "material" in primitive:
                material = doc["materials"][primitive["material"]]
                assert set(material) == {"pbrMetallicRoughness"} and set(material["pbrMetallicRoughness"]) == {"baseColorTexture"}
                image = doc["images"][doc["textures"][material["pbrMetallicRoughness"]["baseColorTexture"]["index"]]["source"]]
                view = doc["bufferViews"][image["bufferView"]]
                assert image["mimeType"] == "image/png" and binary[view["byteOffset"]:view["byteOffset"] + 8] == b"\x89PNG\r\n\x1a\n"
    for camera in doc.get("cameras", []):
        assert camera["type"] == "perspective" and camera["perspective"]["yfov"] > 0 and camera["perspective"]["znear"] > 0
    return doc, binary


def assemble(meshes, names, quantize=False, lut=None, matrix=None, textures=None, camera=None):
    """A whole GLB blob of host meshes by the rules above (one scene, the root "world" with a column-major matrix, the children named ``names``); ``textures``:
    one PNG byte string per mesh with uv."""
    views, total = layout(meshes, quantize)
    binary, bounds = pack(meshes, quantize, lut)
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}], "buffers": [{"byteLength": 0}], "bufferViews": [], "accessors": [], "meshes": [],
           "nodes": [{"name": "world", "matrix": [float(v) for v in np.asarray(np.eye(4) if matrix is None else matrix, np.float64).T.ravel()],
                      "children": list(range(1, len(meshes) + 1))}]}
    if camera is not None:
        (w, h), (fx, fy) = camera["resolution"], camera["focal"]
        doc["cameras"] = [{"type": "perspective", "perspective": {"yfov": 2 * float(np.arctan2(h, 2 * fy)), "aspectRatio": w / h, "znear": 0.01},
                           "extras": {"resolution": [w, h], "focal": [fx, fy]}}]
        doc["nodes"][0]["camera"] = 0
    if quantize:
        doc["extensionsUsed"] = doc["extensionsRequired"] = ["KHR_mesh_quantization"]

    def accessor(view, component, kind, count, target=34962, stride=None, **extra):
        doc["bufferViews"].append({"buffer": 0, "byteOffset": view[0], "byteLength": view[1], "target": target, **({"byteStride": stride} if stride else {})})
        doc["accessors"].append({"bufferView": len(doc["bufferViews"]) - 1, "componentType": component, "type": kind, "count": count, **extra})
        return len(doc["accessors"]) - 1
    textures = list(textures or [])
    for k, (mesh, name, row) in enumerate(zip(meshes, names, views)):
        V, F = len(mesh["vertices"]), len(mesh["faces"])
        lo, hi = bounds[k]
        node = {"name": name, "mesh": k}
        if quantize:
            q, lo, s = quantise_positions(mesh["vertices"])
            node["scale"], node["translation"] = [float(v) for v in s], [float(v) for v in lo]
            attributes = {"POSITION": accessor(row[POSITION], 5123, "VEC3", V, stride=8, min=[int(v) for v in q.min(axis=0)], max=[int(v) for v in q.max(axis=0)])}
        else:
            attributes = {"POSITION": accessor(row[POSITION], 5126, "VEC3", V, min=[float(v) for v in lo.astype(np.float32)], max=[float(v) for v in hi.astype(np.float32)])}
        primitive = {"attributes": attributes, "mode": 4}
        if mesh.get("uv") is not None:
            attributes["TEXCOORD_0"] = accessor(row[TEXCOORD], 5123 if quantize else 5126, "VEC2", V, **({"normalized": True} if quantize else {}))
        if mesh.get("colors") is not None:
            attributes["COLOR_0"] = accessor(row[COLOR], 5121, "VEC4", V, normalized=True)
        primitive["indices"] = accessor(row[INDICES], 5123 if quantize and V <= 65535 else 5125, "SCALAR", 3 * F, target=34963)
        doc["nodes"].append(node)
        doc["meshes"].append({"primitives": [primitive]})
    for k, mesh in enumerate(meshes):
        if mesh.get("uv") is None:
            continue
        png = textures.pop(0)
        for key in ("images", "textures", "materials"):
            doc.setdefault(key, [])
        doc["bufferViews"].append({"buffer": 0, "byteOffset": len(binary), "byteLength": len(png)})
        doc["images"].append({"bufferView": len(doc["bufferViews"]) - 1, "mimeType": "image/png"})
        doc["textures"].append({"source": len(doc["images"]) - 1})
        doc["materials"].append({"pbrMetallicRoughness": {"baseColorTexture": {"index": len(doc["textures"]) - 1}}})
        doc["meshes"][k]["primitives"][0]["material"] = len(doc["materials"]) - 1
        binary += png + b"\0" * (-len(png) % 4)
    doc["buffers"][0]["byteLength"] = len(binary)
    return container(doc, binary), doc, binary
