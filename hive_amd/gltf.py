"""glTF 2.0 export of the 3-D video: ``Scene`` (what the reference builds with ``trimesh.Scene``, /root/reference/hive/pipeline.py:636-648), ``write_glb`` (where
the reference calls ``trimesh.exchange.export.export_scene``, :921-936, and ``draco_transcoder``, :938-980) and a strict ``read_glb``.

The geometry of a scene is packed on the device into the file's final byte layout by csrc/gltf.hip (``hive_gltf_layout`` / ``hive_gltf_pack``: three launches
per scene, the rules in include/hive_mi355x.h) and comes to the host in ONE copy.  trimesh, pygltflib and draco_transcoder are absent here: the container is
written from the glTF 2.0 specification (and KHR_mesh_quantization in place of draco) and is not pinned against trimesh's exporter, not pinned against three.js.
No NORMAL is written: the viewer and the experiments' renderer are unlit.  Textures are embedded as PNG (the default: a host encoder, the reference's format) or,
with ``texture_format="jpeg"``, as baseline JPEG encoded on the device by csrc/jpeg.hip: every texture of the scene in one call and one download.
"""
import io
import json
import logging
import struct
from collections import OrderedDict

import numpy as np

from hive_amd import _lib
from hive_amd._pictures import is_torch as _is_torch
from hive_amd.mesh import Mesh

GLB_MAGIC, GLB_VERSION, CHUNK_JSON, CHUNK_BIN = 0x46546C67, 2, 0x4E4F534A, 0x004E4942
FLOAT, UNSIGNED_BYTE, UNSIGNED_SHORT, UNSIGNED_INT = 5126, 5121, 5123, 5125
ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 34962, 34963
QUANTIZATION = "KHR_mesh_quantization"
KNOWN_EXTENSIONS = (QUANTIZATION,)
TEXTURE_FORMATS = ("png", "jpeg")
_COMPONENT = {FLOAT: "<f4", UNSIGNED_BYTE: "u1", UNSIGNED_SHORT: "<u2", UNSIGNED_INT: "<u4"}
_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}


class GltfError(ValueError):
    """A .glb that ``read_glb`` refuses."""


def mesh_fields(mesh):
    """(vertices, faces, uv, texture, colours) of a ``mesh.Mesh`` / trimesh (vertex colours) or a ``foreground.process_frame`` dict (uv and an atlas; a dict with
    ``vertex_colors`` is taken as coloured), as they are (numpy arrays or device tensors)."""
    if isinstance(mesh, dict):
        return mesh.get("vertices"), mesh.get("faces"), mesh.get("uv"), mesh.get("texture"), mesh.get("vertex_colors")
    return mesh.vertices, mesh.faces, None, None, getattr(getattr(mesh, "visual", None), "vertex_colors", None)


def _mesh_is_empty(mesh):
    vertices, faces = mesh_fields(mesh)[:2]
    return vertices is None or faces is None or len(vertices) == 0 or len(faces) == 0


class Scene:
    """An ordered map node name -> mesh under one root transform, with the camera of ``_create_empty_scene``.  A mesh is a ``mesh.Mesh`` (vertex colours) or a
    ``process_frame`` dict (uv and an atlas), on the host or on the device; the scene never modifies it."""

    def __init__(self, camera=None):
        """``camera``: ``dict(resolution=(width, height), focal=(fx, fy))`` or None."""
        self.geometry = OrderedDict()
        self.transform = np.eye(4, dtype=np.float64)
        self.camera = None if camera is None else {"resolution": tuple(int(v) for v in camera["resolution"]), "focal": tuple(float(v) for v in camera["focal"])}
        self._packed = {}  # quantize -> (device buffer, names, views, local bounds): valid until the next add_geometry

    def add_geometry(self, mesh, node_name=None):
        name = f"geometry_{len(self.geometry)}" if node_name is None else str(node_name)
        if name in self.geometry:
            raise ValueError(f"the scene already has a node {name!r}")
        self.geometry[name] = mesh
        self._packed = {}
        return name

    @property
    def is_empty(self):
        return all(_mesh_is_empty(m) for m in self.geometry.values())

    def _drawn(self):
        return [(name, m) for name, m in self.geometry.items() if not _mesh_is_empty(m)]

    def _local_bounds(self):
        """(n, 2, 3) float64 bounds of the non-empty meshes in their own frame: numpy for host meshes, the packer's bounds pass when one is on the device."""
        drawn = self._drawn()
        if any(_is_torch(mesh_fields(m)[0]) for _, m in drawn):
            return next(iter(self._packed.values()))[3] if self._packed else _pack(self, False)[3]
        return np.array([[np.asarray(mesh_fields(m)[0], np.float64).min(axis=0), np.asarray(mesh_fields(m)[0], np.float64).max(axis=0)] for _, m in drawn])

    @property
    def bounds(self):
        """(2, 3): min and max over the corners of every mesh's box under the root transform (trimesh's ``Scene.bounds``); None for an empty scene."""
        if self.is_empty:
            return None
        local = self._local_bounds()
        pick = np.array([[(c >> k) & 1 for k in range(3)] for c in range(8)])
        corners = np.stack([local[:, pick[:, k], k] for k in range(3)], axis=-1).reshape(-1, 3)  # (n * 8, 3)
        world = corners @ self.transform[:3, :3].T + self.transform[:3, 3]
        return np.stack([world.min(axis=0), world.max(axis=0)])

    def apply_transform(self, matrix):
        matrix = np.asarray(matrix, dtype=np.float64)
        if matrix.shape != (4, 4):
            raise ValueError(f"a 4 x 4 matrix, got {matrix.shape}")
        self.transform = matrix @ self.transform
        return self

    def copy(self):
        other = Scene(self.camera)
        other.geometry = OrderedDict(self.geometry)
        other.transform = self.transform.copy()
        other._packed = dict(self._packed)  # the meshes are shared and never written to
        return other

    def meshes(self, apply_transform=False):
        """The non-empty meshes in node order; with ``apply_transform`` host copies whose vertices are under the root transform (float64)."""
        out = []
        for _, m in self._drawn():
            if apply_transform:
                vertices, faces, uv, texture, colors = mesh_fields(m)
                v = np.asarray(vertices.cpu() if _is_torch(vertices) else vertices, np.float64) @ self.transform[:3, :3].T + self.transform[:3, 3]
                host = lambda a: a.cpu().numpy() if _is_torch(a) else np.asarray(a)
                m = {"vertices": v, "faces": host(faces), "uv": host(uv), "texture": host(texture)} if colors is None else Mesh(v, host(faces), host(colors))
            out.append(m)
        return out


def _pack(scene, quantize, lut=None, ctx=None):
    """(device uint8 buffer, node names, views (n, 4, 2) int64, bounds (n, 2, 3) float64) of the scene's non-empty meshes: hive_gltf_layout + hive_gltf_pack.  Kept
    on the scene per (quantize, lut)."""
    import torch
    key = (bool(quantize), None if lut is None else bytes(bytearray(lut)))
    if key in scene._packed:
        return scene._packed[key]
    drawn = scene._drawn()
    if not drawn:
        raise ValueError("an empty scene has nothing to pack")
    ctx = ctx or _lib.default_context()
    ctx.follow_torch_stream()
    dev = torch.device("cuda", ctx.device)
    keep, table = [], (_lib.GltfMesh * len(drawn))()

    def on_device(a, dtypes):
        t = a if _is_torch(a) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype not in dtypes:
            t = t.to(dtypes[-1])
        t = t.to(dev).contiguous()
        keep.append(t)
        return t
    for row, (name, m) in zip(table, drawn):
        vertices, faces, uv, texture, colors = mesh_fields(m)
        v, f = on_device(vertices, (torch.float32, torch.float64)), on_device(faces, (torch.int32, torch.int64))
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError(f"node {name!r}: vertices (V, 3) and faces (F, 3), got {tuple(v.shape)} and {tuple(f.shape)}")
        row.vertices, row.faces, row.n_vertices, row.n_faces = v.data_ptr(), f.data_ptr(), v.shape[0], f.shape[0]
        row.vertex_dtype = _lib.GLTF_F64 if v.dtype == torch.float64 else _lib.GLTF_F32
        row.face_dtype = _lib.GLTF_I64 if f.dtype == torch.int64 else _lib.GLTF_I32
        if colors is not None:
            c = on_device(colors, (torch.uint8,))
            if c.dim() != 2 or c.shape[0] != v.shape[0] or c.shape[1] not in (3, 4):
                raise ValueError(f"node {name!r}: vertex colours (V, 3) or (V, 4), got {tuple(c.shape)}")
            row.colors, row.color_channels = c.data_ptr(), c.shape[1]
        elif uv is not None and texture is not None:
            u = on_device(uv, (torch.float64,))
            if tuple(u.shape) != (v.shape[0], 2):
                raise ValueError(f"node {name!r}: uv (V, 2), got {tuple(u.shape)}")
            row.uv = u.data_ptr()
        else:
            raise ValueError(f"node {name!r}: a mesh needs vertex colours, or uv and a texture")
    n = len(drawn)
    views = (_lib.GltfView * (4 * n))()
    total = _lib.c_int64(0)
    lib = ctx.lib
    _lib.check(lib.hive_gltf_layout(table, n, int(bool(quantize)), views, total))
    out = torch.empty(total.value, dtype=torch.uint8, device=dev)
    bounds = np.empty((n, 2, 3), np.float64)
    table_lut = None if lut is None else np.ascontiguousarray(lut, dtype=np.uint8).reshape(256)
    ctx.check(lib.hive_gltf_pack(ctx.handle, table, n, int(bool(quantize)), _lib.ptr(table_lut), out.data_ptr(), total.value, _lib.ptr(bounds)))
    view_array = np.array([[v.offset, v.length] for v in views], np.int64).reshape(n, 4, 2)
    scene._packed[key] = (out, [name for name, _ in drawn], view_array, bounds)
    return scene._packed[key]


def quantisation_step(lo, hi):
    """s of KHR_mesh_quantization as the packer takes it: (hi - lo) / 65535.0 per axis, 1.0 on a flat axis (float64)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return np.where(hi == lo, 1.0, (hi - lo) / 65535.0)


def _png_bytes(texture):
    from PIL import Image
    a = texture.cpu().numpy() if _is_torch(texture) else np.asarray(texture)
    out = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(a[:, :, :3], dtype=np.uint8)).save(out, format="PNG")
    return out.getvalue()


def _pad4(data, fill):
    return data + fill * (-len(data) % 4)


def camera_json(camera):
    """The perspective camera of a ``Scene.camera``: yfov from the vertical focal length, the picture's aspect ratio, znear 0.01 and no zfar (infinite)."""
    (w, h), (fx, fy) = camera["resolution"], camera["focal"]
    return {"type": "perspective", "perspective": {"yfov": float(2.0 * np.arctan2(h, 2.0 * fy)), "aspectRatio": float(w) / float(h), "znear": 0.01},
            "extras": {"resolution": [w, h], "focal": [fx, fy]}}


def write_glb(path, scene, quantize=False, lut=None, ctx=None, timings=None, texture_format="png", jpeg_quality=90, jpeg_subsampling="4:2:0", png_encoder="host"):
    """Write the scene as one binary glTF 2.0 file.  Geometry: layout, pack, ONE device-to-host copy.  Every textured mesh gets its atlas as an embedded PNG with
    one image, texture and material (``baseColorTexture`` only); with ``texture_format="jpeg"`` the atlases are baseline JPEG files (``image/jpeg``) of
    ``jpeg_quality`` and ``jpeg_subsampling``, all encoded on the device in one call (``hive_amd.jpeg.encode``) and downloaded once, and ``timings`` gets a
    ``jpeg`` key in place of ``png``.  ``png_encoder="gpu"`` (with ``texture_format="png"``): the PNG files are compressed on the device too
    (``hive_amd.png.encode``: the same pixels, the device encoder's bytes), all atlases in one call; the default ``"host"`` is Pillow.  One scene; its root node ``"world"`` carries the scene transform as a column-major ``matrix``
    (and the camera), its children are the scene's nodes in order.  Meshes without faces are left out.  ``quantize``: KHR_mesh_quantization (uint16 positions
    under a node scale / translation, uint16 uv, uint16 indices up to 65535 vertices).  ``lut``: 256 bytes applied to the RGB of vertex colours.  Returns the
    byte counts per kind (``geometry``, ``images``, ``json``, ``total``).  ``timings``: a dict that receives the seconds of pack, download, png and file write."""
    import time
    if texture_format not in TEXTURE_FORMATS:
        raise ValueError(f"texture_format {texture_format!r} is not one of {TEXTURE_FORMATS}")
    from hive_amd import png as png_module
    png_module.check_encoder(png_encoder)
    if texture_format == "jpeg":
        from hive_amd import jpeg
        jpeg.check_settings(jpeg_quality, jpeg_subsampling)
    clock = [time.perf_counter()]

    def lap(key):
        now = time.perf_counter()
        if timings is not None:
            timings[key] = timings.get(key, 0.0) + now - clock[0]
        clock[0] = now
    for name, m in scene.geometry.items():
        if _mesh_is_empty(m):
            logging.info(f"glTF export: node {name!r} has no faces and is left out of {path}.")
    drawn = scene._drawn()
    quantize = bool(quantize)
    doc = {"asset": {"version": "2.0", "generator": "hive_amd"}, "scene": 0, "scenes": [{"nodes": [0]}],
           "nodes": [{"name": "world", "matrix": [float(v) for v in scene.transform.T.reshape(-1)]}]}
    if scene.camera is not None:
        doc["cameras"] = [camera_json(scene.camera)]
        doc["nodes"][0]["camera"] = 0
    binary, n_geometry, n_images = b"", 0, 0
    if drawn:
        buffer, names, views, bounds = _pack(scene, quantize, lut, ctx)
        lap("pack")  # (hive_gltf_pack returns after the device has finished)
        binary = buffer.cpu().numpy().tobytes()
        n_geometry = len(binary)
        lap("download")
        doc["nodes"][0]["children"] = list(range(1, len(drawn) + 1))
        doc.update(meshes=[], accessors=[], bufferViews=[])
        if quantize:
            doc["extensionsUsed"] = doc["extensionsRequired"] = [QUANTIZATION]

        def add_view(offset, length, target=None, stride=None):
            view = {"buffer": 0, "byteOffset": int(offset), "byteLength": int(length)}
            if stride:
                view["byteStride"] = stride
            if target:
                view["target"] = target
            doc["bufferViews"].append(view)
            return len(doc["bufferViews"]) - 1

        def add_accessor(view, component, kind, count, **extra):
            doc["accessors"].append({"bufferView": view, "componentType": component, "type": kind, "count": int(count), **extra})
            return len(doc["accessors"]) - 1
        for k, (name, m) in enumerate(drawn):
            vertices, faces, uv, texture, colors = mesh_fields(m)
            V, F = len(vertices), len(faces)
            lo, hi = bounds[k]
            node = {"name": name, "mesh": k}
            if quantize:
                s = quantisation_step(lo, hi)
                node["scale"], node["translation"] = [float(v) for v in s], [float(v) for v in lo]
                top = np.minimum(65535.0, np.rint((hi - lo) / s))
                position = add_accessor(add_view(*views[k, _lib.GLTF_POSITION], ARRAY_BUFFER, 8), UNSIGNED_SHORT, "VEC3", V, min=[0, 0, 0], max=[int(v) for v in top])
            else:
                position = add_accessor(add_view(*views[k, _lib.GLTF_POSITION], ARRAY_BUFFER), FLOAT, "VEC3", V, min=[float(v) for v in lo.astype(np.float32)],
                                        max=[float(v) for v in hi.astype(np.float32)])
            primitive = {"attributes": {"POSITION": position}, "mode": 4}
            if views[k, _lib.GLTF_TEXCOORD, 1]:
                extra = {"normalized": True} if quantize else {}
                primitive["attributes"]["TEXCOORD_0"] = add_accessor(add_view(*views[k, _lib.GLTF_TEXCOORD], ARRAY_BUFFER), UNSIGNED_SHORT if quantize else FLOAT, "VEC2", V,
                                                                     **extra)
            if views[k, _lib.GLTF_COLOR, 1]:
                primitive["attributes"]["COLOR_0"] = add_accessor(add_view(*views[k, _lib.GLTF_COLOR], ARRAY_BUFFER), UNSIGNED_BYTE, "VEC4", V, normalized=True)
            short = quantize and V <= 65535
            primitive["indices"] = add_accessor(add_view(*views[k, _lib.GLTF_INDICES], ELEMENT_ARRAY_BUFFER), UNSIGNED_SHORT if short else UNSIGNED_INT, "SCALAR", 3 * F)
            doc["nodes"].append(node)
            doc["meshes"].append({"primitives": [primitive]})
        lap("json")
        textured = [k for k in range(len(drawn)) if views[k, _lib.GLTF_TEXCOORD, 1]]
        encoded = {}
        if textured and (texture_format == "jpeg" or png_encoder == "gpu"):
            atlases = [mesh_fields(drawn[k][1])[3] for k in textured]
            atlases = [a if a.shape[2] == 3 else a[:, :, :3] for a in atlases]
            files = jpeg.encode(atlases, jpeg_quality, jpeg_subsampling, ctx) if texture_format == "jpeg" else png_module.encode(atlases, ctx)
            encoded = dict(zip(textured, files))
        for k, (name, m) in enumerate(drawn):
            texture = mesh_fields(m)[3]
            if not views[k, _lib.GLTF_TEXCOORD, 1]:
                continue
            png = encoded[k] if k in encoded else _png_bytes(texture)
            for key in ("images", "textures", "materials"):
                doc.setdefault(key, [])
            doc["images"].append({"bufferView": add_view(len(binary), len(png)), "mimeType": "image/" + texture_format})
            doc["textures"].append({"source": len(doc["images"]) - 1})
            doc["materials"].append({"pbrMetallicRoughness": {"baseColorTexture": {"index": len(doc["textures"]) - 1}}})
            doc["meshes"][k]["primitives"][0]["material"] = len(doc["materials"]) - 1
            binary += _pad4(png, b"\0")
            n_images += len(png)
        doc["buffers"] = [{"byteLength": len(binary)}]
        lap(texture_format)
    text = _pad4(json.dumps(doc, separators=(",", ":")).encode("utf-8"), b" ")
    chunks = struct.pack("<II", len(text), CHUNK_JSON) + text
    if binary:
        chunks += struct.pack("<II", len(binary), CHUNK_BIN) + binary
    with open(path, "wb") as f:
        f.write(struct.pack("<III", GLB_MAGIC, GLB_VERSION, 12 + len(chunks)))
        f.write(chunks)
    lap("file")
    return {"geometry": n_geometry, "images": n_images, "json": len(text), "total": 12 + len(chunks)}


def _require(ok, message):
    if not ok:
        raise GltfError(message)


def split_glb(blob):
    """(JSON document, BIN chunk or b"") of a GLB container after checking the magic, the version, the lengths and the 4-byte alignment of every chunk."""
    _require(len(blob) >= 20, f"{len(blob)} bytes: shorter than a GLB header and one chunk header")
    magic, version, length = struct.unpack_from("<III", blob, 0)
    _require(magic == GLB_MAGIC, f"magic {magic:#x} is not 'glTF'")
    _require(version == GLB_VERSION, f"container version {version}, expected 2")
    _require(length == len(blob), f"the header says {length} bytes, the file has {len(blob)}")
    _require(length % 4 == 0, f"the length {length} is not a multiple of 4")
    at, chunks = 12, []
    while at < length:
        _require(at + 8 <= length, f"a chunk header at byte {at} passes the end of the file")
        size, kind = struct.unpack_from("<II", blob, at)
        _require(size % 4 == 0, f"the chunk at byte {at} has {size} bytes: not a multiple of 4")
        _require(at + 8 + size <= length, f"the chunk at byte {at} ({size} bytes) passes the end of the file")
        chunks.append((kind, blob[at + 8:at + 8 + size]))
        at += 8 + size
    _require(chunks and chunks[0][0] == CHUNK_JSON, "the first chunk is not JSON")
    _require(len(chunks) == 1 or chunks[1][0] == CHUNK_BIN, "the second chunk is not BIN")
    _require(not any(kind in (CHUNK_JSON, CHUNK_BIN) for kind, _ in chunks[2:]), "more than one JSON or BIN chunk")
    try:
        doc = json.loads(chunks[0][1].decode("utf-8"))
    except (UnicodeDecodeError, json.JSONDecodeError) as e:
        raise GltfError(f"the JSON chunk does not parse: {e}")
    return doc, (chunks[1][1] if len(chunks) > 1 else b"")


def _accessor_array(doc, binary, index, components, kinds):
    """The (count, width) array of an accessor after checking its type, its view and that its last element ends inside the view and the view inside the buffer."""
    accessors, views = doc.get("accessors", []), doc.get("bufferViews", [])
    _require(isinstance(index, int) and 0 <= index < len(accessors), f"accessor {index} does not exist")
    a = accessors[index]
    _require(a.get("componentType") in components and a.get("type") in kinds, f"accessor {index}: {a.get('type')} of {a.get('componentType')} is not allowed here")
    _require(isinstance(a.get("bufferView"), int) and 0 <= a["bufferView"] < len(views), f"accessor {index} has no buffer view")
    _require("sparse" not in a, f"accessor {index} is sparse")
    view = views[a["bufferView"]]
    dtype, width, count = np.dtype(_COMPONENT[a["componentType"]]), _WIDTH[a["type"]], a.get("count", 0)
    offset, length, start = view.get("byteOffset", 0), view.get("byteLength", 0), a.get("byteOffset", 0)
    element = dtype.itemsize * width
    stride = view.get("byteStride", element)
    _require(view.get("buffer") == 0, f"buffer view {a['bufferView']} is not in buffer 0")
    _require(offset % 4 == 0 and offset >= 0 and length >= 0, f"buffer view {a['bufferView']} starts at byte {offset}: not on a 4-byte boundary")
    _require(offset + length <= len(binary), f"buffer view {a['bufferView']} ends at byte {offset + length}, the buffer has {len(binary)}")
    _require(count >= 1 and start >= 0 and start % dtype.itemsize == 0 and (offset + start) % dtype.itemsize == 0, f"accessor {index}: bad count or offset")
    _require(stride >= element and stride % dtype.itemsize == 0, f"accessor {index}: stride {stride} under the element size {element}")
    _require(start + stride * (count - 1) + element <= length, f"accessor {index} ends at byte {start + stride * (count - 1) + element} of a view of {length}")
    rows = np.lib.stride_tricks.as_strided(np.frombuffer(binary, dtype, width, offset + start), (count, width), (stride, dtype.itemsize))
    return np.array(rows), a


def read_glb(path):
    """Read a .glb of the form ``write_glb`` writes back into a ``Scene`` of numpy meshes, strictly: the magic, the lengths, 4-byte alignment, every accessor
    inside its view and every view inside the buffer, every index inside [0, V), and every required extension known (GltfError otherwise).  Textured meshes
    return as ``process_frame`` dicts (float64 vertices, int64 faces, float64 uv in the atlas's bottom-left convention, the uint8 atlas), coloured ones as
    ``mesh.Mesh`` (RGBA colours); quantised meshes come back through their node's scale and translation.  The root's matrix becomes the scene transform."""
    from PIL import Image
    with open(path, "rb") as f:
        blob = f.read()
    doc, binary = split_glb(blob)
    _require(doc.get("asset", {}).get("version") == "2.0", f"asset version {doc.get('asset', {}).get('version')!r}, expected '2.0'")
    unknown = [e for e in doc.get("extensionsRequired", []) if e not in KNOWN_EXTENSIONS]
    _require(not unknown, f"required extensions {unknown} are not known")
    buffers = doc.get("buffers", [])
    _require(len(buffers) <= 1, f"{len(buffers)} buffers: one binary buffer at most")
    if buffers:
        _require("uri" not in buffers[0], "buffer 0 is external")
        size = buffers[0].get("byteLength", -1)
        _require(0 < size <= len(binary) < size + 4, f"buffer 0 has {size} bytes, the BIN chunk {len(binary)}")
        binary = binary[:size]
    scenes, nodes = doc.get("scenes", []), doc.get("nodes", [])
    _require(len(scenes) == 1 and len(scenes[0].get("nodes", [])) == 1, "one scene with one root node")
    root_index = scenes[0]["nodes"][0]
    _require(isinstance(root_index, int) and 0 <= root_index < len(nodes), "the root node does not exist")
    root = nodes[root_index]
    camera = None
    if "camera" in root:
        cameras = doc.get("cameras", [])
        _require(isinstance(root["camera"], int) and 0 <= root["camera"] < len(cameras), "the root's camera does not exist")
        extras = cameras[root["camera"]].get("extras", {})
        if "resolution" in extras and "focal" in extras:
            camera = {"resolution": extras["resolution"], "focal": extras["focal"]}
    scene = Scene(camera)
    matrix = root.get("matrix", [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0])
    _require(len(matrix) == 16, "the root's matrix has 16 numbers")
    scene.transform = np.array(matrix, np.float64).reshape(4, 4).T.copy()
    quantised = QUANTIZATION in doc.get("extensionsUsed", [])
    for child in root.get("children", []):
        _require(isinstance(child, int) and 0 <= child < len(nodes) and child != root_index, f"child node {child} does not exist")
        node = nodes[child]
        meshes = doc.get("meshes", [])
        _require(isinstance(node.get("mesh"), int) and 0 <= node["mesh"] < len(meshes), f"node {node.get('name')!r} has no mesh")
        primitives = meshes[node["mesh"]].get("primitives", [])
        _require(len(primitives) == 1 and primitives[0].get("mode", 4) == 4, f"node {node.get('name')!r}: one primitive of triangles")
        primitive = primitives[0]
        attributes = primitive.get("attributes", {})
        _require("POSITION" in attributes and "indices" in primitive, f"node {node.get('name')!r}: POSITION and indices")
        q, a = _accessor_array(doc, binary, attributes["POSITION"], (FLOAT, UNSIGNED_SHORT) if quantised else (FLOAT,), ("VEC3",))
        vertices = q.astype(np.float64)
        _require("matrix" not in node and "rotation" not in node, f"node {node.get('name')!r}: only scale and translation")
        if "scale" in node or "translation" in node:
            vertices = vertices * np.array(node.get("scale", [1.0, 1.0, 1.0]), np.float64) + np.array(node.get("translation", [0.0, 0.0, 0.0]), np.float64)
        idx, _ = _accessor_array(doc, binary, primitive["indices"], (UNSIGNED_SHORT, UNSIGNED_INT), ("SCALAR",))
        _require(len(idx) % 3 == 0, f"node {node.get('name')!r}: {len(idx)} indices are not whole triangles")
        _require(int(idx.max()) < len(vertices), f"node {node.get('name')!r}: index {int(idx.max())} outside [0, {len(vertices)})")
        faces = idx.reshape(-1, 3)
        if "COLOR_0" in attributes:
            c, a = _accessor_array(doc, binary, attributes["COLOR_0"], (UNSIGNED_BYTE,), ("VEC4",))
            _require(a.get("normalized") is True and len(c) == len(vertices), f"node {node.get('name')!r}: COLOR_0 is normalised uint8, one per vertex")
            mesh = Mesh(vertices, faces.astype(np.int32), c)
        else:
            _require("TEXCOORD_0" in attributes and "material" in primitive, f"node {node.get('name')!r}: vertex colours, or uv and a material")
            t, a = _accessor_array(doc, binary, attributes["TEXCOORD_0"], (FLOAT, UNSIGNED_SHORT) if quantised else (FLOAT,), ("VEC2",))
            _require(len(t) == len(vertices), f"node {node.get('name')!r}: one TEXCOORD_0 per vertex")
            uv = t.astype(np.float64)
            if a["componentType"] == UNSIGNED_SHORT:
                _require(a.get("normalized") is True, f"node {node.get('name')!r}: uint16 TEXCOORD_0 is normalised")
                uv = uv / 65535.0
            uv[:, 1] = 1.0 - uv[:, 1]  # back to the atlas's bottom-left origin
            try:
                material = doc["materials"][primitive["material"]]
                image = doc["images"][doc["textures"][material["pbrMetallicRoughness"]["baseColorTexture"]["index"]]["source"]]
                view = doc["bufferViews"][image["bufferView"]]
                start, size = view.get("byteOffset", 0), view["byteLength"]
            except (KeyError, IndexError, TypeError) as e:
                raise GltfError(f"node {node.get('name')!r}: the material's base colour texture does not resolve ({e!r})")
            _require(image.get("mimeType") in ("image/png", "image/jpeg") and 0 <= start and start % 4 == 0 and start + size <= len(binary),
                     f"node {node.get('name')!r}: the image is a PNG or a JPEG in a 4-byte aligned view inside the buffer")
            _require(image["mimeType"] == "image/png" or binary[start:start + size][:3] == b"\xFF\xD8\xFF", f"node {node.get('name')!r}: the image/jpeg view does not start FF D8 FF")
            texture = np.array(Image.open(io.BytesIO(binary[start:start + size])).convert("RGB"))
            mesh = {"vertices": vertices, "faces": faces.astype(np.int64), "uv": uv, "texture": texture}
        scene.add_geometry(mesh, node.get("name"))
    return scene
