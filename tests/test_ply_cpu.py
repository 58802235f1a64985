"""write_ply's optional texture form (vertex uv + TextureFile comment) and its unchanged default output."""
import numpy as np


def _legacy_bytes(vertices, faces, colors, normals):
    """The file write_ply wrote before the texture keywords existed, restated."""
    v = np.empty(len(vertices), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                       ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    v["x"], v["y"], v["z"] = np.asarray(vertices, np.float32).T
    v["nx"], v["ny"], v["nz"] = np.asarray(normals, np.float32).T
    v["red"], v["green"], v["blue"] = colors.T
    f = np.empty(len(faces), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    f["n"], f["i"] = 3, faces
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z",
              "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green", "property uchar blue",
              f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(header) + "\n").encode() + v.tobytes() + f.tobytes()


def test_write_ply_default_output_unchanged(tmp_path):
    from hive_amd.pipeline import write_ply
    rng = np.random.default_rng(0)
    verts, normals = rng.random((7, 3)), rng.random((7, 3))
    colors = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    faces = rng.integers(0, 7, (5, 3)).astype(np.int32)
    write_ply(str(tmp_path / "a.ply"), verts, faces, colors, normals)
    assert (tmp_path / "a.ply").read_bytes() == _legacy_bytes(verts, faces, colors, normals)


def test_write_ply_texture_coordinates_and_texture_file(tmp_path):
    from hive_amd.pipeline import write_ply
    rng = np.random.default_rng(1)
    verts, uv = rng.random((6, 3)), rng.random((6, 2))
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    write_ply(str(tmp_path / "t.ply"), verts, faces, vertex_uv=uv, texture_file="000004.png")
    data = (tmp_path / "t.ply").read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode().splitlines()
    assert header[:3] == ["ply", "format binary_little_endian 1.0", "comment TextureFile 000004.png"]
    assert header[3:9] == ["element vertex 6", "property float x", "property float y", "property float z", "property float texture_u",
                           "property float texture_v"]
    v = np.frombuffer(data, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("u", "<f4"), ("v", "<f4")], count=6, offset=end)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), verts.astype(np.float32))
    assert np.array_equal(np.stack([v["u"], v["v"]], 1), uv.astype(np.float32))
    f = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=2, offset=end + v.nbytes)
    assert np.array_equal(f["i"], faces) and (f["n"] == 3).all() and end + v.nbytes + f.nbytes == len(data)
