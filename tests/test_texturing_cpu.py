"""Texturing without a GPU: the rules of include/hive_mi355x.h (above hive_texture_select) through tests/texturing_restatement.py -- the layout's invariants,
closed-form and hand-worked known answers, that a textured render is closer to the frame than the vertex-coloured one -- and the host side of
``hive_amd.texturing`` (refusals, the C layout, the declarations, the pipeline switch when it is off)."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import render_restatement as RR  # noqa: E402
import texturing_cases as C  # noqa: E402
import texturing_restatement as TR  # noqa: E402

NAMES = ("hive_texture_select", "hive_texture_layout", "hive_texture_unweld", "hive_texture_fill")


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("S", [6, 7, 8, 9, 16, 64])
@pytest.mark.parametrize("nf", [1, 2, 3, 7, 8, 9, 50])
def test_layout_owners_corners_and_uv(nf, S):
    from hive_amd import texturing
    Wt, Ht, per_row = TR.layout(nf, S)
    blocks = -(-nf // 2)
    assert per_row == int(np.ceil(np.sqrt(blocks))) and Wt == per_row * S and Ht == -(-blocks // per_row) * S
    assert texturing.atlas_layout(nf, S) == (Wt, Ht, per_row), "the library's host arithmetic"
    cols, rows = np.meshgrid(np.arange(Wt), np.arange(Ht))
    owners = np.vectorize(lambda c, r: TR.owner(c, r, S, per_row))(cols, rows)
    for k in range(blocks):  # every texel of a used block has exactly one owner, one of the block's two faces, and both own some
        block = owners[(k // per_row) * S:(k // per_row + 1) * S, (k % per_row) * S:(k % per_row + 1) * S]
        assert set(np.unique(block)) == {2 * k, 2 * k + 1} and (block == 2 * k).sum() == S * (S + 1) // 2
    mesh = dict(vertices=np.arange(9 * nf, dtype=np.float64).reshape(-1, 3), faces=np.arange(3 * nf).reshape(nf, 3))
    vertices, faces, uv = TR.unweld(mesh, S)
    assert np.array_equal(faces, np.arange(3 * nf).reshape(nf, 3)) and np.array_equal(vertices, mesh["vertices"])
    for f in range(nf):
        for k, (col, row) in enumerate(TR.corners(f, S, per_row)):
            assert owners[row, col] == f, "a corner texel is its face's own"
            u, v = uv[3 * f + k]  # back to the texel under hive_render_shade's nearest-texel rule
            assert int(np.clip(np.floor(u * Wt + 0.5), 0, Wt - 1)) == col and int(np.clip(np.floor((1.0 - v) * Ht + 0.5), 0, Ht - 1)) == row
            b = np.array(TR.barycentrics(col, row, S))
            assert np.array_equal(b, np.eye(3)[k]), "the barycentric map is the identity at the corners"


@pytest.mark.parametrize("S", [6, 8])
def test_a_bilinear_fetch_inside_a_triangle_stays_on_its_owner(S):
    """Exhaustive on a grid of 1/16 texel: the four taps of every point inside (or on) either triangle belong to that triangle's face."""
    grid = np.arange(0, (S - 1) * 16 + 1) / 16.0
    x, y = np.meshgrid(grid, grid)
    tri = {0: (x >= 1) & (y >= 1) & (x + y <= S - 3), 1: (x <= S - 2) & (y <= S - 2) & (x + y >= S + 1)}
    for face, inside in tri.items():
        assert inside.any()
        px, py = x[inside], y[inside]
        for dx in (0, 1):
            for dy in (0, 1):
                tx = np.where((dx == 1) & (px == np.floor(px)), np.floor(px), np.floor(px) + dx).astype(int)  # a tap with weight 0 is not read into the result
                ty = np.where((dy == 1) & (py == np.floor(py)), np.floor(py), np.floor(py) + dy).astype(int)
                assert ((tx >= 0) & (tx < S) & (ty >= 0) & (ty < S)).all(), "never another block's texel"
                assert np.array_equal(np.where(tx + ty <= S - 1, 0, 1), np.full(len(tx), face))


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("S", [6, 7, 9, 13])
def test_every_texel_of_a_quad_equals_the_ramp_in_closed_form(S):
    """S - 5 is a power of two, the quad lies on z = 1 before a camera with fx = fy = 32 and the frame is an integer affine ramp: every sample point is exactly
    representable and bilinear interpolation is exact, so every texel, gutters included, is the ramp at its point after the stated rounding.  The expected
    atlas is worked out here from the rule alone."""
    sx0, sx1, sy0, sy1 = C.QUAD_CORNERS
    out = TR.texture_mesh(C.quad(*C.QUAD_CORNERS), C.ramp_frame()[None], C.K, C.IDENTITY[None], cell=S)
    assert out["texture"].shape == (S, S, 3) and out["views"].tolist() == [0, 0]
    for y in range(S):
        for x in range(S):
            if x + y <= S - 1:
                sx, sy = sx0 + (sx1 - sx0) * (x - 1) / (S - 5), sy0 + (sy1 - sy0) * (y - 1) / (S - 5)
            else:
                sx, sy = sx1 - (sx1 - sx0) * (S - 2 - x) / (S - 5), sy1 - (sy1 - sy0) * (S - 2 - y) / (S - 5)
            assert 0 <= sx <= C.W - 1 and 0 <= sy <= C.H - 1
            want = np.minimum(255, np.floor(C.ramp(sx, sy) + 0.5)).astype(np.uint8)
            assert np.array_equal(out["texture"][y, x], want), (x, y)


@pytest.mark.parametrize("gap, labels", C.TWO_QUAD_LABELS)
def test_selection_two_parallel_quads(gap, labels):
    mesh, poses = C.two_quads(gap)
    for order in (None, [1, 0]):  # the order of the votes does not matter
        best = TR.select(mesh, C.K, poses, C.H, C.W, depth_tolerance=C.TOLERANCE, order=order)
        assert TR.views_of(best).tolist() == labels


def test_selection_ties_masks_near_and_screen():
    mesh = C.quad(*C.QUAD_CORNERS)
    two = np.stack([C.IDENTITY, C.IDENTITY])
    for order in (None, [1, 0]):
        assert TR.views_of(TR.select(mesh, C.K, two, C.H, C.W, order=order)).tolist() == [0, 0], "identical poses: the lower index"
    masks = np.zeros((2, C.H, C.W), np.uint8)
    masks[0, 22, 31] = 7  # the nearest pixel of v00 = (30.5, 22.25): (22, 31); only the even face has that vertex
    assert TR.views_of(TR.select(mesh, C.K, two, C.H, C.W, masks=masks)).tolist() == [1, 0]
    # a vertex behind near, and one whose nearest pixel is column 64 (63.6) against one that stays on column 63 (63.4)
    behind = C.quad(*C.QUAD_CORNERS)
    behind["vertices"][0, 2] = 0.01
    assert TR.views_of(TR.select(behind, C.K, C.IDENTITY[None], C.H, C.W)).tolist() == [-1, 0]
    assert TR.views_of(TR.select(C.quad(60.0, 63.6, 10.0, 14.0), C.K, C.IDENTITY[None], C.H, C.W)).tolist() == [-1, -1]
    assert TR.views_of(TR.select(C.quad(60.0, 63.4, 10.0, 14.0), C.K, C.IDENTITY[None], C.H, C.W)).tolist() == [0, 0]


def test_a_mesh_no_view_sees_takes_its_vertex_colours():
    away = np.diag([-1.0, 1.0, -1.0, 1.0])  # looks the other way
    mesh = C.quad(*C.QUAD_CORNERS, colour=(10, 200, 90))
    out = TR.texture_mesh(mesh, C.ramp_frame()[None], C.K, away[None], cell=8)
    assert out["views"].tolist() == [-1, -1] and (out["texture"] == np.array([10, 200, 90], np.uint8)).all(), "a uniform mesh gives a uniform atlas"
    mesh["vertex_colors"] = np.array([[0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    out = TR.texture_mesh(mesh, C.ramp_frame()[None], C.K, away[None], cell=8)
    for f in range(2):  # the corner texels carry the corner colours; the gutter extrapolates and clamps
        for k, (col, row) in enumerate(TR.corners(f, 8, 1)):
            assert np.array_equal(out["texture"][row, col], mesh["vertex_colors"][mesh["faces"][f][k]])
    one = dict(vertices=mesh["vertices"], faces=mesh["faces"][:1], vertex_colors=mesh["vertex_colors"])
    out = TR.texture_mesh(one, C.ramp_frame()[None], C.K, away[None], cell=8)
    x, y = np.meshgrid(np.arange(8), np.arange(8))
    assert (out["texture"][x + y > 7] == 0).all(), "the missing odd face of the last block is 0"


@pytest.mark.parametrize("name", ["two_quads", "soup_257"])
def test_reversing_the_views_maps_the_labels_and_keeps_the_atlas(name):
    """What tests/test_texturing_gpu.py asks of the kernels on the same cases holds for the rule itself (no two views tie in these cases)."""
    if name == "two_quads":
        mesh, poses = C.two_quads(1.0)
        case = dict(mesh=mesh, frames=C.frames_for(2), poses=poses, masks=None, cell=8)
    else:
        case = C.soup_case(257, 9, 3, True)
    n = len(case["poses"])
    a = TR.texture_mesh(case["mesh"], case["frames"], C.K, case["poses"], masks=case["masks"], cell=case["cell"])
    b = TR.texture_mesh(case["mesh"], case["frames"][::-1], C.K, case["poses"][::-1], masks=None if case["masks"] is None else case["masks"][::-1], cell=case["cell"])
    assert np.array_equal(C.reverse_labels(b["views"], n), a["views"]) and np.array_equal(a["texture"], b["texture"])
    assert (a["views"] >= 0).any() and (a["views"] < 0).any() if name != "two_quads" else True


# ------------------------------------------------------------------------------------------------ it is worth doing
def test_a_textured_render_is_closer_to_the_frame_than_the_vertex_coloured_one():
    """The synthetic room fused into a 32^3 volume by the oracle, textured from frames 0 and 2 at the default cell of 8, rendered by the render restatement.
    Measured here (PSNR in dB over the pixels both renders cover, vertex-coloured -> textured): from frame 1's pose, which took no part, 32.77 -> 32.85; from
    frame 0's pose 33.28 -> 34.69 (at cell 16: 34.27 and 41.17).  The yardstick is the vertex-coloured mesh the export ships without the switch."""
    from hive_amd.render import psnr
    mesh, seq, w2c = C.room()
    textured = TR.texture_mesh(mesh, seq["color"][[0, 2]], seq["K"].astype(np.float64), w2c[[0, 2]], cell=8)
    assert (textured["views"] >= 0).mean() > 0.5
    for view in (1, 0):
        R, t = w2c[view][:3, :3], w2c[view][:3, 3]
        coloured, _, face_a, _ = RR.render([mesh], seq["K"].astype(np.float64), R, t, C.H, C.W)
        picture, _, face_b, _ = RR.render([textured], seq["K"].astype(np.float64), R, t, C.H, C.W)
        both = (face_a >= 0) & (face_b >= 0)
        before, after = psnr(coloured, seq["color"][view], both), psnr(picture, seq["color"][view], both)
        print(f"pose of frame {view}: vertex-coloured {before:.2f} dB, textured {after:.2f} dB over {int(both.sum())} pixels")
        assert both.mean() > 0.8 and after > before


# ------------------------------------------------------------------------------------------------ refusals and plumbing
def test_refusals():
    from hive_amd import texturing
    mesh, frame, poses = C.quad(*C.QUAD_CORNERS), C.ramp_frame()[None], C.IDENTITY[None]
    empty = dict(vertices=np.zeros((0, 3)), faces=np.zeros((0, 3), np.int32), vertex_colors=np.zeros((0, 3), np.uint8))
    bare = dict(vertices=mesh["vertices"], faces=mesh["faces"])
    big = dict(vertices=mesh["vertices"], faces=np.zeros((2 * 256 * 256 + 1, 3), np.int32), vertex_colors=mesh["vertex_colors"])  # 257 blocks of 64 texels a row
    many = np.broadcast_to(frame, (65536, C.H, C.W, 3))
    for what, call in [("an empty mesh", lambda: texturing.texture_mesh(empty, frame, C.K, poses)),
                       ("no frame", lambda: texturing.texture_mesh(mesh, frame[:0], C.K, poses[:0])),
                       ("too many frames", lambda: texturing.texture_mesh(mesh, many, C.K, np.broadcast_to(poses, (65536, 4, 4)))),
                       ("frames of mixed size", lambda: texturing.texture_mesh(mesh, [frame[0], frame[0][:-1]], C.K, np.stack([poses[0]] * 2))),
                       ("cell below the range", lambda: texturing.texture_mesh(mesh, frame, C.K, poses, cell=5)),
                       ("cell above the range", lambda: texturing.texture_mesh(mesh, frame, C.K, poses, cell=65)),
                       ("an atlas over 16384", lambda: texturing.texture_mesh(big, frame, C.K, poses, cell=64)),
                       ("no vertex colours", lambda: texturing.texture_mesh(bare, frame, C.K, poses))]:
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"{what} was not refused")
    assert texturing.atlas_layout(2 * 256 * 256, 64) == (16384, 16384, 256), "the largest atlas is allowed"
    with pytest.raises(ValueError):
        TR.layout(2 * 256 * 256 + 1, 64)


def test_entry_points_are_declared_exported_bound_and_stubbed():
    import ctypes
    from hive_amd import _lib
    header = open(os.path.join(ROOT, "include", "hive_mi355x.h")).read()
    stubs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        declaration = re.search(rf"^int {name}\((.*?)\);", header, flags=re.M | re.S)
        assert declaration, name
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name in stubs, name
        assert len(declaration.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), f"{name}: the header and SIGNATURES disagree on the argument count"
        assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[name][1]
    assert int(re.search(r"#define HIVE_ABI_VERSION (\d+)", header).group(1)) == 9 == _lib.ABI_VERSION == _lib.load().hive_abi_version(), "additions only"
    for word in ("no back-face test", "|A| << 16 | (65535 - view_index)", "x + y <= S - 1", "b0 = (1 - b1) - b2", "top + ay (bottom - top)"):
        assert word in header, word
    assert "texture.o" in open(os.path.join(ROOT, "hive_amd", "csrc", "Makefile")).read()


def test_the_options_and_the_switch_when_it_is_off():
    from hive_amd import gltf
    from hive_amd.mesh import Mesh
    from hive_amd.options import PipelineOptions
    from hive_amd.pipeline import Pipeline
    defaults = PipelineOptions()
    assert (defaults.texture_background, defaults.texture_cell, defaults.texture_max_views) == (False, 8, 32)
    parser = argparse.ArgumentParser()
    PipelineOptions.add_args(parser)
    assert PipelineOptions.from_args(parser.parse_args([])) == defaults
    on = PipelineOptions.from_args(parser.parse_args(["--texture_background", "--texture_cell", "12", "--texture_max_views", "4"]))
    assert (on.texture_background, on.texture_cell, on.texture_max_views) == (True, 12, 4) and on.copy() == on

    class Dataset:
        camera_matrix, frame_width, frame_height, fps, base_path, num_frames = C.K, C.W, C.H, 30.0, "/data/room", 3
    quad = C.quad(*C.QUAD_CORNERS)
    mesh = Mesh(quad["vertices"], quad["faces"], quad["vertex_colors"])
    pipeline = Pipeline(PipelineOptions(num_frames=3))
    scene, lut = pipeline._create_background_scene(Dataset(), mesh)
    assert isinstance(scene, gltf.Scene) and list(scene.geometry) == ["000000"] and scene.geometry["000000"] is mesh
    assert np.array_equal(lut, (255 * np.power(np.arange(256) / 255, 2.2)).astype(np.uint8))
    metadata = pipeline._get_webxr_metadata(Dataset(), 3)
    assert list(metadata) == ["fps", "fov_y", "num_frames", "use_vertex_colour_for_bg", "add_ground_plane", "add_sky_box"] and metadata["use_vertex_colour_for_bg"] is True
    assert Pipeline(PipelineOptions(num_frames=3, texture_background=True))._get_webxr_metadata(Dataset(), 3)["use_vertex_colour_for_bg"] is False


def test_texturing_imports_without_a_gpu():
    from hive_amd import texturing
    assert callable(texturing.texture_mesh) and texturing.MAX_VIEWS == 65535
