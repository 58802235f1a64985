"""Known answers of the rasteriser's rules on the numpy restatement (tests/render_restatement.py) -- no GPU.  What the restatement gets right here, the kernels
must reproduce bit for bit (test_render_gpu.py)."""
import numpy as np
import pytest

import render_cases as C
import render_restatement as RR


def _render(meshes, K, pose, H, W, **kw):
    return RR.render(meshes, K, pose[:3, :3], pose[:3, 3], H, W, **kw)


@pytest.mark.parametrize("pose", [C.IDENTITY, C.general_pose()], ids=["identity", "general"])
def test_grid_round_trip(pose):
    """A 24 x 32 grid mesh from a random depth image, rendered from its own pose: exactly the block [0:H-1, 0:W-1] = 713 pixels, each once; the image's depth
    bits; the image's colours through the texture and through vertex colours.  The same after moving world and camera by a general rigid transform."""
    H, W = 24, 32
    s = C.grid_scene(H, W, pose=pose)
    assert np.array_equal(s["K"][:2], [[58, 0, 15.5], [0, 58, 11.5]])
    for name in ("textured", "coloured"):
        color, depth, face, cover = _render([s[name]], s["K"], pose, H, W)
        block = np.zeros((H, W), bool)
        block[:H - 1, :W - 1] = True
        assert np.array_equal(cover, block.astype(np.int32)) and cover.sum() == 713
        assert np.array_equal(face >= 0, block)
        assert np.array_equal(depth[block].view(np.uint32), s["depth"][block].view(np.uint32))
        assert np.array_equal(color[block], s["image"][block])
        assert (color[~block] == 255).all() and (depth[~block] == 0).all()


def test_screen_filling_quad_and_winding():
    H, W = 48, 64
    K, quad = C.quad_scene(H, W)
    color, depth, face, cover = _render([quad], K, C.IDENTITY, H, W)
    assert (cover == 1).all()
    assert (depth.view(np.uint32) == np.float32(2.0).view(np.uint32)).all()
    assert set(np.unique(face)) == {0, 1}
    flipped = dict(quad, faces=quad["faces"][:, ::-1])
    color2, depth2, face2, cover2 = _render([flipped], K, C.IDENTITY, H, W)
    assert np.array_equal(cover, cover2) and np.array_equal(depth.view(np.uint32), depth2.view(np.uint32))
    assert np.array_equal(face, face2) and np.array_equal(color, color2)


def test_fan_covers_no_pixel_twice():
    H, W = 48, 64
    K, fan = C.fan_scene(H, W)
    _, _, face, cover = _render([fan], K, C.IDENTITY, H, W)
    assert cover.max() == 1 and cover.sum() > 200
    assert len(np.unique(face[face >= 0])) > 8  # (a thin spoke may hold no sample)


def test_ties_go_to_the_smaller_face_index():
    H, W = 48, 64
    K, tie = C.tie_scene(H, W)
    _, _, face, cover = _render([tie], K, C.IDENTITY, H, W)
    assert cover.max() == 3 and set(np.unique(face)) == {-1, 0}
    # the same triangle in two meshes: the global index decides
    one = dict(tie, faces=tie["faces"][:1])
    _, _, face, _ = _render([one, one], K, C.IDENTITY, H, W)
    assert set(np.unique(face)) == {-1, 0}


def test_rejection_rules():
    """near (no clipping), the guard band and zero area discard the whole face."""
    H, W = 48, 64
    K = C.intrinsics(H, W)
    tri = lambda z: C.unproject(K, [5.0, 40.0, 5.0], [5.0, 5.0, 40.0], z)
    faces = [[0, 1, 2]]
    covered = lambda v, f=faces, **kw: int(_render([C.coloured(v, f)], K, C.IDENTITY, H, W, **kw)[3].sum())
    assert covered(tri(2.0)) > 0
    assert covered(tri([2.0, 2.0, 0.04])) == 0 and covered(tri([2.0, 2.0, 0.05])) > 0  # !(z >= near)
    assert covered(tri(-2.0)) == 0
    assert covered(tri(2.0), near=2.5) == 0
    assert covered(C.unproject(K, [5.0, 65536.0, 5.0], [5.0, 5.0, 40.0], 2.0)) == 0  # the guard band
    assert covered(C.unproject(K, [5.0, 65535.0, 5.0], [5.0, 5.0, 40.0], 2.0)) > 0
    assert covered(tri(2.0), [[0, 1, 1]]) == 0 and covered(C.unproject(K, [5.0, 10.0, 15.0], [5.0, 10.0, 15.0], 2.0)) == 0  # zero area


def test_new_entry_points_are_declared():
    from hive_amd import _lib
    for name in ("hive_render_clear", "hive_render_draw", "hive_render_shade", "hive_render_resolve"):
        assert name in _lib.SIGNATURES


def test_psnr():
    from hive_amd.render import psnr
    a = np.zeros((4, 4, 3), np.uint8)
    b = a.copy()
    assert psnr(a, b) == float("inf")
    b[0, 0] = 255
    assert psnr(a, b) == pytest.approx(10 * np.log10(16.0))
    mask = np.zeros((4, 4), bool)
    mask[0, 0] = True
    assert psnr(a, b, mask) == 0.0
    with pytest.raises(ValueError):
        psnr(a, b[:2])


def test_arguments_are_checked_before_any_device_work():
    from hive_amd.render import render_mesh
    K = C.intrinsics(4, 4)
    with pytest.raises(ValueError):
        render_mesh(K, C.IDENTITY, size=(4, 4), near=0.0)
    with pytest.raises(ValueError):
        render_mesh(K, C.IDENTITY, size=(0, 4))
    with pytest.raises(ValueError):
        render_mesh(K, C.IDENTITY)
