"""Premises of tests/test_tsdf_sweep_gpu.py, checked with the C oracle and numpy only: the scenes of tsdf_sweep_cases.py form the
groups, reach the row decompositions and camera positions, and produce the updates that the GPU tests rely on -- so that none of them
passes vacuously.  Runs anywhere."""
import numpy as np
import pytest

import tsdf_sweep_cases as cases


@pytest.mark.parametrize("cfg", cases.CONFIGS + [cases.WIDE], ids=lambda c: c["name"])
def test_random_pose_scene_premises(oracle_lib, cfg):
    s = cases.random_pose_scene(cfg)
    assert cases.dims_of(s["bounds"], s["voxel"]) == cfg["dims"]
    X, Y, Z = cfg["dims"]
    H, W = cfg["image"]
    assert H * W <= 4400 and X * Y * Z <= 342_000
    if cfg["name"] == "v030":
        assert (X * Y) % 4 == 2 and W % 4 != 0
    if cfg["name"] == "v041":
        assert Z < 64 and Z % 2 == 1 and W % 4 != 0
    if cfg["name"] == "v050":
        assert W % 4 == 0
    side = cases.longest_side(s["bounds"], s["voxel"])
    groups = cases.predict_groups(s["poses"], side)
    assert groups == s["lengths"], "the greedy rule must find the groups the generator laid out"
    assert sum(groups) == len(s["poses"]) and 24 <= len(s["poses"]) <= 27
    assert set(groups) == {1, 2, 3, 4}
    assert any(groups[i] == 1 and groups[i - 1] > 1 and groups[i + 1] > 1 for i in range(1, len(groups) - 1)), "no single frame between two fused groups"
    assert any(g == 3 for g in groups[:-1]), "no group of three followed by more frames"
    # every decision has margin: a rounding difference between this restatement and the host cannot flip one
    dec = cases.decisions(s["poses"], side)
    assert any(ok for *_, ok in dec) and any(not ok for *_, ok in dec)
    for first, other, angle, dist, ok in dec:
        assert not (30.0 <= angle <= 45.0) and not (0.2 <= dist <= 0.3), (first, other, angle, dist)
        assert ok == (angle < 30.0 and dist < 0.2)
    starts = cases.group_starts(groups)
    fused_first = [s["poses"][st] for st, g in zip(starts, groups) if g > 1]
    along_y = sum(bool(cases.lanes_along_y(p)) for p in fused_first)
    assert along_y >= 2 and along_y < len(fused_first), "both row decompositions of the work-list kernel must be reached"
    b = s["bounds"]
    inside = [bool(np.all((p[:3, 3] > b[:, 0]) & (p[:3, 3] < b[:, 1]))) for p in s["poses"]]
    assert any(inside) and not all(inside)
    for kind in ("noise", "patchy"):
        r = cases.oracle_run(oracle_lib, s, kind)
        assert r["dims"] == cfg["dims"]
        n = r["n_updated"]
        zs = s["zero_frame"]
        st = max(t for t in starts if t <= zs)
        g = groups[starts.index(st)]
        assert g == 4 and n[zs] == 0 and max(n[st:st + g]) > 0, "a frame without updates inside a group whose other frames update"
        share = float((r["passes"][-1][2] > 0).mean())
        # noise: depths to 4 m reach through the whole volume; patchy: the near tiles (<= 0.8 m + truncation) reach a thin shell only
        assert share >= (0.1 if kind == "noise" else 0.01), (kind, share)
    assert min(cases.oracle_run(oracle_lib, s, "noise")["n_updated"]) == 0


def test_the_small_images_have_a_tile_table_the_row_cut_cannot_use():
    """Why the WIDE configuration exists: with at most 2 x 2 tiles of 32 pixels the 3 x 3 dilation makes every entry the frame's maximum."""
    for cfg in cases.CONFIGS:
        H, W = cfg["image"]
        assert (H + 31) // 32 <= 2 and (W + 31) // 32 <= 2
    H, W = cases.WIDE["image"]
    assert (W + 31) // 32 == 5
    d = cases.random_pose_scene(cases.WIDE)["depth"]["patchy"]
    live = [i for i in range(len(d)) if d[i].any()]
    assert all(d[i][:, :64].max() <= 0.8 and d[i][:, 64:128].max() == 0.0 and d[i][:, 128:].max() == 4.0 for i in live)
    assert any(0.0 < d[i][:, :64].max() for i in live)


def test_chunk_straddle_premises(oracle_lib):
    s = cases.chunk_straddle_scene()
    assert cases.dims_of(s["bounds"], s["voxel"]) == (32, 32, 32)
    side = cases.longest_side(s["bounds"], s["voxel"])
    groups = cases.predict_groups(s["poses"], side)
    assert groups == [3] + [4] * 33 == s["lengths"] and len(s["poses"]) == 135
    starts = cases.group_starts(groups)
    assert 127 in starts and 127 + 4 > 128, "a group must begin before frame 128 and end after it"
    angle, dist = cases.fuse_measures(s["poses"][0], s["poses"][3], side)
    assert angle >= 50.0 or dist >= 0.4
    for first, other, angle, dist, ok in cases.decisions(s["poses"], side):
        assert not (30.0 <= angle <= 45.0) and not (0.2 <= dist <= 0.3)
    r = cases.oracle_run(oracle_lib, s, "noise")
    n = r["n_updated"]
    assert min(n[124:135]) > 1000, "the frames on both sides of the chunk boundary update the volume"
    assert float((r["passes"][-1][2] > 0).mean()) >= 0.1
    # frames differ, so that a sweep handed the wrong frame of the re-prepared chunk cannot give the same volume
    assert len({s["depth"]["noise"][i].tobytes() for i in range(120, 135)}) == 15


@pytest.mark.parametrize("kind,beyond_expected", [("nan", True), ("inf", True), ("neg", False), ("negzero", False)])
def test_special_depth_premises(oracle_lib, kind, beyond_expected):
    """What the contract does with a non-finite or negative depth, on the oracle alone: NaN and +inf update voxels far beyond the plane's
    far cut (0.5 m + truncation + a voxel); -0.05 and -0.0 do not."""
    s = cases.special_depth_scene(kind)
    assert cases.dims_of(s["bounds"], s["voxel"]) == (42, 36, 48)
    side = cases.longest_side(s["bounds"], s["voxel"])
    assert cases.predict_groups(s["poses"][:2], side) == [2] and cases.predict_groups(s["poses"], side) == [4]
    r = cases.oracle_run(oracle_lib, s, "plane", frames=[0])
    weight = r["passes"][0][2]
    cam_z = cases.camera_depth_of_voxels(s, s["poses"][0])
    beyond = int(np.count_nonzero((weight > 0) & (cam_z > cases.SPECIAL_PLANE + 5 * s["voxel"] + s["voxel"])))
    assert r["n_updated"][0] == int(np.count_nonzero(weight)) > 1000
    assert (beyond > 0) == beyond_expected, beyond
    if kind in ("nan", "inf"):
        assert beyond > 100
        far = (weight > 0) & (cam_z > 1.0)
        assert np.all(r["passes"][0][0][far] == 1.0), "dist = fminf(1, NaN or inf) = 1"


def test_special_depth_blocks_do_not_overlap():
    s = cases.special_depth_scene("all")
    d = s["depth"]["plane"][0]
    assert np.isnan(d).sum() == 16 and np.isposinf(d).sum() == 16 and (d == np.float32(-0.05)).sum() == 16
    assert (np.signbit(d) & (d == 0)).sum() == 16 and (d == cases.SPECIAL_PLANE).sum() == 48 * 64 - 64


def test_far_offset_scene_needs_the_clip_widening(oracle_lib):
    """The volume at z = 131072 m: by the float32 restatement of the row clip (cases.clip_rows), the oracle updates voxels that lie outside
    their row's analytic interval unless it is widened by 2 / 3 voxels -- in most frames -- and none outside the widened interval.  The
    scenes near the origin have none either way: they cannot tell whether the widening is there."""
    s = cases.far_offset_scene()
    assert cases.dims_of(s["bounds"], s["voxel"]) == (40, 36, 48)
    side = cases.longest_side(s["bounds"], s["voxel"])
    assert cases.predict_groups(s["poses"], side) == [4, 4, 4] == s["lengths"]
    for first, other, angle, dist, ok in cases.decisions(s["poses"], side):
        assert not (30.0 <= angle <= 45.0) and not (0.2 <= dist <= 0.3)
    n = len(s["poses"])
    narrow = [cases.updates_outside_clip(oracle_lib, s, "noise", i, widen=False) for i in range(n)]
    wide = [cases.updates_outside_clip(oracle_lib, s, "noise", i, widen=True) for i in range(n)]
    assert min(u for _, u in narrow) > 1000, "every frame updates the volume"
    assert sum(e > 0 for e, _ in narrow) >= 8 and sum(e for e, _ in narrow) >= 20, narrow
    assert all(e == 0 for e, _ in wide), wide
    near = cases.random_pose_scene(cases.CONFIGS[1])
    assert all(cases.updates_outside_clip(oracle_lib, near, "noise", i, widen=False)[0] == 0 for i in range(len(near["poses"])))


def test_degenerate_volume_premises(oracle_lib):
    s = cases.degenerate_scene()
    assert cases.dims_of(s["bounds"], s["voxel"]) == (5, 3, 3)
    side = cases.longest_side(s["bounds"], s["voxel"])
    assert cases.predict_groups(s["poses"], side) == [4] and cases.predict_groups(s["poses"][:3], side) == [3]
    r = cases.oracle_run(oracle_lib, s, "noise")
    assert min(r["n_updated"]) >= 30 and float((r["passes"][-1][2] > 0).mean()) == 1.0
