"""The exposure-gain and seam-levelling rules through tests/texture_levelling_restatement.py (no GPU): samples, gains and offsets by hand, the recovery of known
exposure factors on the fused room, what levelling does to the seam texels, the refusals, the options and the plumbing."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import texture_levelling_cases as LC  # noqa: E402
import texture_levelling_restatement as LR  # noqa: E402
import texture_smoothing_restatement as SR  # noqa: E402
import texturing_cases as C  # noqa: E402
import texturing_restatement as TR  # noqa: E402

NAMES = ("hive_texture_samples", "hive_texture_exposure_sums", "hive_texture_level", "hive_texture_fill_adjusted")


# ------------------------------------------------------------------------------------------------ samples
def quad_table(frame):
    quad = C.quad(*C.QUAD_CORNERS)
    area = SR.vote(SR.signed_areas(quad, C.K, C.IDENTITY[None], C.H, C.W))
    return quad, area, LR.samples(quad, frame[None], C.K, C.IDENTITY[None], area)


def test_samples_on_the_ramp_in_closed_form():
    quad, area, table = quad_table(C.ramp_frame())
    assert (area != 0).all() and table.shape == (1, 2, 3) and table.dtype == np.uint16
    # corners (30.5 | 33.5, 22.25 | 25.25) snap to 1/256 pixel exactly; (X + 128) >> 8 rounds halves up: columns 31 | 34, rows 22 | 25
    pixel = {0: (31, 22), 1: (34, 22), 2: (31, 25), 3: (34, 25)}
    for f, tri in enumerate(quad["faces"]):
        want = sum(C.ramp(*pixel[int(v)]) for v in tri)
        assert np.array_equal(table[0, f], want.astype(np.uint16)), (f, table[0, f], want)
        assert 3 <= table[0, f].min() and table[0, f].max() <= 762


@pytest.mark.parametrize("byte, valid", [(0, False), (1, True), (254, True), (255, False)])
def test_a_clipped_vertex_pixel_makes_the_sample_invalid(byte, valid):
    frame = np.full((C.H, C.W, 3), 100, np.uint8)
    frame[22, 31, 1] = byte  # vertex 0's pixel: face 0 holds it, face 1 does not
    _, _, table = quad_table(frame)
    assert np.array_equal(table[0, 0], [300, 200 + byte, 300] if valid else [0, 0, 0]) and np.array_equal(table[0, 1], [300, 300, 300])


# ------------------------------------------------------------------------------------------------ gains
def doubled_pair():
    rng = np.random.default_rng(5)
    a = rng.integers(1, 121, (C.H, C.W, 3), dtype=np.uint8)
    mesh = C.soup(64, 11)
    frames, poses = np.stack([a, 2 * a]), np.stack([C.IDENTITY, C.IDENTITY])
    area = SR.vote(SR.signed_areas(mesh, C.K, poses, C.H, C.W))
    return mesh, frames, poses, area


def test_gains_of_a_frame_and_its_double_in_closed_form():
    from hive_amd import texturing
    mesh, frames, poses, area = doubled_pair()
    table = LR.samples(mesh, frames, C.K, poses, area)
    G, D, N = LR.sums(table)
    assert N[0, 1] == N[1, 0] > 20 and N[0, 0] == N[1, 1] == 0 and np.array_equal(table[1], 2 * table[0])
    assert np.array_equal(G[:, 0, 1], 2 * D[:, 0, 1]) and np.array_equal(D[:, 1, 0], 4 * D[:, 0, 1]) and np.array_equal(G, G.transpose(0, 2, 1))
    for lam in (0.01, 0.5):
        q, fallback, raw = LR.solve(G, D, lam)
        g_a, g_b = (3 + lam) / (2 + lam), (3 + 2 * lam) / (2 * (2 + lam))
        assert fallback == []
        for c in range(3):
            assert abs(raw[c][0] - g_a) <= 1e-12 and abs(raw[c][1] - g_b) <= 1e-12, (lam, raw[c])
        # the renormalisation: weights e_A = D, e_B = 4 D
        scale = 5.0 / (g_a + 4.0 * g_b)
        want = [int(np.clip(np.floor(g * scale * 65536.0 + 0.5), 16384, 262144)) for g in (g_a, g_b)]
        assert (np.abs(q.astype(np.int64) - np.asarray(want)[:, None]) <= 1).all(), (q, want)  # (one Q16 step: the closed form rounds elsewhere than the solve)
        assert abs(q[0, 0] / q[1, 0] - 2.0 * (3 + lam) / (3 + 2 * lam)) < 1e-4
        mine, mine_fallback = texturing.solve_gains(G, D, lam)
        assert mine.dtype == np.uint32 and np.array_equal(mine, q) and mine_fallback == []


def test_without_an_overlap_every_gain_is_one():
    from hive_amd import texturing
    mesh, frames, poses, area = doubled_pair()
    one = LR.sums(LR.samples(mesh, frames[:1], C.K, poses[:1], area[:1]))
    assert all((x == 0).all() for x in one) and (LR.solve(one[0], one[1])[0] == 65536).all()
    apart = area.copy()
    apart[0, ::2], apart[1, 1::2] = 0, 0  # no face has both views
    G, D, N = LR.sums(LR.samples(mesh, frames, C.K, poses, apart))
    assert (N == 0).all() and (G == 0).all() and (D == 0).all()
    for solve in (lambda: LR.solve(G, D)[:2], lambda: texturing.solve_gains(G, D)):
        q, fallback = solve()
        assert (q == 65536).all() and fallback == []


def test_a_solve_that_gives_no_positive_gain_falls_back():
    from hive_amd import texturing
    # G larger than the energies allow (not what sums() can give): the solution of channel 1 is negative
    D = np.zeros((3, 2, 2), np.int64)
    G = np.zeros((3, 2, 2), np.int64)
    D[:, 0, 1], D[:, 1, 0], G[:, 0, 1], G[:, 1, 0] = 100, 100, 90, 90
    G[1, 0, 1] = G[1, 1, 0] = 500
    q, fallback, _ = LR.solve(G, D, 0.01)
    assert fallback == [1] and (q[:, 1] == 65536).all() and (q[:, 0] != 0).all()
    mine, mine_fallback = texturing.solve_gains(G, D, 0.01)
    assert np.array_equal(mine, q) and mine_fallback == [1]


@pytest.mark.parametrize("n_views", [2, 3])
def test_the_room_recovers_the_factors(n_views):
    room = LC.room(n_views)
    out = LC.room_restated(n_views, True, False)
    stats = out["stats"]["exposure"]
    g, t, N = stats["gains"], room["factors"], stats["pair_counts"]
    ratio = g * t / (g[0] * t[0])
    print(f"{n_views} views: gains {g.tolist()}, gain x factor relative to view 0 {ratio.tolist()}, common valid faces {N.tolist()}")
    assert stats["fallback_channels"] == [] and np.abs(ratio - 1.0).max() <= 0.03
    assert (N[~np.eye(n_views, dtype=bool)] > 0).all() and np.array_equal(N, N.T)


def covered_psnr(room, textured):
    """PSNR from frame 1's pose (held out of the two-view case) against the clean frame 1 over the pixels the mesh covers."""
    mesh = dict(vertices=textured["vertices"], faces=textured["faces"], uv=textured["uv"], texture=textured["texture"])
    import render_restatement as RR
    R, t = TR.pose_parts(room["all_poses"][1])
    colour, _, face, _ = RR.render([mesh], room["K"], R, t, C.H, C.W)
    return LR.psnr(colour, room["all_clean"][1], face >= 0), int((face >= 0).sum())


def test_on_the_room_exposure_raises_the_psnr_of_the_held_out_frame():
    room = LC.room(2)
    plain = dict(zip(("vertices", "faces", "uv"), TR.unweld(room["mesh"], 8)))
    best = TR.select(room["mesh"], room["K"], room["poses"], C.H, C.W)
    plain["texture"] = TR.fill(room["mesh"], best, room["frames"], room["K"], room["poses"], 8)
    with_gains = LC.room_restated(2, True, False)
    assert np.array_equal(with_gains["views"], TR.views_of(best)), "smoothness 0, no culling: select's keys"
    (before, pixels), (after, _) = covered_psnr(room, plain), covered_psnr(room, with_gains)
    print(f"pose of frame 1, {pixels} covered pixels: scaled frames {before:.2f} dB, with exposure gains {after:.2f} dB")
    assert pixels > 0.8 * C.H * C.W and after > before


# ------------------------------------------------------------------------------------------------ levelling
def test_two_quads_by_hand():
    case = LC.level_case("two quads")
    half = (np.asarray(LC.COLOUR_B, np.float64) - np.asarray(LC.COLOUR_A, np.float64)) / 2.0
    faces = case["mesh"]["faces"]
    at_rest, stats = LC.levelled("two quads", 0)
    assert stats == dict(seam_vertices=2, sweeps=0, max_offset=10.0)
    for f in range(4):
        for k in range(3):
            seam = int(faces[f, k]) in (1, 4)
            want = (half if f < 2 else -half) if seam else np.zeros(3)
            assert np.array_equal(at_rest[f, k], want), (f, k, at_rest[f, k])
    once, _ = LC.levelled("two quads", 1)
    # vertex 0 (view 0) lies in face (0, 1, 3) alone: the mean of vertices 1 (the seam: +half) and 3 (0)
    assert np.array_equal(once[0, 0], (half + 0.0) / 2.0)
    # vertex 3 (view 0): face (0, 1, 3) gives vertices 0 and 1, face (4, 3, 1) gives vertices 1 and 4: (0 + half + half + half) / 4
    assert np.array_equal(once[0, 2], ((((0.0 + 0.0) + half) + half) + half) / 4.0) and np.array_equal(once[1, 1], once[0, 2])
    # vertex 2 (view 1): faces (1, 2, 4) and (5, 4, 2): vertices 4, 1, then 5, 4: three seam corners at -half, one 0
    assert np.array_equal(once[2, 1], -3.0 * half / 4.0) and np.array_equal(once[3, 2], once[2, 1])
    assert np.array_equal(once[0, 1], half) and np.array_equal(once[2, 0], -half), "a fixed node keeps its offset"


def test_equal_frames_give_no_offsets_and_the_plain_atlas():
    case = LC.level_case("patched grid")
    frames = np.repeat(case["frames"][:1], 3, axis=0)
    poses = np.repeat(case["poses"][:1], 3, axis=0)
    offsets, stats = LR.level(case["mesh"], case["labels"], frames, C.K, poses, None, 8)
    assert stats["seam_vertices"] > 0 and stats["max_offset"] == 0.0 and not offsets.any()
    best = np.array([(1 << 16) | (65535 - int(l)) for l in case["labels"]], np.uint64)
    unit = np.full((3, 3), 65536, np.uint32)
    assert np.array_equal(LR.fill_adjusted(case["mesh"], best, frames, C.K, poses, 8, unit, offsets), TR.fill(case["mesh"], best, frames, C.K, poses, 8))


@pytest.mark.parametrize("name", list(LC.LEVEL_CASES))
def test_offsets_are_one_value_per_node_and_bounded_by_the_seams(name):
    case = LC.level_case(name)
    faces, labels = case["mesh"]["faces"], case["labels"]
    part = LR.participating(faces, labels, len(case["mesh"]["vertices"]), len(case["frames"]))
    fixed, _ = LC.levelled(name, 0)
    for sweeps in LC.SWEEPS:
        offsets, stats = LC.levelled(name, sweeps)
        assert not offsets[~part].any() and stats["sweeps"] == sweeps
        node = {}
        for f in np.flatnonzero(part):
            for k in range(3):
                assert np.array_equal(node.setdefault((int(faces[f, k]), int(labels[f])), offsets[f, k]), offsets[f, k])
        assert np.abs(offsets).max() <= np.abs(fixed).max() + 1e-9, "a mean never leaves the range of the fixed values"
        assert stats["seam_vertices"] == len(LR.seam_nodes(case["mesh"], labels, len(case["frames"])))


def corner_steps(room, textured):
    """Per seam vertex the largest difference, over channels, between the atlas corner texels of its participating faces."""
    labels, S = textured["views"], 8
    _, _, per_row = TR.layout(len(labels), S)
    steps = []
    for v, corners in LR.seam_nodes(room["mesh"], labels, len(room["frames"])).items():
        texels = np.array([textured["texture"][row, col] for f, k in corners for col, row in [TR.corners(f, S, per_row)[k]]], np.int64)
        steps.append(int((texels.max(axis=0) - texels.min(axis=0)).max()))
    return np.asarray(steps)


def test_on_the_room_levelling_closes_the_steps_at_the_seam_vertices():
    room = LC.room(2)
    without, levelled = corner_steps(room, LC.room_restated(2, False, False, 0)), corner_steps(room, LC.room_restated(2, False, True))
    print(f"{len(without)} seam vertices: corner texel step without levelling mean {without.mean():.1f} max {without.max()}, with levelling mean "
          f"{levelled.mean():.2f} max {levelled.max()}")
    assert len(without) == LC.room_restated(2, False, True)["stats"]["levelling"]["seam_vertices"] > 10
    assert levelled.max() <= 1 and without.max() > 20


# ------------------------------------------------------------------------------------------------ plumbing
def test_refusals_that_need_no_gpu():
    from hive_amd import texturing
    mesh, frame, poses = C.quad(*C.QUAD_CORNERS), C.ramp_frame()[None], C.IDENTITY[None]
    for bad in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="exposure_prior"):
            texturing.texture_mesh(mesh, frame, C.K, poses, exposure=True, exposure_prior=bad)
        with pytest.raises(ValueError):
            LR.texture_mesh(mesh, frame, C.K, poses, exposure=True, exposure_prior=bad)
    for bad in (-1, 4097):
        with pytest.raises(ValueError, match="levelling_sweeps"):
            texturing.texture_mesh(mesh, frame, C.K, poses, levelling=True, levelling_sweeps=bad)
        with pytest.raises(ValueError):
            LR.texture_mesh(mesh, frame, C.K, poses, levelling=True, levelling_sweeps=bad)
    many = np.broadcast_to(frame, (257, C.H, C.W, 3))
    with pytest.raises(ValueError, match="256"):
        texturing.texture_mesh(mesh, many, C.K, np.broadcast_to(poses, (257, 4, 4)), exposure=True)
    with pytest.raises(ValueError):
        texturing.solve_gains(np.zeros((3, 2, 2), np.int64), np.zeros((3, 2, 3), np.int64))


def test_entry_points_are_declared_exported_and_bound():
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
    assert "texture_level.o" in open(os.path.join(ROOT, "hive_amd", "csrc", "Makefile")).read()


def test_the_options_and_the_record_with_the_switches_off():
    from hive_amd.options import PipelineOptions
    from hive_amd.pipeline import Pipeline
    defaults = PipelineOptions()
    assert (defaults.texture_exposure, defaults.texture_levelling, defaults.texture_levelling_sweeps) == (False, False, 64)
    parser = argparse.ArgumentParser()
    PipelineOptions.add_args(parser)
    assert PipelineOptions.from_args(parser.parse_args([])) == defaults
    on = PipelineOptions.from_args(parser.parse_args(["--texture_background", "--texture_exposure", "--texture_levelling", "--texture_levelling_sweeps", "8"]))
    assert (on.texture_exposure, on.texture_levelling, on.texture_levelling_sweeps) == (True, True, 8) and on.copy() == on and on != defaults
    five = dict(rounds=0, label_changes=0, seam_entries_before=3, seam_entries_after=3, area_given_up_px2=0.0)
    counts = {"key_frames", "faces", "faces_with_a_view", "atlas"}
    assert set(Pipeline._texturing_record([0, 2], 10, 8, (16, 24, 3), None, False)) == counts, "every switch off: no new key"
    assert set(Pipeline._texturing_record([0, 2], 10, 8, (16, 24, 3), five, True)) == counts | {"smoothing"}
    stats = dict(five, exposure=dict(gains=np.ones((2, 3)), pair_counts=np.zeros((2, 2), np.int64), fallback_channels=[]),
                 levelling=dict(seam_vertices=4, sweeps=64, max_offset=1.5))
    record = Pipeline._texturing_record([0, 2], 10, 8, (16, 24, 3), stats, False)
    assert set(record) == counts | {"exposure", "levelling"} and record["atlas"] == [24, 16] and record["exposure"]["gains"] == [[1.0] * 3] * 2
    import json
    json.dumps(record)
