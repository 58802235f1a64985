"""Label smoothing without a GPU: the rules of include/hive_mi355x.h (above hive_texture_vote) through tests/texture_smoothing_restatement.py -- hand-worked
flips, the energy argument, the fixed point, the fused room's figures, the adjacency against a dict of edges -- and the options."""
import argparse
import collections
import itertools
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import texture_smoothing_cases as SC  # noqa: E402
import texture_smoothing_restatement as SR  # noqa: E402
import texturing_cases as C  # noqa: E402
import texturing_restatement as TR  # noqa: E402

NAMES = ("hive_texture_vote", "hive_mesh_face_neighbours", "hive_texture_smooth")
PAIR = SR.face_neighbours(np.array([[0, 1, 2], [2, 1, 3]]), 4)  # two faces on one edge


def labels_of(best):
    return TR.views_of(best).tolist()


# ------------------------------------------------------------------------------------------------ hand-worked
def test_mix32_is_the_decimations_bijection():
    shared, decimate = (open(os.path.join(ROOT, "hive_amd", "csrc", name)).read() for name in ("hive_internal.hpp", "decimate.hip"))
    definition = "unsigned mix32(unsigned x) {"
    assert definition in shared and "0x7feb352du" in shared and "0x846ca68bu" in shared and definition not in decimate and "mix32(" in decimate, "one definition, shared"
    x = 1
    x ^= x >> 16
    x = (x * 0x7FEB352D) % 2 ** 32
    x ^= x >> 15
    x = (x * 0x846CA68B) % 2 ** 32
    assert SR.mix32(1) == x ^ (x >> 16)
    assert len({SR.mix32(i) for i in range(4096)}) == 4096


def test_two_faces_flip_exactly_when_the_seam_costs_more_than_the_area():
    """Face 0 sees 100 in view 0 and 90 in view 1, face 1 sees 50 and 200: labels (0, 1), one seam.  Moving face 0 to view 1 gains seam_cost - 10, moving face 1
    to view 0 gains seam_cost - 150."""
    area = np.array([[100, 50], [90, 200]], np.int64)
    best, labels, stats = SR.smooth(area, *PAIR, 10)
    assert labels.tolist() == [0, 1] and stats.tolist() == [0, 0, 1, 1, 0], "a gain of 0 is no gain"
    assert best.tolist() == [(100 << 16) | 65535, (200 << 16) | 65534]
    best, labels, stats = SR.smooth(area, *PAIR, 11)
    assert labels.tolist() == [1, 1] and stats.tolist() == [1, 1, 1, 0, 10]
    assert best.tolist() == [(90 << 16) | 65534, (200 << 16) | 65534]
    # both propose (gains 1 and 141): only the larger gain applies, and then the other has nothing left to gain
    trace = []
    _, labels, stats = SR.smooth(area, *PAIR, 151, on_round=trace.append)
    assert [t.tolist() for t in trace] == [[0, 1], [1, 1]] and stats.tolist() == [1, 1, 1, 0, 10]


def test_equal_gains_the_lower_mix32_applies_and_the_other_looks_again():
    """A strip of triangles in which only one adjacent pair (f, g) is labelled -- the first pair whose hash order is the reverse of its index order -- with the
    areas mirrored so that both gain 10 at seam cost 20."""
    faces, nv = SC.grid(16, 1)
    offsets, neighbours = SR.face_neighbours(faces, nv)
    f, g = next((f, int(g)) for f in range(len(faces)) for g in neighbours[offsets[f]:offsets[f + 1]] if g > f and SR.mix32(f) > SR.mix32(int(g)))
    area = np.zeros((2, len(faces)), np.int64)
    area[:, f], area[:, g] = (100, 90), (90, 100)
    trace = []
    _, labels, stats = SR.smooth(area, offsets, neighbours, 20, on_round=trace.append)
    assert trace[0][f] == 0 and trace[0][g] == 1 and len(trace) == 2, "one round: both proposed, one applied, and in the next look neither proposes"
    assert labels[g] == 0 and labels[f] == 0, "g, the later index, has the lower hash and moved to f's view"
    assert stats.tolist() == [1, 1, 1, 0, 10] and (np.delete(labels, [f, g]) == -1).all()
    # with unequal areas the other face would still have had a positive gain in round 0; after g moved it has none: it re-evaluated
    assert SR.proposal(area, trace[0], offsets, neighbours, 20, f) == (10, 1) and SR.proposal(area, labels, offsets, neighbours, 20, f) is None


def test_an_unlabelled_neighbour_costs_nothing():
    faces, nv = SC.grid(2, 1)  # a strip of four faces 0 - 1 - 2 - 3
    offsets, neighbours = SR.face_neighbours(faces, nv)
    assert [neighbours[offsets[f]:offsets[f + 1]].tolist() for f in range(4)] == [[1], [0, 2], [1, 3], [2]]
    area = np.array([[100, 0, 1, 1], [99, 0, 50, 50]], np.int64)  # face 1 has no view; 0 -> view 0; 2, 3 -> view 1
    best, labels, stats = SR.smooth(area, offsets, neighbours, 2 ** 40 - 1)
    assert labels.tolist() == [0, -1, 1, 1] and stats.tolist() == [0, 0, 0, 0, 0] and best[1] == 0, "no seam runs through a face without a view, at any cost"
    area[:, 1] = (0, 7)  # now face 1 can only be textured from view 1: face 0 gives up one unit for the seam
    _, labels, stats = SR.smooth(area, offsets, neighbours, 2)
    assert labels.tolist() == [1, 1, 1, 1] and stats.tolist() == [1, 1, 1, 0, 1]
    area[1, 0] = 0  # ... unless view 1 does not see face 0 at all
    assert SR.smooth(area, offsets, neighbours, 2 ** 40 - 1)[1].tolist() == [0, 1, 1, 1]


# ------------------------------------------------------------------------------------------------ invariants
@pytest.mark.parametrize("seam_cost", SC.SEAM_COSTS)
@pytest.mark.parametrize("family", SC.FAMILIES)
@pytest.mark.parametrize("name", ["8 x 8", "fan of 64"])
def test_the_energy_falls_every_round_and_the_end_is_a_fixed_point(name, family, seam_cost):
    faces, _, n = SC.SMOOTH_MESHES[name]
    offsets, neighbours = SC.adjacency(name)
    area = SC.table(family, n, len(faces))
    trace = []
    best, labels, stats = SR.smooth(area, offsets, neighbours, seam_cost, on_round=trace.append)
    energies = [SR.energy(area, L, offsets, neighbours, seam_cost) for L in trace]
    assert all(b < a for a, b in zip(energies, energies[1:])) and len(trace) == stats[0] + 1
    assert stats[1] == sum(int((a != b).sum()) for a, b in zip(trace, trace[1:])) and (stats[1] >= stats[0])
    assert stats[4] == sum(int(area[a, f]) - int(area[b, f]) for f, (a, b) in enumerate(zip(trace[0], trace[-1])) if a >= 0) >= 0
    if seam_cost == 0:
        assert stats[0] == 0 and np.array_equal(labels, SR.start_labels(area))
    # the fixed point, from the outputs alone: the keys give the labels, and no single face has a move of positive gain
    final = TR.views_of(best)
    assert np.array_equal(final, labels) and np.array_equal(final < 0, area.max(axis=0) == 0)
    for f in range(len(faces)):
        if final[f] < 0:
            continue
        assert int(best[f]) >> 16 == area[final[f], f]
        around = collections.Counter(int(final[g]) for g in neighbours[offsets[f]:offsets[f + 1]])
        for l in around:
            if l >= 0 and l != final[f] and area[l, f] != 0:
                assert int(area[l, f]) - int(area[final[f], f]) + seam_cost * (around[l] - around[final[f]]) <= 0, (f, l)


@pytest.mark.parametrize("nf, cell, n, with_masks", [(257, 9, 3, True), (255, 6, 3, False), (3, 6, 1, False)])
def test_without_a_seam_cost_the_keys_are_selects(nf, cell, n, with_masks):
    case = C.soup_case(nf, cell, n, with_masks)
    want = TR.select(case["mesh"], C.K, case["poses"], C.H, C.W, case["masks"])
    area = SR.vote(SR.signed_areas(case["mesh"], C.K, case["poses"], C.H, C.W, case["masks"]))
    offsets, neighbours = SR.face_neighbours(case["mesh"]["faces"], len(case["mesh"]["vertices"]))
    assert len(neighbours) == 0, "a soup has no shared edge"
    best, labels, stats = SR.smooth(area, offsets, neighbours, 0)
    assert np.array_equal(best, want) and stats.tolist() == [0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the fused room
def test_the_room_has_fewer_seams_and_patches():
    """The tests' fused room, all three frames.  Expected from a separate numpy prototype of the same rule: per-face argmax 176 seam edges in 33 patches; at
    4 px^2 137 seams, 16 patches, 5.9 of 5 102 px^2 given up, 2 rounds and 24 label changes; at 0.25 px^2 142 seams, 16 patches, 1 round.  Of the candidates in
    the three views 7 / 9 / 31 have A > 0 and 881 / 1 090 / 1 163 have A < 0."""
    mesh, seq, w2c = C.room()
    K = seq["K"].astype(np.float64)
    signed = SR.signed_areas(mesh, K, w2c, C.H, C.W)
    print(f"room: {len(mesh['faces'])} faces; candidates with A > 0 per view {(signed > 0).sum(axis=1).tolist()}, with A < 0 {(signed < 0).sum(axis=1).tolist()}")
    assert len(mesh["faces"]) == 2052 and (signed > 0).sum(axis=1).tolist() == [7, 9, 31] and (signed < 0).sum(axis=1).tolist() == [881, 1090, 1163]
    area = SR.vote(signed)
    offsets, neighbours = SR.face_neighbours(mesh["faces"], len(mesh["vertices"]))
    assert len(neighbours) <= 3 * len(mesh["faces"]) and np.diff(offsets).max() <= 3, "manifold, degree <= 3"
    best0, labels0, stats0 = SR.smooth(area, offsets, neighbours, 0)
    assert np.array_equal(best0, TR.select(mesh, K, w2c, C.H, C.W)), "seam_cost 0 is the per-face selection"
    rows = {0.0: (stats0, SR.patches(labels0, offsets, neighbours))}
    for smoothness in (0.25, 4.0):
        _, labels, stats = SR.smooth(area, offsets, neighbours, SR.seam_cost_of(smoothness))
        rows[smoothness] = (stats, SR.patches(labels, offsets, neighbours))
    total = int(area.max(axis=0).sum())
    for smoothness, (stats, count) in rows.items():
        print(f"room at {smoothness} px^2: seam entries {stats[2]} -> {stats[3]}, {count} patches, {stats[0]} rounds, {stats[1]} label changes, "
              f"{stats[4] / SR.UNITS_PER_PX2:.2f} of {total / SR.UNITS_PER_PX2:.0f} px^2 given up")
    assert (rows[0.0][0][3], rows[0.0][1]) == (176, 33) and round(total / SR.UNITS_PER_PX2) == 5102
    assert (rows[4.0][0][3], rows[4.0][1], rows[4.0][0][0], rows[4.0][0][1]) == (137, 16, 2, 24) and round(rows[4.0][0][4] / SR.UNITS_PER_PX2, 1) == 5.9
    assert (rows[0.25][0][3], rows[0.25][1], rows[0.25][0][0]) == (142, 16, 1)
    for smoothness in (0.25, 4.0):
        assert rows[smoothness][0][3] < rows[0.0][0][3] and rows[smoothness][1] < rows[0.0][1], "strictly fewer seam entries and patches than per-face argmax"


# ------------------------------------------------------------------------------------------------ neighbours
def by_edges(faces, nv):
    """The adjacency from a dict of edges: every unordered vertex pair of a valid face -> the faces that have it."""
    faces = np.asarray(faces)
    valid = [f for f, t in enumerate(faces) if all(0 <= v < nv for v in t) and len(set(t.tolist())) == 3]
    of_edge = collections.defaultdict(list)
    for f in valid:
        for a, b in itertools.combinations(sorted(faces[f].tolist()), 2):
            of_edge[(a, b)].append(f)
    lists = [[] for _ in faces]
    for sharing in of_edge.values():
        for f in sharing:
            lists[f] += [g for g in sharing if g != f]
    return [sorted(l) for l in lists]


@pytest.mark.parametrize("name", ["one face", "two faces on an edge", "tetrahedron", "fan of 5", "duplicate faces", "a repeated id and an id out of range", "257 faces"])
def test_neighbours_against_a_dict_of_edges(name):
    faces, nv = SC.NEIGHBOUR_CASES[name]
    offsets, neighbours = SR.face_neighbours(faces, nv)
    got = [neighbours[offsets[f]:offsets[f + 1]].tolist() for f in range(len(faces))]
    assert got == by_edges(faces, nv) and offsets[0] == 0 and offsets[-1] == len(neighbours)
    if name == "tetrahedron":
        assert got == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    if name == "fan of 5":
        assert all(got[f] == [g for g in range(5) if g != f] for f in range(5)), "an edge with m faces gives each of them m - 1 entries"
    if name == "duplicate faces":
        assert got[0] == [1, 1, 1, 2, 2, 2, 3] and got[3] == [0, 1, 2], "duplicates (whatever their winding) list each other three times"
    if name == "a repeated id and an id out of range":
        assert got[1] == got[4] == got[5] == [] and not any(g in (1, 4, 5) for l in got for g in l) and got[0] == [2, 3, 6]


# ------------------------------------------------------------------------------------------------ plumbing
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
    assert int(re.search(r"#define HIVE_ABI_VERSION (\d+)", header).group(1)) == 9 == _lib.ABI_VERSION, "additions only"
    for word in ("front-facing means A < 0", "mix32(f) < mix32(g)", "seam_cost (cnt(l) - cnt(cur))", "LOCAL optimum", "m - 1 entries"):
        assert word in header, word
    assert "texture_smooth.o" in open(os.path.join(ROOT, "hive_amd", "csrc", "Makefile")).read()


def test_refusals_that_need_no_gpu():
    from hive_amd import texturing
    mesh, frame, poses = C.quad(*C.QUAD_CORNERS), C.ramp_frame()[None], C.IDENTITY[None]
    for bad in (-1.0, float("nan"), float("inf"), 2.0 ** 23):
        with pytest.raises(ValueError):
            texturing.texture_mesh(mesh, frame, C.K, poses, smoothness=bad)
    wide = dict(mesh, faces=np.zeros((2 ** 15 + 1, 3), np.int32))  # 65535 x 32769 >= 2^31
    many = np.broadcast_to(frame, (2 ** 16 - 1, C.H, C.W, 3))
    with pytest.raises(ValueError, match="2\\^31"):
        texturing.texture_mesh(wide, many, C.K, np.broadcast_to(poses, (2 ** 16 - 1, 4, 4)), smoothness=1.0, cell=6)
    assert SR.seam_cost_of(4.0) == 524288 and SR.seam_cost_of(2.0 ** -18) == 1 and SR.seam_cost_of(0.0) == 0


def test_the_options():
    from hive_amd.options import PipelineOptions
    defaults = PipelineOptions()
    assert (defaults.texture_smoothness, defaults.texture_cull_back_faces) == (0.0, False)
    parser = argparse.ArgumentParser()
    PipelineOptions.add_args(parser)
    assert PipelineOptions.from_args(parser.parse_args([])) == defaults
    on = PipelineOptions.from_args(parser.parse_args(["--texture_background", "--texture_smoothness", "4", "--texture_cull_back_faces"]))
    assert (on.texture_background, on.texture_smoothness, on.texture_cull_back_faces) == (True, 4.0, True) and isinstance(on.texture_smoothness, float)
    assert on.copy() == on and on != defaults and PipelineOptions(texture_smoothness=4.0) != defaults and PipelineOptions(texture_cull_back_faces=True) != defaults
    assert on.copy().texture_smoothness == 4.0 and on.copy().texture_cull_back_faces is True
