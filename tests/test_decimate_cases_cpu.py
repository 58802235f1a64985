"""The premises of tests/test_decimate_edges_gpu.py, checked with the restatement alone (tests/decimate_restatement.py): every case of
tests/decimate_cases.py is what its name says -- which rule rejects, on which side of the face cap a spindle lies, the signs and bands of the costs, the
classes of face area, where a wide round is cut, how many rounds a budget takes -- so that a case cannot quietly stop reaching the kernel path it is
there for.  No GPU."""
import numpy as np
import pytest

import decimate_cases as C
import decimate_restatement as D


def first_round(name, max_error=1e9):
    """[(v0, v1, cost)] of every legal halfedge collapse of a case's input mesh, and the census of the rules that reject the others."""
    verts, faces = C.case(name)
    f = np.asarray(faces, np.int64)
    m = D._Mesh(f, np.ones(len(f), bool))
    q = D.vertex_quadrics(verts, f)
    locked = D.locked_vertices(len(verts), f)
    legal, census = [], {}
    for v0 in m.vf:
        for v1 in m.nbrs(v0):
            rule, cost, _ = D.collapse_check(m, q, verts, locked, v0, v1, max_error)
            census[rule] = census.get(rule, 0) + 1
            if rule is None:
                legal.append((v0, v1, cost))
    return legal, census


@pytest.mark.parametrize("name,budget,max_error", C.runs())
def test_invariants(name, budget, max_error):
    verts, faces = C.case(name)
    budget = C.budget_of(name, budget)
    out, kept, (rounds, collapses, locked), _ = C.restated(name, budget, max_error)
    chi, loops, _ = D.euler_and_loops(len(verts), faces)
    assert D.euler_and_loops(len(kept), out)[:2] == (chi, loops)
    assert np.all((out[:, 0] != out[:, 1]) & (out[:, 1] != out[:, 2]) & (out[:, 0] != out[:, 2])), "degenerate face"
    if name != "pillow":  # (the input itself is two faces on one vertex triple)
        assert len(np.unique(np.sort(out, axis=1), axis=0)) == len(out), "duplicate face"
    assert np.all(np.diff(kept) > 0) and (len(kept) == 0 or (kept.min() >= 0 and kept.max() < len(verts)))
    assert len(kept) == len(verts) - collapses
    print(f"{name} budget {budget} max_error {max_error}: {len(faces)} -> {len(out)} faces, (rounds, collapses, locked) = {(rounds, collapses, locked)}")


@pytest.fixture(scope="module")
def censuses():
    """name -> rule_census at budget 1 for max_error 1e9 and 1e-6, summed (every case but the wide lattice, whose rounds take minutes to restate)."""
    out = {}
    for name in C.CASES:
        if name == "wide_lattice":
            continue
        total = {}
        for max_error in (1e9, 1e-6):
            for rule, n in C.rule_census(*C.case(name), 1, max_error).items():
                total[rule] = total.get(rule, 0) + n
        out[name] = total
    return out


def test_rule_union(censuses):
    """Every rule of collapse_check but `edge faces` (unreachable: see its docstring) is the first to reject somewhere in the new cases."""
    seen = set().union(*censuses.values())
    assert seen - {None} <= set(C.RULES)
    for rule in ("locked", "v0 faces < 2", "fan cap", "vl == vr", "boundary", "link", "side edges", "valence 3", "max_error"):
        assert rule in seen, rule
    assert "edge faces" not in seen
    assert None in seen
    print("rule census, budget 1, max_error 1e9 + 1e-6:", {name: c for name, c in censuses.items()})


def test_rules_per_case(censuses):
    assert set(censuses["pillow"]) == {"vl == vr"}
    assert set(censuses["tetrahedron"]) == {"valence 3"}
    assert set(censuses["torus_3x3"]) == {"link"}
    assert "side edges" in censuses["flag"]
    for name in ("tetrahedron", "pillow", "torus_3x3"):
        for max_error in (1e9, 1e-6):
            assert C.restated(name, 1, max_error)[2] == (0, 0, 0)


def test_census_agrees_with_the_final_mesh_census():
    """rule_census's last round is decimate's own census of the mesh where the rounds ended; a run of one round adds the first round to it."""
    verts, faces = C.case("book_3")
    last = {}
    D.decimate(verts, faces, 1, 1e9, census=last)
    total = C.rule_census(verts, faces, 1, 1e9)
    assert last and all(total[rule] >= n for rule, n in last.items()) and sum(total.values()) > sum(last.values())
    one = C.rule_census(verts, faces, len(faces) - 1, 1e9)  # one round, ended by the budget: only the input mesh is judged
    assert one == first_round("book_3")[1]


def test_book_spine_is_locked_and_survives():
    n = C.BOOK_PAGE
    verts, faces = C.case("book_3")
    assert np.array_equal(np.nonzero(D.locked_vertices(len(verts), faces))[0], np.arange(n))
    assert D.euler_and_loops(len(verts), faces)[2] == 3
    out, kept, stats, trace = C.restated("book_3", 1, 1e9)
    assert stats[2] == n and set(range(n)) <= set(kept.tolist()) and len(out) > 1
    assert not set(range(n)) & {v for _, applied, _ in trace for pair in applied for v in pair}
    verts2, faces2 = C.case("book_2")  # two pages: an ordinary sheet, nothing locked
    assert not D.locked_vertices(len(verts2), faces2).any()


@pytest.mark.parametrize("k", [23, 24, 25, 40])
def test_spindle_apexes_and_the_face_cap(k):
    """faces(v0) + faces(v1) - 2 > 24 keeps an apex out of every collapse until it has at most 22 faces (a ring vertex has 4); with 25 or more faces
    `gather` gives up on the apex itself."""
    verts, faces = C.case(f"spindle_{k}")
    assert C.face_counts(faces, len(verts))[[k, k + 1]].tolist() == [k, k]
    assert D.euler_and_loops(len(verts), faces) == (2, 0, 2)
    for max_error in (1e9, 1e-6):
        trace = C.restated(f"spindle_{k}", 1, max_error)[3]
        assert trace
        for _, applied, live in trace:
            count = C.face_counts(live, len(verts))
            for v0, v1 in applied:
                assert count[v0] + count[v1] - 2 <= D.MAX_FACES
                if max(v0, v1) >= k:  # an apex takes part: only once the ring has shrunk
                    assert count[max(v0, v1)] <= D.MAX_FACES - 2 < k


def test_spindle_censuses_pin_the_side_of_the_cap(censuses):
    """Which side of `> MAX_FACES` an input lies on.  A ring vertex has 4 faces and an apex k: 4 + 22 - 2 = 24 is allowed, so at k = 22 the cap rejects
    nothing in the first round and the apexes have legal collapses; at k = 23 (25 > 24) all 4 k halfedges at the apexes fall to it, and so at 24 (the
    last k at which `gather` still holds an apex's ring) and 25 (the first at which it does not)."""
    legal, first = first_round("spindle_22")
    assert "fan cap" not in first and any(v0 >= 22 for v0, _, _ in legal) and any(v1 >= 22 for _, v1, _ in legal)
    for k in (23, 24, 25, 40):
        legal, first = first_round(f"spindle_{k}")
        assert first["fan cap"] == 4 * k and not any(max(v0, v1) >= k for v0, v1, _ in legal)
    caps = [censuses[f"spindle_{k}"].get("fan cap", 0) for k in (22, 23, 24, 25, 40)]
    assert len(set(caps)) == 5 and caps == sorted(caps), caps  # over all rounds: each ring size its own count
    print("spindle fan-cap rejections (22, 23, 24, 25, 40), budget 1, max_error 1e9 + 1e-6:", caps)


def test_large_spindles_never_collapse_an_apex_above_the_cap():
    """At 25 and 40 ring vertices no collapse has an apex for v0 or v1 while the apex has more than 22 faces; the ring shrinks first.  (The last
    collapses of a run to budget 1 do involve an apex: a ring of three vertices has no other legal collapse, and the run ends at a tetrahedron.)"""
    for k in (25, 40):
        verts, _ = C.case(f"spindle_{k}")
        out, _, _, trace = C.restated(f"spindle_{k}", 1, 1e9)
        assert len(out) == 4
        with_apex = [(r, pair) for r, (_, applied, _) in enumerate(trace) for pair in applied if max(pair) >= k]
        for r, pair in with_apex:
            assert C.face_counts(trace[r][2], len(verts))[max(pair)] <= D.MAX_FACES - 2
        # budget 2 k - 4: the ring loses two vertices and both apexes stay above 22 faces throughout -- no apex in any collapse
        trace = C.restated(f"spindle_{k}", C.spindle_high_budget(k), 1e9)[3]
        assert trace and not [pair for _, applied, _ in trace for pair in applied if max(pair) >= k]


@pytest.mark.parametrize("name", ["flat_spindle_23", "tilted_plane"])
def test_results_depend_on_the_cap_being_24(name, monkeypatch):
    """The spindles of full height pin the cap's side in the census only: their apex collapses cost bands more than the ring's, so the result would be
    the same with a cap of 23 or 25.  These two cases are the ones whose result at budget 1 changes with either: a kernel whose cap (or whose ring
    buffer) is off by one cannot match the restatement on them."""
    verts, faces = C.case(name)
    want = C.restated(name, 1, 1e9)
    for cap in (D.MAX_FACES - 1, D.MAX_FACES + 1):
        monkeypatch.setattr(D, "MAX_FACES", cap)
        out, kept, stats = D.decimate(verts, faces, 1, 1e9)
        assert stats != want[2] or not np.array_equal(kept, want[1]) or not np.array_equal(out, want[0]), cap
        monkeypatch.undo()


def test_fans():
    verts, faces = C.case("fan_25")
    assert C.face_counts(faces, len(verts))[0] == 25
    legal, census = first_round("fan_25")
    assert census["fan cap"] > 0 and all(v0 != 0 and v1 != 0 for v0, v1, _ in legal)  # 25 faces: the apex is in no collapse of the first round
    legal12, census12 = first_round("fan_12")
    assert "fan cap" not in census12 and any(v0 == 0 for v0, _, _ in legal12)  # 12 faces: the apex may slide along a boundary edge


def test_tilted_plane_costs():
    legal, _ = first_round("tilted_plane")
    costs = np.array([c for _, _, c in legal])
    bands = {D.cost_bits(c) >> D.KEY_BAND_SHIFT for c in costs}
    print(f"tilted_plane: {len(costs)} legal collapses, {(costs < 0).sum()} negative, {(costs == 0).sum()} zero, {(costs > 0).sum()} positive; bands {sorted(bands)}")
    assert (costs < 0).any() and (costs == 0).any() and (costs > 0).any()
    assert len(bands) >= 3
    assert any(D.cost_bits(c) < 0x80000000 for c in costs)  # the negative arm of cost_bits
    stats = C.restated("tilted_plane", 1, 1e9)[2]
    print("tilted_plane to budget 1: rounds, collapses, locked =", stats)  # a slow schedule (few collapses per round), on record; not tuned here


def _areas(name):
    verts, faces = C.case(name)
    p = verts[faces.astype(np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return np.sqrt((n * n).sum(1))


def test_area_classes():
    tiny = _areas("scaled_1e-20")
    assert np.all(tiny > 0) and np.all(tiny <= D.FLT_MIN)  # face_quadric's arm without normalisation, on every face
    deg = _areas("degenerate")
    assert np.any(deg == 0) and np.isnan(deg).any() and np.any(deg > D.FLT_MIN)
    nan_vertex = C.degenerate_nan_vertex(12)
    for budget in (1, 121):
        assert nan_vertex in C.restated("degenerate", budget, 1e9)[1].tolist()  # a NaN cost is never < max_error: the vertex stays
    assert np.all(_areas("scaled_1e25") > D.FLT_MIN)


def test_nan_costs_fall_to_max_error():
    """Every halfedge at the NaN vertex that reaches the cost has a NaN cost, which is below no max_error, infinity included."""
    verts, faces = C.case("degenerate")
    f = np.asarray(faces, np.int64)
    m = D._Mesh(f, np.ones(len(f), bool))
    q = D.vertex_quadrics(verts, f)
    locked = D.locked_vertices(len(verts), f)
    nan_vertex = C.degenerate_nan_vertex(12)
    assert np.isnan(q[nan_vertex]).all() and len(m.nbrs(nan_vertex)) == 6
    for w in m.nbrs(nan_vertex):
        for v0, v1 in ((nan_vertex, w), (w, nan_vertex)):
            assert np.isnan(D.qeval(q[v0] + q[v1], verts[v1]))
            for max_error in (1e9, float("inf")):
                assert D.collapse_check(m, q, verts, locked, v0, v1, max_error)[0] == "max_error"
    out, kept, stats, _ = C.restated("degenerate", 1, float("inf"))
    assert nan_vertex in kept.tolist() and stats[1] > 0


def test_huge_costs_cast_to_infinity():
    legal, census = first_round("scaled_1e25", float("inf"))
    assert legal and None in census
    costs = np.array([c for _, _, c in legal])
    assert np.all(np.isfinite(costs))
    with np.errstate(over="ignore"):
        assert np.all(np.isinf(costs.astype(np.float32)))
    assert {D.cost_bits(c) for c in costs} == {0xff800000}
    assert set(first_round("scaled_1e25", 1e9)[1]) <= {"max_error", "boundary", "v0 faces < 2"}  # finite max_error: nothing is legal
    assert C.restated("scaled_1e25", 1, 1e9)[2] == (0, 0, 0) and C.restated("scaled_1e25", 1, float("inf"))[2][1] > 0


def test_wide_rounds_and_their_cuts():
    """wide_lattice(200): round one selects more collapses than dec_thresh_kernel has threads, and the three budgets cut where they are meant to."""
    (f1, applied1, cum1), (f2, applied2, cum2) = C.wide_rounds()
    assert f1 == len(C.case("wide_lattice")[1]) and f2 == f1 - cum1[-1]
    assert len(applied1) >= 1500
    budgets = C.wide_budgets()
    for key, (budget, rounds, last) in budgets.items():
        out, kept, stats, trace = C.restated("wide_lattice", budget, 1e9)
        assert stats[0] == rounds == len(trace)
        assert len(trace[-1][1]) == last and len(out) in (budget - 1, budget)
        full = (applied1, applied2)[rounds - 1]
        assert trace[-1][1] == full[:last] and last < len(full)  # a proper prefix of the round's selection, in key order
        print(f"wide_lattice ({key}): budget {budget}, round {rounds} selects {len(full)}, cut after key {last}; stats {stats}")
    assert budgets["a"][2] > C.THRESH_THREADS and budgets["b"][2] < C.THRESH_THREADS
    trace_c = C.restated("wide_lattice", budgets["c"][0], 1e9)[3]
    assert trace_c[0][1] == applied1  # (c): all of round one first


def test_batch_boundaries():
    """Budgets on icosphere(2) for which the rounds number exactly 16, 17 and 32 -- one batch of DEC_BATCH = 16 rounds, one more round, two batches --
    and 15 and 33 on their far sides (found by running the restatement at every budget of the mesh)."""
    assert sorted(C.BATCH_BUDGETS) == [15, 16, 17, 32, 33]
    for rounds, budget in C.BATCH_BUDGETS.items():
        assert C.restated(C.BATCH_CASE, budget, 1e9)[2][0] == rounds


def test_tiny_meshes():
    """One face: `v0 faces < 2` everywhere.  Two faces on an edge: the two ends of the shared edge may slide along the boundary onto a wing tip, so a
    budget of 1 is met with one collapse; the other halfedges fall to `boundary` and `v0 faces < 2`."""
    assert C.rule_census(*C.one_face(), 0, 1e9) == {"v0 faces < 2": 6}
    census = C.rule_census(*C.two_faces(), 0, 1e9)
    assert {"boundary", "v0 faces < 2"} <= set(census)
    assert census[None] == 4  # the first round: each end of the shared edge onto either wing tip
    for budget in (0, 1):
        out, kept, stats = D.decimate(*C.two_faces(), budget, 1e9)
        assert stats == (1, 1, 0) and len(out) == 1 and len(kept) == 3
