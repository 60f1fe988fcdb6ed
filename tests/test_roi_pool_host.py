"""ROI max pooling on the host: the numpy reference of tests/roi_pool_ref.py against the oracle (bit for bit, ties included) and
against closed forms that do not depend on it, and the conditions on the tables of tests/test_gpu_roi_pool.py: every branch of
csrc/roi.hip is reached by more than one case, the "ties" maps do tie, every window lies inside its map."""
import numpy as np
import pytest

import roi_pool_ref as ref

IDS = [ref.case_id(c) for c in ref.CASES]


def test_the_cases_are_distinct_and_cover_the_tables():
    assert len(set(ref.CASES)) == len(ref.CASES)
    assert {c[0] for c in ref.CASES} >= set(ref.SHAPES)
    assert {c[1] for c in ref.CASES} == set(ref.GRIDS)
    assert {c[2] for c in ref.CASES} == set(ref.KINDS)
    for g in ref.GRIDS:     # each grid sees ties on the 8 x 29 x 50 map
        assert (ref.MAIN, g, "ties", "edges") in ref.CASES, g
    assert ((64, 29, 50), (7, 7), "ties", 600) in ref.CASES and ((3, 29, 50), (6, 6), "ties", 4097) in ref.CASES
    assert len(ref.windows_of_case(ref.CASES[-2])) == 600 and len(ref.windows_of_case(ref.CASES[-1])) == 4097


@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_every_window_lies_inside_its_map(case):
    (C, H, W), (kh, kw), kind, rows = case
    wins = ref.windows_of_case(case)
    assert wins.dtype == np.int32 and wins.shape[1] == 4 and len(wins) >= 7
    assert np.all(wins[:, 0] >= 1) and np.all(wins[:, 1] >= wins[:, 0]) and np.all(wins[:, 1] <= H)
    assert np.all(wins[:, 2] >= 1) and np.all(wins[:, 3] >= wins[:, 2]) and np.all(wins[:, 3] <= W)
    assert np.array_equal(wins, ref.windows_of(rows, H, W, kh, kw, ref.seed_of(case)))       # (fixed seeds)
    if rows == "edges":
        have = set(map(tuple, wins.tolist()))
        assert {(1, H, 1, W), (1, 1, 1, 1), (1, 1, W, W), (H, H, 1, 1), (H, H, W, W), (H, H, 1, W), (1, H, W, W)} <= have
        assert {(H, H, W - n + 1, W) for n in (1, 2, 3) if n <= W} <= have
        sides_h = {h for h in (kh - 1, kh, kh + 1, 2 * kh + 1) if 1 <= h <= H}
        sides_w = {w for w in (kw - 1, kw, kw + 1, 2 * kw + 1) if 1 <= w <= W}
        assert sides_h <= set((wins[:, 1] - wins[:, 0] + 1).tolist()) and sides_w <= set((wins[:, 3] - wins[:, 2] + 1).tolist())


def test_the_window_builder_refuses_a_window_outside_the_map():
    for bad in ([0, 3, 1, 5], [1, 4, 1, 5], [1, 3, 0, 5], [1, 3, 1, 6], [3, 2, 1, 5], [1, 3, 4, 3]):
        with pytest.raises(AssertionError):
            ref.check_windows(np.array([[1, 3, 1, 5], bad], np.int32), 3, 5)
    ref.check_windows(np.array([[1, 3, 1, 5], [3, 3, 5, 5]], np.int32), 3, 5)


@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_reference_equals_the_oracle(O, case):
    """out and idx bit for bit, every case; the backward pass from a zero map, rounded to fp32, within the bar of the GPU test
    (the oracle accumulates in fp32, one row after the other: an fp32 sum of the same terms)"""
    c = ref.inputs(case)
    shape = (c["C"], c["H"], c["W"])
    want_g = np.zeros(shape, np.float32)
    for r in range(c["R"]):
        wo, wi = O.adaptive_max_pool_fwd(c["fmap"], c["wins"][r], c["kh"], c["kw"])
        assert np.array_equal(c["out"][r].view(np.int32), wo.reshape(-1).view(np.int32)), r
        assert np.array_equal(c["idx"][r], wi.reshape(-1)), r
        O.adaptive_max_pool_bwd(want_g, c["gout"][r].reshape(c["C"], c["kh"], c["kw"]), c["bidx"][r].reshape(c["C"], c["kh"], c["kw"]))
    gm, count, abs_sum = ref.backward(c["gout"], c["bidx"], shape)
    bar = ref.backward_bar(count, abs_sum, False)
    assert np.all(np.abs(gm.astype(np.float32).astype(np.float64) - want_g) <= bar)
    assert np.all((count == 0) == (abs_sum == 0)) and np.all(gm[count == 0] == 0)
    # ... and into the non-zero map: one more term per element
    assert np.array_equal(c["count"], count + 1)
    assert np.allclose(c["gmap"], gm + c["gmap0"], rtol=0, atol=1e-12) and np.allclose(c["abs_sum"], abs_sum + np.abs(c["gmap0"]), rtol=0, atol=1e-12)


def test_backward_counts_what_contributes():
    idx = np.array([[0, 5, 5, -1], [5, 5, 2, 2]], np.int32)      # C = 2 planes of 2 x 3, a 1 x 2 grid
    gout = np.array([[1.0, 2.0, 0.0, 7.0], [0.5, -2.0, 0.0, 4.0]], np.float32)
    gm, count, abs_sum = ref.backward(gout, idx, (2, 2, 3))
    # plane 0, element 5: 2 + 0.5 - 2; plane 1: a zero gradient at element 5, a gradient without a winner, 0 + 4 at element 2
    assert gm.reshape(2, 6).tolist() == [[1.0, 0, 0, 0, 0, 0.5], [0, 0, 4.0, 0, 0, 0]]
    assert count.reshape(2, 6).tolist() == [[1, 0, 0, 0, 0, 3], [0, 0, 1, 0, 0, 0]]
    assert abs_sum.reshape(2, 6).tolist() == [[1.0, 0, 0, 0, 0, 4.5], [0, 0, 4.0, 0, 0, 0]]
    g0 = np.full((2, 2, 3), -3.0, np.float32)
    gm, count, abs_sum = ref.backward(gout, idx, (2, 2, 3), g0)
    assert gm[0, 1, 2] == -2.5 and count[0, 1, 2] == 4 and abs_sum[0, 1, 2] == 7.5 and count[1, 0, 0] == 1
    assert ref.backward_bar(count, abs_sum, False)[0, 1, 2] == 4 * 2.0 ** -23 * 7.5
    assert ref.backward_bar(count, abs_sum, True)[0, 1, 2] == 4 * 2.0 ** -23 * 7.5 + 4 * 2.0 ** -45
    assert ref.backward_bar(np.zeros(1, np.int64), np.zeros(1), True)[0] == 2.0 ** -45


CLOSED = [c for c in ref.CASES if c[2] in ("constant", "ramp_up", "ramp_down")]


@pytest.mark.parametrize("case", CLOSED, ids=[ref.case_id(c) for c in CLOSED])
def test_closed_form_winners(case):
    """a constant plane: the first element of every cell; a plane that rises / falls along its flat index: the last / the first"""
    c = ref.inputs(case)
    want = ref.closed_form_idx(c["kind"], c["wins"], c["C"], c["W"], c["kh"], c["kw"])
    assert np.array_equal(c["idx"], want)
    plane = np.repeat(np.arange(c["C"]), c["kh"] * c["kw"])[None, :]
    assert np.array_equal(c["out"], c["fmap"].reshape(c["C"], -1)[plane, want])


def test_cell_bounds():
    assert ref.cell_bounds(7, 3) == [(0, 3), (2, 5), (4, 7)]
    assert ref.cell_bounds(2, 3) == [(0, 1), (0, 2), (1, 2)]        # a side shorter than the grid: the cells repeat elements
    assert ref.cell_bounds(1, 4) == [(0, 1)] * 4
    assert ref.cell_bounds(6, 6) == [(i, i + 1) for i in range(6)]
    for n in range(1, 40):
        for k in range(1, 20):
            b = ref.cell_bounds(n, k)
            assert b[0][0] == 0 and b[-1][1] == n and all(0 <= s < e <= n for s, e in b)
            assert all(b[i][0] <= b[i + 1][0] and b[i + 1][0] <= b[i][1] for i in range(k - 1))    # no gap between neighbours


def test_a_hand_made_map_with_ties():
    fmap = np.array([[[1, 2, 2, 0],
                      [2, 1, 0, 0],
                      [0, 0, 3, 3]]], np.float32)
    out, idx = ref.forward(fmap, np.array([[1, 3, 1, 4], [1, 2, 1, 4], [2, 3, 2, 4]], np.int32), 1, 2)
    assert out.tolist() == [[2.0, 3.0], [2.0, 2.0], [3.0, 3.0]]
    # (0, 1) before (1, 0); (2, 2) before (2, 3); the overlapping cells of a three-column window both find (2, 2)
    assert idx.tolist() == [[1, 10], [1, 2], [10, 10]]
    out, idx = ref.forward(fmap, np.array([[1, 3, 1, 4]], np.int32), 3, 2)
    assert idx.tolist() == [[1, 2, 4, 6, 8, 10]]


TIES = [c for c in ref.CASES if c[2] == "ties" and c[0][1] * c[0][2] >= 29 * 50]


@pytest.mark.parametrize("case", TIES, ids=[ref.case_id(c) for c in TIES])
def test_the_ties_maps_tie(case):
    """a condition on the inputs: at least a quarter of the cells with four or more elements hold their maximum more than once"""
    c = ref.inputs(case)
    assert set(np.unique(c["fmap"]).tolist()) == {-1.0, 0.0, 1.0, 2.0}
    tied, total = ref.tied_share(c["fmap"], c["wins"], c["kh"], c["kw"])
    print("%s: %d of %d cells tied" % (ref.case_id(case), tied, total))
    assert total > 0 and 4 * tied >= total


def test_ties_cases_exist_where_the_condition_applies():
    assert len(TIES) >= len(ref.GRIDS) + 6


# ---- the labels ---------------------------------------------------------------------------------------------------------
def test_tables_reach_every_branch_more_than_once():
    assert ref.REQUIRED <= ref.labels_of_tables(), sorted(ref.REQUIRED - ref.labels_of_tables())
    reach = {lab: [c for c in ref.CASES if lab in ref.labels_of_case(c)] for lab in ref.REQUIRED}
    for lab, cases in sorted(reach.items()):
        print("%-15s %s" % (lab, ", ".join(ref.case_id(c) for c in cases)))
        assert len(cases) >= 2, (lab, cases)
    for case in ref.CASES:      # no label depends on a single case: the tables without any one of them still reach them all
        assert ref.REQUIRED <= ref.labels_of_tables([c for c in ref.CASES if c != case]), ref.case_id(case)


# what a case is in the tables for: case -> labels it must reach
WANT = {
    (ref.MAIN, (6, 6), "ties", "edges"): {"cells", "idle_threads", "lds", "det_lds"},
    (ref.MAIN, (16, 16), "ties", "edges"): {"cells", "one_group"},
    (ref.MAIN, (15, 17), "ties", "edges"): {"cells", "one_group", "idle_threads"},
    (ref.MAIN, (17, 16), "ties", "edges"): {"generic"},
    (ref.MAIN, (1, 300), "ties", "edges"): {"generic"},
    ((3, 1, 1), (6, 6), "randn", "edges"): {"cells", "hw_lt_4", "one_slice"},
    ((2, 1, 3), (2, 3), "ties", "edges"): {"cells", "hw_lt_4"},
    ((3, 1, 1), (17, 16), "randn", "edges"): {"generic"},
    ((2, 128, 128), (6, 6), "ties", "edges"): {"lds", "det_scratch"},
    ((2, 127, 130), (7, 7), "ties", "edges"): {"atomics", "det_scratch"},
    ((2, 127, 130), (1, 300), "ramp_up", "edges"): {"generic", "atomics"},
    ((2, 64, 128), (6, 6), "randn", "edges"): {"lds", "det_lds"},
    ((2, 91, 91), (7, 7), "ties", "edges"): {"lds", "det_scratch"},
    ((257, 3, 5), (16, 16), "ties", "edges"): {"one_group", "channel_stride"},
    ((257, 3, 5), (15, 17), "randn", "edges"): {"one_group", "channel_stride", "idle_threads"},
    ((64, 29, 50), (7, 7), "ties", 600): {"cells", "channel_stride", "idle_threads"},
    ((3, 29, 50), (6, 6), "ties", 4097): {"cells", "one_slice"},
}


def test_each_case_labels_what_it_is_listed_for():
    for case, want in WANT.items():
        assert case in ref.CASES, case
        got = ref.labels_of_case(case)
        assert want <= got, (ref.case_id(case), sorted(want - got))
    assert "hw_lt_4" not in ref.labels_of_case(((3, 2, 2), (3, 2), "ties", "edges"))          # H W == 4: the 16-byte pieces
    assert "one_slice" not in ref.labels_of_case(((64, 29, 50), (7, 7), "ties", 600))
    assert "channel_stride" not in ref.labels_of_case((ref.MAIN, (16, 16), "ties", "edges"))


def test_the_launch_rules_at_their_edges():
    P = ref.forward_plan
    assert "generic" in P(8, 29, 50, 10, 1, 257) and "cells" in P(8, 29, 50, 10, 1, 256)
    assert "idle_threads" not in P(8, 29, 50, 10, 16, 16) and "idle_threads" not in P(8, 29, 50, 10, 2, 2)
    assert "one_group" in P(8, 29, 50, 10, 1, 129) and "one_group" not in P(8, 29, 50, 10, 1, 128)
    # 600 rows of 64 channels at 7 x 7: 5 channels a block, min(13, 7) slices, 35 channels a pass
    assert "channel_stride" in P(64, 29, 50, 600, 7, 7) and "channel_stride" not in P(35, 29, 50, 600, 7, 7)
    assert "one_slice" in P(64, 29, 50, 4096, 7, 7) and "one_slice" not in P(64, 29, 50, 4095, 7, 7)
    assert "hw_lt_4" in P(2, 1, 3, 5, 2, 3) and "hw_lt_4" not in P(2, 2, 2, 5, 2, 3)
    B = ref.backward_plan
    assert B(128, 128, False) == {"lds"} and B(127, 130, False) == {"atomics"} and 127 * 130 > 16384
    assert B(64, 128, True) == {"det_lds"} and B(91, 91, True) == {"det_scratch"} and 91 * 91 > 8192
    assert ref.plan(2, 64, 128, 9, 6, 6, True) == {"cells", "idle_threads", "one_slice", "det_lds"}
