"""The inputs of tests/test_train_head_edges_gpu.py have the properties its cases rely on, checked on the oracle alone, so a
regenerated input cannot quietly stop testing them; and the hand-written answers of the truncation case agree with the oracle."""
import numpy as np
import pytest

import train_head_abi as A


@pytest.mark.parametrize("h,w", [(24, 40), (40, 24)])
def test_nonsquare_cases_use_the_long_axis(h, w):
    case = A.case_nonsquare(h, w)
    want = A.oracle_targets(**case)
    assert want['heatmap'].shape == (2, 4, h, w)
    live = want['ind'][want['mask'] == 1]
    cy, cx = live // w, live % w
    far = ((cx >= min(h, w)) | (cy >= min(h, w))).sum()
    assert far >= 10, far
    assert want['mask'][:, 1].sum() == 0 and want['mask'][:, 0].sum() > 60           # the empty sample stays empty
    assert set(np.unique(case['labels'][0])) == {-1, 0, 1, 2, 3, 4}


@pytest.mark.parametrize("n_max", [64, 65, 128, 130, 200])
def test_many_boxes_cases_rank_past_one_wave(n_max):
    case = A.case_many(n_max)
    slots = A.expected_slots(case['labels'], case['classes_per_task'])
    assert slots.max() == n_max - 4                                   # sample 1: all rows but the three of no class
    if n_max >= 128:
        assert slots.max() > 64                                        # ranks above one wave's worth of boxes
    if n_max > 64:
        # a box in a row past the 64th is counted by boxes in the first rows: its slot lies below theirs
        assert slots[1, 64] >= 0 and (slots[1, :64] > slots[1, 64]).any()
    for b in range(3):
        live = slots[b] >= 0
        assert sorted(slots[b][live]) == list(range(live.sum()))                      # a permutation ...
        assert (slots[b][live] != np.arange(n_max)[live]).sum() > n_max // 4          # ... that is not the input order
    lab = case['labels']
    assert (lab[0, -9:] == -1).all() and (lab[1] >= 0).sum() == n_max - 1 and (lab == 3).sum() == 6
    # the oracle places every box that lies on the map where the definition says
    want = A.oracle_targets(**case)
    cy, cx, inside = A.cells(case)
    live = (slots >= 0) & inside
    assert live.sum() > 0.8 * (slots >= 0).sum() and want['mask'].sum() == live.sum()
    for b, i in zip(*np.where(live)):
        assert want['mask'][0, b, slots[b, i]] == 1 and want['ind'][0, b, slots[b, i]] == cy[b, i] * 16 + cx[b, i]


def test_cut_cases_have_more_boxes_than_slots():
    for m in (1, 64, 65):
        case = A.case_cut(m)
        want = A.oracle_targets(**case)
        assert (case['labels'] == 0).sum() == 75 > m and want['mask'][0].sum() == m
        assert (want['heatmap'][0, :2] == 1).sum() <= m and want['mask'][1].sum() == 0


def test_edge_cases_cut_the_window_on_every_side():
    cuts = np.array(A.window_cuts(A.case_edges(5, 7)))
    assert cuts.any(0).all()                                          # each of the four sides is cut in some window
    assert cuts.all(1).any()                                          # the map is smaller than the window on both axes
    for h, w in ((1, 9), (1, 1)):
        c = np.array(A.window_cuts(A.case_edges(h, w)))
        assert c[:, 2:].all() and c[:, 0].any() and c[:, 1].any()
    # a window of radius 6 reaches every cell of the 5 x 7 map from every centre
    want = A.oracle_targets(**A.case_edges(5, 7))
    assert (want['heatmap'] > 0).all() and want['mask'].sum() == 5


def test_radius_sweep_spans_many_radii():
    case = A.case_radius_sweep()
    want = A.oracle_targets(**case)
    support = (want['heatmap'] > 0).reshape(1024, -1).sum(1)
    assert len(np.unique(support)) >= 8, np.unique(support)
    assert want['mask'].sum() == 1024


def test_known_answers_agree_with_the_oracle():
    case, K = A.case_known(), A.known_answers()
    want = A.oracle_targets(**case)
    assert np.array_equal(want['mask'][0, 0], K['mask']) and np.array_equal(want['ind'][0, 0], K['ind'])
    assert np.array_equal(want['anno'][0, 0, :, :2], K['res'])
    live = K['mask'] == 1
    np.testing.assert_allclose(want['anno'][0, 0][live][:, 2:], np.tile(K['rest'], (4, 1)), rtol=1e-6)
    assert (want['anno'][0, 0][~live] == 0).all()
    assert sorted(map(tuple, np.argwhere(want['heatmap'][0, 0] == 1))) == sorted(K['peaks'])


def test_max_merge_case_overlaps():
    want = A.oracle_targets(**A.case_max_merge())
    hm = want['heatmap']
    assert hm[0, 1, 6, 5] == 1 and hm[0, 1, 6, 8] == 1 and hm[0, 0].sum() == 0
    solo = A.case_max_merge()
    solo['labels'][0, 1] = -1
    assert 0 < A.oracle_targets(**solo)['heatmap'][0, 1, 6, 8] < 1      # the big box's slope covers the small one's peak
    assert want['ind'][0, 1, 0] == want['ind'][0, 1, 1] and hm[1, 0, 4, 4] == 1 and hm[1, 1, 4, 4] == 1
    assert (hm[1, 0] > 0).sum() > (hm[1, 1] > 0).sum()


def test_shared_cell_cases_share_across_parts():
    for mo in (7, 8, 9, 64, 300):
        part = A.split_parts(mo)
        assert part.max() == min(mo, A.BOX_SPLIT) - 1 or mo == 9
        seen = set()
        for phase in (0, 1):
            inp = A.shared_straddle(mo, phase)
            live = np.where(inp['mask'][0])[0]
            for c in np.unique(inp['ind'][0, live]):
                ks = live[inp['ind'][0, live] == c]
                assert len(ks) == 2 and part[ks[0]] + 1 == part[ks[1]]
                seen.add(int(part[ks[0]]))
        assert seen == set(range(part.max())), (mo, seen)
    inp = A.shared_one_cell(64)
    assert all(len(np.unique(inp['ind'][b])) == 1 for b in range(2)) and inp['mask'].all()
    inp, trio, cell = A.shared_far_trio()
    part = A.split_parts(2100)
    assert (inp['ind'][0][inp['mask'][0] == 1] == cell).sum() == 3
    assert trio[1] - trio[0] > 256 and part[trio[0]] == part[trio[1]] and part[trio[2]] > part[trio[1]]


def test_smooth_logits_stay_clear_of_the_clamp():
    for seed in range(8):
        x = A.loss_inputs(seed, 3, 3, 9, 5, 8)['heat']
        assert (np.abs(np.abs(x.astype(np.float64)) - A.LN9999) > 1e-3).all()
    x = A.smooth_logits(np.random.default_rng(0), (4000,), scale=9.2)      # a draw that does reach the bounds
    assert (np.abs(np.abs(x.astype(np.float64)) - A.LN9999) > 1e-3).all() and np.abs(x).max() > 12


def test_clamp_case_has_cells_on_both_sides_of_both_bounds():
    inp = A.clamp_inputs()
    for row, t in enumerate((1.0, 0.0, 0.5)):
        x = inp['heat'][0, 0, row].astype(np.float64)
        assert (inp['target'][0, 0, row] == t).all()
        assert ((x > A.LN9999).sum() >= 2 and ((x < A.LN9999) & (x > 8)).sum() >= 1 and (x < -A.LN9999).sum() >= 2
                and ((x > -A.LN9999) & (x < -8)).sum() >= 1 and (x == 0).sum() == 1)
