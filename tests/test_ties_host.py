"""Host-side half of the tie / threshold-equality tests (no GPU).

  * every adversarial generator of tests/golden/cases.py delivers the property it exists for -- a later edit that quietly makes one of
    them tie-free again would turn tests/test_gpu_ties.py back into the ordinary parity tests, so the properties are asserted here;
  * the oracle states the project's tie rule (DESIGN.md "Tolerances": among exactly equal scores the larger original index first, in
    soft-NMS at every pick) and the reference's deterministic comparisons (`>` of nms_kernel.cu, `>=` against a double in cpu_nms.pyx,
    `<=` keeps in nms.py, float32 `> 1e-3`, `>=` at the image cut, C round() and first maximum in ROIPooling, floor in the FPN levels).
"""
import numpy as np
import pytest
import torch

import cases
from oracle import fpn as OF
from oracle import nms as ON
from oracle import postprocess as OPP
from oracle import roi_pooling as ORP

F32 = np.float32
THRESHOLDS = (0.3, 0.5, 0.6, 0.7, 0.8, 0.9)          # proposal / class NMS thresholds and the five of nms_multi_target


# ------------------------------------------------------------------------------------------------------------ generators
def test_round_mantissa_8_bits_is_the_bf16_grid():
    x = np.random.default_rng(0).normal(0, 3, 4096).astype(F32)
    want = torch.as_tensor(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(cases.round_mantissa(x, 8), want)
    assert np.array_equal(cases.round_mantissa(x, 24), x)


def test_quantised_scores_tie_groups_and_run_across_the_cut():
    n, K, run = 28728, 6000, 400
    s = cases.quantised_scores(n, 1, 8, straddle=(K, run))
    assert s.dtype == F32 and s.shape == (n,) and (s > 0).all() and (s <= 1).all()
    assert np.array_equal(s, cases.round_mantissa(s, 8))                   # on the bf16 grid
    vals, cnt = np.unique(s, return_counts=True)
    assert (cnt > 1).sum() >= 500 and len(vals) <= 2000                    # tied GROUPS: hundreds of them, thousands of anchors in them
    assert cnt[cnt > 1].sum() >= 0.95 * n
    kth = np.sort(s)[-K]
    above, upto = int((s > kth).sum()), int((s >= kth).sum())
    assert above < K < upto                                                 # the run of the K-th value straddles the cut
    assert upto - above >= run and K - above >= run // 4 and upto - K >= run // 4
    plain = cases.quantised_scores(n, 1, 8)                                 # even without the forced run the K-th score is shared
    kp = np.sort(plain)[-K]
    assert (plain == kp).sum() > 1


def test_lattice_boxes_sit_on_exact_halves_and_borders():
    n = 64
    b = cases.lattice_boxes(n, 2)
    assert b.dtype == F32 and b.shape == (n, 4)
    scaled = b * F32(0.0625)
    half = (np.abs(scaled) % 1 == 0.5)
    assert half.sum() >= 0.75 * b.size                                      # coordinates that scale to k + 0.5 exactly
    assert half.any(axis=1).sum() >= n - 4
    assert (b[:, 0] == 0).sum() >= 5 and (b[:, 2] == cases.IM_W - 1).sum() >= 5 and (b[:, 3] == cases.IM_H - 1).sum() >= 2
    assert (b[:, :2] < 0).any(axis=1).sum() >= 2                            # negative halves: round(-0.5) = -1, clamped window
    assert len({tuple(r) for r in b}) <= n                                  # (duplicates are allowed)
    # C round() against half-to-even: roi [8,8,40,40] pools cells 1..3, not 0..2
    r = np.array([0, 8, 8, 40, 40], F32)
    assert any(np.array_equal(x, r[1:]) for x in b)
    (hs, he), (ws, we) = ORP.roi_windows(r, 38, 63)
    assert hs.min() == 1 and he.max() == 4 and ws.min() == 1 and we.max() == 4
    assert np.rint(F32(8) * F32(0.0625)) == 0 and np.rint(F32(40) * F32(0.0625)) == 2
    # rois beyond the map: every bin empty
    beyond = [x for x in b if x[0] >= cases.IM_W]
    assert len(beyond) == 2
    for x in beyond:
        (hs, he), (ws, we) = ORP.roi_windows(np.concatenate(([0], x)).astype(F32), 38, 63)
        assert (he <= hs).all() and (we <= ws).all()


def _bin_stats(data, rois):
    """over all (roi, bin, channel): non-empty bins, those of more than one cell, bins whose maximum is held by more than one cell (a `>=` scan
    would report another argmax there), all-zero bins."""
    B, C, H, W = data.shape
    n = tied = zero = multi = 0
    for r in rois:
        (hs, he), (ws, we) = ORP.roi_windows(r, H, W)
        for ph in range(7):
            for pw in range(7):
                if he[ph] <= hs[ph] or we[pw] <= ws[pw]:
                    continue
                win = data[int(r[0]), :, hs[ph]:he[ph], ws[pw]:we[pw]].reshape(C, -1)
                m = win.max(axis=1, keepdims=True)
                n += C
                multi += C * (win.shape[1] > 1)
                tied += int(((win == m).sum(axis=1) > 1).sum())
                zero += int((m[:, 0] == 0).sum())
    return n, multi, tied, zero


def test_relu_tied_map_ties_inside_bins():
    data = cases.relu_tied_map(2, 8, 38, 63, 3)
    assert data.dtype == F32 and (data >= 0).all()
    assert np.array_equal(torch.as_tensor(data).to(torch.bfloat16).float().numpy(), data)          # bf16-representable
    assert 0.4 <= (data == 0).mean() <= 0.65
    assert (data[:, 0] == 0).all()
    boxes = cases.lattice_boxes(48, 4)
    rois = np.hstack((np.arange(48)[:, None] % 2, boxes)).astype(F32)
    n, multi, tied, zero = _bin_stats(data, rois)
    print('bins %d, of more than one cell %d, maximum not unique %d, all zero %d' % (n, multi, tied, zero))
    assert n > 10000 and multi >= 0.5 * n
    assert tied >= 0.5 * multi, tied / multi                                # share of the bins that CAN tie (more than one cell) whose maximum is NOT unique
    assert zero / n >= 0.12, zero / n                                       # all-zero bins (ReLU): argmax is the window's first cell
    # and the oracle's argmax is the FIRST maximum in row-major order
    out, arg = ORP.roi_pooling(data, rois, return_argmax=True)
    (hs, he), (ws, we) = ORP.roi_windows(rois[0], 38, 63)
    a = arg[0, 0]                                                           # channel 0 is all zero: first cell of every non-empty window
    for ph in range(7):
        for pw in range(7):
            want = -1 if (he[ph] <= hs[ph] or we[pw] <= ws[pw]) else hs[ph] * 63 + ws[pw]
            assert a[ph, pw] == want


def _iou64(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]) + 1); h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
    return w * h / ((a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - w * h)


@pytest.mark.parametrize('thresh', THRESHOLDS)
def test_iou_boundary_pairs_hit_the_threshold_exactly(thresh):
    p = cases.iou_boundary_pairs(thresh)
    t32 = F32(thresh)
    n_eq = sum(1 for a, b in p['eq'] if ON.iou_f32(a, b[None])[0] == t32 and _iou64(a, b) == thresh)
    assert n_eq == len(p['eq']) == 2                                        # pairs with iou == thresh, in float32 AND in float64
    a, b = p['above']
    assert ON.iou_f32(a, b[None])[0] == np.nextafter(t32, F32(1))
    a, b = p['below']
    assert ON.iou_f32(a, b[None])[0] == np.nextafter(t32, F32(0))
    for a, b in p['eq'] + [p['above'], p['below']]:
        assert np.array_equal(a, np.round(a)) and np.array_equal(b, np.round(b))


@pytest.mark.parametrize('N', [37, 300])
def test_saturated_posteriors_structure(N):
    B, C = 2, 21
    prob, boxes, info = cases.saturated_posteriors(B, N, C, 5)
    assert prob.dtype == F32 and prob.shape == (B, N, C) and boxes.dtype == np.float64 and boxes.shape == (B, N, 4)
    one = prob == F32(1.0)
    for b in range(B):
        per_class = one[b].sum(axis=0)
        assert per_class[1:5].min() >= (2 if N < 64 else 4), per_class      # per class: several rois at exactly 1.0f
    sizes = set()
    same_wave = cross_wave = 0
    for cls, idx in info['clusters']:
        assert (prob[:, idx, cls] == F32(1.0)).all()
        bx = boxes[0, idx]
        assert len({tuple(r) for r in bx}) == len(idx)                      # DISTINCT boxes ...
        for i in range(len(idx)):
            for j in range(i):
                assert _iou64(bx[i], bx[j]) > 0.5                            # ... that overlap
        sizes.add(len(idx))
        w = {i // 64 for i in idx}
        same_wave += len(w) == 1
        cross_wave += len(w) == len(idx) and len(idx) > 1
    assert {2, 3} <= sizes                                                  # two-way and multi-way ties
    assert same_wave >= 1 and (cross_wave >= 2 or N <= 64)
    tr = info['threshold_rows']
    last = C - 1
    assert [len(tr[k]) for k in ('eq', 'up', 'down')] == [3, 3, 2]
    assert (prob[:, tr['eq'], last] == F32(1e-3)).all()
    assert (prob[:, tr['up'], last] == np.nextafter(F32(1e-3), F32(1))).all()
    assert (prob[:, tr['down'], last] == np.nextafter(F32(1e-3), F32(0))).all()
    # tester.py's float32 `> 1e-3`: the rows AT the threshold and below it are no candidates, the next float up is one
    cand = np.where(prob[0, :, last] > 1e-3)[0]
    con = info['constructed']
    assert sorted(cand) == sorted([con[k] for k in ('P1', 'A', 'P2', 'B', 'M1', 'P3', 'M2')] + tr['up'])
    # a tie that arises from rescoring, and one that survives it (oracle): B before A, M2 before M1, equal scores
    b8 = np.concatenate([boxes[0]] * 2, 1)
    dets = OPP.detections(prob[0], b8, C, 1e-3, 0.6, True, 0)[last - 1]
    row = {k: int(np.where((dets[:, :4] == boxes[0, con[k]]).all(axis=1))[0][0]) for k in ('A', 'B', 'M1', 'M2', 'P1', 'P2', 'P3')}
    assert dets[row['A'], 4] == dets[row['B'], 4] < 0.5 and row['B'] + 1 == row['A']
    assert dets[row['M1'], 4] == dets[row['M2'], 4] < 0.25 and row['M2'] + 1 == row['M1']
    assert row['P1'] < row['P2'] < row['P3'] < row['B']


def test_tied_image_lists_tie_at_the_cut():
    dets, counts = cases.tied_image_lists(2, 20, 64, 10, counts_hi=30)
    for b in range(2):
        lists = [dets[b, c, :counts[b, c]] for c in range(20)]
        for d in lists:
            assert (np.diff(d[:, 4]) <= 0).all()
        kept, thr, total = OPP.image_cut(lists, 100)
        assert total > 100 and sum(len(k) for k in kept) > 100              # every detection tied with the 100th is kept
        assert sum(int((d[:, 4] == thr).sum()) for d in lists) > 1


def test_fpn_boundary_rois_and_oracle_levels():
    rois, s = cases.fpn_boundary_rois()
    want_s = []
    for k in (-1, 0, 1):
        want_s += [F32(2.0 ** k), np.nextafter(F32(2.0 ** k), F32(0)), np.nextafter(F32(2.0 ** k), F32(9))]
    assert np.array_equal(s[:9], np.asarray(want_s, F32))
    with np.errstate(divide='ignore'):
        lv = OF.roi_levels(rois)
    # floor of the FLOAT32 sum 2 + log2(s): ON a boundary goes up; one step below 0.5 and 1 stays down; one step below 2 the float32 sum
    # 2 + 0.99999991 already rounds to 3.0 (spacing 2.4e-7 there), so that roi is level 3 in the reference's arithmetic too
    assert list(lv) == [1, 0, 1, 2, 1, 2, 3, 3, 3, 0, 0, 3, 0]


# ------------------------------------------------------------------------------------------------------------ oracle rules
def test_argsort_desc_puts_the_larger_index_first():
    s = np.array([.5, .9, .5, .5, -np.inf, .9, -np.inf], F32)
    assert list(ON.argsort_desc(s)) == [5, 1, 3, 2, 0, 6, 4]
    assert list(ON.argsort_desc(np.full(300, .25))) == list(range(299, -1, -1))      # (numpy's default sort does not give this)


def test_soft_nms_tie_rule_largest_index_at_every_pick():
    d = np.array([[0, 0, 10, 10, .5], [20, 0, 30, 10, .5], [40, 0, 50, 10, .5], [60, 0, 70, 10, .5]])
    rows, keep = ON.soft_nms(d, 0.6, return_index=True)
    assert list(keep) == [3, 2, 1, 0] and (rows[:, 4] == .5).all()
    # distinct overlapping boxes: the NUMBERS depend on the rule, not only the order
    d = np.array([[0, 0, 10, 10, .5], [5, 0, 15, 10, .5], [100, 0, 110, 10, .5], [103, 0, 113, 10, .5]])
    rows, keep = ON.soft_nms(d, 0.6, return_index=True)
    assert list(keep) == [3, 1, 0, 2]
    ov = lambda a, b: _iou64(d[a, :4], d[b, :4])
    np.testing.assert_allclose(rows[:, 4], [.5, .5, .5 * np.exp(-ov(1, 0) ** 2 / 0.6), .5 * np.exp(-ov(3, 2) ** 2 / 0.6)], rtol=1e-15)
    np.testing.assert_allclose(rows[2:, 4], [.39553256, .29014779], rtol=1e-7)
    # a two-way tie that does not involve the first pick
    d = np.array([[0, 0, 10, 10, .9], [200, 0, 210, 10, .5], [400, 0, 410, 10, .5]])
    assert list(ON.soft_nms(d, 0.6, return_index=True)[1]) == [0, 2, 1]


def test_hard_nms_comparisons_at_the_threshold():
    for thresh in THRESHOLDS:
        p = cases.iou_boundary_pairs(thresh)
        for a, b in p['eq']:
            dets = np.array([list(a) + [.9], list(b) + [.8]], F32)
            assert ON.gpu_nms(dets, thresh) == [0, 1]                       # nms_kernel.cu: strict >, float32 against float32(thresh)
            assert list(ON.py_nms(dets.astype(np.float64), thresh)) == [0, 1]            # nms.py: ovr <= thresh keeps
            # cpu_nms.pyx: float32 overlap >= DOUBLE thresh
            assert ON.cpu_nms(dets, thresh) == ([0, 1] if float(F32(thresh)) < thresh else [0])
        for side, kept in (('above', [0]), ('below', [0, 1])):
            a, b = p[side]
            dets = np.array([list(a) + [.9], list(b) + [.8]], F32)
            assert ON.gpu_nms(dets, thresh) == kept and ON.cpu_nms(dets, thresh) == kept
    assert float(F32(0.7)) < 0.7 and float(F32(0.3)) > 0.3                  # both directions of the double compare are exercised


def test_image_cut_keeps_every_detection_tied_with_the_last():
    lists = [np.array([[0, 0, 1, 1, .9], [0, 0, 1, 1, .5], [0, 0, 1, 1, .5]]), np.zeros((0, 5)), np.array([[0, 0, 1, 1, .5], [0, 0, 1, 1, .4]])]
    kept, thr, total = OPP.image_cut(lists, 2)
    assert thr == .5 and total == 5 and [len(k) for k in kept] == [3, 0, 1]
    kept, thr, total = OPP.image_cut(lists, 5)
    assert thr == -np.inf and [len(k) for k in kept] == [3, 0, 2]
