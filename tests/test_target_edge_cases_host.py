"""The cases of tests/target_edge_cases.py are what they claim -- asserted with the oracle alone, no GPU.  Conditions, not measurements: a case
whose cut does not cut, whose quirk does not show or whose filter filters nothing would let a wrong kernel pass tests/test_gpu_target_edges.py.
Every case builder runs here; no case is skipped or filtered, and every index a kernel is handed is in range."""
import numpy as np
import pytest

import target_edge_cases as TC

F32 = np.float32


# =====================================================================================================================
# anchors
# =====================================================================================================================
@pytest.mark.parametrize('name', sorted(TC.ANCHOR_CASES))
def test_anchor_case_is_what_it_claims(name):
    c = TC.anchor_case(name)
    B = len(c['gts'])
    A, (fh, fw) = c['base'].shape[0], c['feat_hw']
    assert B >= 2 and len({len(g) for g in c['gts']}) >= 2                 # image_index and the num_gt padding take part
    assert 1 <= A <= 32 and c['total'] == A * fh * fw <= 3300
    assert c['gt'].shape == (B, max(1, max(len(g) for g in c['gts'])), 5) and c['gt'].dtype == F32
    assert list(c['num_gt']) == [len(g) for g in c['gts']] and (c['num_gt'] <= c['gt'].shape[1]).all()
    if 'total' in TC.ANCHOR_CASES[name]:
        assert c['total'] == TC.ANCHOR_CASES[name]['total']
    for b in range(B):
        lab, bt, bw, lall = TC.anchor_expected(c, b)
        n = TC.anchor_counts(c, b)
        assert lab.shape == lall.shape == (c['total'],) and bt.shape == bw.shape == (4 * A, fh, fw)
        assert lab.dtype == bt.dtype == bw.dtype == F32
        assert n['fg_after'] <= n['num_fg'] and n['fg_after'] + n['bg_after'] <= max(n['batch'], 0)
        assert int((bw.reshape(A, 4, fh, fw)[:, 0].reshape(-1) == 1).sum()) == n['fg_after']
        print('%s image %d: total %d inside %d  fg %d -> %d  bg %d -> %d  (num_fg %d, batch %d)' %
              (name, b, c['total'], n['inside'], n['fg_before'], n['fg_after'], n['bg_before'], n['bg_after'], n['num_fg'], n['batch']))
    n = TC.anchor_counts(c, 0)
    assert ('fg' in c['cut']) == (n['fg_before'] > n['num_fg'])
    assert ('bg' in c['cut']) == (n['bg_before'] > n['batch'] - n['fg_after'])


def test_anchor_cases_cover_what_the_kernel_branches_on():
    cs = {name: TC.anchor_case(name) for name in TC.ANCHOR_CASES}
    inside = lambda name, b=0: TC.anchor_inside(cs[name], b)
    assert inside('border') > inside('defaults_small') > 0
    assert np.array_equal(cs['border']['gt'], cs['defaults_small']['gt'])
    # the clobber pair: same boxes, different labels before sub-sampling (bg wins with the switch on, fg with it off)
    on, off = TC.anchor_expected(cs['overlaps_swapped_clobber'], 0)[3], TC.anchor_expected(cs['overlaps_swapped_noclobber'], 0)[3]
    assert np.array_equal(cs['overlaps_swapped_clobber']['gt'], cs['overlaps_swapped_noclobber']['gt'])
    assert not np.array_equal(on, off) and (on == 1).sum() < (off == 1).sum()
    # gt_off_image: the reference's `overlaps == gt_max_overlaps` is 0 == 0 everywhere: every inside anchor is foreground, then cut to num_fg
    n = TC.anchor_counts(cs['gt_off_image'], 0)
    assert n['fg_before'] == n['inside'] > 0 and n['bg_before'] == 0 and n['fg_after'] == n['num_fg'] == 8
    n = TC.anchor_counts(cs['fg_fraction_0'], 0)
    assert n['num_fg'] == 0 and n['fg_before'] > 0 and n['fg_after'] == 0 and n['bg_after'] == 256
    n = TC.anchor_counts(cs['batch_0'], 0)
    assert n['fg_before'] > 0 and n['bg_before'] > 0 and n['fg_after'] == n['bg_after'] == 0
    assert all(inside('no_inside', b) == 0 for b in range(2)) and (cs['no_inside']['num_gt'] > 0).all()
    assert inside('one_cell') == cs['one_cell']['total'] == 12
    assert cs['a1_stride8']['base'].shape[0] == 1 and cs['a1_stride8']['total'] == 323 and cs['a1_stride8']['kw']['feat_stride'] == 8
    assert cs['a32']['base'].shape[0] == 32
    assert cs['no_gt']['num_gt'][0] == 0 and TC.anchor_counts(cs['no_gt'], 0)['bg_before'] == inside('no_gt')
    assert inside('partial_frame', 1) < inside('partial_frame', 0)
    assert sorted(cs[k]['total'] for k in cs if k.startswith('total_')) == [255, 256, 257, 1023, 1024, 1025]
    # some image of the table has unlabelled anchors inside the image (between the two overlaps) and some a non-zero target
    lab, bt, _, lall = TC.anchor_expected(cs['defaults_small'], 0)
    assert (lall == -1).sum() > cs['defaults_small']['total'] - inside('defaults_small') and np.abs(bt).max() > 0.1


# =====================================================================================================================
# proposal_target, all rows
# =====================================================================================================================
@pytest.mark.parametrize('name', sorted(TC.PT_CASES))
def test_proposal_target_case_is_what_it_claims(name):
    c = TC.pt_case(name)
    B, N, Gmax, D = c['B'], c['N'], c['Gmax'], 4 * c['num_reg']
    assert c['rois'].shape == (B, N, 5) and c['gt'].shape == (B, Gmax, 5) and (c['num_gt'] <= Gmax).all() and N + Gmax > 0
    assert c['num_rois'] is None or ((0 <= c['num_rois']) & (c['num_rois'] <= N)).all()
    for b in range(B):
        ro, lab, bt, bw = TC.pt_expected(c, b)
        assert ro.shape == (N + Gmax, 5) and lab.shape == (N + Gmax,) and bt.shape == bw.shape == (N + Gmax, D)
        nr = N if c['num_rois'] is None else int(c['num_rois'][b])
        G = int(c['num_gt'][b])
        pad = np.ones(N + Gmax, bool)
        pad[:nr] = False
        pad[N:N + G] = False
        assert (lab[pad] == -1).all() and (lab[~pad] >= 0).all() and not ro[pad, 1:].any() and not bw[pad].any() and (ro[pad, 0] == b).all()
        assert (ro[N:, 0] == b).all() and np.array_equal(ro[N:N + G, 1:], c['gt'][b, :G, :4])
        assert (lab[N:N + G] == c['gt'][b, :G, 4]).all()                    # a gt row matches itself
        if G == 0:
            assert (lab[:nr] == 0).all() and not bt.any() and not bw.any()
        elif nr + G > 3:
            assert (lab > 0).any() and (bw.sum(1)[lab > 0] == (4 if c['class_agnostic'] else 4 * (lab[lab > 0] < c['num_reg']))).all()
        print('%s image %d: N %d Gmax %d num_rois %d num_gt %d  fg %d bg %d padding %d' %
              (name, b, N, Gmax, nr, G, (lab > 0).sum(), (lab == 0).sum(), pad.sum()))


def test_proposal_target_cases_cover_the_grid_edge_and_the_paddings():
    cs = {name: TC.pt_case(name) for name in TC.PT_CASES}
    assert sorted(c['N'] + c['Gmax'] for c in cs.values())[-3:] == [255, 256, 257]
    assert any(c['N'] == 0 and c['Gmax'] > 0 for c in cs.values())
    assert any((c['num_gt'] == 0).any() and (c['num_gt'] > 0).any() for c in cs.values())
    nr = cs['rows_257_num_rois']
    assert nr['num_rois'][0] == nr['N'] and 0 < nr['num_rois'][1] < nr['N'] and nr['num_rois'][2] == 0
    c = cs['class_specific_5']
    lab = TC.pt_expected(c, 0)[1]
    assert not c['class_agnostic'] and ((lab > 0) & (lab < 5)).any() and (lab >= 5).any()            # labels on both sides of num_reg
    bw = TC.pt_expected(c, 0)[3]
    assert not bw[lab >= 5].any() and not bw[:, :4].any()
    # the unused gt slots hold a box that WOULD match a proposal: a kernel that read them would label it
    c = cs['rows_256_one_image_without_gt']
    assert c['num_gt'][1] == 0 and np.array_equal(c['gt'][1, 0, :4], c['rois'][0, 0, 1:])


# =====================================================================================================================
# OHEM
# =====================================================================================================================
@pytest.mark.parametrize('name', sorted(TC.OHEM_CASES))
def test_ohem_case_is_what_it_claims(name):
    c = TC.ohem_case(name)
    R, C, D, k = c['R'], c['C'], c['D'], c['roi_per_img']
    assert 1 <= R <= 2048 and C > 1 and D % 4 == 0 and k >= 0
    assert c['cls_score'].shape == (TC.OHEM_B, R, C) and c['bbox_pred'].shape == c['bbox_targets'].shape == c['bbox_weights'].shape == (TC.OHEM_B, R, D)
    lab = c['labels']
    assert ((lab >= -1) & (lab < C)).all() and (lab == np.round(lab)).all()                           # the label indexes the C scores of its row
    assert (lab[c['ignored_rows']] == -1).all() and not c['bbox_weights'][c['ignored_rows']].any() and (lab[~c['ignored_rows']] >= 0).all()
    assert not np.array_equal(c['cls_score'][0], c['cls_score'][1])
    for b in range(TC.OHEM_B):
        lo, wo, loss, order = TC.ohem_expected(c, b)
        nv = len(order)
        assert (lo != -1).sum() == min(k, nv) and (lo[c['ignored_rows'][b]] == -1).all() and not wo[c['ignored_rows'][b]].any()
        assert np.isneginf(loss[c['ignored_rows'][b]]).all() and np.isfinite(loss[~c['ignored_rows'][b]]).all()
        if 0 < k < nv:                       # the cut falls inside the valid rows: the loss bound (rtol 2e-6) cannot move a row across it
            hi, lo_ = loss[order[k - 1]], loss[order[k]]
            assert hi - lo_ > 1e-4 * abs(hi), (name, b, hi, lo_)
        if k >= nv:                          # every valid row is kept
            assert np.array_equal(lo, lab[b]) and np.array_equal(wo, c['bbox_weights'][b])


def test_ohem_cases_cover_the_table():
    cs = TC.OHEM_CASES
    plain = [c for c in cs.values() if c['ignored'] == 'none']
    assert {c['R'] for c in plain} == {1, 2, 3, 1023, 1024, 1025, 2047, 2048}
    for R in {c['R'] for c in plain}:
        assert {c['roi_per_img'] for c in plain if c['R'] == R} == {0, 1, R - 1, R, R + 5}
    assert {c['C'] for c in plain} == {2, 5} and {c['D'] for c in plain} == {4, 8, 20}
    assert {(c['C'], c['D']) for c in plain if c['R'] >= 1023} == {(a, d) for a in (2, 5) for d in (4, 8, 20)}
    t = TC.ohem_case('ignored_tail_inside_the_cut')
    assert all(t['roi_per_img'] > (~t['ignored_rows'][b]).sum() > 0 for b in range(TC.OHEM_B))      # ignored rows rank inside the cut
    t = TC.ohem_case('ignored_interleaved_cut_in_valid')
    assert all(0 < t['roi_per_img'] < (~t['ignored_rows'][b]).sum() for b in range(TC.OHEM_B))


# =====================================================================================================================
# nms_multi_target
# =====================================================================================================================
@pytest.mark.parametrize('name', sorted(TC.NMT_CASES))
def test_nmt_case_is_what_it_claims(name):
    c = TC.nmt_case(name)
    B, F_, C, T = c['B'], c['F'], c['C'], c['T']
    assert 1 <= F_ <= 256 and 1 <= T <= 8 and len(c['thresh']) == T and c['gt'].shape[1] <= 128 and (c['num_gt'] <= c['gt'].shape[1]).all()
    assert c['bbox'].shape == (B, F_, C, 4) and c['score'].shape == (B, F_, C) and (c['score'] > 0).all()
    for b in range(B):
        want = TC.nmt_expected(c, b)
        assert want.shape == (F_, C, T)
        assert (want.sum() > 0) == (c['num_gt'][b] > 0), (name, b)            # every image but the empty ones has a non-zero target
        print('%s image %d: F %d C %d T %d num_gt %d  ones per threshold %s' % (name, b, F_, C, T, c['num_gt'][b], want.sum((0, 1)).astype(int).tolist()))


def test_nmt_cases_cover_the_table():
    cs = {name: TC.nmt_case(name) for name in TC.NMT_CASES}
    assert {1, 63, 64, 65, 255, 256} <= {c['F'] for c in cs.values()}
    assert {c['T'] for c in cs.values()} == {1, 5, 8} and {c['C'] for c in cs.values()} == {1, 2}
    assert {1, 3, 128} <= {int(g) for c in cs.values() for g in c['num_gt']}
    c = cs['F256_128_gts_of_one_class']
    assert c['num_gt'][0] == 128 and (c['gt'][0, :, 4] == 1).all() and c['C'] == 2                    # all of sgt; class 2 without any gt
    assert not TC.nmt_expected(c, 0)[:, 1].any() and TC.nmt_expected(c, 0)[:, 0].sum() > 128
    assert any((c['num_gt'] == 0).any() and (c['num_gt'] > 0).any() for c in cs.values())
    # row0_quirk: row 0 overlaps gt 0 by 0.75 and gt 1 not at all; row 5 (better score, overlap 0.95) is gt 0's pick -- and still
    # want[0] is 1 below 0.75, through the all-zero column of gt 1
    c = cs['row0_quirk']
    ov = TC.OB.bbox_overlaps(c['bbox'][0, :, 0].astype(np.float64), c['gt'][0, :2, :4].astype(np.float64))
    assert ov[0, 0] == 0.75 and not ov[:, 1].any() and ov[5, 0] == 0.95 and c['score'][0, 5, 0] > c['score'][0, 0, 0]
    want = TC.nmt_expected(c, 0)
    assert want[0, 0].tolist() == [1, 1, 1, 0, 0] and want[5, 0].tolist() == [1, 1, 1, 1, 1] and want.sum() == 8
    alone = TC.OT.nms_multi_target(c['bbox'][0], c['gt'][0, :1][None], c['score'][0])                  # without the second gt: no 1 in row 0
    assert not alone[0].any()
    # the winner in the last row of the last wavefront; equal scores across the wavefront boundary 63 | 64: the first wins
    for name in ('F65_winner_in_the_last_row', 'F255_winner_in_the_last_row'):
        c = cs[name]
        want = TC.nmt_expected(c, 0)
        assert want[c['F'] - 1, 0].all() and want[:, 0].sum() == c['T'] and c['score'][0, 63, 1] == c['score'][0, 64, 1]
        assert want[63, 1].all() and not want[64, 1].any() and (c['F'] - 1) // 64 == (c['F'] + 63) // 64 - 1 and c['F'] % 64
        want = TC.nmt_expected(c, 1)
        assert c['num_gt'][1] == 1 and not want[:, 0].any() and want[63, 1].all() and want.sum() == c['T']


# =====================================================================================================================
# bbox_overlaps
# =====================================================================================================================
def test_overlap_cases():
    assert sorted(n * k for n, k in TC.OVERLAP_CASES.values()) == [0, 0, 255, 256, 257, 257]
    for name in sorted(TC.OVERLAP_CASES):
        boxes, query = TC.overlap_case(name)
        want = TC.overlap_expected(boxes, query)
        assert want.shape == TC.OVERLAP_CASES[name] and not np.isnan(want).any()
        assert np.array_equal(boxes, boxes.astype(F32)) and np.array_equal(query, query.astype(F32))
    boxes, query = TC.overlap_case('256')
    want = TC.overlap_expected(boxes, query)
    assert (want > 0).sum() > 16 and (want == 0).sum() > 16
    iw = lambda i, j: min(boxes[i, 2], query[j, 2]) - max(boxes[i, 0], query[j, 0]) + 1
    ih = lambda i, j: min(boxes[i, 3], query[j, 3]) - max(boxes[i, 1], query[j, 1]) + 1
    assert iw(0, 0) == 0 and ih(0, 0) > 0 and want[0, 0] == 0              # touching: the +1 extent is exactly 0
    assert ih(1, 1) == 1 and want[1, 1] == 10 / 190                        # one shared pixel row
    assert want[2, 2] == 1.0                                               # identical
    assert boxes[3, 2] < boxes[3, 0] and not want[3].any()                 # x2 < x1: no overlap with anything, the query around it included
    assert query[3, 0] <= boxes[3, 2] and query[3, 2] >= boxes[3, 0]


# =====================================================================================================================
# decode
# =====================================================================================================================
@pytest.mark.parametrize('name', sorted(TC.DECODE_CASES))
def test_decode_case_is_what_it_claims(name):
    c = TC.decode_case(name)
    H, W = c['map']
    assert c['cls'].shape == (c['B'], 2 * c['A'], H, W) and c['deltas'].shape == (c['B'], 4 * c['A'], H, W)
    assert 1 <= c['h'] <= H and 1 <= c['w'] <= W and c['n'] == c['h'] * c['w'] * c['A'] < 65536
    if c['im_hw'] is None:                   # the wrapper reads (h, w) from im_info: one size per batch
        assert (c['im_info'][:, :2] == c['im_info'][0, :2]).all()
    bg, fg = c['cls'][:, :c['A']], c['cls'][:, c['A']:]
    exact = (bg - fg).astype(np.float64) == bg.astype(np.float64) - fg.astype(np.float64)      # is the float32 difference the true one?
    if c['score_grid'] is None:
        assert (~exact).mean() > 0.2
    else:
        assert exact.all() and len(np.unique(c['cls'])) > 100 and np.array_equal(c['cls'], np.round(c['cls'] / TC.SCORE_GRID) * TC.SCORE_GRID)
    for sp in (False, True):
        boxes, scores = TC.decode_expected(c['cls'], c['deltas'], c['im_info'], c['base'], c['stride'], c['min_size'], c['h'], c['w'], sp)
        assert boxes.shape == (c['B'], c['n'], 4) and boxes.dtype == F32 and scores.shape == (c['B'], c['n'])
        fin = np.isfinite(scores)
        assert (np.isneginf(scores) | fin).all()
        for b in range(c['B']):
            if name == 'all_filtered':
                assert not fin[b].any()
            elif c['min_size'] > 0:
                assert fin[b].any() and not fin[b].all(), (name, b)
            else:
                assert fin[b].all()
            assert (boxes[b, :, 0::2] <= c['im_info'][b, 1] - 1).all() and (boxes[b, :, 1::2] <= c['im_info'][b, 0] - 1).all() and (boxes[b] >= 0).all()
        if sp and fin.any():
            assert ((scores[fin] >= 2.0 ** -120) & (scores[fin] <= 1)).all()                             # normal float32 numbers
        print('%s softmax_pairs=%d: n %d, -inf per image %s' % (name, sp, c['n'], [int((~fin[b]).sum()) for b in range(c['B'])]))


def test_decode_cases_cover_the_table():
    cs = {name: TC.decode_case(name) for name in TC.DECODE_CASES}
    assert {255, 256, 257} <= {c['n'] for c in cs.values()} and {1, 3, 12} <= {c['A'] for c in cs.values()}
    c = cs['cropped']
    assert (c['h'], c['w']) == (9, 17) and c['map'] == (13, 21) and c['B'] == 1
    assert any(c['layout'] == 'mixed_views' and (c['h'], c['w']) != c['map'] for c in cs.values())
    # batch_infos: three different (h, w, scale) rows, and clipping changes at least one box of every image
    c = cs['batch_infos']
    assert len({tuple(r) for r in c['im_info']}) == 3 and c['im_hw'] is not None
    raw = TC.OB.bbox_pred(TC.shifted_anchors(c['h'], c['w'], c['stride'], c['base']), c['deltas'][0, :, :c['h'], :c['w']].transpose(1, 2, 0).reshape(-1, 4))
    boxes, scores = TC.decode_expected(c['cls'], c['deltas'], c['im_info'], c['base'], c['stride'], c['min_size'], c['h'], c['w'], False)
    for b in range(3):
        rawb = TC.OB.bbox_pred(TC.shifted_anchors(c['h'], c['w'], c['stride'], c['base']), c['deltas'][b, :, :c['h'], :c['w']].transpose(1, 2, 0).reshape(-1, 4))
        assert (rawb.astype(F32) != boxes[b]).any(axis=1).sum() > 10
    assert len({int(np.isinf(scores[b]).sum()) for b in range(3)}) == 3
    # scale_min_size: min_size * scale = 24 and 9.6: the same boxes, different filters
    c = cs['scale_min_size']
    assert c['im_info'][:, 2].tolist() == [F32(1.5), F32(0.6)] and c['min_size'] == 16
    boxes, scores = TC.decode_expected(c['cls'], c['deltas'], c['im_info'], c['base'], c['stride'], c['min_size'], c['h'], c['w'], False)
    for b, ms in ((0, 24.0), (1, 16 * float(F32(0.6)))):
        p = TC.OB.clip_boxes(TC.OB.bbox_pred(TC.shifted_anchors(c['h'], c['w'], c['stride'], c['base']),
                                             c['deltas'][b, :, :c['h'], :c['w']].transpose(1, 2, 0).reshape(-1, 4)), (208, 336))
        side = np.minimum(p[:, 2] - p[:, 0] + 1, p[:, 3] - p[:, 1] + 1)
        assert np.array_equal(np.isinf(scores[b]), side < ms)
        assert ((side >= min(ms, 16)) & (side < max(ms, 16))).any()        # boxes that min_size alone would decide the other way
    # wide_logits: the score pairs of confident anchors, up to 60 apart
    for name in ('wide_logits', 'float32_scores_wide'):
        c = cs[name]
        gap = np.abs(c['cls'][:, :c['A']] - c['cls'][:, c['A']:])
        assert gap.max() > 40 and (gap > 8).mean() > 0.3
    # float32_scores: with the float32 differences in the reference the two float64 softmaxes differ by more than the bound of the GPU test:
    # the case would not pass against the plain float64 softmax, and says why
    c = cs['float32_scores']
    a = TC.decode_expected(c['cls'], c['deltas'], c['im_info'], c['base'], c['stride'], 0, c['h'], c['w'], True)[1]
    b = TC.decode_expected(c['cls'], c['deltas'], c['im_info'], c['base'], c['stride'], 0, c['h'], c['w'], True, f32_gap=True)[1]
    assert 1.0 * 2.0 ** -23 < (np.abs(a - b) / a).max() < 8 * 2.0 ** -23
    assert raw.shape == (c['n'], 4)
