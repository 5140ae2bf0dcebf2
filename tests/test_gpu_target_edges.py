"""The training-target kernels (csrc/targets.hip) and the proposal decode (csrc/proposal.hip) at their edges, against the expected arrays of
tests/target_edge_cases.py (the pinned oracle; tests/test_target_edge_cases_host.py asserts that the cases are what they claim).

  assign_anchor      label, label_all, bbox_weight equal; bbox_target within 1e-6 absolute (the bound of test_gpu_targets.py)
  proposal_target    all four outputs bit-equal
  OHEM               labels and weights equal; loss rtol 2e-6 (the bound of test_gpu_targets.py)
  nms_multi_target   equal
  bbox_overlaps      bit-equal
  decode             boxes bit-equal; the -inf pattern equal; scores bit-equal (fg channel) or within 4 * 2**-23 relative of the float64
                     two-way softmax (softmax_pairs; SOFTMAX_RTOL below states what that asks of the scores and what was found)

Every index handed to a kernel is in range and every shape inside the documented limits, apart from the rejected calls, which launch
nothing.  Each test prints its per-case figures."""
import ctypes

import numpy as np
import pytest
import torch

import target_edge_cases as TC
from oracle import proposal as OP

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib, operator_py
    lib.load()
    return ops, operator_py, lib


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _np(t):
    return t.cpu().numpy()


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda', dtype=torch.float32)


def _d4(v):
    return (ctypes.c_double * 4)(*v)


# =====================================================================================================================
# relnet_assign_anchor
# =====================================================================================================================
def _check_anchor(c, L, T, W, Lall):
    for b in range(len(c['gts'])):
        wl, wt, ww, wall = TC.anchor_expected(c, b)
        n = TC.anchor_counts(c, b)
        print('%s image %d: total %d inside %d  fg %d -> %d  bg %d -> %d' %
              (c['name'], b, c['total'], n['inside'], n['fg_before'], n['fg_after'], n['bg_before'], n['bg_after']))
        got = _np(Lall[b])
        assert np.array_equal(got, wall), (c['name'], b, np.flatnonzero(got != wall)[:8])
        got = _np(L[b])
        assert np.array_equal(got, wl), (c['name'], b, int((got != wl).sum()))
        assert np.array_equal(_np(W[b]), ww), (c['name'], b)
        err = np.abs(_np(T[b]) - wt).max()
        assert err <= 1e-6, (c['name'], b, err)


@pytest.mark.parametrize('name', sorted(TC.ANCHOR_CASES))
def test_assign_anchor_edges(rn, name):
    ops, _, _ = rn
    c = TC.anchor_case(name)
    L, T, W, Lall = ops.assign_anchor(_dev(c['gt']), _dev(c['num_gt']), _dev(c['im_info']), c['base'], c['feat_hw'], seed=c['seed'],
                                      want_all=True, **c['kw'])
    _check_anchor(c, L, T, W, Lall)


@pytest.mark.parametrize('name', ['small_batch', 'total_1025', 'no_inside'])
def test_assign_anchor_writes_every_word(rn, name):
    """relnet_assign_anchor through lib.call into NaN-filled outputs: label, label_all, bbox_target and bbox_weight are written everywhere --
    outside anchors, images without gt and the (dirty) best-overlap workspace included."""
    ops, _, lib = rn
    c = TC.anchor_case(name)
    B, A, (fh, fw), G = len(c['gts']), c['base'].shape[0], c['feat_hw'], c['gt'].shape[1]
    L, Lall = _nan(B, c['total']), _nan(B, c['total'])
    T, W = _nan(B, 4 * A, fh, fw), _nan(B, 4 * A, fh, fw)
    ws = torch.full((B, G), -1, device='cuda', dtype=torch.int64)
    gt, num_gt, info, base = _dev(c['gt']), _dev(c['num_gt']), _dev(c['im_info']), np.ascontiguousarray(c['base'])
    k = c['kw']
    lib.call('relnet_assign_anchor', gt.data_ptr(), num_gt.data_ptr(), info.data_ptr(), base.ctypes.data, L.data_ptr(), T.data_ptr(),
             W.data_ptr(), Lall.data_ptr(), ws.data_ptr(), B, A, fh, fw, G, k['feat_stride'], k['rpn_batch_size'],
             int(k['fg_fraction'] * k['rpn_batch_size']), k['negative_overlap'], k['positive_overlap'], int(k['clobber_positives']),
             k['allowed_border'], ctypes.c_ulonglong(c['seed']), 0, ops._stream())
    torch.cuda.synchronize()
    for t in (L, Lall, T, W):
        assert not torch.isnan(t).any()
    _check_anchor(c, L, T, W, Lall)


# =====================================================================================================================
# relnet_proposal_target_ex
# =====================================================================================================================
def _check_pt(c, r, lab, bt, bw):
    for b in range(c['B']):
        wr, wl, wt, ww = TC.pt_expected(c, b)
        print('%s image %d: N %d Gmax %d  fg %d bg %d padding %d' % (c['name'], b, c['N'], c['Gmax'], (wl > 0).sum(), (wl == 0).sum(), (wl < 0).sum()))
        got = _np(lab[b])
        assert np.array_equal(got, wl), (c['name'], b, np.flatnonzero(got != wl)[:8])
        assert np.array_equal(_np(r[b]), wr), (c['name'], b)
        assert np.array_equal(_np(bt[b]), wt), (c['name'], b, np.abs(_np(bt[b]) - wt).max())
        assert np.array_equal(_np(bw[b]), ww), (c['name'], b)


@pytest.mark.parametrize('name', sorted(TC.PT_CASES))
def test_proposal_target_all_rows_edges(rn, name):
    ops, _, _ = rn
    c = TC.pt_case(name)
    num_rois = None if c['num_rois'] is None else _dev(c['num_rois'])
    r, lab, bt, bw = ops.proposal_target(_dev(c['rois']), _dev(c['gt']), _dev(c['num_gt']), num_reg=c['num_reg'],
                                         class_agnostic=c['class_agnostic'], num_rois=num_rois)
    _check_pt(c, r, lab, bt, bw)


@pytest.mark.parametrize('name', ['rows_257_num_rois', 'class_specific_5'])
def test_proposal_target_writes_every_word(rn, name):
    ops, _, lib = rn
    c = TC.pt_case(name)
    B, R, D = c['B'], c['N'] + c['Gmax'], 4 * c['num_reg']
    r, lab, bt, bw = _nan(B, R, 5), _nan(B, R), _nan(B, R, D), _nan(B, R, D)
    rois, gt, num_gt, num_rois = _dev(c['rois']), _dev(c['gt']), _dev(c['num_gt']), _dev(c['num_rois'])
    lib.call('relnet_proposal_target_ex', rois.data_ptr(), gt.data_ptr(), num_gt.data_ptr(), r.data_ptr(), lab.data_ptr(), bt.data_ptr(),
             bw.data_ptr(), B, c['N'], c['Gmax'], c['num_reg'], int(c['class_agnostic']), 0.5, _d4((0, 0, 0, 0)), _d4((0.1, 0.1, 0.2, 0.2)),
             _d4((1, 1, 1, 1)), num_rois.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    for t in (r, lab, bt, bw):
        assert not torch.isnan(t).any()
    _check_pt(c, r, lab, bt, bw)


# =====================================================================================================================
# relnet_box_annotator_ohem
# =====================================================================================================================
def _check_ohem(c, lo, wo, loss):
    for b in range(TC.OHEM_B):
        wlo, wwo, wloss, order = TC.ohem_expected(c, b)
        ok = ~c['ignored_rows'][b]
        got_loss = _np(loss[b])
        np.testing.assert_allclose(got_loss[ok], wloss[ok], rtol=2e-6, atol=0, err_msg='%s image %d' % (c['name'], b))
        assert np.isneginf(got_loss[~ok]).all()
        got = _np(lo[b])
        assert np.array_equal(got, wlo), (c['name'], b, np.flatnonzero(got != wlo)[:8])
        assert np.array_equal(_np(wo[b]), wwo), (c['name'], b)
    print('%s: R %d C %d D %d roi_per_img %d  kept %s  ignored %s' % (c['name'], c['R'], c['C'], c['D'], c['roi_per_img'],
          [int((_np(lo[b]) != -1).sum()) for b in range(TC.OHEM_B)], c['ignored_rows'].sum(1).tolist()))


@pytest.mark.parametrize('R', sorted({c['R'] for c in TC.OHEM_CASES.values() if c['ignored'] == 'none'}))
def test_ohem_edges(rn, R):
    """One R per test, every roi_per_img of {0, 1, R - 1, R, R + 5} in it."""
    ops, _, _ = rn
    names = [n for n, c in sorted(TC.OHEM_CASES.items()) if c['R'] == R and c['ignored'] == 'none']
    assert len(names) == len({0, 1, R - 1, R, R + 5})
    for name in names:
        c = TC.ohem_case(name)
        lo, wo, loss = ops.box_annotator_ohem(_dev(c['cls_score']), _dev(c['bbox_pred']), _dev(c['labels']), _dev(c['bbox_targets']),
                                              _dev(c['bbox_weights']), c['roi_per_img'], want_loss=True)
        _check_ohem(c, lo, wo, loss)


@pytest.mark.parametrize('name', [n for n, c in sorted(TC.OHEM_CASES.items()) if c['ignored'] != 'none'])
def test_ohem_ignored_rows_and_every_word(rn, name):
    """Rows with label -1 (proposal_target's padding) stay ignored with zero weights whatever their rank, and every valid row inside the cut
    is kept.  Through lib.call into NaN-filled outputs: labels, weights and the loss are written everywhere."""
    ops, _, lib = rn
    c = TC.ohem_case(name)
    B, R, C, D = TC.OHEM_B, c['R'], c['C'], c['D']
    lo, wo, loss = _nan(B, R), _nan(B, R, D), _nan(B, R)
    t = [_dev(c[k]) for k in ('cls_score', 'bbox_pred', 'labels', 'bbox_targets', 'bbox_weights')]
    lib.call('relnet_box_annotator_ohem', *[x.data_ptr() for x in t], lo.data_ptr(), wo.data_ptr(), loss.data_ptr(), B, R, C, D,
             c['roi_per_img'], ops._stream())
    torch.cuda.synchronize()
    for x in (lo, wo, loss):
        assert not torch.isnan(x).any()
    _check_ohem(c, lo, wo, loss)


# =====================================================================================================================
# relnet_nms_multi_target
# =====================================================================================================================
def _check_nmt(c, out):
    for b in range(c['B']):
        want = TC.nmt_expected(c, b)
        got = _np(out[b])
        print('%s image %d: F %d C %d T %d num_gt %d  ones per threshold %s' %
              (c['name'], b, c['F'], c['C'], c['T'], c['num_gt'][b], want.sum((0, 1)).astype(int).tolist()))
        assert np.array_equal(got, want), (c['name'], b, np.argwhere(got != want)[:8])


@pytest.mark.parametrize('name', sorted(TC.NMT_CASES))
def test_nms_multi_target_edges(rn, name):
    ops, _, _ = rn
    c = TC.nmt_case(name)
    out = ops.nms_multi_target(_dev(c['bbox']), _dev(c['gt']), _dev(c['score']), _dev(c['num_gt']), target_thresh=c['thresh'])
    _check_nmt(c, out)


@pytest.mark.parametrize('name', ['F65_image_without_gt', 'F256_128_gts_of_one_class'])
def test_nms_multi_target_writes_every_word(rn, name):
    ops, _, lib = rn
    c = TC.nmt_case(name)
    out = _nan(c['B'], c['F'], c['C'], c['T'])
    bbox, gt, num_gt, score = _dev(c['bbox']), _dev(c['gt']), _dev(c['num_gt']), _dev(c['score'])
    th = (ctypes.c_double * c['T'])(*c['thresh'])
    lib.call('relnet_nms_multi_target', bbox.data_ptr(), gt.data_ptr(), num_gt.data_ptr(), score.data_ptr(), out.data_ptr(), c['B'], c['F'],
             c['C'], c['gt'].shape[1], th, c['T'], ops._stream())
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    _check_nmt(c, out)


# =====================================================================================================================
# relnet_bbox_overlaps
# =====================================================================================================================
@pytest.mark.parametrize('name', sorted(TC.OVERLAP_CASES))
def test_bbox_overlaps_edges(rn, name):
    ops, _, _ = rn
    boxes, query = TC.overlap_case(name)
    want = TC.overlap_expected(boxes, query)
    got = _np(ops.bbox_overlaps(_dev(boxes), _dev(query)))
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8])


# =====================================================================================================================
# relnet_proposal_decode
# =====================================================================================================================
# The two-way softmax against float64 (scores on the grid of tests/target_edge_cases.py, where the float32 differences bg - max and
# fg - max that every float32 softmax starts with are exact): two expf results of at most 1 ulp each (the larger argument is
# exp(0) = 1 exactly), one float32 addition and one float32 division -- four relative errors of at most 2**-23 (an ulp; the two
# roundings are half of one), to first order at most 4 * 2**-23 in sum.  Derived, not measured.
#
# The float32_scores cases take unrounded float32 scores.  There the difference itself rounds, by up to |bg - fg| 2**-24, and that is a
# RELATIVE error of the exponential which the four terms above do not contain: measured on the MI355X against the plain float64 softmax,
# 4.7 x 2**-23 at |bg - fg| <= 12 (float32_scores) and 16.5 x 2**-23 at |bg - fg| <= 60 (float32_scores_wide); on the grid the largest
# error of any case is 1.3 x 2**-23.  It is the float32
# SoftmaxActivation's own arithmetic (oracle/network.py:rpn_softmax rounds the same difference, and test_gpu_pipeline.py holds the
# detector's proposals to that form row for row: a kernel that took the difference in float64 met 0.5 x 2**-23 here and changed 2 of 300
# proposal rows of test_detector_bf16_fullsize_stagewise), so it stays.  These two cases are held to the float64 softmax of the float32
# differences -- the same four terms, the same bound -- and print the distance to the plain float64 softmax beside it.
SOFTMAX_RTOL = 4 * 2.0 ** -23


def _decode_operands(c):
    """cls_prob and bbox_deltas on the device in the case's layout."""
    cls, deltas = _dev(c['cls']), _dev(c['deltas'])
    if c['layout'] == 'mixed_views':
        cls = cls.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # channels-last memory, NCHW view
        B, C4, H, W = deltas.shape
        big = torch.full((B + 1, C4 + 3, H + 2, 2 * W + 5), float('nan'), device='cuda')
        view = big[1:, 2:2 + C4, 1:1 + H, 3:3 + 2 * W:2]                    # a slice in every dimension: four non-trivial strides
        view.copy_(deltas)
        deltas = view
        assert not cls.is_contiguous() and not deltas.is_contiguous() and deltas.stride(3) == 2
    return cls, deltas


def _check_decode(c, boxes, scores, softmax_pairs):
    args = (c['cls'], c['deltas'], c['im_info'], c['base'], c['stride'], c['min_size'], c['h'], c['w'], softmax_pairs)
    wb, ws = TC.decode_expected(*args)
    gb, gs = _np(boxes), _np(scores)
    assert gb.shape == wb.shape and gs.shape == ws.shape
    assert np.array_equal(gb, wb), (c['name'], np.argwhere(gb != wb)[:8])
    inf = np.isneginf(ws)
    assert np.array_equal(np.isneginf(gs), inf), c['name']
    rel = lambda want: float((np.abs(gs[~inf].astype(np.float64) - want[~inf]) / want[~inf]).max()) if (~inf).any() else 0.0
    worst, note = 0.0, ''
    if not softmax_pairs:
        assert np.array_equal(gs[~inf], ws[~inf].astype(F32)), c['name']
    elif c['score_grid'] is None:                                          # (see SOFTMAX_RTOL)
        worst = rel(TC.decode_expected(*args, f32_gap=True)[1])
        note = '  (%.2f x 2^-23 from the float64 softmax of the unrounded differences)' % (rel(ws) * 2 ** 23)
    else:
        worst = rel(ws)
    print('%s softmax_pairs=%d: n %d  -inf per image %s  largest softmax relative error %.3g = %.2f x 2^-23%s' %
          (c['name'], softmax_pairs, c['n'], inf.sum(1).tolist(), worst, worst * 2 ** 23, note))
    assert worst <= SOFTMAX_RTOL, (c['name'], worst * 2 ** 23)


@pytest.mark.parametrize('softmax_pairs', [False, True])
@pytest.mark.parametrize('name', sorted(TC.DECODE_CASES))
def test_proposal_decode_edges(rn, name, softmax_pairs):
    ops, _, _ = rn
    c = TC.decode_case(name)
    cls, deltas = _decode_operands(c)
    boxes, scores = ops.proposal_decode(cls, deltas, _dev(c['im_info']), _dev(c['base']), c['stride'], c['min_size'], im_hw=c['im_hw'],
                                        softmax_pairs=softmax_pairs)
    _check_decode(c, boxes, scores, softmax_pairs)


@pytest.mark.parametrize('name,softmax_pairs', [('strided_cropped', True), ('all_filtered', False)])
def test_proposal_decode_writes_every_word(rn, name, softmax_pairs):
    ops, _, lib = rn
    c = TC.decode_case(name)
    cls, deltas = _decode_operands(c)
    boxes, scores = _nan(c['B'], c['n'], 4), _nan(c['B'], c['n'])
    info, base = _dev(c['im_info']), _dev(c['base'])
    st = lambda t: (ctypes.c_long * 4)(*t.stride())
    lib.call('relnet_proposal_decode', cls.data_ptr(), st(cls), deltas.data_ptr(), st(deltas), info.data_ptr(), base.data_ptr(),
             boxes.data_ptr(), scores.data_ptr(), c['B'], c['A'], c['h'], c['w'], c['stride'], c['min_size'], int(softmax_pairs), ops._stream())
    torch.cuda.synchronize()
    assert not torch.isnan(boxes).any() and not torch.isnan(scores).any()
    _check_decode(c, boxes, scores, softmax_pairs)


def test_propose_batch_on_the_cropped_grid(rn):
    """operator_py.proposal.propose_batch on the `cropped` case (h = 9, w = 17 of a 13 x 21 map, min_size 8) against oracle.proposal.proposal:
    order and sorted rows bit-equal, the kept rows bit-equal, the pad rows members of the kept set."""
    _, _, _ = rn
    from relnet_amd.operator_py import proposal as P
    c = TC.decode_case('cropped')
    pre, post = 200, 20
    rois_o, scores_o, dbg = OP.proposal(c['cls'], c['deltas'], c['im_info'], c['stride'], c['scales'], c['ratios'], pre, post, 0.7, c['min_size'],
                                        return_debug=True, rng=np.random.RandomState(0))
    assert len(dbg['order']) == pre and dbg['order'].max() < c['n']
    rois, scores, d = P.propose_batch(_dev(c['cls']), _dev(c['deltas']), _dev(c['im_info']), _dev(c['base']), c['stride'], pre, post, 0.7,
                                      c['min_size'], want_debug=True, im_hw=c['im_hw'])
    assert np.array_equal(_np(d['order'][0]), dbg['order'])
    assert np.array_equal(_np(d['det'][0]), dbg['det'])
    nk = min(int(d['num_keep'][0]), post)
    want_k = min(dbg['n_kept'], post)
    print('cropped: %d candidates, %d sorted, %d kept of %d rows' % (c['n'], pre, dbg['n_kept'], post))
    assert nk == want_k
    assert np.array_equal(_np(d['keep'][0])[:nk], dbg['keep'][:nk])
    got = _np(rois[0])
    assert (got[:, 0] == 0).all() and np.array_equal(got[:nk], rois_o[:nk])
    assert np.array_equal(_np(scores[0])[:nk], scores_o[:nk, 0])
    kept = {tuple(x) for x in got[:nk]}
    assert all(tuple(x) in kept for x in got[nk:])


# =====================================================================================================================
# rejections: a RelnetError, and no kernel runs
# =====================================================================================================================
def test_rejected_shapes(rn):
    ops, _, lib = rn
    z = lambda *s: torch.zeros(s, device='cuda')
    zi = lambda n: torch.zeros(n, device='cuda', dtype=torch.int32)
    with pytest.raises(lib.RelnetError):                                    # OHEM: 2049 keys do not fit the 2048 of LDS
        ops.box_annotator_ohem(z(1, 2049, 2), z(1, 2049, 4), z(1, 2049), z(1, 2049, 4), z(1, 2049, 4), 128)
    with pytest.raises(lib.RelnetError):                                    # nms_multi_target: first_n 257
        ops.nms_multi_target(z(1, 257, 1, 4), z(1, 2, 5), z(1, 257, 1), zi(1))
    with pytest.raises(lib.RelnetError):                                    # 129 gt slots
        ops.nms_multi_target(z(1, 8, 1, 4), z(1, 129, 5), z(1, 8, 1), zi(1))
    with pytest.raises(lib.RelnetError):                                    # 9 thresholds
        ops.nms_multi_target(z(1, 8, 1, 4), z(1, 2, 5), z(1, 8, 1), zi(1), target_thresh=tuple(0.1 * k for k in range(1, 10)))
    with pytest.raises(lib.RelnetError):                                    # assign_anchor: 33 base anchors
        ops.assign_anchor(z(1, 2, 5), zi(1), torch.tensor([[64., 64., 1.]]).cuda(), np.zeros((33, 4)), (2, 2))
    with pytest.raises(lib.RelnetError):                                    # decode: h w A = 65536 (the 16-bit index of the top-K keys)
        ops.proposal_decode(z(1, 2, 256, 256), z(1, 4, 256, 256), torch.tensor([[4096., 4096., 1.]]).cuda(),
                            torch.zeros((1, 4), dtype=torch.float64).cuda(), 16, 0, im_hw=(4096, 4096))
    torch.cuda.synchronize()
