"""The proposal order past 8192 candidates on the device (relnet_topk_sort_large: 8192-anchor ranges sorted in LDS, then every key's
rank across the ranges), from the kernel up to tester.generate_proposals at TEST.PROPOSAL_PRE_NMS_TOP_N 20000 ->
PROPOSAL_POST_NMS_TOP_N 2000.  Every comparison is exact: the composite key (score, index) is a total order, so the result is unique
and the oracle's `argsort_desc` fixes every bit.  The cases are those of tests/proposal_large_cases.py
(tests/test_proposal_large_cases_host.py asserts they have their edges)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proposal_large_cases as PL  # noqa: E402

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


# ---- 1. order and cut ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,K', sorted(PL.TOPK_CASES))
def test_topk_sort_past_the_lds_capacity(rn, n, K):
    ops, _, _ = rn
    scores, boxes, fams = PL.topk_case(n, K)
    det, index, count = ops.topk_sort(_dev(scores), _dev(boxes), K)
    det, index, count = det.cpu().numpy(), index.cpu().numpy(), count.cpu().numpy()
    assert index.shape == (2, K) and det.shape == (2, K, 5)
    for b in range(2):
        want = PL.reference_order(scores[b], K)
        assert np.array_equal(index[b], want), (fams[b], np.flatnonzero(index[b] != want)[:8])
        assert count[b] == int(np.isfinite(scores[b][want]).sum())
        assert np.array_equal(det[b, :, :4], boxes[b][want]) and np.array_equal(det[b, :, 4], scores[b][want])


# ---- 2. the new entry against the old one where both run -------------------------------------------------------------------------
@pytest.mark.parametrize('n,K', PL.SMALL_K_SHAPES)
def test_large_entry_equals_the_lds_entry(rn, n, K):
    ops, _, _ = rn
    scores, boxes = PL.small_k_case(n, K)
    s, bx = _dev(scores), _dev(boxes)
    old = ops.topk_sort(s, bx, K)
    new = ops.topk_sort_large(s, bx, K)
    for a, b, name in zip(old, new, ('det', 'index', 'count')):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), name
    assert np.array_equal(old[1][0].cpu().numpy(), PL.reference_order(scores[0], min(K, n)))


# ---- 3. rejections ------------------------------------------------------------------------------------------------------------
def test_large_entry_rejections(rn):
    _, _, lib = rn
    L = lib.load()
    n = 9000
    need = L.relnet_topk_sort_large_workspace_bytes(1, n)
    assert need == 2 * 8192 * 8
    s = torch.zeros((1, 65536), device='cuda')
    bx = torch.zeros((1, 65536, 4), device='cuda')
    det = torch.full((1, n, 5), 7.0, device='cuda')
    idx = torch.full((1, n), -7, device='cuda', dtype=torch.int32)
    cnt = torch.full((1,), -7, device='cuda', dtype=torch.int32)
    ws = torch.zeros((need // 8,), device='cuda', dtype=torch.int64)

    def call(n_, K_, ws_ptr, ws_bytes):
        return L.relnet_topk_sort_large(s.data_ptr(), bx.data_ptr(), det.data_ptr(), idx.data_ptr(), cnt.data_ptr(), 1, n_, K_, ws_ptr, ws_bytes, None)

    for args, word in (((n, n + 1, ws.data_ptr(), need), b'K <= n'), ((65536, n, ws.data_ptr(), need), b'n < 65536'),
                       ((n, n, None, need), b'workspace'), ((n, n, ws.data_ptr(), need - 8), b'workspace'), ((n, 0, ws.data_ptr(), need), b'0 < K')):
        assert call(*args) != 0 and word in L.relnet_last_error(), (args, L.relnet_last_error())
    with pytest.raises(lib.RelnetError):
        lib.call('relnet_topk_sort_large', s.data_ptr(), bx.data_ptr(), det.data_ptr(), idx.data_ptr(), cnt.data_ptr(), 1, n, n + 1,
                 ws.data_ptr(), need, None)
    torch.cuda.synchronize()
    assert bool((det == 7.0).all()) and bool((idx == -7).all()) and int(cnt[0]) == -7 and int(ws.abs().sum()) == 0     # nothing ran
    assert call(n, n, ws.data_ptr(), need) == 0                            # and the same operands at a valid shape do
    torch.cuda.synchronize()
    assert int(cnt[0]) == n and sorted(idx[0].cpu().tolist()) == list(range(n))


# ---- 4. the whole operator, 5. the fused NMS at 20000 -> 2000 ----------------------------------------------------------------------
@pytest.fixture(scope='module')
def rpn_inputs():
    cs = [PL.tied_rpn_case(seed) for seed in PL.RPN_SEEDS]
    return tuple(_dev(np.concatenate([c[k] for c in cs])) for k in range(3))


@pytest.mark.parametrize('setting', PL.RPN_SETTINGS)
def test_proposal_operator_at_proposal_values(rn, rpn_inputs, setting):
    ops, _, _ = rn
    from relnet_amd.operator_py import proposal as P
    pre, post, thresh, min_size = setting
    anchors = _dev(P.generate_anchors(16, PL.RPN_CFG['ratios'], PL.RPN_CFG['scales']))
    rois, scores, d = P.propose_batch(*rpn_inputs, anchors, 16, pre, post, thresh, min_size, want_debug=True)
    assert rois.shape == (2, post, 5) and d['det'].shape == (2, pre, 5)
    for b, seed in enumerate(PL.RPN_SEEDS):
        rois_o, scores_o, dbg = PL.rpn_oracle(seed, setting)
        det_o, m = dbg['det'], len(dbg['det'])                             # the oracle drops the min_size rows, the device sorts them last as -inf
        det = d['det'][b].cpu().numpy()
        print('%s image %d: %d finite rows of %d, %d kept' % (setting, b, m, pre, dbg['n_kept']))
        assert np.array_equal(d['order'][b].cpu().numpy()[:m], dbg['order'])
        assert np.array_equal(det[:m], det_o) and (det[m:, 4] == -np.inf).all()
        nk = int(d['num_keep'][b])
        assert nk == min(dbg['n_kept'], post)
        assert np.array_equal(d['keep'][b].cpu().numpy()[:nk], dbg['keep'][:nk])
        got, got_s = rois[b].cpu().numpy(), scores[b].cpu().numpy()
        assert (got[:, 0] == b).all()
        assert np.array_equal(got[:nk, 1:], rois_o[:nk, 1:]) and np.array_equal(got_s[:nk], scores_o[:nk, 0])
        kept = {tuple(x) for x in got[:nk]}                                # rows from num_keep up: the cyclic padding repeats kept rows
        assert all(tuple(x) in kept for x in got[nk:])
        if nk < post:
            assert np.array_equal(got[nk:], got[np.arange(nk, post) % nk]) and np.array_equal(got_s[nk:], got_s[np.arange(nk, post) % nk])


def test_fused_nms_equals_mask_and_scan_at_20000(rn, rpn_inputs):
    ops, _, _ = rn
    from relnet_amd.operator_py import proposal as P
    anchors = _dev(P.generate_anchors(16, PL.RPN_CFG['ratios'], PL.RPN_CFG['scales']))
    for thresh, min_size in ((0.7, 0), (0.3, 16)):
        boxes, scores = ops.proposal_decode(rpn_inputs[0], rpn_inputs[1], rpn_inputs[2], anchors, 16, min_size)
        det, _, count = ops.topk_sort(scores, boxes, 20000)
        assert det.shape == (2, 20000, 5)
        a = ops.nms_greedy(det, thresh, 2000, counts=count, want_keep=True)
        b = ops.nms_sorted(det, thresh, post=2000, counts=count, want_keep=True)
        for k in ('rois', 'scores', 'num_keep'):
            assert torch.equal(a[k], b[k]), (thresh, k)
        for i in range(2):
            nk = int(a['num_keep'][i])
            assert torch.equal(a['keep'][i, :nk], b['keep'][i, :nk])


# ---- 6. the CustomOp ------------------------------------------------------------------------------------------------------------
def test_custom_op_at_proposal_values(rn):
    _, operator_py, _ = rn
    from relnet_amd.operator_py import proposal as P
    c = PL.tied_rpn_case(PL.RPN_SEEDS[0])
    prop = operator_py.get_prop('proposal')(feat_stride='16', scales='(4, 8, 16, 32)', ratios='(0.5, 1, 2)', output_score='True',
                                            rpn_pre_nms_top_n='20000', rpn_post_nms_top_n='2000', threshold='0.7', rpn_min_size='0')
    _, out_shapes = prop.infer_shape([c[0].shape, c[1].shape, c[2].shape])
    assert [tuple(s) for s in out_shapes] == [(2000, 5), (2000, 1)]
    op = prop.create_operator(None, None, None)
    ins = [_dev(x) for x in c]
    outs = [torch.empty(s, device='cuda') for s in out_shapes]
    op.forward(False, ['write', 'write'], ins, outs, [])
    anchors = _dev(P.generate_anchors(16, PL.RPN_CFG['ratios'], PL.RPN_CFG['scales']))
    rois, scores = P.propose_batch(ins[0], ins[1], ins[2], anchors, 16, 20000, 2000, 0.7, 0)
    assert torch.equal(outs[0], rois[0]) and torch.equal(outs[1], scores[0].reshape(-1, 1))
    assert np.array_equal(outs[0].cpu().numpy()[:, 1:], PL.rpn_oracle(PL.RPN_SEEDS[0], PL.RPN_SETTINGS[0])[0][:, 1:])


# ---- 7. the public function ------------------------------------------------------------------------------------------------------
def test_generate_proposals_with_proposal_settings(tmp_path):
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, detector, config as C
    from relnet_amd.dataset import loader as LD, tester as TS
    from test_dataset import make_dataset
    db = make_dataset(str(tmp_path), n_images=2, degenerate=False)         # 140 x 210 and 200 x 150: one batch, padded to 432 x 432
    roidb = db.gt_roidb()
    cfg = C.experiment('rcnn_end2end_relation_8epoch')
    cfg.SCALES[0] = (432, 432)
    p = backbone.init_params(seed=2, num_classes=db.num_classes)
    p['rpn_cls_score_weight'] = p['rpn_cls_score_weight'] * 1e-3           # a random-init RPN saturates its softmax: scores of exactly 0 would be cut by `score > thresh`
    dcfg = detector.Config()
    dcfg.num_classes, dcfg.rpn_post_nms_top_n, dcfg.rpn_min_size = db.num_classes, 60, 8
    dcfg.proposal_pre_nms_top_n, dcfg.proposal_post_nms_top_n = 20000, 2000                         # pre clamps to the 27 x 27 x 12 = 8748 anchors
    dcfg.proposal_nms_thresh, dcfg.proposal_min_size = 0.7, 0
    det = detector.Detector(p, dtype=torch.bfloat16, cfg=dcfg, im_hw=(432, 432))

    def loader():
        return LD.TestLoader(roidb, cfg, batch_size=2, has_rpn=True)
    batch = next(iter(loader()))
    assert tuple(batch['data'].shape[2:]) == (432, 432) and (432 // 16) ** 2 * 12 == 8748 > 8192
    boxes = TS.generate_proposals(det, loader(), db, proposal_settings=True)
    assert len(boxes) == db.num_images == 2 and os.path.exists(db.rpn_file())
    for i, b in enumerate(boxes):
        assert b.shape == (2000, 5) and b.dtype == np.float32
        assert b[0, 4] == b[:, 4].max() and b[:, 2].max() <= roidb[i]['width'] + 0.5                # best score first; original-image coordinates
    pkl = db.load_rpn_data()
    assert all(np.array_equal(a, b) for a, b in zip(pkl, boxes))
    dev_boxes, ev = TS.generate_proposals(det, loader(), db, proposal_settings=True, device_recall=True)
    assert len(dev_boxes) == 2 and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(boxes, dev_boxes))
    assert ev.summarize()[0].startswith('percentage of 0-25')
    plain = TS.generate_proposals(det, loader(), db, save=False)            # proposal_settings=False: the detector's rpn_* values, as before
    assert all(b.shape == (60, 5) for b in plain)


# ---- 8. capture --------------------------------------------------------------------------------------------------------------
def test_topk_sort_large_is_capturable(rn):
    ops, _, _ = rn
    n, K = 28728, 20000
    scores, boxes, _ = PL.topk_case(n, K)
    s, bx = _dev(scores), _dev(boxes)
    eager = [t.clone() for t in ops.topk_sort(s, bx, K)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                               # one stream, two kernels in order: no parallel branches
        out = ops.topk_sort(s, bx, K)
    for _ in range(2):
        for t in out:
            t.fill_(-3)
        g.replay()
        torch.cuda.synchronize()
        for a, b, name in zip(eager, out, ('det', 'index', 'count')):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), name
