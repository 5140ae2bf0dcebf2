"""Class-specific box regression (CLASS_AGNOSTIC false) on the device: relnet_detect_head_cs, relnet_class_nms_cs /
relnet_class_nms_topk_cs, relnet_lnms_prepare_cs / relnet_lnms_sort_cs, the detectors, the learn-NMS head and the trainers with
`class_agnostic = False`, against the oracle, the reference's own output (tests/golden/class_specific.npz) and -- bit for bit -- the
class-agnostic kernels handed one class's columns.  Every test calls an entry point or a flag that the class-agnostic code base
does not have."""
import os

import numpy as np
import pytest
import torch

import cases
import class_specific_cases as CS
from oracle import postprocess as OPP
from oracle import targets as OTG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib, backbone, detector, learn_nms, operator_py, train
    lib.load()

    class M(object):
        pass
    m = M()
    m.ops, m.lib, m.backbone, m.detector, m.learn_nms, m.operator_py, m.train = ops, lib, backbone, detector, learn_nms, operator_py, train
    return m


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'class_specific.npz'))


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


IM_INFO = np.array([[600, 1000, 1.5], [600, 1000, 1.0]], np.float32)


def _head_inputs(B, N, C, seed, sigma):
    rng = np.random.default_rng(seed)
    rois = np.stack([np.hstack((np.full((N, 1), b, np.float32), cases.random_boxes(N, seed + 10 + b))) for b in range(B)])
    cls_score = rng.normal(0, 2.5, (B, N, C)).astype(np.float32)
    deltas = rng.normal(0, sigma, (B, N, 4 * C)).astype(np.float32)
    return rois, cls_score, deltas


# ---------------------------------------------------------------------------------------------------------------------
# relnet_detect_head_cs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 65])
@pytest.mark.parametrize('C', [2, 3, 64, 65, 81])           # 64 / 65: one class per lane, then the second trip of the lane loop
def test_detect_head_cs(rn, N, C):
    ops = rn.ops
    B = 2
    rois, cls_score, deltas = _head_inputs(B, N, C, 100 + C, 0.5)
    nv = np.array([N, N - 1], np.int32)
    args = (_d(cls_score.reshape(B * N, C)), _d(deltas.reshape(B * N, 4 * C)), _d(rois.reshape(B * N, 5)), _d(IM_INFO), N)
    prob, boxes = ops.detect_head(*args, n_valid=_d(nv), class_agnostic=False)
    assert boxes.shape == (B * N, C, 4) and boxes.dtype == torch.float64
    prob, boxes = _np(prob).reshape(B, N, C), _np(boxes).reshape(B, N, 4 * C)
    clipped = 0
    for b in range(B):
        k = nv[b]
        assert not prob[b, k:].any() and not boxes[b, k:].any()             # padding rows: zeros for all C boxes
        if k == 0:
            continue
        want_prob = OPP.softmax_rows(cls_score[b, :k])
        np.testing.assert_allclose(prob[b, :k], want_prob, rtol=2e-6, atol=1e-9)
        _, want = OPP.im_detect(rois[b, :k], want_prob, deltas[b, :k], IM_INFO[b])
        assert want.shape == (k, 4 * C)
        np.testing.assert_allclose(boxes[b, :k], want, rtol=1e-12, atol=1e-9)
        clipped += (want == 0).sum()
    assert N == 1 or clipped > 0.02 * boxes.size                             # a sizeable share of the boxes reaches the border
    # class j == the class-agnostic kernel handed that class's four columns, bit for bit
    for j in range(C):
        pj, bj = ops.detect_head(*args, delta_off=4 * j, n_valid=_d(nv))
        assert np.array_equal(_np(bj).reshape(B, N, 4), boxes[:, :, 4 * j:4 * j + 4]), j
    assert np.array_equal(_np(pj).reshape(B, N, C), prob)


def test_detect_head_cs_refuses_a_narrow_bbox_pred(rn):
    rois, cls_score, deltas = _head_inputs(1, 4, 5, 7, 0.1)
    with pytest.raises(ValueError, match='class-specific'):
        rn.ops.detect_head(_d(cls_score[0]), _d(deltas[0, :, :8]), _d(rois[0]), _d(IM_INFO[:1]), 4, class_agnostic=False)


# ---------------------------------------------------------------------------------------------------------------------
# relnet_class_nms_cs / relnet_class_nms_topk_cs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [64, 65, 129, 321, 513, 1000])   # every workgroup size of class_nms_kernel (64 / 128 / 320 / 512 / 1024 threads) at its edge
def test_class_nms_cs(rn, N):
    ops = rn.ops
    B, C = 2, 4
    rois, cls_score, deltas = _head_inputs(B, N, C, 200 + N, 0.2)
    prob, boxes = ops.detect_head(_d(cls_score.reshape(B * N, C)), _d(deltas.reshape(B * N, 4 * C)), _d(rois.reshape(B * N, 5)),
                                  _d(IM_INFO), N, class_agnostic=False)
    prob, boxes = prob.view(B, N, C), boxes.view(B, N, C, 4)
    for soft, param in ((True, 0.6), (False, 0.5)):
        dets, counts, index = ops.class_nms(prob, boxes, 1e-3, param, soft, want_index=True)
        # (a) the oracle on the device's own probabilities and boxes, class j on its columns 4j..4j+3
        for b in range(B):
            raw = OPP.detections(_np(prob[b]), _np(boxes[b]).reshape(N, 4 * C), C, 1e-3, param, soft, -1, class_agnostic=False)
            for c in range(C - 1):
                k = int(counts[b, c])
                assert k == len(raw[c])
                np.testing.assert_allclose(_np(dets[b, c, :k]), raw[c], rtol=1e-10, atol=1e-12)
        out, out_count, thresh, total = ops.image_topk(dets, counts, 100)
        for b in range(B):
            want = OPP.detections(_np(prob[b]), _np(boxes[b]).reshape(N, 4 * C), C, 1e-3, param, soft, 100, class_agnostic=False)
            flat = np.concatenate([np.hstack((np.full((len(w), 1), c + 1.0), w[:, 4:5], w[:, :4])) for c, w in enumerate(want)])
            got = _np(out[b, :int(out_count[b])])
            assert got.shape == flat.shape
            np.testing.assert_allclose(got, flat.astype(np.float32), rtol=1e-6)
        # (b) every class == the single-class form of relnet_class_nms_ex on that class's scores and boxes, picks included
        for j in range(1, C):
            d1, c1, i1 = ops.class_nms(None, boxes[:, :, j].contiguous(), 1e-3, param, soft, scores64=prob[:, :, j].double().contiguous(),
                                       want_index=True)
            assert torch.equal(c1[:, 0], counts[:, j - 1]) and torch.equal(d1[:, 0], dets[:, j - 1]) and torch.equal(i1[:, 0], index[:, j - 1]), j
        # (c) the pruned lists give image_topk exactly what the full lists give it
        full, nf = ops.class_nms(prob, boxes, 1e-3, param, soft, max_picks=100)
        prn, npn = ops.class_nms(prob, boxes, 1e-3, param, soft, max_picks=100, top_k=100)
        assert (npn <= nf).all()
        for b in range(B):
            for c in range(C - 1):
                k = int(npn[b, c])
                assert torch.equal(prn[b, c, :k], full[b, c, :k]) and not prn[b, c, k:].any()
        of, cf, tf, _ = ops.image_topk(full, nf, 100)
        op, cp, tp, _ = ops.image_topk(prn, npn, 100)
        assert torch.equal(cf, cp) and torch.equal(of, op) and torch.equal(tf, tp)
    # the classes do differ: reading class 1's box for every class (the class-agnostic kernel on boxes[:, :, 1]) is another result
    agn, _ = ops.class_nms(prob, boxes[:, :, 1].contiguous(), 1e-3, 0.6, True)
    cs_, _ = ops.class_nms(prob, boxes, 1e-3, 0.6, True)
    assert torch.equal(agn[:, 0], cs_[:, 0]) and not torch.equal(agn[:, 1], cs_[:, 1])


# ---------------------------------------------------------------------------------------------------------------------
# degeneracy: where the two layouts hold the same numbers the two tails give the same bits
# ---------------------------------------------------------------------------------------------------------------------
def _lnms_params(seed=5):
    return {k: torch.as_tensor(v) for k, v in cases.learn_nms_case(8, 1, seed)[5].items()}


@pytest.mark.parametrize('C', [2, 5])
def test_class_specific_tail_degenerates_to_the_class_agnostic_tail(rn, C):
    """C == 2: bbox_pred [R, 8] IS both layouts.  C == 5: the same four deltas in every class's columns against [0 | deltas]."""
    ops = rn.ops
    B, N = 2, 150
    rois, cls_score, deltas = _head_inputs(B, N, 2, 300 + C, 0.2)
    cls_score = np.random.default_rng(301).normal(0, 2.5, (B, N, C)).astype(np.float32)
    d4 = deltas[:, :, 4:8]
    agn_bp = np.concatenate([np.zeros_like(d4), d4], 2) if C > 2 else deltas
    cs_bp = np.tile(d4, (1, 1, C)) if C > 2 else deltas
    common = (_d(rois.reshape(B * N, 5)), _d(IM_INFO), N)
    pa, ba = ops.detect_head(_d(cls_score.reshape(B * N, C)), _d(agn_bp.reshape(B * N, -1)), *common)
    pc, bc = ops.detect_head(_d(cls_score.reshape(B * N, C)), _d(cs_bp.reshape(B * N, -1)), *common, class_agnostic=False)
    assert torch.equal(pa, pc)
    for j in range(1, C):
        assert torch.equal(bc[:, j], ba)
    pa, ba, bc = pa.view(B, N, C), ba.view(B, N, 4), bc.view(B, N, C, 4)
    da, ca = ops.class_nms(pa, ba, 1e-3, 0.6, True, max_picks=100)
    dc, cc = ops.class_nms(pa, bc, 1e-3, 0.6, True, max_picks=100)
    assert torch.equal(da, dc) and torch.equal(ca, cc)
    ta = ops.image_topk(*ops.class_nms(pa, ba, 1e-3, 0.6, True, max_picks=100, top_k=100), 100)
    tc = ops.image_topk(*ops.class_nms(pa, bc, 1e-3, 0.6, True, max_picks=100, top_k=100), 100)
    assert all(torch.equal(x, y) for x, y in zip(ta[:3], tc[:3]))
    # learn-NMS head: sorted boxes, scores and everything computed from them
    feat = _d(np.maximum(np.random.default_rng(302).normal(0, 1, (B, N, 1024)), 0).astype(np.float32))
    p = _lnms_params()
    kw = dict(first_n=40, dtype=torch.float32)
    ra = rn.learn_nms.LearnNMS(p, C - 1, **kw).forward(_d(cls_score), _d(agn_bp), _d(rois), _d(IM_INFO), feat)
    rc = rn.learn_nms.LearnNMS(p, C - 1, class_agnostic=False, **kw).forward(_d(cls_score), _d(cs_bp), _d(rois), _d(IM_INFO), feat)
    for k in ('sorted_bbox', 'sorted_score', 'nms_multi_score', 'nms_final_score', 'detections', 'num_detections'):
        assert torch.equal(ra[k], rc[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# learn-NMS head
# ---------------------------------------------------------------------------------------------------------------------
def _attr(v):
    return 'None' if v is None else str(np.array(v, dtype=float))


@pytest.mark.parametrize('name', sorted(CS.LNMS_CASES))
def test_learn_nms_class_specific_matches_reference_operator(rn, gold, name):
    n, c, first_n, seed, norm = CS.LNMS_CASES[name]
    cls_score, bbox_pred, rois, im_info, feat, p = CS.lnms_case(n, c, seed)
    means, stds = norm if norm else (None, None)
    want_multi = gold[name + '/nms_multi_score']

    def check(multi, sbox, sscore):
        # the tolerances tests/test_gpu_learn_nms.py puts on the same three outputs of the class-agnostic golden
        np.testing.assert_allclose(_np(sscore), gold[name + '/sorted_score'], rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(_np(sbox), gold[name + '/sorted_bbox'], rtol=0, atol=1e-4)
        np.testing.assert_allclose(_np(multi), want_multi, rtol=1e-3, atol=1e-5 * np.abs(want_multi).max())

    m = rn.learn_nms.LearnNMS({k: torch.as_tensor(v) for k, v in p.items()}, c, first_n, bbox_means=means, bbox_stds=stds,
                              dtype=torch.float32, class_agnostic=False)
    r = m.forward(_d(cls_score[None]), _d(bbox_pred[None]), _d(rois[None]), _d(im_info), _d(feat[None]))
    check(r['nms_multi_score'][0], r['sorted_bbox'][0], r['sorted_score'][0])
    # through the mirrored CustomOp protocol with the attribute strings MXNet hands over
    kw = dict(cls_score=_d(cls_score), bbox_pred=_d(bbox_pred), rois=_d(rois), im_info=_d(im_info), fc_all_2_relu=_d(feat))
    kw.update({k: _d(p[k]) for k in cases.LEARN_NMS_ARG_ORDER})
    multi, sbox, sscore = rn.operator_py.Custom(op_type='learn_nms', name='nms_multi_score', num_fg_classes=c, bbox_means=_attr(means),
                                                bbox_stds=_attr(stds), first_n=first_n, class_agnostic='False', num_thresh=5,
                                                class_thresh=0.01, nongt_dim=n, has_non_gt_index=False, **kw)
    check(multi, sbox, sscore)
    assert torch.equal(sbox, r['sorted_bbox'][0]) and torch.equal(sscore, r['sorted_score'][0])


def _prepare_sort(rn, cls_score, bbox_pred, rois, im_info, first_n, class_agnostic, n_valid=None, norm=None):
    """learn_nms.rank_stage (relnet_lnms_prepare* + relnet_lnms_sort*, what LearnNMS.forward and the train branch call) into poisoned prob / boxes
    -> prob, boxes, rank_idx, sorted_score, sorted_bbox, class_boxes, class_max."""
    B, N, C1 = cls_score.shape
    prob = torch.full((B, N, C1 - 1), -1.0, device=cls_score.device, dtype=torch.float32)
    boxes = torch.full((B, N, 4) if class_agnostic else (B, N, C1 - 1, 4), -1.0, device=cls_score.device, dtype=torch.float32)
    means, stds = norm if norm else (None, None)
    return rn.learn_nms.rank_stage(cls_score, bbox_pred, rois, im_info, first_n, class_agnostic, means, stds, n_valid, out=(prob, boxes))


@pytest.mark.parametrize('name', ['cs_n60_c6_f20_norm', 'cs_n120_c80_f30'])
def test_lnms_prepare_sort_cs_kernels(rn, name):
    """rank_idx, sorted_score, class_max: exactly those of the class-agnostic kernels on the same class scores (the boxes play no part in
    the ranking).  Foreground class k's boxes: exactly the class-agnostic kernel at delta_off = 4 (k + 1).  sorted_bbox / class_boxes: an
    exact gather.  Image 1 has n_valid < N: its padding rows are zero and rank behind every real roi."""
    n, c, first_n, seed, norm = CS.LNMS_CASES[name]
    ins = [CS.lnms_case(n, c, seed + b) for b in range(2)]
    cls_score, bbox_pred, rois = (_d(np.stack([i[k] for i in ins])) for k in (0, 1, 2))
    im_info = _d(np.concatenate([i[3] for i in ins]))
    nv_host = [n, n - 7]
    nv = _d(np.array(nv_host, np.int32))
    prob, boxes, idx, ss, sb, cb, cm = _prepare_sort(rn, cls_score, bbox_pred, rois, im_info, first_n, False, nv, norm)
    pa, ba, idx_a, ss_a, _, _, cm_a = _prepare_sort(rn, cls_score, bbox_pred, rois, im_info, first_n, True, nv, norm)
    assert torch.equal(prob, pa) and torch.equal(idx, idx_a) and torch.equal(ss, ss_a) and torch.equal(cm, cm_a)
    assert torch.equal(boxes[:, :, 0], ba)
    import ctypes
    for k in range(1, c):                # every foreground class against the class-agnostic kernel reading that class's columns
        bk = torch.empty_like(ba)
        pk = torch.empty_like(pa)
        cs2, bp2 = cls_score.reshape(2 * n, c + 1), bbox_pred.reshape(2 * n, -1)
        rn.lib.call('relnet_lnms_prepare_ex', cs2.data_ptr(), cs2.stride(0), bp2.data_ptr(), bp2.stride(0), rois.data_ptr(), im_info.data_ptr(),
                    pk.data_ptr(), bk.data_ptr(), 2, n, c + 1, 4 * (k + 1), None if norm is None else (ctypes.c_float * 4)(*norm[0]),
                    None if norm is None else (ctypes.c_float * 4)(*norm[1]), nv.data_ptr(), rn.ops._stream())
        assert torch.equal(boxes[:, :, k], bk), k
    for b in range(2):
        k = nv_host[b]
        assert not boxes[b, k:].any() and not prob[b, k:].any()
        ii = idx[b].long()                                                   # [C, F]
        cls_ax = torch.arange(c, device='cuda')[:, None].expand_as(ii)
        want = boxes[b][ii, cls_ax]                                          # [C, F, 4]
        assert torch.equal(cb[b], want) and torch.equal(sb[b], want.permute(1, 0, 2))
        assert (ii < k).all()
        # the host restatement on the real rows: ranks exact where the device's own probabilities are tie-free, boxes to float32 rounding
        ref = CS.refine_boxes(_np(rois[b, :k]), _np(bbox_pred[b, :k]), _np(im_info[b:b + 1]), *(norm or (None, None)))
        np.testing.assert_allclose(_np(boxes[b, :k]), ref, rtol=0, atol=1e-4)
        pr = _np(prob[b, :k])
        order = np.argsort(-pr, axis=0, kind='stable')[:first_n]
        assert np.array_equal(_np(idx[b]).T, order)


# ---------------------------------------------------------------------------------------------------------------------
# detectors
# ---------------------------------------------------------------------------------------------------------------------
def _check_detections(out, cfg, B):
    C = cfg.num_classes
    N = out['cls_prob'].shape[1]
    assert out['pred_boxes'].shape == (B, N, C, 4)
    for b in range(B):
        prob, full = _np(out['cls_prob'][b]), _np(out['pred_boxes'][b]).reshape(N, 4 * C)
        want = OPP.detections(prob, full, C, cfg.score_thresh, cfg.nms, cfg.softnms, cfg.max_per_image, class_agnostic=False)
        flat = np.concatenate([np.hstack((np.full((len(w), 1), c + 1.0), w[:, 4:5], w[:, :4])) for c, w in enumerate(want)])
        n = int(out['num_detections'][b])
        assert n == len(flat) and n > 0
        np.testing.assert_allclose(_np(out['detections'][b, :n]), flat.astype(np.float32), rtol=1e-5)
        # not the class-agnostic reading of the same head
        agn = OPP.detections(prob, full, C, cfg.score_thresh, cfg.nms, cfg.softnms, cfg.max_per_image, class_agnostic=True)
        assert any(a.shape != w.shape or not np.array_equal(a, w) for a, w in zip(agn[1:], want[1:]))


def _captured_equals_eager(rn, step, keys):
    with torch.no_grad():
        eager = {k: v.clone() for k, v in step().items() if k in keys}
        fl = rn.detector.InFlight([step])
        out = fl.result(fl.submit())
    for k in keys:
        assert torch.equal(out[k], eager[k]), k
    return out


KEYS = ('cls_prob', 'pred_boxes', 'detections', 'num_detections', 'image_thresh')


def test_detector_class_specific_eager_and_captured(rn):
    H, W, NC = 192, 256, 5
    p = rn.backbone.init_params(seed=3, num_classes=NC, num_reg_classes=NC)
    g = torch.Generator().manual_seed(5)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    p['conv_new_1_bias'] = torch.rand(256, generator=g) * 0.1 + 0.05
    data = torch.randn(2, 3, H, W, generator=g).cuda()
    im_info = torch.tensor([[H, W, 1.0], [H, W, 1.0]]).cuda()
    cfg = rn.detector.Config()
    cfg.rpn_post_nms_top_n, cfg.num_classes, cfg.class_agnostic = 100, NC, False
    det = rn.detector.Detector(p, dtype=torch.float32, im_hw=(H, W), cfg=cfg)
    out = _captured_equals_eager(rn, lambda: det.forward(data, im_info), KEYS)
    assert out['bbox_pred'].shape == (2, 100, 4 * NC)
    _check_detections(out, cfg, 2)


def test_fpn_detector_class_specific_eager_and_captured(rn):
    H, W, N, NC = 160, 224, 200, 5
    p = rn.backbone.init_params(seed=21, fpn=True, num_classes=NC, num_reg_classes=NC)
    g = torch.Generator().manual_seed(22)
    p['cls_score_weight'] = torch.randn(p['cls_score_weight'].shape, generator=g) * 0.05
    # (the x 5 pyramid features below give fc_all_2_relu entries of O(10): deltas of O(1), not exp() overflows, need a small box FC)
    p['bbox_pred_weight'] = torch.randn(p['bbox_pred_weight'].shape, generator=g) * 0.001
    for lvl in (4, 8, 16, 32):
        p['fpn_ft%d_1x1_weight' % lvl] = p['fpn_ft%d_1x1_weight' % lvl] * 5
        p['fpn_ft%d_3x3_weight' % lvl] = p['fpn_ft%d_3x3_weight' % lvl] * 5
        p['fpn_ft%d_3x3_bias' % lvl] = torch.rand(256, generator=g) * 0.1
    data = torch.randn(1, 3, H, W, generator=g).cuda()
    boxes = _d(cases.fpn_proposals(N, 23, H, W)[None])
    im_info = torch.tensor([[H, W, 1.0]]).cuda()
    cfg = rn.detector.Config()
    cfg.num_classes, cfg.class_agnostic = NC, False
    det = rn.detector.FPNDetector(p, dtype=torch.float32, cfg=cfg)
    out = _captured_equals_eager(rn, lambda: det.forward(data, boxes, im_info), KEYS)
    rows = int(out['num_rows'][0])
    assert not out['pred_boxes'][0, rows:].any() and not out['cls_prob'][0, rows:].any()      # padding rows: all C boxes zero
    assert torch.isfinite(out['pred_boxes']).all() and float(out['bbox_pred'][0, :rows].abs().max()) < 4.0
    _check_detections(out, cfg, 1)


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
def _feat_size(n):
    n = (n + 2 * 3 - 7) // 2 + 1
    n = -(-(n - 3) // 2) + 1
    n = (n - 1) // 2 + 1
    return (n - 1) // 2 + 1


def _train_setup(rn, B, NC, seed, num_reg=None, H=128, W=160, G=4):
    train = rn.train
    p = rn.backbone.init_params(seed=seed, num_classes=NC, num_reg_classes=NC if num_reg is None else num_reg)
    g = torch.Generator().manual_seed(seed + 1)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    p['conv_new_1_bias'] = torch.rand(256, generator=g) * 0.1 + 0.05
    cfg = train.TrainConfig()
    cfg.rpn_post_nms_top_n, cfg.num_classes = 40, NC
    data = torch.randn(B, 3, H, W, generator=g)
    rng = np.random.default_rng(seed + 2)
    gt = np.zeros((B, G, 5), np.float32)
    x1 = rng.uniform(0, W - 70, (B, G)); y1 = rng.uniform(0, H - 70, (B, G))
    gt[:, :, 0], gt[:, :, 1] = x1, y1
    gt[:, :, 2], gt[:, :, 3] = x1 + rng.uniform(30, 69, (B, G)), y1 + rng.uniform(30, 69, (B, G))
    gt[:, :, 4] = rng.integers(1, NC, (B, G))
    fh, fw = _feat_size(H), _feat_size(W)
    anc = [train.assign_anchor((fh, fw), gt[b], (H, W), cfg, seed=seed + b) for b in range(B)]
    batch = (data.cuda(), torch.tensor([[H, W, 1.0]] * B).cuda(), _d(gt)) + tuple(_d(np.stack([a[k] for a in anc])) for k in range(3))
    return p, cfg, batch, gt


@pytest.mark.parametrize('B', [1, 2])
def test_trainer_class_specific_targets_loss_and_head_gradients(rn, B):
    NC = 5
    p, cfg, batch, gt = _train_setup(rn, B, NC, 41)
    cfg.class_agnostic = False
    tr = rn.train.Trainer(p, cfg, im_hw=(128, 160))
    head, grabbed = tr._head_forward_backward, []
    tr._head_forward_backward = lambda *a, **k: (grabbed.append(head(*a, **k)), grabbed[-1])[1]      # fc_all_2_relu is not among the step's outputs
    out = tr.forward_backward(*batch)
    torch.cuda.synchronize()
    x2 = grabbed[0][1][0]
    N, R = cfg.rpn_post_nms_top_n, cfg.rpn_post_nms_top_n + gt.shape[1]
    assert x2.shape == (B, R, 1024)
    assert out['bbox_target'].shape == (B, R, 4 * NC) and out['bbox_pred'].shape == (B, R, 4 * NC)
    want_w, want_b, l_box = 0, 0, 0.0
    fg_classes = set()
    for b in range(B):
        # targets and weights: oracle proposal_target (bbox_regression.py:129-140 with CLASS_AGNOSTIC false) on the run's own proposals, exactly
        props = _np(out['rois'][b, :N]).copy()
        props[:, 0] = 0                                                          # (the oracle is the one-image-per-executor form)
        r, lab, bt, bw = OTG.proposal_target(props, gt[b], NC, class_agnostic=False)
        assert np.array_equal(_np(out['rois'][b, :, 1:]), r[:, 1:])
        assert np.array_equal(_np(out['bbox_target'][b]), bt)
        lo, wo = _np(out['label'][b]), _np(out['bbox_weight'][b])               # after OHEM: a subset of the rois keeps label and weights
        kept = lo >= 0
        assert np.array_equal(lo[kept], lab[kept]) and np.array_equal(wo[kept], bw[kept]) and not wo[~kept].any()
        fg_classes |= set(int(v) for v in lab[lab > 0])
        for i in np.where(lab > 0)[0]:
            assert bw[i, 4 * int(lab[i]):4 * int(lab[i]) + 4].all() and bw[i].sum() == 4
        # float64 autograd of the head losses on the run's own fc_all_2_relu, labels and weights
        pd = {k: p[k].double().clone().requires_grad_(True) for k in ('cls_score_weight', 'cls_score_bias', 'bbox_pred_weight', 'bbox_pred_bias')}
        l_cls, lb, cs, bp = CS.head_losses(x2[b].double().cpu(), pd, lo, bt, wo, cfg.batch_rois_ohem)
        (l_cls + lb).backward()
        l_box += float(lb.detach()) * cfg.batch_rois_ohem / B      # (MakeLoss: grad_scale 1 / BATCH_ROIS_OHEM is on the gradient, the output is the plain sum)
        want_w = want_w + torch.cat([pd['cls_score_weight'].grad, pd['bbox_pred_weight'].grad], 0)
        want_b = want_b + torch.cat([pd['cls_score_bias'].grad, pd['bbox_pred_bias'].grad], 0)
        # bf16 operands of a K = 1024 product: 2^-8 per operand, far below the spread of the outputs
        assert (out['bbox_pred'][b].double().cpu() - bp.detach()).abs().max() <= 2e-2 * float(bp.detach().abs().max())
    assert len(fg_classes) > 1                                                   # more than one class's columns are in use
    # bbox_loss: the smooth-L1 terms are dominated by the normalised targets (O(1)); bf16 rounding of bbox_pred (relative 2^-8 on
    # values far smaller than the targets) moves the sum by well under 2 %
    print('bbox_loss got %.6f want %.6f' % (float(out['bbox_loss']), l_box))
    assert abs(float(out['bbox_loss']) - l_box) <= 2e-2 * l_box
    # the criterion tests/test_gpu_train_step.py applies to head weight gradients (cosine >= 0.995, norm within 3 %), read as it reads them
    for name, want, got in (('cls_bbox', want_w, tr.W.view(tr.W.grad, 'cls_bbox')), ('bias:cls_bbox', want_b, tr.Bv.view(tr.Bv.grad, 'cls_bbox'))):
        got = got.cpu().double().reshape(want.shape)
        assert got.shape[0] == NC + 4 * NC
        for part, sl in (('cls', slice(0, NC)), ('bbox', slice(NC, None))):
            w_, g_ = want[sl], got[sl]
            cos = float((w_ * g_).sum() / (w_.norm() * g_.norm()))
            print('%s[%s] |want| %.3e |got| %.3e cos %.5f' % (name, part, float(w_.norm()), float(g_.norm()), cos))
            assert cos >= 0.995 and abs(float(g_.norm() / w_.norm()) - 1) <= 0.03, (name, part, cos)


def test_trainer_refuses_a_head_that_contradicts_the_flag(rn):
    p, cfg, _, _ = _train_setup(rn, 1, 5, 43, num_reg=2)
    cfg.class_agnostic = False
    with pytest.raises(ValueError, match='class_agnostic'):
        rn.train.Trainer(p, cfg, im_hw=(128, 160))
    p, cfg, _, _ = _train_setup(rn, 1, 5, 43)
    with pytest.raises(ValueError, match='class_agnostic'):
        rn.train.Trainer(p, cfg, im_hw=(128, 160))


def test_learn_nms_train_branch_class_specific(rn):
    """Trainer._lnms_forward_backward with class-specific boxes on the golden-style inputs: the per-class geometry branch is taken (not the
    per-image shortcut), sorted boxes follow the restatement, nms_multi_target is the oracle's on the device's own sorted boxes / scores,
    the multi scores follow float64 autograd of oracle/train_graph.py:learn_nms_loss, the losses are its formula on the device's own scores."""
    from oracle import train_graph as OT
    B, N, C, F, G = 2, 60, 6, 20, 4
    p = rn.backbone.init_params(seed=3, num_classes=C + 1, num_reg_classes=C + 1)
    g_ = torch.Generator().manual_seed(78)
    p['nms_logit_bias'] = torch.zeros(5)
    for k in ('nms_logit_weight', 'nms_rank_weight', 'roi_feat_embedding_weight', 'nms_query_1_weight', 'nms_key_1_weight',
              'nms_linear_out_1_weight', 'nms_pair_pos_fc1_1_weight'):
        p[k] = torch.randn(p[k].shape, generator=g_) * 0.05
    cfg = rn.train.TrainConfig()
    cfg.learn_nms, cfg.first_n, cfg.num_classes, cfg.class_agnostic = True, F, C + 1, False
    tr = rn.train.Trainer(p, cfg, im_hw=(600, 1000))
    ins = [CS.lnms_case(N, C, 90 + b) for b in range(B)]
    cls_score, bbox_pred, rois = (_d(np.stack([i[k] for i in ins])) for k in (0, 1, 2))
    im_info = _d(np.concatenate([i[3] for i in ins]))
    feat = _d(np.stack([i[4] for i in ins])).to(torch.bfloat16)
    refined = [CS.refine_boxes(i[2], i[1], i[3], cfg.bbox_means, cfg.bbox_stds) for i in ins]
    gt = np.zeros((B, G, 5), np.float32)
    for b in range(B):                       # gt boxes ON the class's own refined box of its top-scoring roi: positive targets exist
        for j in range(G):
            c = 1 + j
            gt[b, j, :4] = refined[b][np.argmax(ins[b][0][:, c]), c - 1]
            gt[b, j, 4] = c
    num_gt = torch.full((B,), G, dtype=torch.int32, device='cuda')
    called = []
    real_call = rn.lib.call
    tr.W.grad.zero_(); tr.Bv.grad.zero_()
    tr._relayout.run()
    try:
        rn.lib.call = lambda name, *a, **k: (called.append(name), real_call(name, *a, **k))[1]
        d_cls, d_feat, lo = tr._lnms_forward_backward(cls_score, bbox_pred, rois, im_info, feat, _d(gt), num_gt)
    finally:
        rn.lib.call = real_call
    tr._flush_wgrads()
    torch.cuda.synchronize()
    assert 'relnet_lnms_prepare_cs' in called and 'relnet_lnms_sort_cs' in called and 'relnet_lnms_gather_bias' not in called
    eps, k_ = cfg.nms_eps, cfg.nms_loss_scale / float(F * 5)
    pos_w = neg_w = 0.0
    names = ['nms_rank', 'roi_feat_embedding', 'nms_pair_pos_fc1_1', 'nms_logit', 'nms_query_1', 'nms_key_1', 'nms_linear_out_1']
    for b in range(B):
        idx, ss, sb = CS.sort_and_pick(ins[b][0], refined[b], F)
        assert np.array_equal(_np(lo['nms_rank_idx'][b]).T, idx)
        np.testing.assert_allclose(_np(lo['nms_class_boxes'][b]).transpose(1, 0, 2), sb, rtol=0, atol=1e-4)
        dev_sb = _np(lo['nms_class_boxes'][b]).transpose(1, 0, 2)
        want_t = OTG.nms_multi_target(dev_sb, gt[b:b + 1], _np(lo['sorted_score'][b]), cfg.nms_target_thresh)
        assert np.array_equal(_np(lo['nms_multi_target'][b]), want_t) and want_t.sum() > 0
        pd = {n + s: p[n + s].double().clone() for n in names for s in ('_weight', '_bias')}
        _, multi = OT.learn_nms_loss(torch.as_tensor(ins[b][0]).double(), feat[b].cpu().double(), pd, _np(lo['nms_rank_idx'][b]),
                                     _np(lo['nms_class_boxes'][b]), want_t, F)
        got_m = lo['nms_multi_score'][b].cpu().double()
        assert (got_m - multi).abs().max() <= 0.03 * multi.abs().max()          # the bound tests/test_gpu_learn_nms_train.py puts on it
        t = torch.as_tensor(want_t, dtype=torch.float64)
        pos_w += float(k_ * (-(t * torch.log(got_m + eps))).sum()) / B
        neg_w += float(k_ * (-((1.0 - t) * torch.log(1.0 - got_m + eps))).sum()) / B
    # float32 logs and a float32 sum of F C T = 600 terms against float64 on the same scores
    print('nms_pos_loss got %.6f want %.6f   nms_neg_loss got %.6f want %.6f' % (float(lo['nms_pos_loss']), pos_w, float(lo['nms_neg_loss']), neg_w))
    assert abs(float(lo['nms_pos_loss']) - pos_w) <= 1e-4 * pos_w and abs(float(lo['nms_neg_loss']) - neg_w) <= 1e-4 * neg_w


@pytest.mark.parametrize('learn_nms', [False, True])
def test_two_class_deterministic_step_is_the_same_in_both_layouts(rn, learn_nms):
    """num_classes == 2: [R, 8] is both layouts, so with deterministic = True the class-specific trainer's losses and every gradient are
    bit-identical to the class-agnostic trainer's (with learn-NMS: per-class geometry branch against the per-image shortcut)."""
    res = []
    for agnostic in (True, False):
        p, cfg, batch, gt = _train_setup(rn, 1, 2, 47)
        cfg.class_agnostic, cfg.deterministic, cfg.learn_nms, cfg.first_n = agnostic, True, learn_nms, 24
        tr = rn.train.Trainer(p, cfg, im_hw=(128, 160))
        out = tr.forward_backward(*batch)
        torch.cuda.synchronize()
        keys = [k for k, v in out.items() if torch.is_tensor(v) and (v.dim() == 0 or 'loss' in k or k.startswith('nms_multi'))]
        res.append(({k: out[k].clone() for k in keys}, tr.W.grad.clone(), tr.Bv.grad.clone()))
    (oa, wa, ba), (oc, wc, bc) = res
    assert 'bbox_loss' in oa and set(oa) == set(oc) and (not learn_nms or 'nms_pos_loss' in oa)
    for k in oa:
        assert torch.equal(oa[k], oc[k]), k
    assert float(wa.abs().max()) > 0 and torch.equal(wa, wc) and torch.equal(ba, bc)


def test_checkpoint_round_trip_tiles_means_and_stds_over_the_classes(rn, tmp_path):
    from relnet_amd import checkpoint as ck
    NC = 5
    p, cfg, batch, gt = _train_setup(rn, 1, NC, 49)
    cfg.class_agnostic = False
    cfg.bbox_means = (0.1, -0.1, 0.05, 0.0)                      # non-zero means so that the bias fold is visible
    tr = rn.train.Trainer(p, cfg, im_hw=(128, 160))
    prefix = str(tmp_path / 'cs')
    tr.save_checkpoint(prefix, 0)
    arg, aux = ck.load_param(prefix, 1, process=False)
    w, b = torch.as_tensor(arg['bbox_pred_weight']).double(), torch.as_tensor(arg['bbox_pred_bias']).double()
    assert w.shape == (4 * NC, 1024)
    stds = torch.tensor(list(cfg.bbox_stds) * NC, dtype=torch.float64)
    means = torch.tensor(list(cfg.bbox_means) * NC, dtype=torch.float64)
    np.testing.assert_allclose(np.asarray(arg['bbox_pred_weight_test'], np.float64), (w * stds[:, None]).numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(np.asarray(arg['bbox_pred_bias_test'], np.float64), (b * stds + means).numpy(), rtol=1e-6, atol=1e-9)
    dcfg = rn.detector.Config()
    dcfg.num_classes, dcfg.class_agnostic, dcfg.rpn_post_nms_top_n = NC, False, 40
    det = rn.detector.Detector.from_checkpoint(prefix, 1, dtype=torch.float32, cfg=dcfg, im_hw=(128, 160))
    arg_t, _ = ck.load_param(prefix, 1, process=True)
    assert np.array_equal(np.asarray(arg_t['bbox_pred_weight']), np.asarray(arg['bbox_pred_weight_test']))
    assert np.array_equal(np.asarray(arg_t['bbox_pred_bias']), np.asarray(arg['bbox_pred_bias_test']))
    out = det.forward(batch[0], batch[1])
    assert out['pred_boxes'].shape[2:] == (NC, 4) and torch.isfinite(out['pred_boxes']).all()
    dcfg.class_agnostic = True
    with pytest.raises(ValueError, match='class_agnostic'):      # the same file read as a class-agnostic head: refused, not mis-decoded
        rn.detector.Detector.from_checkpoint(prefix, 1, dtype=torch.float32, cfg=dcfg, im_hw=(128, 160))


def test_fpn_trainer_class_specific(rn):
    """FPNTrainer with class_agnostic False (given proposals, level-major rows, learn-NMS branch on the n_valid path): every row's target
    and weight are the oracle's for THAT roi ([4 * num_classes] wide, the four entries at 4 * label), the learn-NMS branch ranks
    class-specific boxes, and every gradient is finite."""
    H, W, G, N, NC, F = 128, 160, 4, 60, 5, 24
    p = rn.backbone.init_params(seed=41, fpn=True, num_classes=NC, num_reg_classes=NC)
    g = torch.Generator().manual_seed(42)
    p['cls_score_weight'] = torch.randn(p['cls_score_weight'].shape, generator=g) * 0.05
    p['bbox_pred_weight'] = torch.randn(p['bbox_pred_weight'].shape, generator=g) * 0.05
    for lvl in (4, 8, 16, 32):
        p['fpn_ft%d_1x1_weight' % lvl] = p['fpn_ft%d_1x1_weight' % lvl] * 2
        p['fpn_ft%d_3x3_weight' % lvl] = p['fpn_ft%d_3x3_weight' % lvl] * 2
        p['fpn_ft%d_3x3_bias' % lvl] = torch.rand(256, generator=g) * 0.1
    cfg = rn.train.TrainConfig()
    cfg.fpn, cfg.learn_nms, cfg.first_n, cfg.num_classes, cfg.class_agnostic = True, True, F, NC, False
    data = torch.randn(1, 3, H, W, generator=g)
    props = cases.fpn_proposals(N, 43, H, W)[6:][None]           # (the first six of the generator are sized for an 800 x 1024 canvas)
    props = np.ascontiguousarray(props)
    n = props.shape[1]
    gt = np.zeros((1, G, 5), np.float32)
    gt[0, :, :4] = props[0, [8, 17, 29, 44]]
    gt[0, :, 4] = [1, 2, 2, 4]
    tr = rn.train.FPNTrainer(p, cfg)
    out = tr.forward_backward(data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), _d(gt), _d(props))
    torch.cuda.synchronize()
    R = n + G
    assert out['bbox_target'].shape == (1, R, 4 * NC) and out['bbox_pred'].shape == (1, R, 4 * NC)
    rois, bt, bw, lab = (_np(out[k][0]) for k in ('rois', 'bbox_target', 'bbox_weight', 'label'))
    seen = set()
    for r in range(R):
        roi = rois[r:r + 1].copy(); roi[:, 0] = 0
        _, l1, t1, w1 = OTG.proposal_target(roi, gt[0], NC, class_agnostic=False)
        assert np.array_equal(bt[r], t1[0]), r
        if lab[r] >= 0:                                              # kept by OHEM
            assert lab[r] == l1[0] and np.array_equal(bw[r], w1[0]), r
            seen.add(int(l1[0]))
    assert {1, 2, 4} <= seen
    assert out['nms_class_boxes'].shape == (1, NC - 1, F, 4) and out['nms_multi_target'].shape == (1, F, NC - 1, 5)
    assert torch.isfinite(tr.W.grad).all() and torch.isfinite(tr.Bv.grad).all()
    assert float(tr.W.view(tr.W.grad, 'cls_bbox')[NC:].abs().max()) > 0
