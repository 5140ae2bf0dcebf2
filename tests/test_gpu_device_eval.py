"""COCO bbox evaluation on the device (dataset/device_eval.py, csrc/cocoeval.hip) against the numpy evaluator and the reference
run's own pycocotools output: precision and recall arrays bit for bit (np.array_equal), the 12 statistics exactly."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
from test_dataset import make_dataset  # noqa: E402

import relnet_amd  # noqa: F401,E402
from relnet_amd.dataset import cocoeval, device_eval as DE  # noqa: E402
from eval_edge_cases import synthetic_problem as _problem  # noqa: E402  (shared with the edge suite)

pytestmark = pytest.mark.gpu


def _host(gts, dts, img_ids=None, cat_ids=None):
    ev = cocoeval.COCOeval(gts, dts, img_ids, cat_ids)
    ev.evaluate(); ev.accumulate(); ev.summarize()
    return ev


def _device(gts, dts, img_ids=None, cat_ids=None):
    ev = DE.DeviceCOCOeval.from_lists(gts, dts, img_ids, cat_ids)
    ev.accumulate(); ev.summarize()
    return ev


def _same(a, b):
    assert a.eval['precision'].dtype == b.eval['precision'].dtype == np.float64
    assert a.eval['precision'].shape == b.eval['precision'].shape and a.eval['recall'].shape == b.eval['recall'].shape
    assert a.eval['counts'] == b.eval['counts']
    dp = np.argwhere(a.eval['precision'] != b.eval['precision'])
    assert np.array_equal(a.eval['precision'], b.eval['precision']), ('precision differs at', dp[:5])
    assert np.array_equal(a.eval['recall'], b.eval['recall']), ('recall differs at', np.argwhere(a.eval['recall'] != b.eval['recall'])[:5])
    assert np.array_equal(np.asarray(a.stats), np.asarray(b.stats)), (a.stats, b.stats)


def test_golden_case_equals_reference_pycocotools_and_cocoeval():
    import cases
    g = np.load(os.path.join(HERE, 'golden', 'cocoeval.npz'))
    gts, dts = cases.cocoeval_case()
    dev, host = _device(gts, dts), _host(gts, dts)
    assert np.array_equal(dev.eval['precision'], g['precision']) and np.array_equal(dev.eval['recall'], g['recall'])
    assert np.array_equal(dev.stats, g['stats'])
    _same(dev, host)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_synthetic_problems_equal_cocoeval(seed):
    gts, dts, img_ids, cats = _problem(seed)
    host = _host(gts, dts, img_ids, cats)
    dev = _device(gts, dts, img_ids, cats)
    _same(dev, host)
    p = dev.eval['precision']
    assert (p[:, :, cats.index(11)] == -1).all() and (p[:, :, cats.index(13)] == -1).all()    # npig == 0
    assert (p[:, :, cats.index(9), 0] == 0).all() and (dev.eval['recall'][:, cats.index(9), 0] == 0).all()
    assert (p[:, :, cats.index(2), 0, 2] > 0).any()
    per = {}
    for d in dts:
        per[(d['image_id'], d['category_id'])] = per.get((d['image_id'], d['category_id']), 0) + 1
    assert max(per.values()) >= 150 and max(sum(1 for g in gts if g['image_id'] == i) for i in img_ids) >= 300
    assert len(set(d['score'] for d in dts)) < len(dts) // 10                                 # ties everywhere


def test_one_image_equals_cocoeval():
    gts, dts, img_ids, cats = _problem(4)
    for img in (img_ids[2], img_ids[4]):                       # 150 detections in one category; 300 ground-truth boxes
        g1 = [g for g in gts if g['image_id'] == img]
        d1 = [d for d in dts if d['image_id'] == img]
        _same(_device(g1, d1, [img], cats), _host(g1, d1, [img], cats))
        _same(_device(g1, d1), _host(g1, d1))                  # ids taken from the lists


def test_nan_and_signed_zero_scores_order_like_numpy():
    """numpy's argsort(-scores, kind='mergesort') puts NaN after every number and ties -0.0 with 0.0."""
    gts, dts, img_ids, cats = _problem(6)
    rng = np.random.default_rng(11)
    for d in dts:
        r = rng.random()
        if r < 0.08:
            d['score'] = float('nan')
        elif r < 0.12:
            d['score'] = -0.0
        elif r < 0.16:
            d['score'] = 0.0
    host = _host(gts, dts, img_ids, cats)
    _same(_device(gts, dts, img_ids, cats), host)
    assert (host.eval['precision'] > 0).any()


def test_float32_xyxy_detections_are_scored_like_results_list():
    """The imdb form: float64 rows rounded to float32, boxes (x1, y1, x2, y2) with w = x2 - x1 + 1, class -> category table."""
    gts, dts, img_ids, cats = _problem(5, n_images=12)
    rng = np.random.default_rng(9)
    rows = [[] for _ in img_ids]
    for d in dts:
        x, y, w, h = d['bbox']
        rows[img_ids.index(d['image_id'])].append([cats.index(d['category_id']) + 1, d['score'] + rng.normal(0, 1e-3),
                                                   x, y, x + w - 1, y + h - 1])
    S = max(len(r) for r in rows)
    det = np.zeros((len(img_ids), S, 6))
    for k, r in enumerate(rows):
        if r:
            det[k, :len(r)] = r
    num = np.array([len(r) for r in rows], np.int32)
    # the host side exactly as pred_eval + results_list see it
    d32 = det.astype(np.float32).astype(np.float64)
    hdts = []
    for k, img in enumerate(img_ids):
        for c in range(1, len(cats) + 1):
            sel = d32[k, :num[k]][d32[k, :num[k], 0] == c]
            for r in sel:
                hdts.append(dict(image_id=img, category_id=cats[c - 1], score=float(r[1]),
                                 bbox=[float(r[2]), float(r[3]), float(r[4] - r[2] + 1), float(r[5] - r[3] + 1)]))
    host = _host(gts, hdts, img_ids, cats)
    ev = DE.DeviceCOCOeval.from_lists(gts, [], img_ids, cats, slots=S)
    ev.round_f32, ev.box_xywh = True, False
    ev.class_to_cat = torch.as_tensor(np.arange(-1, len(cats), dtype=np.int32)).cuda()
    ev.add(torch.as_tensor(det).cuda(), torch.as_tensor(num).cuda(), np.arange(len(img_ids)))
    ev.accumulate(); ev.summarize()
    _same(ev, host)


def test_add_captured_in_a_graph_and_added_twice():
    gts, dts, img_ids, cats = _problem(3, n_images=16)
    want = _device(gts, dts, img_ids, cats)
    det, num = DE.pack_detections(dts, img_ids, cats)
    det_d, num_d = torch.as_tensor(det).cuda(), torch.as_tensor(num).cuda()
    pos_d = torch.arange(len(img_ids), dtype=torch.int32, device='cuda')
    # twice, after garbage for the same images: every slot of an added image is rewritten
    ev = DE.DeviceCOCOeval.from_lists(gts, [], img_ids, cats, slots=det.shape[1])
    junk = det_d.clone()
    junk[:, :, 1] = 0.5
    junk[:, :, 2:4] += 7.0
    ev.add(junk, torch.full_like(num_d, det.shape[1]), pos_d)
    ev.add(det_d, num_d, pos_d)
    ev.add(det_d, num_d, pos_d)
    ev.accumulate(); ev.summarize()
    _same(ev, want)
    # captured, replayed twice
    ev = DE.DeviceCOCOeval.from_lists(gts, [], img_ids, cats, slots=det.shape[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev.add(junk, num_d, pos_d)                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev.add(det_d, num_d, pos_d)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    ev.accumulate(); ev.summarize()
    _same(ev, want)


class _Replay(object):
    """Runs the detector once per batch and hands back cloned outputs on the second pass, so both evaluation paths see the
    same detections whether or not two forward passes agree bit for bit."""

    def __init__(self, det):
        self.det, self.outs, self.replay, self.k = det, [], False, 0

    def __setattr__(self, name, value):
        if name == 'im_hw':
            self.det.im_hw = value
        else:
            object.__setattr__(self, name, value)

    def forward(self, *a, **kw):
        if self.replay:
            self.k += 1
            return self.outs[self.k - 1]
        out = self.det.forward(*a, **kw)
        self.outs.append({k: out[k].clone() for k in ('detections', 'num_detections')})
        return out


def _both_ways(db, det, make_loader):
    import relnet_amd.dataset.tester as TS
    rp = _Replay(det)
    res_file = os.path.join(db.result_path, 'results', 'detections_val2014_results.json')
    pkl = os.path.join(db.result_path, db.name + '_detections.pkl')
    info0, stats0, boxes0 = TS.pred_eval(rp, make_loader(), db)
    j0, p0 = open(res_file, 'rb').read(), open(pkl, 'rb').read()
    os.remove(res_file); os.remove(pkl)
    rp.replay = True
    info1, stats1, boxes1 = TS.pred_eval(rp, make_loader(), db, device_eval=True)
    assert rp.k == len(rp.outs) > 0
    j1, p1 = open(res_file, 'rb').read(), open(pkl, 'rb').read()
    assert info1 == info0 and np.array_equal(stats1, stats0)
    assert j1 == j0 and p1 == p0
    for c in range(db.num_classes):
        for i in range(db.num_images):
            assert boxes1[c][i].dtype == boxes0[c][i].dtype and np.array_equal(boxes1[c][i], boxes0[c][i])
    n = len(json.loads(j0))
    assert n > 0 and (stats0 >= -1).all()
    return n


def test_pred_eval_device_equals_default_detector(tmp_path):
    from relnet_amd import backbone, detector, config as C
    from relnet_amd.dataset import loader as LD
    db = make_dataset(str(tmp_path), n_images=8, degenerate=False)
    roidb = db.gt_roidb()
    cfg = C.experiment('rcnn_end2end_relation_8epoch')
    cfg.SCALES[0] = (128, 192)
    p = backbone.init_params(seed=2, num_classes=db.num_classes)
    g = torch.Generator().manual_seed(3)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    dcfg = detector.Config()
    dcfg.num_classes, dcfg.rpn_post_nms_top_n, dcfg.rpn_min_size = db.num_classes, 60, 8
    det = detector.Detector(p, dtype=torch.bfloat16, cfg=dcfg, im_hw=(128, 192))
    _both_ways(db, det, lambda: LD.TestLoader(roidb, cfg, batch_size=2, has_rpn=True))


def test_pred_eval_device_equals_default_fpn_detector(tmp_path):
    from relnet_amd import backbone, detector, config as C
    from relnet_amd.dataset import loader as LD
    db = make_dataset(str(tmp_path), n_images=6, degenerate=False)
    gt = db.gt_roidb()
    rng = np.random.default_rng(4)
    props = []
    for r in gt:
        n = 40
        x1 = rng.uniform(0, r['width'] - 40, n); y1 = rng.uniform(0, r['height'] - 40, n)
        props.append(np.stack([x1, y1, x1 + rng.uniform(10, 39, n), y1 + rng.uniform(10, 39, n), rng.uniform(0, 1, n)], 1).astype(np.float32))
    from oracle import boxes as OB
    roidb = db.create_roidb_from_box_list(props, gt, overlaps_fn=OB.bbox_overlaps)
    fcfg = C.experiment('rcnn_fpn_relation_learn_nms_8epoch')
    fcfg.SCALES[0] = (128, 192)
    p = backbone.init_params(seed=6, fpn=True, num_classes=db.num_classes)
    g = torch.Generator().manual_seed(7)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    dcfg = detector.Config()
    dcfg.num_classes = db.num_classes
    det = detector.FPNDetector(p, dtype=torch.bfloat16, cfg=dcfg)
    _both_ways(db, det, lambda: LD.TestLoader(roidb, fcfg, batch_size=3, has_rpn=False))
