"""Proposal recall on the device (dataset/device_recall.py, csrc/recall.hip) against the host restatement dataset/recall.py,
which tests/test_recall_host.py pins to the reference's own evaluate_recall.  Everything is np.array_equal or string-equal:
recalls, AR, num_pos, the candidate area counts, every image's recorded overlaps and the sorted gt_overlaps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_recall_host import golden_cases  # noqa: E402

pytestmark = pytest.mark.gpu

import relnet_amd  # noqa: F401,E402
from relnet_amd import lib, ops  # noqa: E402
from relnet_amd.dataset import recall as R  # noqa: E402
from relnet_amd.dataset.device_recall import DeviceRecall  # noqa: E402


def _assert_same(host, dev, with_overlaps=True):
    (hlog, h), (dlog, d) = host, dev
    assert dlog == hlog
    assert d['area_counts'] == h['area_counts'] and d['num_images'] == h['num_images']
    for hr, dr in zip(h['ranges'], d['ranges']):
        assert dr['num_pos'] == hr['num_pos'], hr['name']
        assert np.array_equal(dr['hits'], hr['hits']), hr['name']
        assert dr['recalls'].dtype == hr['recalls'].dtype
        assert np.array_equal(dr['recalls'], hr['recalls'], equal_nan=True), hr['name']
        assert np.array_equal(dr['ar'], hr['ar'], equal_nan=True), hr['name']
        if with_overlaps:
            assert np.array_equal(dr['gt_overlaps'], hr['gt_overlaps']), hr['name']
    if with_overlaps:
        assert np.array_equal(d['image_overlaps'], h['image_overlaps'])


@pytest.mark.parametrize('name', ['edges', 'thresholds', 'merged'])
def test_golden_cases(name):
    c = golden_cases()[name]
    thr = None if c['thresholds'] is None else c['thresholds'].copy()
    host = R.evaluate_recall(c['roidb'], len(c['roidb']), c['candidates'], thr)
    ev = DeviceRecall.from_lists(c['roidb'], c['candidates'], thresholds=thr, record_overlaps=True, chunk=5)
    dev = ev.summarize()
    _assert_same(host, dev)
    assert dev[0] == c['log']
    for a in range(7):
        assert np.array_equal(dev[1]['ranges'][a]['gt_overlaps'], c['sorted'][a])
    # one image per call, in reverse order: the same counts
    ev1 = DeviceRecall(c['roidb'], thresholds=thr)
    cands = [R.candidates_of(c['roidb'], i, c['candidates']) for i in range(len(c['roidb']))]
    for i in reversed(range(len(cands))):
        b = np.zeros((1, max(len(cands[i]), 1), 4), np.float32)
        b[0, :len(cands[i])] = cands[i][:, :4]
        ev1.add(torch.as_tensor(b).cuda(), torch.tensor([len(cands[i])], dtype=torch.int32).cuda(), torch.tensor([i]).cuda())
    _assert_same(host, ev1.summarize(), with_overlaps=False)


def _random_case(seed, n_images, P, max_gt):
    """uint16 gt (coco dtype, some areas above 65535) and float32 proposals that are jittered copies of the gts on a 0.5 grid,
    so that high overlaps tie often; raw boxes at the network scale, scores and the image scales."""
    rng = np.random.default_rng(seed)
    roidb, raw, scores, scales = [], [], [], []
    for i in range(n_images):
        G = int(rng.integers(0, max_gt + 1))
        x1 = rng.integers(0, 600, G); y1 = rng.integers(0, 400, G)
        gt = np.stack([x1, y1, x1 + rng.integers(2, 420, G), y1 + rng.integers(2, 420, G)], 1).astype(np.uint16)
        cls = rng.integers(1, 81, G).astype(np.int32)
        ov = np.zeros((G, 81), np.float32)
        ov[np.arange(G), cls] = 1.0
        if G > 3:
            ov[1] = -1.0                                             # a crowd-like row: not scored
        roidb.append(dict(boxes=gt, gt_classes=cls, gt_overlaps=ov))
        scale = np.float32(rng.choice([1.0, 1.6, 0.8333333, 2.0 / 3.0]))
        if G:
            b = gt[rng.integers(0, G, P)].astype(np.float64) + np.round(rng.uniform(-8, 8, (P, 4)) * 2) / 2
        else:
            x = rng.uniform(0, 500, (P, 2))
            b = np.hstack((x, x + rng.uniform(1, 200, (P, 2))))
        b[P // 3:P // 3 + 8] = b[0]                                  # exact duplicates
        raw.append((b * scale).astype(np.float32))
        scores.append(rng.uniform(0, 1, P).astype(np.float32))
        scales.append(scale)
    return roidb, np.stack(raw), np.stack(scores), np.asarray(scales, np.float32)


@pytest.mark.parametrize('P', [1000, 2000])
def test_random_large_scaled_and_thresholded(P):
    roidb, raw, scores, scales = _random_case(7 + P, 500, P, 100)
    thresh = 0.25
    # tester.generate_proposals' expressions: float32 boxes / float(scale), then score > thresh
    cands = []
    for i in range(len(roidb)):
        dets = np.hstack((raw[i] / float(scales[i]), scores[i].reshape(-1, 1))).astype(np.float32)
        cands.append(dets[np.where(dets[:, 4] > thresh)[0], :])
    ev = DeviceRecall(roidb, record_overlaps=True)
    num = torch.full((len(roidb),), P, dtype=torch.int32)
    num[::7] = P - 5                                                  # short lists: the rows behind num_valid are ignored
    for i in range(0, len(roidb), 7):
        cands[i] = cands[i][np.nonzero(np.arange(P)[scores[i] > thresh] < P - 5)[0]]
    host = R.evaluate_recall(roidb, len(roidb), cands)
    rois = torch.zeros((len(roidb), P, 5), dtype=torch.float32)
    rois[:, :, 1:] = torch.as_tensor(raw)
    rois, sc, scl = rois.cuda(), torch.as_tensor(scores).cuda(), torch.as_tensor(scales).cuda()
    for lo in range(0, len(roidb), 16):                              # rois[:, :, 1:]: strided rows, as generate_proposals passes them
        ev.add(rois[lo:lo + 16, :, 1:], num[lo:lo + 16].cuda(), np.arange(lo, min(lo + 16, len(roidb))),
               scores=sc[lo:lo + 16], thresh=thresh, scale=scl[lo:lo + 16])
    _assert_same(host, ev.summarize())
    # another batching of the same images (positions on the device, uneven batches): identical counts
    ev2 = DeviceRecall(roidb)
    order = np.random.default_rng(1).permutation(len(roidb))
    for lo, hi in ((0, 3), (3, 200), (200, 500)):
        idx = torch.as_tensor(order[lo:hi])
        ev2.add(rois[idx.cuda(), :, 1:], num[idx].cuda(), idx.to(torch.int32).cuda(), scores=sc[idx.cuda()], thresh=thresh,
                scale=scl[idx.cuda()])
    for name in ('hits', 'num_pos', 'area_count', 'n_cand', 'added'):
        assert torch.equal(getattr(ev, name), getattr(ev2, name)), name
    _assert_same(host, ev2.summarize(), with_overlaps=False)


def test_limits_are_refused_before_launch():
    roidb = [dict(boxes=np.array([[0, 0, 10, 10]], np.uint16), gt_classes=np.array([1], np.int32),
                  gt_overlaps=np.array([[0, 1]], np.float32))]
    ev = DeviceRecall(roidb)
    with pytest.raises(ValueError):
        ev.add(torch.zeros((1, 2049, 4), device='cuda'), None, [0])
    with pytest.raises(ValueError):
        DeviceRecall.from_lists(roidb, [np.zeros((2049, 5), np.float32)])
    with pytest.raises(ValueError):
        ops.recall_match(torch.zeros((1, 2049, 4), device='cuda'), ev.gt_off[:1].clone(), ev.gt_off, ev.gt_box, ev.gt_mask, ev.thr,
                         ev.area_rng, ev.hits, ev.num_pos, ev.area_count, ev.n_cand, ev.added, ev.gt_cap)
    many = [dict(boxes=np.tile(np.array([[0, 0, 10, 10]], np.uint16), (257, 1)), gt_classes=np.ones(257, np.int32),
                 gt_overlaps=np.tile(np.array([[0, 1]], np.float32), (257, 1)))]
    with pytest.raises(ValueError):
        DeviceRecall(many)
    with pytest.raises(ValueError):
        ops.recall_match(torch.zeros((1, 4, 4), device='cuda'), ev.gt_off[:1].clone(), ev.gt_off, ev.gt_box, ev.gt_mask, ev.thr,
                         ev.area_rng, ev.hits, ev.num_pos, ev.area_count, ev.n_cand, ev.added, 257)
    # the library refuses them as well
    big = torch.zeros((1, 2049, 4), device='cuda')
    rc = lib.load().relnet_recall_match(big.data_ptr(), 2049 * 4, 4, None, None, None, 0.0, ev.gt_off[:1].clone().data_ptr(), ev.gt_off.data_ptr(),
                                        ev.gt_box.data_ptr(), ev.gt_mask.data_ptr(), ev.thr.data_ptr(), ev.area_rng.data_ptr(),
                                        ev.hits.data_ptr(), ev.num_pos.data_ptr(), ev.area_count.data_ptr(), ev.n_cand.data_ptr(),
                                        ev.added.data_ptr(), None, 1, 2049, 1, 7, 10, 1, None)
    assert rc != 0 and b'at most 2048' in lib.load().relnet_last_error()
    assert int(ev.added.sum()) == 0 and int(ev.num_pos.sum()) == 0                 # nothing ran
    with pytest.raises(ValueError):
        ev.summarize()                                                              # image 0 never added


def test_test_rpn_device_and_host_agree(tmp_path):
    from relnet_amd import backbone, detector, config as C
    from relnet_amd.dataset import loader as LD, tester as TS
    from test_dataset import make_dataset
    db = make_dataset(str(tmp_path), degenerate=False)
    roidb = db.gt_roidb()
    cfg = C.experiment('rcnn_end2end_relation_8epoch')
    cfg.SCALES[0] = (128, 192)
    p = backbone.init_params(seed=2, num_classes=db.num_classes)
    dcfg = detector.Config()
    dcfg.num_classes, dcfg.rpn_post_nms_top_n, dcfg.rpn_min_size = db.num_classes, 60, 8
    det = detector.Detector(p, dtype=torch.bfloat16, cfg=dcfg, im_hw=(128, 192))
    scores = np.concatenate([b[:, 4] for b in TS.generate_proposals(det, LD.TestLoader(roidb, cfg, batch_size=2, has_rpn=True), db,
                                                                     save=False)])
    levels = np.unique(scores)                                # (random-init RPN: most scores saturate at 1.0)
    assert len(levels) > 1
    for thresh in (0.0, float(levels[len(levels) // 2])):     # the second keeps the top scores and drops the lowest
        host = TS.test_rpn(det, LD.TestLoader(roidb, cfg, batch_size=2, has_rpn=True), db, thresh=thresh)
        host_pkl = db.load_rpn_data()
        host_full = db.load_rpn_data(full=True) if thresh > 0 else None
        dev = TS.test_rpn(det, LD.TestLoader(roidb, cfg, batch_size=2, has_rpn=True), db, thresh=thresh, device_eval=True)
        dev_pkl = db.load_rpn_data()
        assert dev == host and host.startswith('percentage of 0-25')
        assert len(dev_pkl) == len(host_pkl) == db.num_images
        for a, b in zip(host_pkl, dev_pkl):
            assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b)
        if thresh > 0:
            assert any(len(b) < 60 for b in host_pkl)                 # the threshold removed some proposals
            for a, b in zip(host_full, db.load_rpn_data(full=True)):
                assert np.array_equal(a, b)
    # and generate_proposals' default path is what it was: a list, no evaluator
    boxes = TS.generate_proposals(det, LD.TestLoader(roidb, cfg, batch_size=2, has_rpn=True), db, save=False)
    assert isinstance(boxes, list) and boxes[0].shape == (60, 5)
