#!/usr/bin/env python
"""Generate tests/golden/class_specific.npz by EXECUTING THE REFERENCE'S OWN Python with CLASS_AGNOSTIC false.

Run in the build container only (needs the reference tree; tests read the committed .npz):

    python tests/golden/gen_golden_class_specific.py [--ref /root/reference]

The reference files are loaded from where they lie, through gen_golden.setup_reference (the numpy MXNet stand-in of
tests/golden/refshim).  Inputs are the generators of tests/class_specific_cases.py: those of cases.py with bbox_pred
[n, 4 * num_classes].  Only data goes into the npz:

  <lnms case>/nms_multi_score, sorted_bbox, sorted_score
        operator_py/learn_nms.py LearnNmsOperator.forward with class_agnostic=False (the `pick` branch, :311-321), for every
        entry of class_specific_cases.LNMS_CASES (means / stds None; means / stds of the training graph; 80 foreground classes)
  post/pred, post/boxes lib/bbox/bbox_transform.py nonlinear_pred, then clip_boxes, on [n, 4 C] deltas (core/tester.py:148-156)
  post/nms_keep_<j>     lib/nms/nms.py nms(thresh 0.5) of class j on its own columns 4j..4j+3 (tester.py:244-268)
  post/softnms_<j>      lib/nms/nms.py soft_nms(0.6) likewise
  pt/rois, label, bbox_target, bbox_weight
        core/rcnn.py sample_rois_v2 -> lib/bbox/bbox_regression.py expand_bbox_regression_targets with cfg.CLASS_AGNOSTIC False
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cases  # noqa: E402
import class_specific_cases as CS  # noqa: E402
from gen_golden import setup_reference  # noqa: E402

F32 = np.float32


def gen_learn_nms(lnms, d):
    import mxnet as mx
    for name, (n, c, first_n, seed, norm) in CS.LNMS_CASES.items():
        cls_score, bbox_pred, rois, im_info, feat, p = CS.lnms_case(n, c, seed)
        means, stds = norm if norm else (None, None)
        op = lnms.LearnNmsOperator(num_fg_classes=c, bbox_means=means, bbox_stds=stds, first_n=first_n, class_agnostic=False,
                                   num_thresh=5, class_thresh=0.01, nongt_dim=n, has_non_gt_index=False)
        in_data = [mx.NDArray(x) for x in (cls_score, bbox_pred, rois, im_info, feat)]
        in_data += [mx.NDArray(p[k]) for k in cases.LEARN_NMS_ARG_ORDER]
        outs = [mx.nd.zeros((first_n, c, 5)), mx.nd.zeros((first_n, c, 4)), mx.nd.zeros((first_n, c))]
        mx.TRACE.clear()
        op.forward(False, ['write'] * 3, in_data, outs, [])
        d[name + '/nms_multi_score'] = outs[0].asnumpy()
        d[name + '/sorted_bbox'] = outs[1].asnumpy()
        d[name + '/sorted_score'] = outs[2].asnumpy()
        print('   ', name, 'done', flush=True)


def gen_post(bt, nm, d):
    n, C, seed = CS.POST_CASE
    rois, scores, deltas = CS.post_case(n, C, seed)
    pred = bt.nonlinear_pred(rois[:, 1:], deltas)
    d['post/pred'] = pred
    boxes = bt.clip_boxes(pred.copy(), (cases.IM_H, cases.IM_W))
    d['post/boxes'] = boxes
    for j in range(1, C):
        idx = np.where(scores[:, j] > 1e-3)[0]
        cls_dets = np.hstack((boxes[idx, j * 4:(j + 1) * 4], scores[idx, j, np.newaxis]))
        d['post/nms_keep_%d' % j] = np.asarray(nm.nms(cls_dets.copy(), 0.5), dtype=np.int64)
        d['post/softnms_%d' % j] = nm.soft_nms(cls_dets.copy(), 0.6, -1)


def gen_targets(rcnn, d):
    class _NS(object):
        pass
    cfg = _NS(); cfg.TRAIN = _NS()
    cfg.CLASS_AGNOSTIC = False
    cfg.TRAIN.BG_THRESH_HI = 0.5
    cfg.TRAIN.BBOX_NORMALIZATION_PRECOMPUTED = True
    cfg.TRAIN.BBOX_MEANS = (0.0, 0.0, 0.0, 0.0)
    cfg.TRAIN.BBOX_STDS = (0.1, 0.1, 0.2, 0.2)
    cfg.TRAIN.BBOX_WEIGHTS = np.array([1.0, 1.0, 1.0, 1.0])
    n, g, seed, num_fg = CS.TARGETS_CASE
    rois, gt_boxes, _, _ = cases.targets_case(n, g, seed, num_fg=num_fg)
    all_rois = np.vstack((rois, np.hstack((np.zeros((gt_boxes.shape[0], 1), F32), gt_boxes[:, :-1]))))     # proposal_target.py:64-67
    r, lab, bt_, bw = rcnn.sample_rois_v2(all_rois, num_fg + 1, cfg, gt_boxes=gt_boxes)
    d['pt/rois'], d['pt/label'], d['pt/bbox_target'], d['pt/bbox_weight'] = r, lab, bt_, bw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    ap.add_argument('--out', default=os.path.join(HERE, 'class_specific.npz'))
    a = ap.parse_args()
    ga, bt, nm, rel, lnms = setup_reference(a.ref)
    d = {}
    gen_learn_nms(lnms, d)
    gen_post(bt, nm, d)
    gen_targets(setup_reference.extra[2], d)
    np.savez_compressed(a.out, **d)
    print('wrote', a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
