#!/usr/bin/env python
"""Generate tests/golden/sampled_rois.npz by EXECUTING THE REFERENCE'S OWN `sample_rois` (relation_rcnn/core/rcnn.py:329-397).

Run where the reference tree is available (tests read the committed .npz):

    python tests/golden/gen_golden_sampled_rois.py --ref <reference tree>

core/rcnn.py is loaded from where it lies, through gen_golden.setup_reference (the compiled `bbox_overlaps_cython` replaced by the
reference's own pure-python twin bbox_overlaps_py, as for targets.npz).  Inputs are the cases of tests/sampled_rois_cases.py.  Restated here,
because operator_py/proposal_target.py is Python 2: its glue :64-67 (the gt rows appended to the candidates, with the image's index).

`numpy.random.choice`, which the reference calls through its module-level name `npr`, is replaced for the run by the selection rule of
include/relnet_hip.h (relnet_proposal_target_sample): the `size` members with the smallest word of their stream, in ascending order.  The
three call sites are told apart by their first argument: the padding call passes a `range`, the fg call indices whose overlap reaches
FG_THRESH, the bg call the others; the padding round is counted.  A case that makes no such call (`exact-fit`) is the reference alone; in `tiny` every
call asks for the whole set (padding rounds of all M candidates), which the rule returns as it is.

Outside the reference's domain, as stated in the header: an image without gt boxes (the `batch` case; `overlaps.argmax` of an empty
matrix raises) runs sample_rois in its precomputed form -- labels, overlaps and bbox_targets all zero -- so the selection code is still
the reference's.  `sample_rois` indexes its `gt_lables` argument, which the operator never passes: an unused array is handed in.

Only data goes into the npz: <case>/rois_out, label, bbox_target, bbox_weight, keep_index [B, R, ...] and n_choice [B] (the random
calls the reference made per image), for seed sampled_rois_cases.SEEDS[0].
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import sampled_rois_cases as SC  # noqa: E402
from gen_golden import setup_reference  # noqa: E402

F32 = np.float32


class _NS(object):
    pass


class ChoiceByRule(object):
    """Stands in for the module `numpy.random` inside core/rcnn.py during one sample_rois call."""

    def __init__(self, seed, b, overlaps, fg_thresh):
        self.seed, self.b, self.ov, self.fg_thresh = seed, b, overlaps, fg_thresh
        self.calls, self.round = 0, 0

    def choice(self, a, size, replace):
        assert replace is False
        self.calls += 1
        if isinstance(a, range):
            stream = 2 + self.round
            self.round += 1
        else:
            stream = 0 if self.ov[a[0]] >= self.fg_thresh else 1
        return SC.choose(np.asarray(a), size, self.seed, self.b, stream)


def run_image(rcnn, c, b, seed):
    cfg = _NS(); cfg.TRAIN = _NS()
    cfg.CLASS_AGNOSTIC = bool(c['class_agnostic'])
    cfg.TRAIN.FG_THRESH, cfg.TRAIN.BG_THRESH_HI, cfg.TRAIN.BG_THRESH_LO = c['fg_thresh'], c['bg_thresh_hi'], c['bg_thresh_lo']
    cfg.TRAIN.BBOX_NORMALIZATION_PRECOMPUTED = True
    cfg.TRAIN.BBOX_MEANS, cfg.TRAIN.BBOX_STDS = c['means'], c['stds']
    cfg.TRAIN.BBOX_WEIGHTS = np.array(c['weights'])
    R = c['R']
    nr = c['N'] if c['num_rois'] is None else int(c['num_rois'][b])
    gt_boxes = c['gt'][b, :int(c['num_gt'][b])]
    all_rois = c['rois'][b, :nr]
    if c['append_gt']:      # proposal_target.py:64-67 (the reference writes image index 0: one image per executor; a batch needs b)
        all_rois = np.vstack((all_rois, np.hstack((np.full((gt_boxes.shape[0], 1), b, F32), gt_boxes[:, :-1]))))
    M = all_rois.shape[0]
    fg_rois = int(np.round(c['fg_fraction'] * R))       # proposal_target.py:58,61
    kw = dict(gt_boxes=gt_boxes, gt_lables=np.zeros(M))
    if gt_boxes.shape[0]:
        ov = rcnn.bbox_overlaps(all_rois[:, 1:].astype(np.float64), gt_boxes[:, :4].astype(np.float64)).max(axis=1)
    else:                   # no gt box: every overlap is 0 (see the module docstring)
        ov = np.zeros(M)
        kw.update(labels=np.zeros(M, F32), overlaps=ov, bbox_targets=np.zeros((M, 5), F32))
    hook = ChoiceByRule(seed, b, ov, c['fg_thresh'])
    # the candidate each output row was taken from: sample_rois returns rows only, so an index rides in a spare copy of the call
    saved = rcnn.npr
    rcnn.npr = hook
    try:
        rois, labels, bt, bw, _ = rcnn.sample_rois(all_rois, fg_rois, R, c['num_reg'], cfg, **kw)
        hook2 = ChoiceByRule(seed, b, ov, c['fg_thresh'])
        rcnn.npr = hook2
        tagged = np.hstack((np.arange(M, dtype=np.float64)[:, None], all_rois[:, 1:].astype(np.float64)))
        keep = rcnn.sample_rois(tagged, fg_rois, R, c['num_reg'], cfg, **kw)[0][:, 0].astype(np.int32)
    finally:
        rcnn.npr = saved
    assert hook.calls == hook2.calls and np.array_equal(all_rois[keep], rois)
    return rois.astype(F32), labels.astype(F32), bt, bw, keep, hook.calls


def generate(rcnn, seed=SC.SEEDS[0]):
    d = {}
    for name in SC.CASES:
        c = SC.case(name)
        per = [run_image(rcnn, c, b, seed) for b in range(c['B'])]
        for i, key in enumerate(('rois_out', 'label', 'bbox_target', 'bbox_weight', 'keep_index')):
            d['%s/%s' % (name, key)] = np.stack([p[i] for p in per])
        d[name + '/n_choice'] = np.array([p[5] for p in per], np.int32)
        print('   ', name, 'choice calls', d[name + '/n_choice'].tolist(), flush=True)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True)
    ap.add_argument('--out', default=os.path.join(HERE, 'sampled_rois.npz'))
    a = ap.parse_args()
    setup_reference(a.ref)
    d = generate(setup_reference.extra[2])
    np.savez_compressed(a.out, **d)
    print('wrote', a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
