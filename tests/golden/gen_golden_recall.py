#!/usr/bin/env python
"""Generate tests/golden/recall.npz by EXECUTING THE REFERENCE'S OWN `lib/dataset/imdb.py:evaluate_recall`.

Run in the build container only (needs the reference tree; tests read the committed .npz):

    python tests/golden/gen_golden_recall.py [--ref /root/reference]

lib/dataset/imdb.py is read from where it lies and made importable in memory as gen_golden.py does (`_load_py2`: lib2to3's
fix_print), with the `np.float` alias, `cPickle`, a stub `PIL` module and `bbox.bbox_transform.bbox_overlaps` bound to the
reference's own `bbox_overlaps_py` (lib/bbox/bbox_transform.py, the formula of the Cython extension).  The loaded module's
`np` global is a recording proxy: it hands every call to numpy and keeps a copy of each array passed to `np.sort`, which is
the full-precision sorted `gt_overlaps` of each area range (the log prints three decimals).  No reference text is changed.

Every case is synthetic.  The npz holds, per case, the inputs (roidb rows concatenated with offsets, candidate lists,
thresholds), the reference's all_log_info string and the seven sorted gt_overlaps arrays.
"""
import argparse
import os
import pickle
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import _load_py2  # noqa: E402

NUM_CLASSES = 4


class _RecordingNumpy(object):
    """numpy as seen by the loaded module; np.sort inputs are recorded."""

    def __init__(self):
        self.sorted = []

    def __getattr__(self, name):
        return getattr(np, name)

    def sort(self, a, *args, **kwargs):
        r = np.sort(a, *args, **kwargs)
        self.sorted.append(np.array(r, copy=True))
        return r


def load_reference(ref):
    if not hasattr(np, 'float'):
        np.float = float
    sys.modules['cPickle'] = pickle
    pil = types.ModuleType('PIL'); pil.Image = types.ModuleType('PIL.Image')
    sys.modules['PIL'], sys.modules['PIL.Image'] = pil, pil.Image

    def _no_ext(*a, **k):
        raise RuntimeError("compiled reference extension is not available")
    bb = types.ModuleType('bbox'); bb.__path__ = []; bb.bbox_overlaps_cython = _no_ext
    sys.modules['bbox'] = bb
    bt = _load_py2('ref_bbox_transform', os.path.join(ref, 'lib/bbox/bbox_transform.py'))
    shim = types.ModuleType('bbox.bbox_transform'); shim.bbox_overlaps = bt.bbox_overlaps_py
    sys.modules['bbox.bbox_transform'] = shim
    imdb = _load_py2('ref_imdb', os.path.join(ref, 'lib/dataset/imdb.py'))
    rec = _RecordingNumpy()
    imdb.np = rec
    return imdb, rec


# ---- synthetic cases --------------------------------------------------------------------------------------------------
def _gt_record(boxes, classes, dtype=np.uint16, overlap_rows=None):
    boxes = np.asarray(boxes, dtype).reshape(-1, 4)
    classes = np.asarray(classes, np.int32)
    ov = np.zeros((len(boxes), NUM_CLASSES), np.float32)
    for k, c in enumerate(classes):
        if c > 0:
            ov[k, c] = 1.0
    for k, row in (overlap_rows or {}).items():
        ov[k] = row
    return dict(boxes=boxes, gt_classes=classes, gt_overlaps=ov)


def _cands(boxes, rng=None):
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    s = np.linspace(1.0, 0.1, len(b)).astype(np.float32) if len(b) else np.zeros(0, np.float32)
    return np.hstack((b, s.reshape(-1, 1))).astype(np.float32)


def _jitter(rng, gt, n, step=0.5, spread=6.0):
    """n float32 proposals around random gt boxes, coordinates on a `step` grid so that overlaps tie often."""
    if len(gt) == 0:
        x1 = rng.uniform(0, 400, n); y1 = rng.uniform(0, 300, n)
        b = np.stack([x1, y1, x1 + rng.uniform(4, 120, n), y1 + rng.uniform(4, 120, n)], 1)
    else:
        b = gt[rng.integers(0, len(gt), n)].astype(np.float64) + rng.uniform(-spread, spread, (n, 4))
    return (np.round(b / step) * step).astype(np.float32)


def case_edges(rng):
    recs, cands = [], []
    g0 = [[10, 10, 59, 59], [40, 10, 89, 59], [200, 200, 260, 230], [0, 0, 5, 5]]
    recs.append(_gt_record(g0, [1, 2, 3, 1]))
    cands.append(_cands([[10, 10, 59, 59], [10, 10, 59, 59],            # duplicate of gt 0: two proposals tie
                         [25, 10, 74, 59],                              # same IoU with gt 0 and gt 1: gts tie
                         [40, 10, 89, 59], [40, 10, 89, 59],
                         [300, 300, 310, 310], [0, 0, 5, 5]]))
    # P < G: two proposals, five gts
    recs.append(_gt_record([[0, 0, 30, 30], [5, 5, 35, 35], [100, 100, 140, 160], [50, 0, 70, 20], [0, 50, 10, 90]],
                           [1, 2, 3, 1, 2]))
    cands.append(_cands([[2, 2, 32, 32], [100, 100, 139, 150]]))
    # no candidates, but ground truth (counted in num_pos, skipped otherwise)
    recs.append(_gt_record([[0, 0, 40, 40], [60, 60, 90, 80]], [1, 3]))
    cands.append(np.zeros((0, 5), np.float32))
    # no ground truth, candidates only
    recs.append(_gt_record(np.zeros((0, 4)), []))
    cands.append(_cands([[0, 0, 20, 20], [5, 5, 400, 400], [1, 1, 2, 2]]))
    # uint16 areas above 65535 wrap: 300 x 300 = 90000 -> 24464, 400 x 400 = 160000 -> 28928, 256 x 256 = 65536 -> 0
    recs.append(_gt_record([[0, 0, 299, 299], [10, 10, 409, 409], [0, 0, 255, 255], [500, 0, 799, 199]], [1, 2, 3, 1]))
    cands.append(_cands([[0, 0, 299, 299], [12, 8, 405, 411], [0, 0, 255, 255], [1, 1, 250, 260], [500, 0, 790, 199]]))
    # areas exactly on the range bounds: 25^2, 50^2, 100^2, 200^2, 300^2 (gts and candidates)
    sides = [25, 50, 100, 200, 300, 24, 49]
    recs.append(_gt_record([[0, 0, s - 1, s - 1] for s in sides], [1, 2, 3, 1, 2, 3, 1], overlap_rows={6: [-1, -1, -1, -1]}))
    cands.append(_cands([[0, 0, s - 1, s - 1] for s in sides] + [[0, 0, 24.5, 24], [0.5, 0, 25, 24]]))
    # a crowd-like row (overlaps -1) and a row whose max overlap is 0.5: neither is scored
    recs.append(_gt_record([[10, 10, 50, 50], [20, 20, 60, 60], [0, 0, 100, 100]], [1, 2, 3],
                           overlap_rows={0: [-1, -1, -1, -1], 1: [0, 0, 0.5, 0]}))
    cands.append(_cands([[10, 10, 50, 50], [20, 20, 60, 60], [0, 0, 99, 99]]))
    # jittered images with many ties
    for i in range(12):
        G = int(rng.integers(0, 14))
        x1 = rng.integers(0, 500, G); y1 = rng.integers(0, 400, G)
        gt = np.stack([x1, y1, x1 + rng.integers(3, 330, G), y1 + rng.integers(3, 330, G)], 1)
        recs.append(_gt_record(gt, rng.integers(1, NUM_CLASSES, G)))
        P = int(rng.integers(0, 40)) if i % 4 else int(rng.integers(0, max(G, 1)))
        c = _jitter(rng, gt, P)
        if P > 3:
            c[P // 2:P // 2 + 2] = c[0]                               # exact duplicates
        cands.append(_cands(c))
    return recs, cands


def case_merged(rng):
    """rpn_roidb(append_gt=True): float32 proposal rows (gt_classes 0) above uint16 gt rows -> float32 boxes."""
    recs = []
    for i in range(8):
        G = int(rng.integers(0, 8))
        x1 = rng.integers(0, 300, G); y1 = rng.integers(0, 300, G)
        gt = _gt_record(np.stack([x1, y1, x1 + rng.integers(10, 200, G), y1 + rng.integers(10, 200, G)], 1),
                        rng.integers(1, NUM_CLASSES, G))
        P = int(rng.integers(0, 30))
        props = _jitter(rng, gt['boxes'], P)
        pov = np.zeros((P, NUM_CLASSES), np.float32)
        if P and G:
            props[0] = gt['boxes'][0]                                 # a proposal on a gt: overlap row max 1, gt_classes 0
            pov[0, gt['gt_classes'][0]] = 1.0
        recs.append(dict(boxes=np.concatenate((props, gt['boxes'])), gt_classes=np.concatenate((np.zeros(P, np.int32), gt['gt_classes'])),
                         gt_overlaps=np.concatenate((pov, gt['gt_overlaps']))))
    return recs


def pack_case(d, name, recs, cands, thresholds, log, sorted_ov):
    off = np.concatenate([[0], np.cumsum([len(r['boxes']) for r in recs])]).astype(np.int64)
    d[name + '/boxes'] = np.concatenate([r['boxes'] for r in recs])
    d[name + '/roi_off'] = off
    d[name + '/gt_classes'] = np.concatenate([r['gt_classes'] for r in recs]).astype(np.int32)
    d[name + '/gt_overlaps'] = np.concatenate([r['gt_overlaps'] for r in recs]).astype(np.float32)
    if cands is not None:
        d[name + '/cand'] = np.concatenate(cands).astype(np.float32)
        d[name + '/cand_off'] = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64)
    if thresholds is not None:
        d[name + '/thresholds'] = np.asarray(thresholds, np.float64)
    d[name + '/log'] = np.array(log)
    assert len(sorted_ov) == 7, len(sorted_ov)
    for a, s in enumerate(sorted_ov):
        d['%s/sorted/%d' % (name, a)] = np.asarray(s, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    ap.add_argument('--out', default=HERE)
    args = ap.parse_args()
    imdb, rec = load_reference(args.ref)

    def run(recs, cands, thresholds):
        rec.sorted = []
        self = types.SimpleNamespace(num_images=len(recs))
        log = imdb.IMDB.evaluate_recall(self, recs, candidate_boxes=cands, thresholds=thresholds)
        return log, list(rec.sorted)

    rng = np.random.default_rng(2024)
    d = {}
    recs, cands = case_edges(rng)
    pack_case(d, 'edges', recs, cands, None, *run(recs, cands, None))
    thr = np.array([0.0, 0.25, 0.5, 0.7, 0.95, 1.0])
    pack_case(d, 'thresholds', recs, cands, thr, *run(recs, cands, thr.copy()))
    merged = case_merged(rng)
    pack_case(d, 'merged', merged, None, None, *run(merged, None, None))
    d['cases'] = np.array(['edges', 'thresholds', 'merged'])
    np.savez_compressed(os.path.join(args.out, 'recall.npz'), **d)


if __name__ == '__main__':
    main()
