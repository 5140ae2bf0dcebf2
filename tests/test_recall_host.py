"""Proposal recall on the host (dataset/recall.py, IMDB.evaluate_recall) against the reference's own
`lib/dataset/imdb.py:evaluate_recall` (tests/golden/recall.npz, gen_golden_recall.py): the log string is equal and every
full-precision sorted gt_overlaps array is np.array_equal.  No GPU."""
import os

import numpy as np
import pytest

import relnet_amd  # noqa: F401
from relnet_amd.dataset import recall as R
from relnet_amd.dataset.imdb import IMDB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'recall.npz')


def golden_cases():
    """-> {name: dict(roidb, candidates (list or None), thresholds (or None), log, sorted [7 arrays])}."""
    d = np.load(GOLDEN)
    out = {}
    for name in d['cases'].tolist():
        off = d[name + '/roi_off']
        roidb = [dict(boxes=d[name + '/boxes'][lo:hi], gt_classes=d[name + '/gt_classes'][lo:hi],
                      gt_overlaps=d[name + '/gt_overlaps'][lo:hi]) for lo, hi in zip(off[:-1], off[1:])]
        cands = None
        if name + '/cand' in d.files:
            co = d[name + '/cand_off']
            cands = [d[name + '/cand'][lo:hi] for lo, hi in zip(co[:-1], co[1:])]
        thr = d[name + '/thresholds'] if name + '/thresholds' in d.files else None
        out[name] = dict(roidb=roidb, candidates=cands, thresholds=thr, log=str(d[name + '/log']),
                         sorted=[d['%s/sorted/%d' % (name, a)] for a in range(7)])
    return out


def _imdb(n):
    db = IMDB('synthetic', 'val', '/nonexistent', '/nonexistent')
    db.num_images = n
    return db


@pytest.mark.parametrize('name', ['edges', 'thresholds', 'merged'])
def test_evaluate_recall_matches_reference(name):
    c = golden_cases()[name]
    thr = None if c['thresholds'] is None else c['thresholds'].copy()
    assert _imdb(len(c['roidb'])).evaluate_recall(c['roidb'], candidate_boxes=c['candidates'], thresholds=thr) == c['log']
    log, res = R.evaluate_recall(c['roidb'], len(c['roidb']), c['candidates'], thr)
    assert log == c['log']
    assert [r['name'] for r in res['ranges']] == R.AREA_NAMES
    for a, r in enumerate(res['ranges']):
        assert r['gt_overlaps'].dtype == np.float64 and np.array_equal(r['gt_overlaps'], c['sorted'][a]), r['name']
        assert r['hits'].dtype == np.int64 and len(r['recalls']) == len(res['thresholds'])


def test_golden_covers_the_quirks():
    cases = golden_cases()
    e = cases['edges']
    _, res = R.evaluate_recall(e['roidb'], len(e['roidb']), e['candidates'])
    assert any(len(c) == 0 for c in e['candidates']) and any(len(r['boxes']) == 0 for r in e['roidb'])
    assert e['roidb'][0]['boxes'].dtype == np.uint16
    assert res['ranges'][6]['num_pos'] == 0 and np.isnan(res['ranges'][6]['ar'])      # 300^2 and larger wrapped below 65536
    assert 'nan' in e['log']
    # P < G: the unfilled rounds count as 0, which a threshold of 0.0 counts as a hit
    t = cases['thresholds']
    _, rt = R.evaluate_recall(t['roidb'], len(t['roidb']), t['candidates'], t['thresholds'].copy())
    assert t['thresholds'][0] == 0.0 and (rt['ranges'][0]['gt_overlaps'] == 0).any()
    assert cases['merged']['candidates'] is None and cases['merged']['roidb'][0]['boxes'].dtype == np.float32


def test_uint16_area_wrap_and_half_open_ranges():
    boxes = np.array([[0, 0, 299, 299], [0, 0, 24, 24], [0, 0, 255, 255]], np.uint16)
    m = R.area_masks(boxes)
    assert m[:, 0].tolist() == [True, False, False, False, True, False, False]         # 90000 -> 24464: 100-200
    assert m[:, 1].tolist() == [True, False, True, False, False, False, False]         # 625 = 25^2: 25-50, not 0-25
    assert m[:, 2].tolist() == [True, True, False, False, False, False, False]         # 65536 -> 0: 0-25
    assert R.area_masks(boxes.astype(np.float32))[6, 0]                                  # no wrap in float32


def test_greedy_cover_tie_order():
    # gt 0 and gt 1 tie at 0.5; the lower gt index is taken first, with the lower proposal index of its column
    ov = np.array([[0.5, 0.5, 0.1],
                   [0.5, 0.2, 0.1],
                   [0.0, 0.5, 0.3]])
    rec = R.greedy_cover(ov.copy())
    # round 0: gt 0 <- proposal 0 (0.5); round 1: gt 1 <- proposal 2 (0.5); round 2: gt 2 <- proposal 1 (0.1)
    assert rec.tolist() == [0.5, 0.5, 0.1]
    assert R.greedy_cover(np.array([[0.9, 0.8, 0.7]])).tolist() == [0.9, 0.0, 0.0]       # P < G
    assert R.greedy_cover(np.zeros((3, 0))).shape == (0,)


def test_overlaps_formula():
    b = np.array([[0, 0, 9, 9], [5, 5, 14, 14], [20, 20, 10, 10]], np.float64)
    q = np.array([[0, 0, 9, 9], [10, 0, 19, 9]], np.float64)
    ov = R.bbox_overlaps(b, q)
    assert ov[0, 0] == 1.0 and ov[0, 1] == 0.0 and ov[2].tolist() == [0.0, 0.0]
    assert ov[1, 0] == 25.0 / (100.0 + 100.0 - 25.0)


def _brute_force_cover(ov):
    """The cover's definition searched pair by pair: every round the largest overlap among unused (proposal, gt) pairs, the
    lowest gt index among its ties, then the lowest proposal index; G - rounds zeros at the end."""
    P, G = ov.shape
    free_p, free_g, out = set(range(P)), set(range(G)), []
    for _ in range(min(P, G)):
        best = None
        for g in sorted(free_g):
            for p in sorted(free_p):
                if best is None or ov[p, g] > best[0]:
                    best = (ov[p, g], g, p)
        out.append(best[0])
        free_g.discard(best[1]); free_p.discard(best[2])
    return np.array(out + [0.0] * (G - len(out)))


def test_cached_cover_is_the_brute_force_definition():
    rng = np.random.default_rng(11)
    for trial in range(300):
        P, G = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        levels = int(rng.integers(1, 6))                       # few distinct values: ties everywhere
        ov = np.round(rng.uniform(0, 1, (P, G)) * levels) / levels
        ov[rng.uniform(0, 1, (P, G)) < 0.3] = 0.0
        assert np.array_equal(R.greedy_cover(ov.copy()), _brute_force_cover(ov)), trial
