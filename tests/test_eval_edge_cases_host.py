"""tests/eval_edge_cases.py checked on the host: the constants it writes out are the sources', every case reaches the structural edge
it is named for, the restatements equal dataset/cocoeval.py and dataset/recall.py bit for bit, every non-degenerate case has ground
truth in at least 90 % of its (category, area) cells and a precision strictly between 0 and 1, and a numpy model of each plausible
defect changes the expected output of the cases named for it (and leaves the case on the safe side of the boundary alone).
Run with -s to see the table of cases and the sizes of the pre-existing synthetic problems."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import relnet_amd  # noqa: F401,E402
import eval_edge_cases as E  # noqa: E402
from relnet_amd.dataset import recall as R  # noqa: E402
from test_recall_host import golden_cases  # noqa: E402


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _expected(name):
    ev = E.coco_expected(name)
    return ev.eval['precision'], ev.eval['recall']


def test_constants_are_the_sources():
    for name, (value, fname, line) in E.CONSTANTS.items():          # (the line is where it stood when the table was written)
        m = re.search(r'^constexpr int %s = (\d+);' % name, open(os.path.join(E.CSRC, fname)).read(), re.M)
        assert m and int(m.group(1)) == value, (name, fname, line)
    src = open(os.path.join(E.CSRC, 'cocoeval.hip')).read()
    assert '__launch_bounds__(1024) void coco_scan_kernel' in src and 'const long per = (len + 1023) / 1024;' in src
    assert 'if (K > 255) pass(8);' in src and 'iou_thr[tid] < 1.0 - 1e-10' in src
    assert (E.MATCH_THREADS, E.MAX_SLOTS, E.MAX_PAIRS, E.MAX_DETS_LEN, E.MAX_AREAS, E.SORT_TILE, E.RADIX) == \
        tuple(E.CONSTANTS[k][0] for k in ('kCocoMatchThreads', 'kCocoMaxSlots', 'kCocoMaxPairs', 'kCocoMaxDetsLen', 'kCocoMaxAreas',
                                          'kSortTile', 'kSortThreads'))
    assert (E.RECALL_THREADS, E.RECALL_MAX_CAND, E.RECALL_MAX_GT) == tuple(E.CONSTANTS[k][0] for k in ('kRecallThreads', 'kRecallMaxCand', 'kRecallMaxGt'))
    assert E.CAND_PER_THREAD == E.RECALL_MAX_CAND // E.RECALL_THREADS and E.RECALL_THREADS // E.WAVE == 4


def test_preexisting_problems_sit_in_one_corner():
    """The synthetic problems of test_gpu_device_eval.py: at most 5 categories, one word per scan thread, no second unit trip."""
    print()
    for seed, n_images in ((0, 24), (1, 24), (2, 24), (3, 16), (4, 24), (5, 12), (6, 24)):
        gts, dts, img_ids, cats = E.synthetic_problem(seed, n_images)
        c = dict(gts=gts, dts=dts, img_ids=img_ids, cat_ids=cats)
        c['slots'] = int(E.rows_per_image(c).max())
        s = E.structure(c)
        print('  synthetic_problem(%d, %d): %d slots per image, %d slots, %d tiles, %d word(s) per scan thread, %d units, K %d'
              % (seed, n_images, c['slots'], s['n_slots'], s['tiles'], s['per'], s['units'], s['K']))
        assert s['per'] == 1 and s['tiles'] <= 4 and s['units'] <= 200 and s['K'] == 5 and s['S_in'] < 1024


STRUCTURE = {
    'units1200': dict(units=1200, A=4, T=10), 'units1024': dict(units=1024, A=4, T=8), 'units1056': dict(units=1056, A=4, T=8),
    'rows1024': dict(S_in=1024), 'rows1025': dict(S_in=1025), 'rows2047': dict(S_in=2047), 'rows2048': dict(S_in=2048),
    'slots1': dict(n_slots=1, tiles=1, tail=1), 'slots2047': dict(n_slots=2047, tiles=1, tail=2047), 'slots2048': dict(n_slots=2048, tiles=1, tail=2048),
    'slots2049': dict(n_slots=2049, tiles=2, tail=1), 'slots9k': dict(n_slots=9 * 1024, tiles=5, per=2), 'slots40k': dict(n_slots=40 * 1024, tiles=20, per=5),
    'K255': dict(K=255, category_passes=1), 'K256': dict(K=256, category_passes=2), 'K257': dict(K=257, category_passes=2),
    'K300': dict(K=300, category_passes=2), 'maxdets1': dict(M=1), 'maxdets1237': dict(M=4), 'maxdets100': dict(M=3),
    'A7T9': dict(A=7, T=9, R=1), 'A4T16': dict(A=4, T=16, R=101), 'odd_values': dict(), 'no_gt': dict(),
}


@pytest.mark.parametrize('name', sorted(E.COCO_BUILDERS))
def test_coco_case_reaches_its_edge_and_keeps_the_caps(name):
    c, s = E.coco_case(name), E.structure(E.coco_case(name))
    print('\n  %-12s %s | units %d S_in %d slots %d tiles %d tail %d per %d K %d A %d T %d M %d R %d' % (
        name, c['edge'], s['units'], s['S_in'], s['n_slots'], s['tiles'], s['tail'], s['per'], s['K'], s['A'], s['T'], s['M'], s['R']))
    for k, v in STRUCTURE[name].items():
        assert s[k] == v, (name, k, s[k], v)
    assert s['A'] * s['T'] <= E.MAX_PAIRS and s['A'] <= E.MAX_AREAS and s['M'] <= E.MAX_DETS_LEN and s['S_in'] <= c['slots'] <= E.MAX_SLOTS
    if name == 'A4T16':
        assert s['A'] * s['T'] == E.MAX_PAIRS
    precision, recall = _expected(name)
    if c['degenerate']:
        assert (precision == -1).all() and (recall == -1).all()
        return
    cells = (precision[0, 0, :, :, -1] == -1)
    assert cells.mean() <= 0.10, cells.mean()
    assert ((precision > 0) & (precision < 1)).any()
    if name != 'slots1':                                  # (one detection: its precision is 1 / (1 + eps))
        assert ((precision > 0.01) & (precision < 0.99)).any()
    rows = E.rows_per_image(c)
    if name.startswith('rows'):
        assert sorted(rows.tolist()) == [3, s['S_in']]
        per_cat = {}
        for d in c['dts']:
            per_cat[(d['image_id'], d['category_id'])] = per_cat.get((d['image_id'], d['category_id']), 0) + 1
        assert max(per_cat.values()) > 100                                   # more rows of one category than maxDets[-1]
    if name.startswith('K'):
        live = {c['cat_ids'].index(d['category_id']) for d in c['dts']}
        want = {0, 254} | {k for k in (255, 256) if k < s['K']} | {s['K'] - 1}
        assert want <= live and 100 not in live and (precision[:, :, 100] == -1).all()
    if name in ('slots9k', 'slots40k'):
        # equal scores on both sides of the boundary between sort tiles 0 and 1, in different images, in one category
        sl = E.host_slots(E.coco_expected(name), c['slots'])
        cat, score = sl[0].reshape(-1), sl[1].reshape(-1)
        left, right = E.SORT_TILE - 1, E.SORT_TILE
        assert cat[left] >= 0 and cat[right] >= 0 and score[left] == score[right] == 0.5
        assert (cat[right:right + 128] == cat[left]).any() and left // c['slots'] != right // c['slots']
        assert (rows == 0).mean() > 0.9 and (rows == c['slots']).sum() >= 3     # most images empty, a few full


@pytest.mark.parametrize('name', ['synthetic', 'maxdets1237', 'A7T9', 'K257', 'odd_values'])
def test_slot_restatement_equals_cocoeval_accumulate(name):
    if name == 'synthetic':
        gts, dts, img_ids, cats = E.synthetic_problem(0)
        c = E.Case(gts=gts, dts=dts, img_ids=img_ids, cat_ids=cats)
        ev = E.host_eval(c)
        c['slots'] = int(E.rows_per_image(c).max())
    else:
        c, ev = E.coco_case(name), E.coco_expected(name)
    slots = E.host_slots(ev, c['slots'])
    got = E.accumulate_case_slots(c, slots)
    assert np.array_equal(got[0], ev.eval['precision']) and np.array_equal(got[1], ev.eval['recall'])
    assert (ev.eval['precision'] > 0).any()
    # the numpy model of the device sort gives the order of the stable argsort
    p = E.case_params(c)
    seq = E.radix_sort_model(slots[0], slots[1], slots[2], len(c['cat_ids']), p.maxDets[-1])
    assert _same(E.accumulate_case_slots(c, slots, sequence=seq), got)
    cat, score = slots[0].reshape(-1), slots[1].reshape(-1)
    live = np.nonzero((cat >= 0) & (slots[2].reshape(-1) < p.maxDets[-1]))[0]
    ref = live[np.lexsort((live, E.desc_score_key(score[live]), cat[live]))]
    assert np.array_equal(seq, ref)


@pytest.mark.parametrize('name', sorted(E.HAND_CASES))
def test_hand_built_slots_hold_every_class(name):
    h = E.hand_case(name)
    cat, score, rank, code, npig = h['slots']
    K, md = npig.shape[0], h['max_dets']
    p, r = E.hand_expected(name)
    if name == 'hand_M1_one_slot':
        assert cat.size == 1 and not (p == -1).any()
        return
    assert cat.min() < -1 and cat.max() > K - 1 and (cat == -1).any()
    for m in md:
        assert (rank == m - 1).any() and (rank == m).any()
    assert (rank == E.EMPTY_RANK).any() and set(np.unique(code)) == {0, 1, 2}
    assert np.isnan(score).any() and np.isposinf(score).any() and np.isneginf(score).any()
    assert (np.signbit(score) & (score == 0)).any() and (~np.signbit(score) & (score == 0)).any()
    assert (npig == 0).any() and (p[:, :, npig == 0] == -1).all() and (p[:, :, npig > 0] != -1).all()
    assert ((p > 0.01) & (p < 0.99)).any()
    # the sort model agrees here too (NaN last, -0.0 tied with 0.0, slots of categories outside 0..K-1 not evaluated)
    seq = E.radix_sort_model(cat, score, rank, K, md[-1])
    assert _same(E.accumulate_slots(*h['slots'], h['iou'], h['area'], h['rec'], md, sequence=seq), (p, r))


# ---- discrimination: a model of each plausible defect changes the expected output -----------------------------------
@pytest.mark.parametrize('name,changes', [('units1200', True), ('units1056', True), ('K300', True), ('units1024', False)])
def test_dropping_the_units_of_a_second_trip_is_seen(name, changes):
    c, ev = E.coco_case(name), E.coco_expected(name)
    slots = E.host_slots(ev, c['slots'])
    got = E.accumulate_case_slots(c, E.drop_units_from(c, slots))
    assert _same(got, _expected(name)) != changes


@pytest.mark.parametrize('name,changes', [('rows1025', True), ('rows2047', True), ('rows2048', True), ('rows1024', False)])
def test_dropping_the_rows_of_a_second_trip_is_seen(name, changes):
    c = E.coco_case(name)
    ev = E.host_eval(c, dts=E.drop_rows_from(c))
    assert _same((ev.eval['precision'], ev.eval['recall']), _expected(name)) != changes


@pytest.mark.parametrize('name,cut_changes,one_pass_changes', [('K255', False, False), ('K256', False, True), ('K257', True, True), ('K300', True, True)])
def test_a_category_digit_of_one_byte_is_seen(name, cut_changes, one_pass_changes):
    c, ev = E.coco_case(name), E.coco_expected(name)
    slots = E.host_slots(ev, c['slots'])
    K, max_det = len(c['cat_ids']), E.case_params(c).maxDets[-1]
    # (a) the category truncated to 8 bits when the sort key is built: categories 256.. fall into 0.. (none at K = 256)
    cut = (np.where(slots[0] >= 0, slots[0] & 255, -1).astype(np.int32),) + slots[1:]
    assert _same(E.accumulate_case_slots(c, cut), _expected(name)) != cut_changes
    # (b) the sort run with one category pass: the digits are no longer in order, so the segments are not the categories.  At
    # K = 256 it is the not-evaluated digit 256 that lands among category 0: rows cut at maxDets that outscore some of its rows.
    cat, score, rank = slots[:3]
    assert ((cat == 7) & (rank >= max_det)).sum() >= 20
    _, digit = E.radix_sort_model(cat, score, rank, K, max_det, category_bytes=1, full=True)
    assert (np.diff(digit) >= 0).all() != one_pass_changes
    _, digit = E.radix_sort_model(cat, score, rank, K, max_det, full=True)
    assert (np.diff(digit) >= 0).all()


@pytest.mark.parametrize('name,changes', [('slots9k', True), ('slots40k', True), ('slots2049', False), ('rows2048', False)])
def test_a_scan_of_the_first_word_per_thread_is_seen(name, changes):
    c, ev = E.coco_case(name), E.coco_expected(name)
    slots = E.host_slots(ev, c['slots'])
    seq = E.radix_sort_model(slots[0], slots[1], slots[2], len(c['cat_ids']), E.case_params(c).maxDets[-1], scan='first_word')
    assert _same(E.accumulate_case_slots(c, slots, sequence=seq), _expected(name)) != changes


@pytest.mark.parametrize('name', ['maxdets100', 'A7T9', 'units1024'])
def test_a_strict_iou_threshold_is_seen(name):
    c = E.coco_case(name)
    ev = E.host_eval(c, iou=E.strictly_above(E.case_params(c).iouThrs))
    assert not _same((ev.eval['precision'], ev.eval['recall']), _expected(name))


def test_thresholds_of_one_and_above_are_the_clamp():
    """A7T9: IoU thresholds 1 - 1e-10, 1.0, 1.0 + 2^-52 and 1.5 give one and the same result, with matches (exact copies)."""
    p, r = _expected('A7T9')
    for t in (6, 7, 8):
        assert np.array_equal(p[t], p[5]) and np.array_equal(r[t], r[5])
    assert (r[5] > 0).any() and not np.array_equal(r[3], r[5])            # (0.75 against the clamp)


# ---- recall ------------------------------------------------------------------------------------------------------------
def test_recall_restatement_equals_evaluate_recall():
    for name in ('edges', 'merged'):
        c = golden_cases()[name]
        n = len(c['roidb'])
        _, want = R.evaluate_recall(c['roidb'], n, c['candidates'])
        got = E.recall_reference([R.valid_gt(c['roidb'][i]) for i in range(n)], [R.candidates_of(c['roidb'], i, c['candidates']) for i in range(n)],
                                 R.default_thresholds(), R.AREA_RANGES)
        assert np.array_equal(got['overlaps'], want['image_overlaps']) and got['area_count'].tolist() == want['area_counts']
        for a, r in enumerate(want['ranges']):
            assert np.array_equal(got['hits'][a], r['hits']) and got['num_pos'][a] == r['num_pos']
        # and the plain form of the cover that the defect models are variants of
        plain = E.recall_reference([R.valid_gt(c['roidb'][i]) for i in range(n)], [R.candidates_of(c['roidb'], i, c['candidates']) for i in range(n)],
                                   R.default_thresholds(), R.AREA_RANGES, cover=E.cover_variant())
        assert np.array_equal(plain['overlaps'], got['overlaps'])


RECALL_STRUCTURE = {'G64': dict(G=64, A=7, T=10), 'G65': dict(G=65, A=7, T=10), 'G255': dict(G=255, A=2, T=10), 'G256': dict(G=256, A=8, T=256),
                    'P2047': dict(P=2047, A=2, T=1), 'P2048': dict(P=2048, A=7, T=10)}


@pytest.mark.parametrize('name', sorted(E.RECALL_CASES))
def test_recall_case_reaches_its_edge(name):
    c, e = E.recall_case(name), E.recall_expected(name)
    G, P = max(len(g) for g in c['gts']), max(len(b) for b in c['cands'])
    print('\n  %-6s %s | G %d (in range 0: %d) P %d A %d T %d' % (name, c['edge'], G, e['num_pos'][0], P, len(c['ranges']), len(c['thr'])))
    s = dict(G=G, P=P, A=len(c['ranges']), T=len(c['thr']))
    for k, v in RECALL_STRUCTURE[name].items():
        assert s[k] == v
    assert G <= E.RECALL_MAX_GT and P <= E.RECALL_MAX_CAND
    in0 = E.range_masks(c['gts'][0], c['ranges'])[0]
    assert in0.all()                                                          # every box of the image is in range 0: G lanes
    assert 0 < e['hits'][0, -1] <= e['num_pos'][0]
    if name == 'G256':
        assert c['thr'][0] == 0.0 and c['thr'][-1] == 1.0 and e['hits'][0, -1] > 0 and (e['hits'][:, 0] == e['num_pos']).all()
    if name.startswith('P'):
        b = c['cands'][0]
        assert np.array_equal(b[400:430], b[464:494]) and P - 1 >= (E.RECALL_THREADS - 1) * E.CAND_PER_THREAD
        # the last row matters: without it ground-truth box 29 has no exact copy
        less = E.recall_reference(c['gts'], [b[:-1]], c['thr'], c['ranges'])
        assert not np.array_equal(less['overlaps'], e['overlaps'])


@pytest.mark.parametrize('name,width,changes', [('G65', 64, True), ('G255', 64, True), ('G255', 128, True), ('G256', 128, True), ('G256', 192, True),
                                                ('G64', 64, False)])
def test_an_argmax_over_the_first_waves_is_seen(name, width, changes):
    c, e = E.recall_case(name), E.recall_expected(name)
    got = E.recall_reference(c['gts'], c['cands'], c['thr'], c['ranges'], cover=E.cover_variant(gt_first=width))
    assert (np.array_equal(got['overlaps'], e['overlaps']) and np.array_equal(got['hits'], e['hits'])) != changes


@pytest.mark.parametrize('name', ['G64', 'G65', 'G255', 'G256'])
def test_the_highest_tied_box_is_seen(name):
    c, e = E.recall_case(name), E.recall_expected(name)
    got = E.recall_reference(c['gts'], c['cands'], c['thr'], c['ranges'], cover=E.cover_variant(gt_last=True))
    assert not np.array_equal(got['hits'], e['hits'])


@pytest.mark.parametrize('name', ['P2047', 'P2048'])
def test_the_highest_tied_candidate_is_seen(name):
    c, e = E.recall_case(name), E.recall_expected(name)
    got = E.recall_reference(c['gts'], c['cands'], c['thr'], c['ranges'], cover=E.cover_variant(box_last=True))
    assert not np.array_equal(got['hits'], e['hits'])


def test_a_strict_recall_threshold_is_seen():
    c, e = E.recall_case('G256'), E.recall_expected('G256')
    got = E.recall_reference(c['gts'], c['cands'], E.strictly_above(c['thr']), c['ranges'])
    assert got['hits'][0, 0] < e['hits'][0, 0] and got['hits'][0, -1] == 0 < e['hits'][0, -1]      # at 0.0 and at 1.0


def test_score_filter_leaves_0_1_and_fewer_than_G():
    gts, raw, scores, thresh, num_valid = E.recall_filter_case(7)
    kept = E.filtered(raw, scores, thresh, num_valid)
    assert [len(k) for k in kept] == [0, 1, len(gts[2]) - 1, 0] and num_valid[3] == 0 and (scores[3] > thresh).all()
    e = E.recall_reference(gts, kept, [0.0, 0.5, 1.0], E.RANGES2)
    # the rounds stop at n: the rest is recorded as 0 and a threshold of 0.0 counts it; `>` in its place would not
    assert e['hits'][0, 0] == len(gts[1]) + len(gts[2]) and e['num_pos'][0] == sum(len(g) for g in gts)
    strict = E.recall_reference(gts, kept, E.strictly_above([0.0, 0.5, 1.0]), E.RANGES2)
    assert strict['hits'][0, 0] < e['hits'][0, 0]
