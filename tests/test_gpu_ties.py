"""Exact ties and threshold equalities in every ordering kernel, against the CPU oracle on the same input.

The rest of the suite feeds every discrete decision inputs on which no decision is close (tie-free scores, integer-free boxes).  The
product sees the opposite: a bf16 trunk hands the RPN 8-bit mantissas (thousands of anchors share a score), a trained head saturates
softmax to exactly 1.0f for several rois of one object, clip_boxes puts proposals on the integer image borders, one roi coordinate in
sixteen scales to an exact half, ReLU makes whole pooling bins tie at 0.  tests/golden/cases.py builds those inputs
(tests/test_ties_host.py asserts they have the property) and every test here compares the kernel with the oracle EXACTLY: indices,
kept sets, counts, argmax and boxes bit for bit.  The one exception are soft-NMS rescored values, which keep the bound the project
already uses for float64 post-processing (rtol 1e-10, DESIGN.md "Tolerances"; test_gpu_pipeline.py::test_postprocess_softnms_and_nms).

The rules held (DESIGN.md "Tolerances", "Ties"): equal scores -> larger original index first (proposal top-K, every NMS flavour,
soft-NMS at every pick); learn-NMS ranks -> smaller roi index first; `>` in nms_kernel.cu, `>=` against a double in cpu_nms.pyx,
`ovr <= thresh` keeps in nms.py; float32 `score > 1e-3`; `>=` at the image cut; C round() and the first maximum in ROIPooling; floor
in the FPN level.  No case is filtered or skipped; every index handed to a kernel is in range.
"""
import ctypes

import numpy as np
import pytest
import torch

import cases
from oracle import fpn as OF
from oracle import nms as ON
from oracle import postprocess as OPP
from oracle import proposal as OP
from oracle import roi_pooling as ORP

pytestmark = pytest.mark.gpu

F32 = np.float32
CFG = dict(feat_stride=16, scales=(4, 8, 16, 32), ratios=(0.5, 1, 2))
THRESHOLDS = (0.3, 0.5, 0.6, 0.7, 0.8, 0.9)


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib, operator_py
    lib.load()
    return ops, operator_py, lib


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


# =====================================================================================================================
# 1. proposal order and cut: relnet_topk_sort, propose_batch
# =====================================================================================================================
def _topk_case(name):
    """-> scores [B,n] float32, K"""
    n, K = 28728, 6000                                                     # 38 x 63 x 12 anchors, RPN_PRE_NMS_TOP_N
    if name == 'quantised_run_across_K':                                   # image 0: a run of 400 equal scores across position K; image 1: plain bf16 scores
        return np.stack([cases.quantised_scores(n, 1, 8, straddle=(K, 400)), cases.quantised_scores(n, 2, 8)]), K
    if name == 'all_equal':
        return np.stack([np.full(n, 0.5, F32), np.full(n, -np.inf, F32)]), K
    if name == 'neg_inf_rows':                                             # fewer finite scores than K: the -inf rows (min_size) tie among themselves INSIDE the top K
        s = np.stack([cases.quantised_scores(n, 3, 8), cases.quantised_scores(n, 4, 6)])
        rng = np.random.default_rng(5)
        s[0, rng.permutation(n)[:24000]] = -np.inf
        s[1, rng.permutation(n)[:n - K]] = -np.inf                         # exactly K finite
        return s, K
    if name == 'K_ge_n':
        return np.stack([cases.quantised_scores(5000, 6, 8), cases.quantised_scores(5000, 7, 4)]), K
    if name == 'per64_above_32768':                                        # the second instantiation of the kernel (n > 32 x 1024)
        m = 40000
        return np.stack([cases.quantised_scores(m, 8, 8, straddle=(K, 400)), np.full(m, 0.25, F32)]), K
    if name == 'per32_at_32768':
        m = 32768
        return np.stack([cases.quantised_scores(m, 9, 8, straddle=(8192, 64)), cases.quantised_scores(m, 10, 5)]), 8192
    raise KeyError(name)


@pytest.mark.parametrize('name', ['quantised_run_across_K', 'all_equal', 'neg_inf_rows', 'K_ge_n', 'per64_above_32768', 'per32_at_32768'])
def test_topk_sort_order_among_equal_scores(rn, name):
    ops, _, _ = rn
    scores, K = _topk_case(name)
    B, n = scores.shape
    boxes = np.stack([cases.random_boxes(n, 50 + b) for b in range(B)])
    det, index, count = ops.topk_sort(_dev(scores), _dev(boxes), K)
    det, index, count = det.cpu().numpy(), index.cpu().numpy(), count.cpu().numpy()
    k = min(K, n)
    assert index.shape == (B, k)
    for b in range(B):
        want = ON.argsort_desc(scores[b])[:k]
        tied = len(want) - len(np.unique(scores[b][want]))
        print('%s image %d: %d of the top %d share a score with another; run of the last score: %d' %
              (name, b, tied, k, int((scores[b] == scores[b][want[-1]]).sum())))
        assert tied > 0
        assert np.array_equal(index[b], want), (name, b, np.flatnonzero(index[b] != want)[:8])
        assert count[b] == int(np.isfinite(scores[b][want]).sum())
        assert np.array_equal(det[b, :, :4], boxes[b][want]) and np.array_equal(det[b, :, 4], scores[b][want])


def _tied_rpn_case(seed, height=38, width=63, num_anchors=12):
    """rpn_case with what the bf16 trunk and clip_boxes make of it: fg scores on the bf16 grid (thousands of ties) and deltas on a
    grid of 0.5, large enough that many proposals are clipped to the image borders and to the SAME box."""
    rng = np.random.default_rng(seed)
    fg = cases.quantised_scores(num_anchors * height * width, seed, 8).reshape(1, num_anchors, height, width)
    cls_prob = np.concatenate((F32(1) - fg, fg), axis=1).astype(F32)
    deltas = (np.round(rng.normal(0, 0.7, (1, 4 * num_anchors, height, width)) * 2) / 2).astype(F32)
    im_info = np.array([[cases.IM_H, cases.IM_W, 1.0]], dtype=F32)
    return cls_prob, deltas, im_info


@pytest.mark.parametrize('seed,thresh,min_size', [(21, 0.7, 0), (22, 0.7, 16), (23, 0.3, 16)])
def test_proposal_operator_on_tied_scores_and_duplicated_boxes(rn, seed, thresh, min_size):
    ops, _, _ = rn
    from relnet_amd.operator_py import proposal as P
    cs = [_tied_rpn_case(seed), _tied_rpn_case(seed + 100)]
    anchors = _dev(P.generate_anchors(16, CFG['ratios'], CFG['scales']))
    rois, scores, d = P.propose_batch(_dev(np.concatenate([c[0] for c in cs])), _dev(np.concatenate([c[1] for c in cs])),
                                      _dev(np.concatenate([c[2] for c in cs])), anchors, 16, 6000, 300, thresh, min_size, want_debug=True)
    for b, c in enumerate(cs):
        rois_o, scores_o, dbg = OP.proposal(*c, pre_nms_top_n=6000, post_nms_top_n=300, threshold=thresh, min_size=min_size,
                                            return_debug=True, **CFG)
        det_o = dbg['det']
        dup = len(det_o) - len({tuple(r) for r in det_o[:, :4]})
        tied = len(det_o) - len(np.unique(det_o[:, 4]))
        print('image %d: %d of 6000 sorted rows repeat a box, %d share a score, %d kept' % (b, dup, tied, dbg['n_kept']))
        assert dup >= 50 and tied > 3000
        assert np.array_equal(d['order'][b].cpu().numpy(), dbg['order'])
        assert np.array_equal(d['det'][b].cpu().numpy(), det_o)
        nk = int(d['num_keep'][b])
        keep = d['keep'][b].cpu().numpy()[:min(nk, 300)]
        assert np.array_equal(keep, dbg['keep'][:len(keep)])
        got = rois[b].cpu().numpy()
        assert (got[:, 0] == b).all()
        if dbg['n_kept'] >= 300:
            assert np.array_equal(got[:, 1:], rois_o[:, 1:])
            assert np.array_equal(scores[b].cpu().numpy().reshape(-1, 1), scores_o)
        else:                                                              # fewer survivors than rows: the pad rows repeat kept rows
            assert nk == dbg['n_kept']
            assert np.array_equal(got[:nk, 1:], rois_o[:nk, 1:])
            kept = {tuple(x) for x in got[:nk]}
            assert all(tuple(x) in kept for x in got[nk:])


# =====================================================================================================================
# 2. proposal NMS: relnet_nms_mask/_scan, relnet_nms_greedy, _nms, gpu_nms, cpu_nms
# =====================================================================================================================
def _boundary_dets(thresh, n=200):
    """[n,5] float32 rows in descending score order (row order == scan order): disjoint filler boxes, and pairs whose IoU is exactly
    the threshold, one float32 step above it and one below it, at chosen scan positions: inside one 64-box tile of the suppression
    mask, across the tile edge 63 | 64 and 127 | 128, and tiles apart.  Every pair sits at its own translation, far from the others."""
    p = cases.iou_boundary_pairs(thresh)
    dets = np.zeros((n, 5), F32)
    for i in range(n):
        dets[i, :4] = [40 * i, 30000, 40 * i + 9, 30009]
    dets[:, 4] = np.linspace(0.99, 0.01, n).astype(F32)
    place = [('eq', p['eq'][0], 5, 6), ('eq', p['eq'][1], 63, 64), ('eq', p['eq'][0], 20, 190), ('eq', p['eq'][1], 127, 128),
             ('above', p['above'], 60, 61), ('above', p['above'], 62, 129), ('above', p['above'], 126, 131),
             ('below', p['below'], 100, 101), ('below', p['below'], 59, 65), ('below', p['below'], 125, 192)]
    kinds = {}
    for j, (kind, (a, b), ia, ib) in enumerate(place):
        off = np.array([6000 * j, 0, 6000 * j, 0], F32)
        dets[ia, :4] = a + off
        dets[ib, :4] = b + off
        kinds[ib] = kind
    assert len(np.unique(dets[:, 4])) == n
    return dets, kinds


@pytest.mark.parametrize('thresh', THRESHOLDS)
def test_proposal_nms_at_the_threshold(rn, thresh):
    """IoU == thresh: `>` keeps (nms_kernel.cu:71).  One float32 step above: suppressed.  One below: kept.  cpu_nms compares the float32
    overlap `>=` the DOUBLE thresh (cpu_nms.pyx): at 0.7 and 0.9 an overlap of exactly float32(thresh) lies below the double and is
    kept, at the others it is suppressed."""
    ops, _, lib = rn
    from relnet_amd import nms as NT
    dets, kinds = _boundary_dets(thresh)
    n = len(dets)
    want = ON.gpu_nms(dets, thresh)
    want_cpu = ON.cpu_nms(dets, thresh)
    for ib, kind in kinds.items():                                         # the construction does what it says, in the oracle
        assert (ib in want) == (kind != 'above'), (ib, kind)
        assert (ib in want_cpu) == (kind == 'below' or (kind == 'eq' and float(F32(thresh)) < thresh)), (ib, kind)
    d = _dev(dets[None])
    r = ops.nms_sorted(d, thresh, want_keep=True)
    assert r['keep'][0, :int(r['num_keep'][0])].cpu().tolist() == want
    r = ops.nms_greedy(d, thresh, n, want_keep=True)
    assert r['keep'][0, :int(r['num_keep'][0])].cpu().tolist() == want
    keep = np.zeros(n, dtype=np.int32)
    num = ctypes.c_int(0)
    lib.load()._nms(keep.ctypes.data, ctypes.addressof(num), dets.ctypes.data, n, 5, thresh, 0)
    assert keep[:num.value].tolist() == want
    assert [int(i) for i in NT.gpu_nms(dets, thresh)] == want
    assert NT.gpu_nms_wrapper(thresh, 0)(dets) is not None
    assert [int(i) for i in NT.cpu_nms(dets, thresh)] == want_cpu
    assert [int(i) for i in NT.cpu_nms_wrapper(thresh)(dets)] == want_cpu
    # the same rows as float64 `dets` through nms.py's greedy NMS (ovr <= thresh keeps; N = 200 -> the 5-wavefront launch)
    d64 = dets.astype(np.float64)
    want_py = [int(i) for i in ON.py_nms(d64, thresh)]
    for ib, kind in kinds.items():
        assert (ib in want_py) == (kind != 'above')
    assert [int(i) for i in NT.nms(d64, thresh)] == want_py
    assert [int(i) for i in NT.py_nms_wrapper(thresh)(d64)] == want_py


@pytest.mark.parametrize('thresh', [0.3, 0.7])
def test_proposal_nms_twins_on_tied_scores_and_duplicated_boxes(rn, thresh):
    _, _, _ = rn
    from relnet_amd import nms as NT
    n = 300
    dets = np.hstack((cases.lattice_boxes(n, 31), cases.quantised_scores(n, 32, 4)[:, None])).astype(F32)
    dets[1::5, :4] = dets[0:-1:5, :4][:len(dets[1::5])]                    # duplicated boxes, some with tied scores
    assert len(np.unique(dets[:, 4])) < n // 4 and len({tuple(r) for r in dets[:, :4]}) < n
    assert [int(i) for i in NT.gpu_nms(dets, thresh)] == [int(i) for i in ON.gpu_nms(dets, thresh)]
    assert [int(i) for i in NT.cpu_nms(dets, thresh)] == ON.cpu_nms(dets, thresh)
    d64 = dets.astype(np.float64)
    assert [int(i) for i in NT.nms(d64, thresh)] == [int(i) for i in ON.py_nms(d64, thresh)]


# =====================================================================================================================
# 3 + 4. class threshold, per-class soft-NMS and NMS: relnet_class_nms(_ex, _topk), nms / soft_nms / py_*_wrapper
# =====================================================================================================================
def _oracle_class_lists(prob, boxes, thresh, param, soft):
    """tester.py:244-268 per class on one image -> list over classes 1..C-1 of (rows [k,5] float64 in pick order, roi index of every pick)."""
    out = []
    for j in range(1, prob.shape[1]):
        idx = np.where(prob[:, j] > thresh)[0]                             # numpy compares the float32 column with float32(1e-3)
        cls_dets = np.hstack((boxes[idx], prob[idx, j, None].astype(np.float64)))
        if soft:
            rows, keep = ON.soft_nms(cls_dets, param, -1, return_index=True)
        else:
            keep = np.asarray(ON.py_nms(cls_dets, param), dtype=np.intp)
            rows = cls_dets[keep] if len(keep) else np.zeros((0, 5))
        out.append((rows, idx[keep] if len(keep) else np.zeros(0, np.intp)))
    return out


def _same_rows(got, want, soft, what):
    assert np.array_equal(got[:, :4], want[:, :4]), what
    if soft:                                                               # float64 post-processing bound of DESIGN.md; exp() is the only inexact step
        np.testing.assert_allclose(got[:, 4], want[:, 4], rtol=1e-10, atol=0, err_msg=str(what))
    else:
        assert np.array_equal(got[:, 4], want[:, 4]), what


# one N per launch shape of launch_class_nms: <= 64, <= 128, <= 320, <= 512, <= 1024 candidates = 1, 2, 5, 8, 16 wavefronts
@pytest.mark.parametrize('N', [37, 100, 300, 500, 1004])
@pytest.mark.parametrize('soft,param', [(True, 0.6), (False, 0.5)])
def test_class_nms_on_saturated_posteriors(rn, N, soft, param):
    ops, _, _ = rn
    B, C = 2, 21
    prob, boxes, info = cases.saturated_posteriors(B, N, C, 300 + N)
    dp, db = _dev(prob), _dev(boxes)
    full, nf, index = ops.class_nms(dp, db, 1e-3, param, soft, want_index=True)
    prn, npn = ops.class_nms(dp, db, 1e-3, param, soft, max_picks=100, top_k=100)
    full, nf, index, prn, npn = (t.cpu().numpy() for t in (full, nf, index, prn, npn))
    out, cnt, thr, tot = ops.image_topk(_dev(prn), _dev(npn), 100)
    out, cnt, thr, tot = (t.cpu().numpy() for t in (out, cnt, thr, tot))
    waves = {len({i // 64 for i in idx}) for _, idx in info['clusters']}
    assert 1 in waves and (N <= 64 or max(waves) > 1)                      # tied candidates inside one wavefront AND in different ones
    tied_picks = 0
    for b in range(B):
        lists = _oracle_class_lists(prob[b], boxes[b], 1e-3, param, soft)
        for c, (rows, picks) in enumerate(lists):
            what = (N, soft, b, c + 1)
            k = len(rows)
            tied_picks += k - len(np.unique(rows[:, 4]))
            # the unpruned kernel: the whole list, and the roi index of every pick
            assert nf[b, c] == k, what
            assert np.array_equal(index[b, c, :k], picks), (what, index[b, c, :k][:12], picks[:12])
            _same_rows(full[b, c, :k], rows, soft, what)
            assert not full[b, c, k:].any() and (index[b, c, k:] == -1).all()
            # the pruned kernel: a prefix of the ORACLE's list
            kp = npn[b, c]
            assert kp <= min(k, 100) and (kp >= 1 or k == 0), what
            _same_rows(prn[b, c, :kp], rows[:kp], soft, what)
            assert not prn[b, c, kp:].any()
        # the constructed class: the rows AT float32(1e-3) and below are no candidates, the three one float above are
        assert nf[b, C - 2] == (10 if soft else len(lists[C - 2][0])) and len(lists[C - 2][0]) >= 8
        con = info['constructed']
        lastp = list(lists[C - 2][1])
        assert all(i in lastp for i in info['threshold_rows']['up'])
        assert not any(i in lastp for i in info['threshold_rows']['eq'] + info['threshold_rows']['down'])
        if soft:                                                           # ties after a rescoring: larger roi index first
            assert lastp.index(con['B']) + 1 == lastp.index(con['A']) and lastp.index(con['M2']) + 1 == lastp.index(con['M1'])
            assert lastp[-3:] == info['threshold_rows']['up'][::-1]
        # the image cut over the pruned lists == the oracle's over its full lists
        kept, othr, ototal = OPP.image_cut([rows for rows, _ in lists], 100)
        n_kept = sum(len(x) for x in kept)
        assert cnt[b] == min(n_kept, out.shape[1])
        if soft:
            np.testing.assert_allclose(thr[b], othr, rtol=1e-10, atol=0)
        else:
            assert thr[b] == othr
        pos = 0
        for c, x in enumerate(kept):                                       # class-major, pick order; float32 of the (verified) float64 rows
            for q in range(len(x)):
                if pos < out.shape[1]:
                    assert out[b, pos, 0] == c + 1 and np.array_equal(out[b, pos, 2:], x[q, :4].astype(F32)), (N, b, c, q)
                    assert out[b, pos, 1] == F32(prn[b, c, q, 4])
                pos += 1
    print('N=%d soft=%s: %d picks share their final score with another pick of their class' % (N, soft, tied_picks))
    assert tied_picks > 0


SOFT_NMS_CASES = {
    # name: float64 dets, expected pick order (the rule: at each pick the largest original index among equal CURRENT scores)
    'four_disjoint_all_tied': ([[0, 0, 10, 10, .5], [20, 0, 30, 10, .5], [40, 0, 50, 10, .5], [60, 0, 70, 10, .5]], [3, 2, 1, 0]),
    'two_overlapping_pairs_all_tied': ([[0, 0, 10, 10, .5], [5, 0, 15, 10, .5], [100, 0, 110, 10, .5], [103, 0, 113, 10, .5]], [3, 1, 0, 2]),
    'tie_behind_the_first_pick': ([[0, 0, 10, 10, .9], [200, 0, 210, 10, .5], [400, 0, 410, 10, .5]], [0, 2, 1]),
}


@pytest.mark.parametrize('name', sorted(SOFT_NMS_CASES))
def test_soft_nms_twins_small_tie_cases(rn, name):
    """The cases of the tie rule written out by hand: kernel (through nms/nms.py), oracle and the expected order agree, and the
    rescored numbers with them (with overlapping tied boxes the NUMBERS depend on the order, not only the order itself)."""
    from relnet_amd import nms as NT
    rows, order = SOFT_NMS_CASES[name]
    dets = np.array(rows, dtype=np.float64)
    want, keep = ON.soft_nms(dets, 0.6, return_index=True)
    assert list(keep) == order
    if name == 'two_overlapping_pairs_all_tied':
        np.testing.assert_allclose(want[:, 4], [.5, .5, .39553256, .29014779], rtol=1e-7)
    for fn in (lambda d: NT.soft_nms(d, 0.6, -1), NT.py_softnms_wrapper(0.6)):
        d = dets.copy()
        got = fn(d)
        assert np.array_equal(got[:, :4], want[:, :4])
        np.testing.assert_allclose(got[:, 4], want[:, 4], rtol=1e-10, atol=0)
        np.testing.assert_allclose(d[keep, 4], want[:, 4], rtol=1e-10, atol=0)          # written back into the caller's array (nms.py:114)
    got = NT.soft_nms(dets.copy(), 0.6, 2)
    assert np.array_equal(got[:, :4], want[:2, :4])


@pytest.mark.parametrize('N', [37, 300, 1004])
def test_nms_twins_on_a_saturated_class(rn, N):
    """nms / soft_nms of nms/nms.py (float64 `dets`, the scores64 form of the kernel) on the candidates of one saturated class."""
    from relnet_amd import nms as NT
    prob, boxes, info = cases.saturated_posteriors(1, N, 21, 300 + N)
    for j in (2, 4):
        idx = np.where(prob[0, :, j] > 1e-3)[0]
        dets = np.hstack((boxes[0, idx], prob[0, idx, j, None].astype(np.float64)))
        assert (dets[:, 4] == 1.0).sum() >= 2
        want, keep = ON.soft_nms(dets, 0.6, return_index=True)
        got = NT.soft_nms(dets.copy(), 0.6, -1)
        assert np.array_equal(got[:, :4], want[:, :4])
        np.testing.assert_allclose(got[:, 4], want[:, 4], rtol=1e-10, atol=0)
        assert [int(i) for i in NT.nms(dets, 0.5)] == [int(i) for i in ON.py_nms(dets, 0.5)]


# =====================================================================================================================
# 5. image cut: relnet_image_topk
# =====================================================================================================================
@pytest.mark.parametrize('name,NC,N,seed,kw,path,overflow', [
    ('lds_ties_kept', 20, 64, 10, dict(counts_hi=30), 'lds', False),
    ('lds_more_ties_than_rows', 20, 64, 9, dict(counts_hi=64), 'lds', True),
    ('general_ties_kept', 80, 100, 11, dict(counts_hi=100, counts_lo=70, levels=400), 'general', False),
    ('general_more_ties_than_rows', 80, 100, 12, dict(counts_hi=100, counts_lo=70), 'general', True)])
def test_image_topk_ties_at_the_cut(rn, name, NC, N, seed, kw, path, overflow):
    """Every detection tied with the max_per_image-th score is kept (tester.py:273 `>=`), so more than max_per_image rows come out; when
    they exceed the max_per_image + 28 rows of `out`, out_count == max_out and the rows are the class-major prefix of the oracle's list."""
    ops, _, _ = rn
    B, mpi = 2, 100
    dets, counts = cases.tied_image_lists(B, NC, N, seed, **kw)
    out, cnt, thr, tot = (t.cpu().numpy() for t in ops.image_topk(_dev(dets), _dev(counts), mpi))
    max_out = out.shape[1]
    assert max_out == mpi + 28
    for b in range(B):
        lists = [dets[b, c, :counts[b, c]] for c in range(NC)]
        kept, othr, ototal = OPP.image_cut(lists, mpi)
        n_kept = sum(len(x) for x in kept)
        print('%s image %d: total %d, kept %d, threshold %r' % (name, b, ototal, n_kept, othr))
        assert (ototal > 6144) == (path == 'general')                      # (kTopkKeys: which path of the kernel the case takes)
        assert n_kept > mpi and (n_kept > max_out) == overflow
        assert tot[b] == ototal and thr[b] == othr
        assert cnt[b] == min(n_kept, max_out)
        want = np.array([[c + 1, x[q, 4], x[q, 0], x[q, 1], x[q, 2], x[q, 3]] for c, x in enumerate(kept) for q in range(len(x))]).astype(F32)
        assert np.array_equal(out[b, :cnt[b]], want[:cnt[b]])
        assert not out[b, cnt[b]:].any()


# =====================================================================================================================
# 6. ROI max pooling: relnet_roi_pool_fwd / _fpn_fwd (both kernels), relnet_roi_pool_bwd (scatter and owner form)
# =====================================================================================================================
def _lattice_rois(R, B, seed, stride=16):
    boxes = cases.lattice_boxes(R, seed, stride=stride)
    bidx = (np.arange(R) * 7 % B).astype(F32)                              # batch indices inside [0, B)
    return np.hstack((bidx[:, None], boxes)).astype(F32)


def _bwd_definition(argmax, gout, rois, B, C, H, W):
    """grad_in[b, c, argmax[r, c, ph, pw]] += grad_out[r, c, ph, pw] in float64."""
    want = np.zeros((B, C, H * W))
    R = argmax.shape[0]
    a = argmax.reshape(R, C, -1); v = gout.reshape(R, C, -1).astype(np.float64)
    for r in range(R):
        for k in range(a.shape[2]):
            ok = a[r, :, k] >= 0
            np.add.at(want[int(rois[r, 0])], (np.nonzero(ok)[0], a[r, ok, k]), v[r, ok, k])
    return want.reshape(B, C, H, W)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_roi_pool_nchw_values_and_argmax_on_tied_bins(rn, dtype):
    """roi_pool_fwd_kernel<float> and <bf16> (NCHW maps): values AND argmax against the oracle on lattice rois over a ReLU-tied map; then
    the scatter backward on that argmax against the definition."""
    ops, _, _ = rn
    B, C, H, W, R = 2, 16, 38, 63, 64
    data = cases.relu_tied_map(B, C, H, W, 41)
    rois = _lattice_rois(R, B, 42)
    want, warg = ORP.roi_pooling(data, rois, return_argmax=True)
    assert (warg == -1).sum() >= 2 * 49 * C and (want == 0).mean() > 0.1
    out, arg = ops.roi_pool(_dev(data).to(dtype), _dev(rois), want_argmax=True)
    assert np.array_equal(out.float().cpu().numpy(), want)
    assert np.array_equal(arg.cpu().numpy(), warg), int((arg.cpu().numpy() != warg).sum())
    gout = np.random.default_rng(43).normal(0, 1, want.shape).astype(F32)
    gin = ops.roi_pool_bwd(_dev(gout), arg, _dev(rois), (B, C, H, W))
    ref = _bwd_definition(warg, gout, rois, B, C, H, W)
    assert np.abs(gin.double().cpu().numpy() - ref).max() <= 2e-5 * np.abs(ref).max()


def test_roi_pool_channels_last_values_argmax_and_both_backward_forms(rn):
    """roi_pool_fwd_cl_kernel<ARGMAX = true / false> (bf16 channels-last, the pipeline's kernel): values and ARGMAX against the oracle --
    half-away rounding of the roi corners, first maximum in row-major order, all-zero bins, empty bins -> -1.  Then relnet_roi_pool_bwd_cl
    in owner form (2 images x 1024 channels: one workgroup per (image, 8 channels)) and in scatter form on that argmax, against the
    definition in float64 at 2e-5 of scale."""
    ops, _, lib = rn
    B, C, H, W, R = 2, 1024, 38, 63, 48
    data = cases.relu_tied_map(B, C, H, W, 44)
    rois = _lattice_rois(R, B, 45)
    want, warg = ORP.roi_pooling(data, rois, return_argmax=True)
    cl = _dev(data).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    drois = _dev(rois)
    out, arg = ops.roi_pool(cl, drois, channels_last_out=True, want_argmax=True)
    assert out.permute(0, 2, 3, 1).is_contiguous()
    assert np.array_equal(out.float().cpu().numpy(), want)
    got = arg.cpu().numpy()
    assert np.array_equal(got, warg), (int((got != warg).sum()), got.size)
    out2 = ops.roi_pool(cl, drois, channels_last_out=True)                # ARGMAX = false instantiation
    assert np.array_equal(out2.float().cpu().numpy(), want)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(46)).cuda().contiguous(memory_format=torch.channels_last)
    assert gout.stride() == arg.stride()
    ref = _bwd_definition(warg, gout.cpu().numpy(), rois, B, C, H, W)
    scale = np.abs(ref).max()
    for mode in (1, 0):                                                    # 1: atomic scatter kernel only; 0: owner form where it applies (it does here)
        lib.load().relnet_roi_pool_bwd_debug(mode)
        try:
            gin = ops.roi_pool_bwd(gout, arg, drois, (B, C, H, W), channels_last=True).clone()
        finally:
            lib.load().relnet_roi_pool_bwd_debug(0)
        assert np.abs(gin.double().cpu().numpy() - ref).max() <= 2e-5 * scale, mode


@pytest.mark.parametrize('layout', ['nchw_f32', 'cl_bf16'])
def test_roi_pool_fpn_values_and_argmax_on_tied_bins(rn, layout):
    """relnet_roi_pool_fpn_fwd: every pyramid level gets rois on ITS half lattice (odd multiples of stride / 2), level-sorted."""
    ops, _, _ = rn
    B, C = 2, (16 if layout == 'nchw_f32' else 256)
    strides = (4, 8, 16, 32)
    feats = [cases.relu_tied_map(B, C, -(-cases.IM_H // s), -(-cases.IM_W // s), 50 + s) for s in strides]
    per = [_lattice_rois(24, B, 60 + s, stride=s) for s in strides]
    rois = np.concatenate(per)
    level = np.repeat(np.arange(4), 24).astype(np.int32)
    wants = [ORP.roi_pooling(feats[l], per[l], (7, 7), 1.0 / s, return_argmax=True) for l, s in enumerate(strides)]
    want = np.concatenate([w[0] for w in wants]); warg = np.concatenate([w[1] for w in wants])
    if layout == 'nchw_f32':
        lv = [_dev(f) for f in feats]
        out, arg = ops.roi_pool_fpn(lv, [1.0 / s for s in strides], _dev(rois), _dev(level), want_argmax=True)
    else:
        lv = [_dev(f).to(torch.bfloat16).contiguous(memory_format=torch.channels_last) for f in feats]
        out, arg = ops.roi_pool_fpn(lv, [1.0 / s for s in strides], _dev(rois), _dev(level), channels_last_out=True, want_argmax=True)
    assert np.array_equal(out.float().cpu().numpy(), want)
    assert np.array_equal(arg.cpu().numpy(), warg)


# =====================================================================================================================
# 7. FPN level assignment: relnet_fpn_roi_dispatch(_ex)
# =====================================================================================================================
def test_fpn_dispatch_on_the_level_boundaries(rn):
    ops, _, _ = rn
    edge, s = cases.fpn_boundary_rois()
    boxes = np.stack([np.concatenate((edge, cases.fpn_proposals(51, 71))), np.concatenate((cases.fpn_proposals(51, 72), edge[::-1]))])
    rois, level, perm, counts = ops.fpn_roi_dispatch(_dev(boxes))
    with np.errstate(divide='ignore'):
        for b in range(2):
            wr, wl, wp, wc = OF.roi_dispatch(boxes[b], dummy_for_empty=False)
            wr[:, 0] = b
            assert np.array_equal(counts[b].cpu().numpy(), wc)
            assert np.array_equal(level[b].cpu().numpy(), wl)
            assert np.array_equal(perm[b].cpu().numpy(), wp)
            assert np.array_equal(rois[b].cpu().numpy(), wr)
        lv = OF.roi_levels(edge)
    assert lv[0] == 1 and lv[1] == 0 and lv[3] == 2 and lv[4] == 1 and lv[6] == 3          # ON a boundary: up; one float32 step below: down


def test_fpn_dispatch_tied_level_counts_and_empty_levels(rn):
    """Equal counts in several levels and empty levels with pad_empty: the dummy rows of rcnn.py:61-71, level-major order kept."""
    ops, _, _ = rn
    edge, _ = cases.fpn_boundary_rois()
    with np.errstate(divide='ignore'):
        lv = OF.roi_levels(edge)
        img0 = np.concatenate([edge[lv == 1][:3], edge[lv == 3][:3], edge[lv == 2][:3]])             # 0 / 3 / 2 / 3
        img1 = np.concatenate([edge[lv == 2][:2], edge[lv == 0][:2], edge[lv == 0][:2], edge[lv == 2][:3]])[:9]      # 4 / 0 / 4 / 0
        boxes = np.stack([img0, img1])
        rois, level, perm, counts, n_rows = ops.fpn_roi_dispatch(_dev(boxes), pad_empty=True)
        for b in range(2):
            wr, wl, wp, wc = OF.roi_dispatch(boxes[b], dummy_for_empty=True)
            wr[:, 0] = b
            n = int(n_rows[b])
            assert n == len(wr) and np.array_equal(counts[b].cpu().numpy(), wc)
            assert np.array_equal(rois[b, :n].cpu().numpy(), wr)
            assert np.array_equal(level[b, :n].cpu().numpy(), wl)
            assert np.array_equal(perm[b, :n].cpu().numpy(), wp)
            assert (perm[b, n:] == -1).all() and (rois[b, n:, 1:] == 0).all()
    assert counts[0].cpu().tolist() == [0, 3, 2, 3] and counts[1].cpu().tolist() == [4, 0, 4, 0]


# =====================================================================================================================
# 8. learn-NMS ranks: relnet_lnms_sort
# =====================================================================================================================
@pytest.mark.parametrize('N,C,first_n', [(300, 80, 100), (37, 6, 20), (1000, 8, 150), (1024, 4, 1024)])
def test_lnms_sort_tied_class_scores(rn, N, C, first_n):
    """Tied class scores: the reference's `argsort(-prob, kind='stable')` (operator_py/learn_nms.py) puts the SMALLER roi index first.
    rank_idx, sorted_score, sorted_bbox (and the class-major copy, the class maximum) exact.  N not a power of two (and one that is)."""
    ops, _, lib = rn
    B = 2
    rng = np.random.default_rng(80 + N)
    prob = np.stack([cases.quantised_scores(N * C, 81 + b, 4).reshape(N, C) for b in range(B)])
    prob[:, 1::3] = prob[:, 0:-1:3][:, :prob[:, 1::3].shape[1]]            # duplicated posterior rows: ties in every class at once
    prob[1, :, 0] = F32(0.125)                                             # a class in which every roi ties
    boxes = np.stack([cases.random_boxes(N, 90 + b) for b in range(B)])
    F = first_n
    dev = 'cuda'
    rank_idx = torch.empty((B, C, F), device=dev, dtype=torch.int32)
    sorted_score = torch.empty((B, F, C), device=dev, dtype=torch.float32)
    sorted_bbox = torch.empty((B, F, C, 4), device=dev, dtype=torch.float32)
    class_boxes = torch.empty((B, C, F, 4), device=dev, dtype=torch.float32)
    class_max = torch.empty((B, C), device=dev, dtype=torch.float32)
    dp, db = _dev(prob), _dev(boxes)
    lib.call('relnet_lnms_sort', dp.data_ptr(), db.data_ptr(), rank_idx.data_ptr(), sorted_score.data_ptr(), sorted_bbox.data_ptr(),
             class_boxes.data_ptr(), class_max.data_ptr(), B, N, C, F, ops._stream())
    torch.cuda.synchronize()
    for b in range(B):
        rank = np.argsort(-prob[b], axis=0, kind='stable')[:F]              # oracle/learn_nms.py: [F, C]
        ss = np.take_along_axis(prob[b], rank, axis=0)
        assert (np.diff(ss, axis=0) == 0).sum() > F                        # the ranked lists do contain ties
        assert np.array_equal(rank_idx[b].cpu().numpy(), rank.T)
        assert np.array_equal(sorted_score[b].cpu().numpy(), ss)
        assert np.array_equal(sorted_bbox[b].cpu().numpy(), boxes[b][rank])
        assert np.array_equal(class_boxes[b].cpu().numpy(), boxes[b][rank].transpose(1, 0, 2))
        assert np.array_equal(class_max[b].cpu().numpy(), ss[0])


# =====================================================================================================================
# 9. training targets: relnet_assign_anchor, relnet_proposal_target_ex, relnet_box_annotator_ohem, relnet_nms_multi_target
# =====================================================================================================================
def _anchor_tie_gts():
    """gt boxes placed against the ratio-1 / scale-8 anchors (128 x 128 at [8 + 16 i, 8 + 16 j, 135 + 16 i, 135 + 16 j], base anchor 5):
      0      == anchor (2, 2): overlap exactly 1;
      1, 2   anchor (20, 2) moved 8 left and 8 right: that anchor overlaps BOTH equally (argmax -> the first gt), and each of the two
             lies midway between two anchors, which tie for its best overlap (rpn.py:170: every anchor that ties -> 1);
      3      100 x 100 inside four anchors at once: all four tie at 10000 / 16384 < 0.7 and are fg by the tie rule alone;
      4      overlap with anchor (30, 12) exactly 0.7 = 11648 / 16640 in float64 (`>= 0.7` -> fg);
      5      overlap with anchor (45, 12) exactly 0.3 = 4992 / 16640 (`< 0.3` is false -> not bg)."""
    return np.array([[40, 40, 167, 167, 1], [320, 40, 447, 167, 2], [336, 40, 463, 167, 3], [94, 222, 193, 321, 4],
                     [525, 200, 617, 327, 5], [817, 200, 857, 327, 6]], F32)


def test_assign_anchor_ties_and_threshold_equalities(rn):
    ops, _, _ = rn
    from oracle import anchors as OA
    from relnet_amd.operator_py.proposal import generate_anchors
    gt = _anchor_tie_gts()
    fh, fw, A = 38, 63, 12
    base = generate_anchors(16, (0.5, 1, 2), (4, 8, 16, 32))
    assert np.array_equal(base[5], [-56, -56, 71, 71])
    gts = [gt, gt[::-1].copy(), gt[[1, 2]]]
    B, G = len(gts), 6
    pad = np.zeros((B, G, 5), F32)
    for b, x in enumerate(gts):
        pad[b, :len(x)] = x
    num_gt = torch.tensor([len(x) for x in gts], dtype=torch.int32).cuda()
    im_info = torch.tensor([[600, 1000, 1.0]] * B).cuda()
    seed = 77
    L, T, W, Lall = ops.assign_anchor(_dev(pad), num_gt, im_info, base, (fh, fw), seed=seed, want_all=True)
    at = lambda i, j: 5 * fh * fw + (4 + j) * fw + (4 + i)                # label index of anchor (i, j) of base anchor 5
    for b in range(B):
        with np.errstate(divide='ignore'):                                 # (the oracle masks the quotients of disjoint pairs afterwards)
            wl, wt, ww, wall = OA.assign_anchor((fh, fw), gts[b], (600, 1000), sampler='hash', seed=seed, image_index=b, return_all=True)
        assert np.array_equal(Lall[b].cpu().numpy(), wall), (b, np.flatnonzero(Lall[b].cpu().numpy() != wall)[:8])
        assert np.array_equal(L[b].cpu().numpy(), wl), b
        assert np.array_equal(W[b].cpu().numpy(), ww), b
        assert np.abs(T[b].cpu().numpy() - wt).max() <= 1e-6, b
    # the construction, in the oracle: exact equalities exist and decide labels
    with np.errstate(divide='ignore'):
        wl, wt, ww, wall = OA.assign_anchor((fh, fw), gt, (600, 1000), sampler='hash', seed=seed, return_all=True)
        wt2 = OA.assign_anchor((fh, fw), gt[::-1].copy(), (600, 1000), sampler='hash', seed=seed, image_index=1)[1]
    anc = lambda i, j: np.array([[8 + 16 * i, 8 + 16 * j, 135 + 16 * i, 135 + 16 * j]], np.float64)
    assert OA.overlaps64(anc(30, 12), gt[4:5, :4])[0, 0] == 0.7 and OA.overlaps64(anc(45, 12), gt[5:6, :4])[0, 0] == 0.3
    assert wall[at(30, 12)] == 1 and wall[at(45, 12)] == -1
    assert all(wall[at(i, j)] == 1 for i in (4, 5) for j in (12, 13))                  # four anchors tie gt 3's best overlap
    assert OA.overlaps64(anc(4, 12), gt[3:4, :4])[0, 0] == OA.overlaps64(anc(5, 13), gt[3:4, :4])[0, 0] < 0.7
    assert wall[at(19, 2)] == 1 and wall[at(20, 2)] == 1 and wall[at(21, 2)] == 1
    assert wt[5 * 4, 4 + 2, 4 + 20] == F32(-8.0 / 128)                                 # anchor (20, 2): the FIRST of its two equal gts
    assert wt2[5 * 4, 4 + 2, 4 + 20] == F32(8.0 / 128)                                 # gt order reversed: the other one


def test_proposal_target_ties_and_fg_threshold_equality(rn):
    """sample_rois_v2 (rcnn.py:303-316): `overlaps.argmax(axis=1)` -> the FIRST of two gts with the same overlap; `max_overlaps < 0.5` -> bg,
    so an overlap of exactly 0.5 is foreground."""
    ops, _, _ = rn
    from oracle import targets as OT
    gt = np.array([[100, 100, 109, 109, 7], [300, 100, 319, 119, 9], [292, 100, 311, 119, 11], [500, 300, 599, 399, 13], [500, 300, 599, 399, 14]], F32)
    rois = [[100, 100, 109, 104], [100, 100, 109, 109], [100, 100, 106, 106], [100, 100, 109, 105],       # 0.5 exactly, 1, 0.49, 0.6
            [296, 100, 315, 119],                                                                         # equal overlap with gt 1 and gt 2
            [500, 300, 599, 399], [500, 300, 599, 349], [510, 310, 589, 389]]                             # duplicated gt 3 / gt 4: first wins
    rois += [list(r) for r in cases.random_boxes(24, 95)]
    rois = np.hstack((np.zeros((len(rois), 1), F32), np.asarray(rois, F32)))
    wr, wl, wt, ww = OT.proposal_target(rois, gt)
    assert list(wl[:8]) == [7, 7, 0, 7, 9, 13, 13, 13]
    both = np.stack([rois, rois[::-1].copy()])
    gts = np.stack([gt, gt[[2, 1, 0, 4, 3]]])
    r, lab, bt, bw = ops.proposal_target(_dev(both), _dev(gts))
    for b in range(2):
        wr, wl, wt, ww = OT.proposal_target(both[b], gts[b])
        wr = wr.copy(); wr[len(rois):, 0] = b
        assert np.array_equal(lab[b].cpu().numpy(), wl), (b, lab[b].cpu().numpy()[:8], wl[:8])
        assert np.array_equal(r[b].cpu().numpy(), wr)
        assert np.array_equal(bt[b].cpu().numpy(), wt) and np.array_equal(bw[b].cpu().numpy(), ww)


def test_ohem_tied_losses_across_the_cut(rn):
    """box_annotator_ohem.py: `argsort(loss)[::-1][roi_per_img:]` are switched off; with exactly tied losses (identical rois: the appended gt
    boxes and clipped duplicates) the project's stable rule keeps the LARGER index.  Every loss occurs three times and 128 = 42 x 3 + 2, so
    the cut goes through a triple."""
    ops, _, _ = rn
    from oracle import targets as OT
    rng = np.random.default_rng(96)
    B, R0, C, D = 2, 100, 81, 8
    cs = rng.normal(0, 2, (B, R0, C)).astype(F32); bp = rng.normal(0, 0.5, (B, R0, D)).astype(F32)
    lab = rng.integers(0, C, (B, R0)).astype(F32); lab[:, ::2] = 0
    bt = rng.normal(0, 1, (B, R0, D)).astype(F32); bw = np.zeros((B, R0, D), F32)
    bw[..., 4:] = (lab > 0)[..., None]
    tile = lambda x: np.concatenate([x, x, x], axis=1)
    cs, bp, lab, bt, bw = (tile(x) for x in (cs, bp, lab, bt, bw))
    lo, wo, loss = ops.box_annotator_ohem(_dev(cs), _dev(bp), _dev(lab), _dev(bt), _dev(bw), 128, want_loss=True)
    for b in range(B):
        olo, owo, oloss = OT.box_annotator_ohem(cs[b], bp[b], lab[b], bt[b], bw[b], 128)
        order = np.argsort(oloss, kind='stable')[::-1]
        assert oloss[order[127]] == oloss[order[128]]                       # the cut separates rows with the same loss
        np.testing.assert_allclose(loss[b].cpu().numpy(), oloss, rtol=2e-6)
        got = lo[b].cpu().numpy()
        assert np.array_equal(got, olo), (b, np.flatnonzero(got != olo)[:8])
        assert np.array_equal(wo[b].cpu().numpy(), owo)
        assert (olo != -1).sum() == 128


def test_nms_multi_target_threshold_equalities_and_tied_scores(rn):
    """nms_multi_target.py:24-74: `overlap > thresh` is strict (a box AT the threshold is no candidate), `argmax` over the candidates of a gt takes
    the FIRST of equal scores, and a box with the same overlap to two gts belongs to the first."""
    ops, _, _ = rn
    from oracle import targets as OT
    F_, C = 24, 4
    bbox = np.zeros((F_, C, 4), F32)
    for c in range(C):
        for f in range(F_):
            bbox[f, c] = [2000 + 40 * f, 50 * c, 2009 + 40 * f, 50 * c + 9]     # disjoint filler, far from every gt
    score = np.tile(np.linspace(0.95, 0.05, F_).astype(F32)[:, None], (1, C))
    gt = np.array([[100, 100, 109, 109, 1], [300, 100, 309, 109, 2], [500, 100, 519, 119, 3], [492, 100, 511, 119, 3], [700, 100, 709, 109, 4]], F32)
    # class 1: the only candidates overlap the gt by exactly 0.5, 0.6, 0.7, 0.8, 0.9 (rows 3..7, scores descending)
    for q, k in enumerate((5, 6, 7, 8, 9)):
        bbox[3 + q, 0] = [100, 100, 109, 100 + k - 1]
    # class 2: exact copies of the gt with TIED scores (rows 2, 3, 4) and a better-scored box AT 0.9 (row 0)
    bbox[0, 1] = [300, 100, 309, 108]
    for f in (2, 3, 4):
        bbox[f, 1] = [300, 100, 309, 109]
    score[2:5, 1] = score[2, 1]
    # class 3: one box midway between two gts of the class (equal overlap with both), one box on the second gt only
    bbox[1, 2] = [496, 100, 515, 119]; bbox[5, 2] = [492, 100, 511, 119]
    # class 4: tied scores between two different boxes above every threshold but 0.9
    bbox[6, 3] = [700, 100, 709, 109]; bbox[7, 3] = [700, 100, 709, 109]; score[6:8, 3] = score[6, 3]
    want = OT.nms_multi_target(bbox, gt[None], score)
    assert [int(np.flatnonzero(want[:, 0, t])[0]) if want[:, 0, t].any() else -1 for t in range(5)] == [4, 5, 6, 7, -1]
    assert np.flatnonzero(want[:, 1, 4]).tolist() == [2] and np.flatnonzero(want[:, 1, 0]).tolist() == [0]
    assert np.flatnonzero(want[:, 3, 0]).tolist() == [6]
    B = 2
    bb = np.stack([bbox, bbox]); sc = np.stack([score, score]); gg = np.stack([gt, gt[[0, 1, 3, 2, 4]]])
    got = ops.nms_multi_target(_dev(bb), _dev(gg), _dev(sc))
    for b in range(B):
        w = OT.nms_multi_target(bb[b], gg[b][None], sc[b])
        assert np.array_equal(got[b].cpu().numpy(), w), (b, np.argwhere(got[b].cpu().numpy() != w)[:8])
