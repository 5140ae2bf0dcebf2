"""Case builders for the proposal order past 8192 candidates (relnet_topk_sort_large: TEST.PROPOSAL_PRE_NMS_TOP_N 20000 ->
PROPOSAL_POST_NMS_TOP_N 2000).  No test here: tests/test_proposal_large_cases_host.py asserts that every case has the edge it
names, tests/test_gpu_proposal_large.py runs them on the device.

The kernel sorts index ranges of CHUNK = 8192 anchors and ranks every key across the ranges, so the edges are: ties inside the top
K, a run of equal scores across position K, a run of equal scores whose INDICES lie on both sides of a multiple of 8192, -inf rows
inside the top K, and sizes one past a range (8193, 16385) up to the 16-bit index limit (65535)."""
import functools

import numpy as np

import cases
from oracle import nms as ON
from oracle import proposal as OP

F32 = np.float32
CHUNK = 8192

# (n, K) -> the score family of image 0 and of image 1
TOPK_CASES = {
    (8193, 8193): ('chunk_edge_run', 'all_equal'),
    (16384, 8193): ('run_across_K', 'fewer_finite_than_K'),
    (16385, 16385): ('chunk_edge_run', 'all_neg_inf'),
    (28728, 20000): ('run_across_K', 'exactly_K_finite'),
    (40000, 12000): ('run_across_K', 'chunk_edge_run'),
    (65535, 20000): ('run_across_K', 'fewer_finite_than_K'),
    (65535, 65535): ('chunk_edge_run', 'all_equal'),
}
# the new entry against relnet_topk_sort where both run
SMALL_K_SHAPES = [(28728, 6000), (32768, 8192), (5000, 5000), (100, 7)]


def family_scores(family, n, K, seed):
    """[n] float32 scores of one image."""
    if family == 'run_across_K':                       # bf16-quantised scores, a run of 400 equal ones across position K
        return cases.quantised_scores(n, seed, 8, straddle=(K, 400))
    if family == 'chunk_edge_run':                     # 200 equal scores on indices m - 100 .. m + 99 for every multiple m of CHUNK, high enough to be in the top K
        s = cases.quantised_scores(n, seed, 8)
        v = np.sort(s)[::-1][min(K, n) // 4]
        for m in range(CHUNK, n, CHUNK):
            s[m - 100:min(m + 100, n)] = v
        return s
    if family == 'all_equal':
        return np.full(n, 0.5, F32)
    if family == 'all_neg_inf':
        return np.full(n, -np.inf, F32)
    s = cases.quantised_scores(n, seed, 8)
    rng = np.random.default_rng(seed + 1000)
    if family == 'fewer_finite_than_K':                # K // 2 finite: the -inf rows (min_size) tie among themselves INSIDE the top K
        s[rng.permutation(n)[:n - K // 2]] = -np.inf
        return s
    if family == 'exactly_K_finite':
        s[rng.permutation(n)[:n - K]] = -np.inf
        return s
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def topk_case(n, K):
    """-> scores [2,n] float32, boxes [2,n,4] float32, families (2 names)"""
    fams = TOPK_CASES[(n, K)]
    scores = np.stack([family_scores(f, n, K, 7 * n + K + b) for b, f in enumerate(fams)])
    boxes = np.stack([cases.random_boxes(n, 50 + b) for b in range(2)])
    return scores, boxes, fams


@functools.lru_cache(maxsize=None)
def small_k_case(n, K):
    scores = np.stack([cases.quantised_scores(n, 11 * n + K, 8, straddle=(min(K, n - 1), min(64, n // 2))), cases.quantised_scores(n, n + K, 5)])
    boxes = np.stack([cases.random_boxes(n, 60 + b) for b in range(2)])
    return scores, boxes


def reference_order(scores, K):
    """The contract of both top-K entries: descending, equal scores by descending original index."""
    return ON.argsort_desc(scores)[:K]


def claims(family, scores, K):
    """What the reference order alone shows about one image: dict of booleans / counts the host test holds against `family`."""
    n = len(scores)
    order = ON.argsort_desc(scores)
    want = order[:K]
    top = np.zeros(n, bool)
    top[want] = True
    edges = [m for m in range(CHUNK, n, CHUNK) if scores[m - 1] == scores[m] and top[m - 1] and top[m]]
    return dict(tied_in_top=int(len(want) - len(np.unique(scores[want]))),
                run_across_cut=bool(K < n and scores[order[K - 1]] == scores[order[K]]),
                chunk_edges_inside_a_tied_run=len(edges), chunk_edges=len(range(CHUNK, n, CHUNK)),
                finite=int(np.isfinite(scores).sum()), finite_in_top=int(np.isfinite(scores[want]).sum()))


# ---- the whole operator: the tied RPN case of tests/test_gpu_ties.py (38 x 63 x 12 = 28 728 anchors), restated ----------------
RPN_CFG = dict(feat_stride=16, scales=(4, 8, 16, 32), ratios=(0.5, 1, 2))
RPN_SEEDS = (21, 121)
# (pre_nms_top_n, post_nms_top_n, nms thresh, min_size): the experiment files' PROPOSAL_* values, the reference's TRAIN.RPN_* defaults,
# a threshold at which fewer than 2000 boxes survive (the padding path), a min_size at which fewer than 20000 candidates are finite
RPN_SETTINGS = [(20000, 2000, 0.7, 0), (12000, 2000, 0.7, 16), (20000, 2000, 0.3, 16), (20000, 2000, 0.7, 64)]


@functools.lru_cache(maxsize=None)
def tied_rpn_case(seed, height=38, width=63, num_anchors=12):
    """fg scores on the bf16 grid (thousands of ties) and deltas on a grid of 0.5, large enough that many proposals are clipped to the
    image borders and to the SAME box -> cls_prob [1,2A,H,W], deltas [1,4A,H,W], im_info [1,3]."""
    rng = np.random.default_rng(seed)
    fg = cases.quantised_scores(num_anchors * height * width, seed, 8).reshape(1, num_anchors, height, width)
    cls_prob = np.concatenate((F32(1) - fg, fg), axis=1).astype(F32)
    deltas = (np.round(rng.normal(0, 0.7, (1, 4 * num_anchors, height, width)) * 2) / 2).astype(F32)
    im_info = np.array([[cases.IM_H, cases.IM_W, 1.0]], dtype=F32)
    return cls_prob, deltas, im_info


@functools.lru_cache(maxsize=None)
def rpn_oracle(seed, setting):
    """oracle.proposal.proposal on tied_rpn_case(seed) at one of RPN_SETTINGS -> rois [post,5], scores [post,1], debug dict.  Computed once
    per process and shared: callers must not write into it."""
    pre, post, thresh, min_size = setting
    return OP.proposal(*tied_rpn_case(seed), pre_nms_top_n=pre, post_nms_top_n=post, threshold=thresh, min_size=min_size,
                       return_debug=True, rng=np.random.default_rng(0), **RPN_CFG)
