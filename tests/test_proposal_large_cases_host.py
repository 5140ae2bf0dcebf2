"""Host side of the proposal order past 8192 candidates: the cases of tests/proposal_large_cases.py have the edges they name (so a
case that lost its edge fails here, not silently on the GPU), the two new C-ABI entries are declared, exported and bound, and the
PROPOSAL_* values reach detector.Config and tester.generate_proposals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proposal_large_cases as PL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('relnet_topk_sort_large', 'relnet_topk_sort_large_workspace_bytes')


@pytest.mark.parametrize('n,K', sorted(PL.TOPK_CASES))
def test_cases_have_the_edges_they_name(n, K):
    scores, boxes, fams = PL.topk_case(n, K)
    assert scores.shape == (2, n) and boxes.shape == (2, n, 4) and scores.dtype == np.float32
    assert 8192 < K <= n < 65536 and fams[0] != fams[1]
    for b, fam in enumerate(fams):
        c = PL.claims(fam, scores[b], K)
        print('(%d, %d) image %d %s: %s' % (n, K, b, fam, c))
        assert c['tied_in_top'] > 0                                        # every family: ties inside the top K
        if fam == 'run_across_K':
            assert K < n and c['run_across_cut'] and c['finite'] == n
            run = int((scores[b] == scores[b][PL.reference_order(scores[b], K)[-1]]).sum())
            assert run >= 400
        elif fam == 'chunk_edge_run':                                      # EVERY multiple of 8192 inside (0, n) lies inside a tied run of the top K
            assert c['chunk_edges'] >= 1 and c['chunk_edges_inside_a_tied_run'] == c['chunk_edges']
        elif fam == 'all_equal':
            assert len(np.unique(scores[b])) == 1 and c['finite'] == n and K == n        # pure index order over every range
            assert c['chunk_edges_inside_a_tied_run'] == c['chunk_edges'] >= 1
        elif fam == 'all_neg_inf':
            assert c['finite'] == 0 and c['finite_in_top'] == 0
        elif fam == 'fewer_finite_than_K':
            assert 0 < c['finite'] < K and c['finite_in_top'] == c['finite'] and c['run_across_cut']       # the cut falls among the -inf rows
        elif fam == 'exactly_K_finite':
            assert c['finite'] == K and c['finite_in_top'] == K and K < n
        else:
            raise AssertionError(fam)
    used = {f for fs in PL.TOPK_CASES.values() for f in fs}
    assert used == {'run_across_K', 'chunk_edge_run', 'all_equal', 'all_neg_inf', 'fewer_finite_than_K', 'exactly_K_finite'}


def test_small_k_shapes_are_the_old_entrys():
    for n, K in PL.SMALL_K_SHAPES:
        scores, boxes = PL.small_k_case(n, K)
        assert min(K, n) <= 8192 and scores.shape == (2, n) and boxes.shape == (2, n, 4)
        for b in range(2):
            want = PL.reference_order(scores[b], K)
            assert len(want) - len(np.unique(scores[b][want])) > 0


def test_new_entries_declared_exported_and_bound():
    import relnet_amd  # noqa: F401
    from relnet_amd import lib
    hdr = open(os.path.join(ROOT, 'include', 'relnet_hip.h')).read()
    for sym in NEW_SYMBOLS:
        decl = re.search(r'\b(int|long)\s+%s\s*\(' % sym, hdr)
        assert decl, '%s is not declared in include/relnet_hip.h' % sym
        assert sym in lib._SIGNATURES and sym in lib.exported_symbols()
        assert 'proposal.py:140-144' in hdr[max(0, decl.start() - 1400):decl.end() + 200]          # each entry cites the reference lines
    assert os.path.exists(lib.LIB_PATH), 'build the library first'
    so = ctypes.CDLL(lib.LIB_PATH)                                         # the built library itself, not the binding's table
    for sym in NEW_SYMBOLS:
        assert hasattr(so, sym), '%s is not exported by %s' % (sym, lib.LIB_PATH)
    # the workspace size is a host function: [B, ceil(n / 8192), 8192] 8-byte keys, -1 for a shape the entry refuses
    wb = lib.load().relnet_topk_sort_large_workspace_bytes
    assert wb(1, 1) == 8192 * 8 and wb(2, 8192) == 2 * 8192 * 8 and wb(2, 8193) == 2 * 2 * 8192 * 8 and wb(3, 65535) == 3 * 8 * 8192 * 8
    assert wb(1, 65536) == -1 and wb(0, 100) == -1 and wb(1, 0) == -1


def test_config_carries_the_proposal_values():
    import relnet_amd  # noqa: F401
    from relnet_amd import detector
    c = detector.Config.from_experiment('rcnn_fpn_relation_learn_nms_8epoch')
    assert c.proposal_pre_nms_top_n == 20000 and c.proposal_post_nms_top_n == 2000
    assert c.proposal_nms_thresh == 0.7 and c.proposal_min_size == 0
    assert (c.rpn_pre_nms_top_n, c.rpn_post_nms_top_n) == (6000, 300)      # the detector's own values are not the proposal ones
    p = detector.Config()
    assert p.proposal_pre_nms_top_n is None and p.proposal_post_nms_top_n is None
    assert p.proposal_nms_thresh is None and p.proposal_min_size is None


class _NoDevice(object):
    """A detector whose every attribute but cfg raises: the ValueError must come before anything touches the device."""
    def __init__(self, cfg):
        self.cfg = cfg

    def __getattr__(self, name):
        raise AssertionError('generate_proposals touched detector.%s before refusing the settings' % name)


class _NoLoader(object):
    def __iter__(self):
        raise AssertionError('generate_proposals read a batch before refusing the settings')


@pytest.mark.parametrize('device_recall', [False, True])
def test_proposal_settings_refused_when_unset(device_recall):
    import relnet_amd  # noqa: F401
    from relnet_amd import detector
    from relnet_amd.dataset import tester as TS
    cfg = detector.Config()
    with pytest.raises(ValueError, match='proposal_pre_nms_top_n'):
        TS.generate_proposals(_NoDevice(cfg), _NoLoader(), None, proposal_settings=True, device_recall=device_recall)
    cfg.proposal_pre_nms_top_n, cfg.proposal_post_nms_top_n, cfg.proposal_nms_thresh = 20000, 2000, 0.7
    with pytest.raises(ValueError, match='proposal_min_size'):
        TS.generate_proposals(_NoDevice(cfg), _NoLoader(), None, proposal_settings=True, device_recall=device_recall)
    with pytest.raises(ValueError, match='proposal_min_size'):
        TS.test_rpn(_NoDevice(cfg), _NoLoader(), None, proposal_settings=True, device_eval=device_recall)


def test_whole_operator_case_is_past_the_old_capacity():
    """The end-to-end case of test_gpu_proposal_large: more than 8192 anchors, and the figures the settings were chosen for."""
    cls_prob, deltas, im_info = PL.tied_rpn_case(PL.RPN_SEEDS[0])
    n = cls_prob.shape[1] // 2 * cls_prob.shape[2] * cls_prob.shape[3]
    assert n == 28728 > 8192 and deltas.shape[1] == 2 * cls_prob.shape[1]
    cropped = int(im_info[0, 0] / 16) * int(im_info[0, 1] / 16) * 12       # the grid proposal.py:85 keeps of the 38 x 63 map
    assert cropped == 27528 > 20000
    kept = {}
    for setting in PL.RPN_SETTINGS:
        pre, post, thresh, min_size = setting
        rois, scores, dbg = PL.rpn_oracle(PL.RPN_SEEDS[0], setting)
        assert rois.shape == (post, 5) and scores.shape == (post, 1)
        kept[setting] = (len(dbg['det']), dbg['n_kept'])
        print(setting, 'sorted rows %d, kept %d' % kept[setting])
    assert kept[(20000, 2000, 0.7, 0)][0] == 20000 and kept[(20000, 2000, 0.7, 0)][1] >= 2000           # the early stop at 2000 keeps
    assert kept[(12000, 2000, 0.7, 16)][0] == 12000 and kept[(12000, 2000, 0.7, 16)][1] >= 2000
    assert kept[(20000, 2000, 0.3, 16)][0] == 20000 and kept[(20000, 2000, 0.3, 16)][1] < 2000          # the padding path
    assert 8192 < kept[(20000, 2000, 0.7, 64)][0] < 20000                                               # a count below K, still past the old capacity
