"""The COCO evaluation kernels (csrc/cocoeval.hip) and the proposal-recall kernel (csrc/recall.hip) at their capacity edges, on the
cases of tests/eval_edge_cases.py (checked on the host by tests/test_eval_edge_cases_host.py).  Every comparison is np.array_equal /
torch.equal against the numpy definitions dataset/cocoeval.py and dataset/recall.py: bit identity is the kernels' contract.

Non-default Params go through ops.coco_match / ops.coco_accumulate with pack_params / pack_ground_truth, the recall cases through
ops.recall_match (DeviceRecall has the reference's seven area ranges built in)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import relnet_amd  # noqa: F401,E402
import eval_edge_cases as E  # noqa: E402
from relnet_amd import lib, ops  # noqa: E402
from relnet_amd.dataset import cocoeval, device_eval as DE  # noqa: E402

pytestmark = pytest.mark.gpu

R_THR = np.array([0.0, 0.3, 0.5, 0.7, 1.0])


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


class Dev(object):
    """DeviceCOCOeval._setup / add / accumulate with the case's own Params."""

    def __init__(self, c, slots=None, class_to_cat=None, round_f32=False, box_xywh=True):
        self.c, self.N, self.K = c, len(c['img_ids']), len(c['cat_ids'])
        iou, area, rec, md = DE.pack_params(E.case_params(c))
        gt = DE.pack_ground_truth(c['gts'], c['img_ids'], c['cat_ids'], area)
        self.S, self.AT = int(slots or c['slots']), len(iou) * len(area)
        self.iou, self.area, self.rec, self.md = _dev(iou), _dev(area), _dev(rec), _dev(md)
        self.max_det, self.gt_cap = int(md[-1]), gt['gt_cap']
        self.gt_off, self.gt_box, self.gt_flags, self.npig = _dev(gt['gt_off']), _dev(gt['gt_box']), _dev(gt['gt_flags']), _dev(gt['npig'])
        self.class_to_cat = _dev(np.arange(self.K, dtype=np.int32) if class_to_cat is None else class_to_cat)
        self.round_f32, self.box_xywh = round_f32, box_xywh
        self.slot_cat = torch.full((self.N, self.S), -1, device='cuda', dtype=torch.int32)
        self.slot_score = torch.zeros((self.N, self.S), device='cuda', dtype=torch.float64)
        self.slot_rank = torch.full((self.N, self.S), 2 ** 31 - 1, device='cuda', dtype=torch.int32)
        self.slot_code = torch.zeros((self.N, self.S, self.AT), device='cuda', dtype=torch.uint8)

    def add(self, det, num, pos):
        ops.coco_match(_dev(det), _dev(np.asarray(num, np.int32)), _dev(np.asarray(pos, np.int32)), self.class_to_cat, self.gt_off,
                       self.gt_box, self.gt_flags, self.iou, self.area, self.slot_cat, self.slot_score, self.slot_rank, self.slot_code,
                       self.gt_cap, self.max_det, round_f32=self.round_f32, box_xywh=self.box_xywh)
        return self

    def add_case(self, chunk=None):
        det, num = DE.pack_detections(self.c['dts'], self.c['img_ids'], self.c['cat_ids'])
        chunk = chunk or self.N
        for lo in range(0, self.N, chunk):
            n = num[lo:lo + chunk]
            self.add(det[lo:lo + chunk, :max(int(n.max()), 1)], n, np.arange(lo, lo + len(n)))
        return self

    def slots(self):
        return tuple(t.cpu().numpy() for t in (self.slot_cat, self.slot_score, self.slot_rank, self.slot_code))

    def accumulate(self):
        p, r = ops.coco_accumulate(self.slot_cat, self.slot_score, self.slot_rank, self.slot_code, self.npig, self.rec, self.md, self.max_det)
        return p.cpu().numpy(), r.cpu().numpy()


def _assert_same(got, want, what=''):
    for name, g, w in zip(('precision', 'recall'), got, want):
        assert g.dtype == w.dtype == np.float64 and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, 'differs at', np.argwhere(g != w)[:5].tolist(), int((g != w).sum()))


def _expected(name):
    ev = E.coco_expected(name)
    return ev.eval['precision'], ev.eval['recall']


# ---- matching and accumulation on every case ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(E.COCO_BUILDERS))
def test_coco_case_equals_cocoeval(name):
    c = E.coco_case(name)
    d = Dev(c).add_case(c['chunk'])
    _assert_same(d.accumulate(), _expected(name), name)
    want = E.host_slots(E.coco_expected(name), c['slots'])            # and the slots themselves, the rows cut at maxDets included
    for what, g, w in zip(('slot_cat', 'slot_score', 'slot_rank', 'slot_code'), d.slots(), want):
        assert np.array_equal(g, w, equal_nan=(what == 'slot_score')), (name, what, np.argwhere(g != w)[:5].tolist())
    assert np.array_equal(d.npig.cpu().numpy(), want[4])


@pytest.mark.parametrize('name', ['slots9k', 'K257'])
def test_batching_does_not_change_slots_or_results(name):
    c = E.coco_case(name)
    runs = [Dev(c).add_case(chunk) for chunk in (1, 7, None)]
    for d in runs[1:]:
        for a, b in zip(d.slots(), runs[0].slots()):
            assert np.array_equal(a, b)
    for d in runs:
        _assert_same(d.accumulate(), _expected(name), name)


def test_default_params_case_through_device_cocoeval():
    """The public class on a case with a second unit trip and on the one with 40960 slots: from_lists, accumulate, summarize."""
    for name in ('units1200', 'slots40k'):
        c, host = E.coco_case(name), E.coco_expected(name)
        ev = DE.DeviceCOCOeval.from_lists(c['gts'], c['dts'], c['img_ids'], c['cat_ids'], slots=c['slots'], chunk=97)
        ev.accumulate()
        _assert_same((ev.eval['precision'], ev.eval['recall']), _expected(name), name)
        assert np.array_equal(ev.summarize(), host.summarize())


# ---- sanitation of the rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('counts', ['exact', 'clamped'])
def test_rows_that_are_not_detections_are_dropped(counts):
    c = E.coco_case('maxdets1237')
    det, num, table = E.dirty_rows(c, 31)
    if counts == 'clamped':                          # num_det < 0: no row; num_det > S_in: every row, the filler behind included
        num = num.copy()
        num[0], num[1], num[2] = -3, det.shape[1] + 5, 2 ** 31 - 1
    keep = E.surviving_rows(det, num, table, c['img_ids'], c['cat_ids'])
    assert 0 < len(keep) < int(np.clip(num, 0, det.shape[1]).sum())
    host = E.host_eval(c, dts=keep)
    d = Dev(c, slots=det.shape[1], class_to_cat=table).add(det, num, np.arange(len(num)))
    _assert_same(d.accumulate(), (host.eval['precision'], host.eval['recall']), counts)
    # with the exact counts what survives is the clean case; the clamped counts lose image 0 and gain the rows behind num_det
    assert np.array_equal(host.eval['precision'], _expected('maxdets1237')[0]) == (counts == 'exact')
    # the float32 form of the same rows
    d32 = Dev(c, slots=det.shape[1], class_to_cat=table).add(det.astype(np.float32), num, np.arange(len(num)))
    keep32 = E.surviving_rows(det.astype(np.float32).astype(np.float64), num, table, c['img_ids'], c['cat_ids'])
    host32 = E.host_eval(c, dts=keep32)
    _assert_same(d32.accumulate(), (host32.eval['precision'], host32.eval['recall']), counts + ' float32')


def test_device_image_positions_out_of_range_are_skipped():
    c = E.coco_case('A4T16')
    det, num = DE.pack_detections(c['dts'], c['img_ids'], c['cat_ids'])
    N = len(num)
    d = Dev(c)
    d.add(det[[0, 1, 2, 3]], num[[0, 1, 2, 3]], [-1, N, 2, 2 ** 31 - 1])          # only batch row 2 is image 2's
    keep = [x for x in c['dts'] if x['image_id'] == c['img_ids'][2]]
    host = E.host_eval(c, dts=keep)
    _assert_same(d.accumulate(), (host.eval['precision'], host.eval['recall']))
    cat = d.slots()[0]
    assert (cat[[0, 1, 3, 4]] == -1).all() and (cat[2] >= 0).any()


def test_adding_an_image_again_with_fewer_rows_resets_its_slots():
    c = E.coco_case('maxdets100')
    det, num = DE.pack_detections(c['dts'], c['img_ids'], c['cat_ids'])
    d = Dev(c).add_case()
    assert num[2] == 400
    d.add(det[2:3, :3], [3], [2])                                                  # image 2: 400 rows, then its first 3
    seen, keep = 0, []
    for x in c['dts']:
        if x['image_id'] == c['img_ids'][2]:
            seen += 1
            if seen > 3:
                continue
        keep.append(x)
    host = E.host_eval(c, dts=keep)
    _assert_same(d.accumulate(), (host.eval['precision'], host.eval['recall']))
    cat, score, rank, _ = d.slots()
    assert (cat[2] >= 0).sum() == 3 and (cat[2, 3:] == -1).all() and (score[2, 3:] == 0).all() and (rank[2, 3:] == E.EMPTY_RANK).all()


# ---- accumulation from hand-built slots ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(E.HAND_CASES))
def test_hand_built_slots_accumulate_like_the_restatement(name):
    h = E.hand_case(name)
    cat, score, rank, code, npig = h['slots']
    p, r = ops.coco_accumulate(_dev(cat[None]), _dev(score[None]), _dev(rank[None]), _dev(code[None]), _dev(npig), _dev(h['rec']),
                               _dev(np.asarray(h['max_dets'], np.int32)), int(h['max_dets'][-1]))
    _assert_same((p.cpu().numpy(), r.cpu().numpy()), E.hand_expected(name), name)


# ---- refusals: before anything is launched, with the limit named and the outputs untouched ---------------------------
def _raw_accumulate(n, K, A, T, R, M, short=0):
    """relnet_coco_accumulate on n empty slots -> (return code, message, precision and recall as left behind)."""
    L = lib.load()
    AT = A * T
    cat = torch.full((n,), -1, device='cuda', dtype=torch.int32)
    score = torch.zeros((n,), device='cuda', dtype=torch.float64)
    rank = torch.full((n,), 2 ** 31 - 1, device='cuda', dtype=torch.int32)
    code = torch.zeros((n, AT), device='cuda', dtype=torch.uint8)
    npig = torch.ones((K, A), device='cuda', dtype=torch.int64)
    rec = torch.linspace(0, 1, R, device='cuda', dtype=torch.float64)
    md = torch.arange(1, M + 1, device='cuda', dtype=torch.int32)
    precision = torch.full((T, R, K, A, M), 7.0, device='cuda', dtype=torch.float64)
    recall = torch.full((T, K, A, M), 7.0, device='cuda', dtype=torch.float64)
    need = L.relnet_coco_accumulate_workspace_bytes(n, K, min(AT, E.MAX_PAIRS))
    ws = torch.zeros((need,), device='cuda', dtype=torch.uint8)
    rc = L.relnet_coco_accumulate(cat.data_ptr(), score.data_ptr(), rank.data_ptr(), code.data_ptr(), n, npig.data_ptr(), rec.data_ptr(),
                                  md.data_ptr(), precision.data_ptr(), recall.data_ptr(), ws.data_ptr(), need - short, K, A, T, R, M, M, None)
    msg = L.relnet_last_error().decode() if rc else ''
    torch.cuda.synchronize()
    return rc, msg, precision.cpu().numpy(), recall.cpu().numpy()


def test_accumulate_refuses_what_it_cannot_hold():
    for kw, text in ((dict(A=5, T=13, M=3), '65 (area, IoU) pairs (at most %d)' % E.MAX_PAIRS),
                     (dict(A=4, T=10, M=5), '5 maxDets (at most %d)' % E.MAX_DETS_LEN), (dict(A=4, T=10, M=3, short=1), 'needed')):
        rc, msg, p, r = _raw_accumulate(300, 3, R=11, **kw)
        assert rc != 0 and text in msg, (kw, rc, msg)
        assert (p == 7.0).all() and (r == 7.0).all(), kw
    rc, msg, p, r = _raw_accumulate(300, 3, 4, 16, 11, 4)                          # 64 pairs, 4 maxDets, the exact workspace: accepted
    assert rc == 0 and (p == 0.0).all() and (r == 0.0).all()                       # (ground truth and no detections)


def test_match_refuses_what_it_cannot_hold():
    c = E.coco_case('maxdets1')
    d = Dev(c)
    before = d.slots()

    def refused(text, **kw):
        args = dict(det=torch.zeros((1, 4, 6), device='cuda', dtype=torch.float64), slot=d, iou=d.iou, area=d.area, code=d.slot_code)
        args.update(kw)
        s = args['slot']
        with pytest.raises(lib.RelnetError, match=re.escape(text)):
            ops.coco_match(args['det'], _dev(np.array([4], np.int32)), _dev(np.array([0], np.int32)), d.class_to_cat, d.gt_off, d.gt_box,
                           d.gt_flags, args['iou'], args['area'], s.slot_cat, s.slot_score, s.slot_rank, args['code'], d.gt_cap, d.max_det,
                           box_xywh=True)
        torch.cuda.synchronize()

    big = Dev(c, slots=E.MAX_SLOTS + 1)
    refused('%d detection slots per image, at most %d' % (E.MAX_SLOTS + 1, E.MAX_SLOTS), det=torch.ones((1, E.MAX_SLOTS + 1, 6), device='cuda', dtype=torch.float64), slot=big,
            code=big.slot_code)
    assert (big.slot_cat == -1).all() and (big.slot_code == 0).all()
    area5, iou13 = _dev(np.asarray(E.AREA7[:5])), _dev(np.linspace(0.3, 0.9, 13))
    refused('65 (area, IoU) pairs (at most %d)' % E.MAX_PAIRS, area=area5, iou=iou13, code=torch.zeros((d.N, d.S, 65), device='cuda', dtype=torch.uint8))
    area8, iou8 = _dev(np.asarray(E.RANGES8)), _dev(np.asarray(E.IOU8))
    refused('8 area ranges (at most %d)' % E.MAX_AREAS, area=area8, iou=iou8, code=torch.zeros((d.N, d.S, 64), device='cuda', dtype=torch.uint8))
    for a, b in zip(d.slots(), before):
        assert np.array_equal(a, b)
    # and the host side names the same limits
    p = cocoeval.Params()
    for field, value, text in (('areaRng', E.RANGES8, '7 area ranges'), ('iouThrs', np.linspace(0.3, 0.9, 17), '%d' % E.MAX_PAIRS),
                               ('maxDets', [1, 2, 3, 4, 5], '4 maxDets'), ('maxDets', [10, 1], 'ascending'), ('maxDets', [], '4 maxDets')):
        q = cocoeval.Params()
        setattr(q, field, value)
        with pytest.raises(ValueError, match=text):
            DE.pack_params(q)
    assert len(DE.pack_params(p)) == 4
    with pytest.raises(ValueError, match='%d' % E.MAX_SLOTS):
        DE.DeviceCOCOeval.from_lists(c['gts'], c['dts'], slots=E.MAX_SLOTS + 1)
    row = dict(c['dts'][0])
    with pytest.raises(ValueError, match='%d' % E.MAX_SLOTS):
        DE.pack_detections([row] * (E.MAX_SLOTS + 1), c['img_ids'], c['cat_ids'])


# ---- proposal recall -------------------------------------------------------------------------------------------------
class RecallDev(object):
    def __init__(self, gts, ranges, thr, record=True):
        N, A = len(gts), len(ranges)
        masks = [E.range_masks(g, ranges) for g in gts]
        bits = [np.bitwise_or.reduce([m[a].astype(np.uint8) << a for a in range(A)]) if len(g) else np.zeros(0, np.uint8)
                for g, m in zip(gts, masks)]
        self.gt_cap = max(len(g) for g in gts)
        self.gt_off = _dev(np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32))
        self.gt_box = _dev(np.concatenate([g.astype(np.float64).reshape(-1, 4) for g in gts]))
        self.gt_mask = _dev(np.concatenate(bits).astype(np.uint8))
        self.thr, self.area = _dev(np.asarray(thr, np.float64)), _dev(np.asarray(ranges, np.float64))
        z = lambda shape, dt: torch.zeros(shape, device='cuda', dtype=dt)
        self.hits, self.num_pos, self.area_count = z((A, len(thr)), torch.int64), z((A,), torch.int64), z((A - 1,), torch.int64)
        self.n_cand, self.added = z((N,), torch.int32), z((N,), torch.int32)
        self.overlaps = z((N, A, self.gt_cap), torch.float64) if record else None

    def add(self, boxes, pos, num_valid=None, scores=None, thresh=0.0):
        ops.recall_match(boxes, _dev(np.asarray(pos, np.int32)), self.gt_off, self.gt_box, self.gt_mask, self.thr, self.area, self.hits,
                         self.num_pos, self.area_count, self.n_cand, self.added, self.gt_cap,
                         num_valid=None if num_valid is None else _dev(np.asarray(num_valid, np.int32)),
                         scores=None if scores is None else scores, thresh=float(np.float32(thresh)), overlaps=self.overlaps)
        return self

    def result(self):
        out = {k: getattr(self, k).cpu().numpy() for k in ('hits', 'num_pos', 'area_count', 'n_cand', 'added')}
        out['overlaps'] = None if self.overlaps is None else self.overlaps.cpu().numpy()
        return out


def _pad(cands):
    P = max(max(len(b) for b in cands), 1)
    boxes = np.zeros((len(cands), P, 4), np.float32)
    for i, b in enumerate(cands):
        boxes[i, :len(b)] = b[:, :4]
    return boxes, np.array([len(b) for b in cands], np.int32)


def _assert_recall(got, want, what=''):
    for k in ('hits', 'num_pos', 'area_count', 'n_cand'):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert (got['added'] == 1).all()
    if got['overlaps'] is not None:
        assert np.array_equal(got['overlaps'], want['overlaps']), (what, 'overlaps', np.argwhere(got['overlaps'] != want['overlaps'])[:5].tolist())


@pytest.mark.parametrize('name', sorted(E.RECALL_CASES))
def test_recall_case_equals_evaluate_recall(name):
    c, want = E.recall_case(name), E.recall_expected(name)
    boxes, num = _pad(c['cands'])
    N = len(num)
    got = RecallDev(c['gts'], c['ranges'], c['thr']).add(_dev(boxes), np.arange(N), num).result()
    _assert_recall(got, want, name)
    # one image per call, in reverse order, the rows with stride 5 (rois[:, :, 1:]): the same counts
    rois = torch.zeros((N, boxes.shape[1], 5), device='cuda', dtype=torch.float32)
    rois[:, :, 1:] = _dev(boxes)
    d = RecallDev(c['gts'], c['ranges'], c['thr'], record=False)
    for i in reversed(range(N)):
        d.add(rois[i:i + 1, :, 1:], [i], num[i:i + 1])
    _assert_recall(d.result(), want, name + ' one by one')


def test_recall_score_filter_leaves_0_1_and_fewer_than_G():
    gts, raw, scores, thresh, num_valid = E.recall_filter_case(7)
    thr = [0.0, 0.5, 1.0]
    want = E.recall_reference(gts, E.filtered(raw, scores, thresh, num_valid), thr, E.RANGES2)
    got = RecallDev(gts, E.RANGES2, thr).add(_dev(raw), np.arange(4), num_valid, scores=_dev(scores), thresh=thresh).result()
    _assert_recall(got, want)
    assert got['n_cand'].tolist() == [0, 1, len(gts[2]) - 1, 0] and got['hits'][0, 0] == len(gts[1]) + len(gts[2])


def test_recall_one_candidate_list_for_every_image_of_the_batch():
    """Batch stride 0: every image reads the same rows and filters them with its own scores and its own num_valid."""
    gts, raw, _, _, _ = E.recall_filter_case(8)
    rng = np.random.default_rng(3)
    scores = rng.random((4, raw.shape[1])).astype(np.float32)
    num_valid = np.array([raw.shape[1], raw.shape[1] - 7, 1, 0], np.int32)
    shared = np.stack([raw[1]] * 4)
    want = E.recall_reference(gts, E.filtered(shared, scores, 0.5, num_valid), R_THR, E.RANGES8)
    one = _dev(raw[1:2])
    boxes = one.expand(4, -1, -1)
    assert boxes.stride(0) == 0
    got = RecallDev(gts, E.RANGES8, R_THR).add(boxes, np.arange(4), num_valid, scores=_dev(scores), thresh=0.5).result()
    _assert_recall(got, want)
    assert (want['n_cand'][:2] > 1).all() and want['hits'].sum() > 0

