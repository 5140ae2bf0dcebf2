"""The proposal order and NMS at TEST.PROPOSAL_* (20000 -> 2000) beside the detector's RPN_* (6000 -> 300), one MI355X, one process
-> profiles/r26_notes/proposal_large.txt.
Inputs: the tied RPN case of tests/proposal_large_cases.py at B = 2 and B = 8 images (seeds 21, 121, ...) with a 608 x 1008 image, so
that all 38 x 63 x 12 = 28 728 anchors are candidates, decoded once.  Per call time of ops.topk_sort at K = 20000 (relnet_topk_sort_large) and K = 6000
(relnet_topk_sort), and of ops.nms_greedy at 20000 -> 2000 and 6000 -> 300 (threshold 0.7), plus ops.topk_sort_large at K = 6000:
5 warm-up calls, then 20 windows of 20 calls between device events; median, min and max of the windows.
    python tools/proposal_large_probe.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import relnet_amd  # noqa: F401,E402
from relnet_amd import ops  # noqa: E402
from relnet_amd.operator_py import proposal as P  # noqa: E402
import proposal_large_cases as PL  # noqa: E402


def timeit(f, reps=20, inner=20):
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            f()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner * 1e3)
    ts = np.array(ts)
    return dict(median_us=round(float(np.median(ts)), 1), min_us=round(float(ts.min()), 1), max_us=round(float(ts.max()), 1))


res = {'device': torch.cuda.get_device_name(0)}
anchors = torch.as_tensor(P.generate_anchors(16, PL.RPN_CFG['ratios'], PL.RPN_CFG['scales'])).cuda()
for B in (2, 8):
    cs = [PL.tied_rpn_case(21 + 100 * b) for b in range(B)]
    cls_prob, deltas, im_info = (torch.as_tensor(np.concatenate([c[k] for c in cs])).cuda() for k in range(3))
    im_info[:, 0], im_info[:, 1] = 608, 1008                               # the whole 38 x 63 map: n = 28 728
    boxes, scores = ops.proposal_decode(cls_prob, deltas, im_info, anchors, 16, 0)
    r = {'n': int(scores.shape[1])}
    det = {}
    for K in (20000, 6000):
        det[K], _, cnt = ops.topk_sort(scores, boxes, K)
        r['topk_sort_K%d' % K] = timeit(lambda: ops.topk_sort(scores, boxes, K))
    r['topk_sort_large_K6000'] = timeit(lambda: ops.topk_sort_large(scores, boxes, 6000))
    for K, post in ((20000, 2000), (6000, 300)):
        out = ops.nms_greedy(det[K], 0.7, post)
        r['nms_greedy_%d_to_%d' % (K, post)] = dict(timeit(lambda: ops.nms_greedy(det[K], 0.7, post)), num_keep=out['num_keep'].cpu().tolist())
    res['B%d' % B] = r
    print('B = %d' % B, json.dumps(r))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], 'w') as f:
        json.dump(res, f, indent=1)
