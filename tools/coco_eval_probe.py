"""COCO bbox evaluation: dataset/cocoeval.py (numpy) against dataset/device_eval.py (HIP) on a seeded synthetic problem, one process.
  numpy: COCOeval.evaluate() and .accumulate(), wall clock;
  device: the match launch per 8-image batch (as pred_eval(device_eval=True) adds them) and for all images at once, and the
  sort + accumulation launch, HIP events; then the host copy of the arrays.  Both must give equal precision / recall / stats.
    python tools/coco_eval_probe.py [--images 5000] [--skip-numpy]
The sort / scan split inside relnet_coco_accumulate comes from a kernel trace of the --skip-numpy run."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relnet_amd  # noqa: F401,E402
from relnet_amd import ops  # noqa: E402
from relnet_amd.dataset import cocoeval, device_eval as DE  # noqa: E402


def problem(n_images, n_cats=80, dets_per_image=100, seed=0):
    """1 to 14 ground-truth boxes per image (8 % crowd), 100 detections per image: 60 % jittered copies of a ground-truth box,
    the rest anywhere in any category."""
    rng = np.random.default_rng(seed)
    cat_ids = list(range(1, n_cats + 1))
    gts, dts = [], []
    for img in range(n_images):
        ng = int(rng.integers(1, 15))
        gw = np.exp(rng.uniform(np.log(6), np.log(400), ng)); gh = gw * np.exp(rng.uniform(-0.7, 0.7, ng))
        gx, gy = rng.uniform(0, 640 - gw), rng.uniform(0, 480 - np.minimum(gh, 470))
        gc = rng.integers(1, n_cats + 1, ng)
        crowd = rng.random(ng) < 0.08
        for k in range(ng):
            gts.append(dict(id=len(gts) + 1, image_id=img, category_id=int(gc[k]), bbox=[float(gx[k]), float(gy[k]), float(gw[k]), float(gh[k])],
                            area=float(gw[k] * gh[k] * rng.uniform(0.6, 1.0)), iscrowd=int(crowd[k])))
        near = rng.random(dets_per_image) < 0.6
        src = rng.integers(0, ng, dets_per_image)
        j = rng.normal(0, 0.15, (dets_per_image, 4))
        rw, rh = rng.uniform(8, 300, dets_per_image), rng.uniform(8, 300, dets_per_image)
        rx, ry = rng.uniform(0, 600, dets_per_image), rng.uniform(0, 450, dets_per_image)
        rc = rng.integers(1, n_cats + 1, dets_per_image)
        sc = rng.random(dets_per_image)
        for d in range(dets_per_image):
            if near[d]:
                s = src[d]
                b = [gx[s] + j[d, 0] * gw[s], gy[s] + j[d, 1] * gh[s], gw[s] * np.exp(j[d, 2]), gh[s] * np.exp(j[d, 3])]
                c = int(gc[s])
            else:
                b, c = [rx[d], ry[d], rw[d], rh[d]], int(rc[d])
            dts.append(dict(image_id=img, category_id=c, bbox=[float(v) for v in b], score=float(sc[d])))
    return gts, dts, list(range(n_images)), cat_ids


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--skip-numpy', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    t = time.perf_counter()
    gts, dts, img_ids, cat_ids = problem(a.images)
    print('problem: %d images, %d categories, %d ground-truth boxes, %d detections (built in %.1f s)'
          % (len(img_ids), len(cat_ids), len(gts), len(dts), time.perf_counter() - t))

    host = None
    if not a.skip_numpy:
        host = cocoeval.COCOeval(gts, dts, img_ids, cat_ids)
        t0 = time.perf_counter(); host.evaluate()
        t1 = time.perf_counter(); host.accumulate()
        t2 = time.perf_counter(); host.summarize()
        print('numpy  evaluate %.2f s  accumulate %.2f s  total %.2f s' % (t1 - t0, t2 - t1, t2 - t0))

    t0 = time.perf_counter()
    ev = DE.DeviceCOCOeval.from_lists(gts, [], img_ids, cat_ids, slots=100)
    det, num = DE.pack_detections(dts, img_ids, cat_ids)
    det_d, num_d = torch.as_tensor(det).cuda(), torch.as_tensor(num).cuda()
    torch.cuda.synchronize()
    print('device setup (ground-truth table + detection packing + upload, host) %.2f s' % (time.perf_counter() - t0))
    N, B = len(img_ids), 8
    pos = [torch.arange(lo, min(lo + B, N), dtype=torch.int32, device='cuda') for lo in range(0, N, B)]
    pos_all = torch.arange(N, dtype=torch.int32, device='cuda')
    res = {'match_batched': [], 'match_one_launch': [], 'sort_accumulate': []}
    for _ in range(a.reps):
        e0, e1 = events()
        e0.record()
        for k, p in enumerate(pos):
            ev.add(det_d[k * B:k * B + len(p)], num_d[k * B:k * B + len(p)], p)
        e1.record(); torch.cuda.synchronize()
        res['match_batched'].append(e0.elapsed_time(e1))
        e0, e1 = events()
        e0.record()
        ev.add(det_d, num_d, pos_all)
        e1.record(); torch.cuda.synchronize()
        res['match_one_launch'].append(e0.elapsed_time(e1))
        e0, e1 = events()
        e0.record()
        ops.coco_accumulate(ev.slot_cat, ev.slot_score, ev.slot_rank, ev.slot_code, ev.npig, ev.rec_thr, ev.max_dets, ev.max_det)
        e1.record(); torch.cuda.synchronize()
        res['sort_accumulate'].append(e0.elapsed_time(e1))
    for k, v in res.items():
        print('device %-17s median %8.3f ms  min %8.3f ms  (%d reps)' % (k, float(np.median(v)), min(v), len(v)))
    t0 = time.perf_counter()
    ev.accumulate(); ev.summarize()
    print('device accumulate() incl. host copy %.1f ms' % ((time.perf_counter() - t0) * 1e3))
    print('stats', np.array2string(ev.stats, precision=4))
    if host is not None:
        assert np.array_equal(ev.eval['precision'], host.eval['precision']), 'precision differs'
        assert np.array_equal(ev.eval['recall'], host.eval['recall']), 'recall differs'
        assert np.array_equal(ev.stats, host.stats), 'stats differ'
        print('precision, recall and stats: equal to the numpy evaluator (np.array_equal)')


if __name__ == '__main__':
    main()
