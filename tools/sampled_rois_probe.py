#!/usr/bin/env python
"""Step time of the plain Faster R-CNN training graph (cfg.relation False) with a sampled ROI minibatch (cfg.batch_rois 128, ENABLE_OHEM
false: relnet_proposal_target_sample, a 128-roi head) against today's way to train on 128 rois per image (batch_rois -1 + OHEM 128: all 300
proposals + gt rows through the head, BoxAnnotatorOHEM keeps 128), on the same random-init parameters and the same seeded batch: 8 images,
600 x 1000, anchor targets made on the device.  Forward + backward, eager (wall clock around a synchronised step) and as one captured
hipGraph (HIP events around the replay): 3 warm-up steps, then the median of --steps, the two variants alternating step by step in one process.
python tools/sampled_rois_probe.py [--images 8] [--steps 15]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relnet_amd  # noqa: F401,E402
from relnet_amd import backbone, train  # noqa: E402


def make_batch(B, H, W, G=8, seed=3):
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    data = torch.randn(B, 3, H, W, generator=g).cuda()
    gt = np.zeros((B, G, 5), np.float32)
    x1 = rng.uniform(0, W - 260, (B, G)); y1 = rng.uniform(0, H - 260, (B, G))
    gt[..., 0], gt[..., 1] = x1, y1
    gt[..., 2], gt[..., 3] = x1 + rng.uniform(40, 250, (B, G)), y1 + rng.uniform(40, 250, (B, G))
    gt[..., 4] = rng.integers(1, 81, (B, G))
    return data, torch.tensor([[H, W, 1.0]] * B).cuda(), torch.as_tensor(gt).cuda()


def build(p, H, W, batch_rois):
    cfg = train.TrainConfig()
    cfg.relation = False
    cfg.batch_rois, cfg.enable_ohem = (batch_rois, False) if batch_rois > 0 else (-1, True)
    return train.Trainer(p, cfg, im_hw=(H, W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--steps', type=int, default=15)
    ap.add_argument('--hw', type=int, nargs=2, default=[600, 1000])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sampled_rois_probe needs a GPU: a step time is measured on the device or not at all')
    H, W = a.hw
    p = backbone.init_params(seed=1)
    batch = make_batch(a.images, H, W)
    trainers = {'batch_rois 128': build(p, H, W, 128), 'batch_rois -1 + OHEM 128': build(p, H, W, -1)}
    eager = {k: [] for k in trainers}
    with torch.no_grad():
        for it in range(3 + a.steps):
            for k, tr in trainers.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = tr.forward_backward(*batch)
                torch.cuda.synchronize()
                if it >= 3:
                    eager[k].append(1e3 * (time.perf_counter() - t0))
        rows = {k: int(tr.forward_backward(*batch)['rois'].shape[1]) for k, tr in trainers.items()}
        steps = {k: train.CapturedStep(tr, batch) for k, tr in trainers.items()}
        cap = {k: [] for k in trainers}
        for it in range(3 + a.steps):
            for k, st in steps.items():
                s, e = torch.cuda.Event(True), torch.cuda.Event(True)
                s.record()
                out = st.replay()
                e.record()
                e.synchronize()
                if it >= 3:
                    cap[k].append(s.elapsed_time(e))
        del out
    for k in trainers:
        print('%d images %d x %d, %-26s %4d head rows per image: eager %.2f ms (min %.2f max %.2f), captured %.2f ms (min %.2f max %.2f)'
              % (a.images, H, W, k + ',', rows[k], statistics.median(eager[k]), min(eager[k]), max(eager[k]),
                 statistics.median(cap[k]), min(cap[k]), max(cap[k])), flush=True)
    a_, b_ = (statistics.median(cap[k]) for k in trainers)
    print('captured: sampled minibatch %+.2f ms = %+.1f %% against all rows + OHEM' % (a_ - b_, 100 * (a_ / b_ - 1)))


if __name__ == '__main__':
    main()
