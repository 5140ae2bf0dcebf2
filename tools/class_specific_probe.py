#!/usr/bin/env python
"""Cost of class-specific box regression (cfg.class_agnostic = False) in the inference step: the captured step of the
class-specific Detector (bbox_pred [R, 4 * 81], relnet_detect_head_cs -> boxes [R, 81, 4] float64, relnet_class_nms_topk_cs)
against the class-agnostic one on the same random-init trunk and the same seeded images, 600 x 1000, bf16, at 8 and 108 images
per step.  Each step is one hipGraph replay timed with HIP events: 3 warm-up replays, then the median of 15, the two variants
alternating replay by replay.  python tools/class_specific_probe.py [--batches 8 108]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relnet_amd  # noqa: F401,E402
from relnet_amd import backbone, detector  # noqa: E402


def build(class_agnostic, num_classes=81, std=0.05):
    p = backbone.init_params(seed=1, num_classes=num_classes, num_reg_classes=2 if class_agnostic else num_classes)
    g = torch.Generator().manual_seed(2)
    p['cls_score_weight'] = torch.randn(p['cls_score_weight'].shape, generator=g) * std
    p['bbox_pred_weight'] = torch.randn(p['bbox_pred_weight'].shape, generator=g) * std
    cfg = detector.Config()
    cfg.class_agnostic = class_agnostic
    return detector.Detector(p, dtype=torch.bfloat16, cfg=cfg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[8, 108])
    ap.add_argument('--replays', type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('class_specific_probe needs a GPU: a step time is measured on the device or not at all')
    dets = {'class-agnostic': build(True), 'class-specific': build(False)}
    for B in a.batches:
        g = torch.Generator().manual_seed(10 + B)
        data = torch.randn(B, 3, 600, 1000, generator=g).cuda()
        im_info = torch.tensor([[600, 1000, 1.0]] * B).cuda()
        with torch.no_grad():
            fl = {k: detector.InFlight([lambda d=d: d.forward(data, im_info)]) for k, d in dets.items()}
        times = {k: [] for k in fl}
        for it in range(3 + a.replays):
            for k, f in fl.items():
                s, e = torch.cuda.Event(True), torch.cuda.Event(True)
                with torch.cuda.stream(f.streams[0]):
                    s.record()
                    f.graphs[0].replay()
                    e.record()
                e.synchronize()
                if it >= 3:
                    times[k].append(s.elapsed_time(e))
        med = {k: statistics.median(v) for k, v in times.items()}
        n_det = {k: int(f.outs[0]['num_detections'].sum()) for k, f in fl.items()}
        boxes_mb = fl['class-specific'].outs[0]['pred_boxes'].numel() * 8 / 1e6
        print('%3d images: class-agnostic %.3f ms (min %.3f max %.3f), class-specific %.3f ms (min %.3f max %.3f): %+.3f ms = %+.2f %%; '
              'pred_boxes %.1f MB float64; detections %s'
              % (B, med['class-agnostic'], min(times['class-agnostic']), max(times['class-agnostic']), med['class-specific'],
                 min(times['class-specific']), max(times['class-specific']), med['class-specific'] - med['class-agnostic'],
                 100 * (med['class-specific'] / med['class-agnostic'] - 1), boxes_mb, n_det), flush=True)
        del fl, data
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
