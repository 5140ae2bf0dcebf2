"""ROIAlign backward and training step, one box, one process -> profiles/r07_notes/roi_align.txt.
  1. the backward at the C4 8-image training shape (310 rois per image, 256 channels, 38 x 63 map, bf16 output gradient, NHWC fp32
     gradient) and at the FPN 8 x 1000-roi shape on four levels of an 800 x 1024 image: the per-sample scatter (relnet_roi_align_bwd,
     one launch per level) against the separable-patch form (relnet_roi_align_levels_bwd, one launch);
  2. one captured 8-image Trainer step with cfg.roi_align on and off, the two alternating.
    python tools/roi_align_probe.py [--skip-step]"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relnet_amd  # noqa: F401,E402
from relnet_amd import ops  # noqa: E402


def timed(fn, iters=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def random_rois(B, n, H, W, lo, hi, g):
    side = torch.exp(torch.empty(B, n).uniform_(math.log(lo), math.log(hi), generator=g))
    ar = torch.exp(torch.empty(B, n).uniform_(-0.7, 0.7, generator=g))
    bw, bh = (side * ar).clamp(max=W - 2), (side / ar).clamp(max=H - 2)
    x1 = torch.rand(B, n, generator=g) * (W - 1 - bw)
    y1 = torch.rand(B, n, generator=g) * (H - 1 - bh)
    return torch.stack([x1, y1, x1 + bw, y1 + bh], 2)


def bwd_shapes():
    g = torch.Generator().manual_seed(0)
    # C4: 8 images x 310 rois (RPN post-NMS 300 + gt rows), conv_new_1_relu 38 x 63 x 256 of a 600 x 1000 image, scale 1/16
    B, n, C, H, W = 8, 310, 256, 38, 63
    box = random_rois(B, n, 600, 1000, 32, 500, g)
    rois = torch.cat([torch.arange(B, dtype=torch.float32).view(B, 1, 1).expand(B, n, 1), box], 2).reshape(-1, 5).contiguous().cuda()
    dy = torch.randn(B * n, 7, 7, C, generator=g).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)
    old = lambda: ops.roi_align_bwd(dy, rois, (B, C, H, W), 1 / 16.0, 2, channels_last=True)
    new = lambda: ops.roi_align_fpn_bwd(dy, rois, None, [(B, C, H, W)], [1 / 16.0], 2, channels_last=True)
    a, b = old()[0], new()[0][0]
    err = float((a - b).abs().max() / a.abs().max())
    t_old, t_new = timed(old), timed(new)
    print('C4  8 x %d rois, %d ch, %dx%d: scatter %.1f us, patch %.1f us (x%.2f), max rel diff %.1e (incl. the zero fill)'
          % (n, C, H, W, t_old, t_new, t_old / t_new, err), flush=True)
    # FPN: 8 images x 1000 proposals, log-uniform sides 16..640 on an 800 x 1024 image, levels 1/4 .. 1/32
    B, n, IH, IW = 8, 1000, 800, 1024
    scales = (1 / 4.0, 1 / 8.0, 1 / 16.0, 1 / 32.0)
    rois, level, _, _ = ops.fpn_roi_dispatch(random_rois(B, n, IH, IW, 16, 640, g).cuda().contiguous())
    rois, level = rois.view(-1, 5).contiguous(), level.view(-1).contiguous()
    shapes = [(B, C, IH // s, IW // s) for s in (4, 8, 16, 32)]
    dy = torch.randn(B * n, 7, 7, C, generator=g).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)
    sel = [torch.nonzero(level == l).view(-1) for l in range(4)]
    parts = [(dy[s], rois[s].contiguous()) for s in sel]
    counts = [int(s.numel()) for s in sel]

    def old_fpn():
        return [ops.roi_align_bwd(d, r, sh, sc, 2, channels_last=True) for (d, r), sh, sc in zip(parts, shapes, scales)]

    def new_fpn():
        return ops.roi_align_fpn_bwd(dy, rois, level, shapes, scales, 2, channels_last=True)
    err = max(float((a - b).abs().max() / max(float(a.abs().max()), 1e-30)) for a, b in zip(old_fpn(), new_fpn()))
    t_old, t_new = timed(old_fpn, 20), timed(new_fpn, 20)
    print('FPN 8 x %d rois (per level %s), %d ch: scatter %.1f us (4 launches), patch %.1f us (x%.2f), max rel diff %.1e (incl. the zero fill)'
          % (n, counts, C, t_old, t_new, t_old / t_new, err), flush=True)
    zero = lambda: [torch.zeros((s[0], s[2], s[3], s[1]), device='cuda') for s in shapes]
    print('    (the zero fill of the four fp32 gradients alone: %.1f us)' % timed(zero, 20), flush=True)


def train_step(rounds=4, steps=10):
    from relnet_amd import backbone, train
    H, W, G, B = 600, 1000, 8, 8
    params = backbone.init_params(seed=1)
    g = torch.Generator().manual_seed(1000)
    data = torch.randn(B, 3, H, W, generator=g).cuda()
    im_info = torch.tensor([[float(H), float(W), 1.0]] * B).cuda()
    rng = np.random.default_rng(2)
    gt = np.zeros((B, G, 5), np.float32)
    for b in range(B):
        bw, bh = rng.uniform(32, 400, G), rng.uniform(32, 400, G)
        x1, y1 = rng.uniform(0, W - 1 - bw), rng.uniform(0, H - 1 - bh)
        gt[b] = np.stack([x1, y1, x1 + bw, y1 + bh, rng.integers(1, 81, G)], 1)
    batch = (data, im_info, torch.as_tensor(gt).cuda())
    steps_of = {}
    with torch.no_grad():
        for align in (False, True):
            cfg = train.TrainConfig()
            cfg.roi_align = align
            cfg.lr = cfg.lr * 0.5
            tr = train.Trainer(params, cfg, im_hw=(H, W))
            for _ in range(2):
                tr.step(*batch)
            steps_of[align] = (tr, train.CapturedStep(tr, batch))
        res = {False: [], True: []}
        for _ in range(rounds):
            for align in (False, True):
                tr, graph = steps_of[align]

                def one():
                    graph.replay()
                    tr.all_reduce(wait=False)
                    tr.update()
                res[align].append(timed(one, steps, 2) / 1e3)
        for align in (False, True):
            print('Trainer step, 8 images, roi_align=%s: %s ms per step' % (align, ' '.join('%.2f' % v for v in res[align])), flush=True)
        ratio = np.median(res[True]) / np.median(res[False])
        print('ROIAlign / ROIPooling step (medians): %.3f' % ratio, flush=True)


if __name__ == '__main__':
    print(torch.cuda.get_device_name(0), flush=True)
    bwd_shapes()
    if '--skip-step' not in sys.argv:
        train_step()
