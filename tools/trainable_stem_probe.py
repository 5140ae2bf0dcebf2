"""What training conv1 and res2 costs: one training step (forward_backward + update) of the learn-NMS preset at 600 x 1000 with the shipped
FIXED_PARAMS list (conv1 / res2 fixed, on the inference kernels) and with FIXED_PARAMS = ['gamma', 'beta'] (both trainable), in ONE process,
at 1 and at 8 images.

    python tools/trainable_stem_probe.py [--batches 1,8] [--windows 5] [--per-window 10]

The two trainers are built from the same parameters and alternate window by window (HIP events around `--per-window` steps each, a device
synchronisation between windows); prints one `TRAINABLE_STEM_COST {json}` line: per batch size the per-step times of every window, their
medians and spread, and the difference.  The two new kernels' own times:
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/trainable_stem_probe.py --batches 8 --windows 1 --only trainable`."""
import argparse, json, os, sys
ap = argparse.ArgumentParser()
ap.add_argument('--batches', default='1,8'); ap.add_argument('--windows', type=int, default=5); ap.add_argument('--per-window', type=int, default=10)
ap.add_argument('--only', default='', choices=['', 'shipped', 'trainable'])
a = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
import relnet_amd  # noqa
from relnet_amd import backbone, train
H, W, G = 600, 1000, 8
params = backbone.init_params(seed=1)
variants = [v for v in ('shipped', 'trainable') if a.only in ('', v)]
res = {}
for B in [int(b) for b in a.batches.split(',')]:
    trainers = {}
    for name in variants:
        cfg = train.TrainConfig.from_experiment('rcnn_end2end_relation_learn_nms_8epoch', train=True)
        if name == 'trainable':
            cfg.fixed_params = ['gamma', 'beta']
        trainers[name] = train.Trainer(params, cfg, im_hw=(H, W))
        assert trainers[name].stem_trainable == (name == 'trainable')
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

    def step(tr):
        tr.forward_backward(*batch)
        tr.all_reduce()
        tr.update()
    with torch.no_grad():
        for tr in trainers.values():                    # warm-up: code objects, scratch buffers, the allocator's blocks
            for _ in range(3):
                step(tr)
        torch.cuda.synchronize()
        ms = {name: [] for name in variants}
        for w in range(len(variants) * a.windows):
            name = variants[w % len(variants)]
            tr = trainers[name]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.per_window):
                step(tr)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.per_window)
    med = lambda v: sorted(v)[len(v) // 2]
    r = {'steps_per_window': a.per_window}
    for name in variants:
        r[name + '_ms_windows'] = [round(x, 3) for x in ms[name]]
        r[name + '_ms_median'] = round(med(ms[name]), 3)
        r[name + '_ms_spread'] = round(max(ms[name]) - min(ms[name]), 3)
        r[name + '_gradient_slices'] = len(trainers[name].W.slices)
    if len(variants) == 2:
        r['trainable_cost_ms'] = round(med(ms['trainable']) - med(ms['shipped']), 3)
        r['trainable_cost_percent'] = round(100.0 * (med(ms['trainable']) / med(ms['shipped']) - 1.0), 1)
    res['batch_%d' % B] = r
    del trainers
    torch.cuda.empty_cache()
print('TRAINABLE_STEM_COST ' + json.dumps(res), flush=True)
