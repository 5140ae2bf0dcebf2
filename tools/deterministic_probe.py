"""What train.TrainConfig.deterministic costs: one training step (forward_backward + update) of the learn-NMS preset at 600 x 1000 with the
default trainer and with a deterministic one, in ONE process, at 1 and at 8 images.

    python tools/deterministic_probe.py [--batches 1,8] [--windows 5] [--per-window 10]

The two trainers are built from the same parameters and alternate window by window (HIP events around `--per-window` steps each, a device
synchronisation between windows); prints one `DETERMINISTIC_COST {json}` line: per batch size the per-step times of every window, their
medians and spread, the difference, and whether two deterministic steps from the same state gave the same gradient bits.  The kernels' own
times: `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/deterministic_probe.py --batches 8 --windows 1 --only deterministic`
(and `--only default` for the kernels they stand in for)."""
import argparse, json, os, sys
ap = argparse.ArgumentParser()
ap.add_argument('--batches', default='1,8'); ap.add_argument('--windows', type=int, default=5); ap.add_argument('--per-window', type=int, default=10)
ap.add_argument('--only', default='', choices=['', 'default', 'deterministic'])
a = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
import relnet_amd  # noqa
from relnet_amd import backbone, train
H, W, G = 600, 1000, 8
params = backbone.init_params(seed=1)
variants = [v for v in ('default', 'deterministic') if a.only in ('', v)]
res = {}
for B in [int(b) for b in a.batches.split(',')]:
    trainers = {}
    for name in variants:
        cfg = train.TrainConfig.from_experiment('rcnn_end2end_relation_learn_nms_8epoch', train=True)
        cfg.deterministic = name == 'deterministic'
        trainers[name] = train.Trainer(params, cfg, im_hw=(H, W))
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
    same_bits = None
    with torch.no_grad():
        for tr in trainers.values():                    # warm-up: code objects, scratch buffers, the allocator's blocks
            for _ in range(3):
                step(tr)
        if 'deterministic' in trainers:                  # two steps from the same state (weights, momentum, anchor sampler) -> the same gradient bits?
            tr = trainers['deterministic']
            state = [t.clone() for t in (tr.W.master, tr.W.mom, tr.W.work, tr.Bv.master, tr.Bv.mom, tr._anchor_step)]
            grads = []
            for _ in range(2):
                for t, s in zip((tr.W.master, tr.W.mom, tr.W.work, tr.Bv.master, tr.Bv.mom, tr._anchor_step), state):
                    t.copy_(s)
                tr.forward_backward(*batch)
                grads.append((tr.W.grad.clone(), tr.Bv.grad.clone()))
            same_bits = bool(torch.equal(grads[0][0].view(torch.int32), grads[1][0].view(torch.int32)) and
                             torch.equal(grads[0][1].view(torch.int32), grads[1][1].view(torch.int32)))
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
    r = {'steps_per_window': a.per_window, 'same_gradient_bits_on_rerun': same_bits}
    for name in variants:
        r[name + '_ms_windows'] = [round(x, 3) for x in ms[name]]
        r[name + '_ms_median'] = round(med(ms[name]), 3)
        r[name + '_ms_spread'] = round(max(ms[name]) - min(ms[name]), 3)
    if len(variants) == 2:
        r['deterministic_cost_ms'] = round(med(ms['deterministic']) - med(ms['default']), 3)
        r['deterministic_cost_percent'] = round(100.0 * (med(ms['deterministic']) / med(ms['default']) - 1.0), 1)
    res['batch_%d' % B] = r
    del trainers
    torch.cuda.empty_cache()
print('DETERMINISTIC_COST ' + json.dumps(res), flush=True)
