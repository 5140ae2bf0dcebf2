"""What train.GradGuard costs: Trainer.update() of the learn-NMS preset (600 x 1000) with and without a neutral guard, in ONE process,
on the gradients of one real forward_backward.

    python tools/grad_guard_probe.py [--batch 8] [--windows 7] [--per-window 50]

The two variants alternate window by window (HIP events around `--per-window` updates each, a device synchronisation between windows);
prints one `GUARD_COST {json}` line: the median per-update time of each variant, their difference, the bytes the statistics pass reads and
the guard's own report.  The kernels' own times: `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/grad_guard_probe.py
--windows 1`."""
import argparse, json, os, sys
ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=8); ap.add_argument('--windows', type=int, default=7); ap.add_argument('--per-window', type=int, default=50)
a = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
import relnet_amd  # noqa
from relnet_amd import backbone, train
H, W, G, B = 600, 1000, 8, a.batch
params = backbone.init_params(seed=1)
cfg = train.TrainConfig.from_experiment('rcnn_end2end_relation_learn_nms_8epoch', train=True)
tr = train.Trainer(params, cfg, im_hw=(H, W))
g = torch.Generator().manual_seed(1000)
data = torch.randn(B, 3, H, W, generator=g).cuda()
im_info = torch.tensor([[float(H), float(W), 1.0]] * B).cuda()
rng = np.random.default_rng(2)
gt = np.zeros((B, G, 5), np.float32)
for b in range(B):
    bw, bh = rng.uniform(32, 400, G), rng.uniform(32, 400, G)
    x1, y1 = rng.uniform(0, W - 1 - bw), rng.uniform(0, H - 1 - bh)
    gt[b] = np.stack([x1, y1, x1 + bw, y1 + bh, rng.integers(1, 81, G)], 1)
guard = train.GradGuard()
with torch.no_grad():
    tr.forward_backward(data, im_info, torch.as_tensor(gt).cuda())
    tr.all_reduce()
    state0 = [t.clone() for t in (tr.W.master, tr.W.mom, tr.W.work, tr.Bv.master, tr.Bv.mom)]
    for gd in (None, guard, None, guard):              # warm-up of both variants (code objects, the guard's workspace)
        tr.guard = gd
        for _ in range(5):
            tr.update()
    torch.cuda.synchronize()
    guard.reset()
    ms = {'plain': [], 'guarded': []}
    for w in range(2 * a.windows):
        name, tr.guard = ('plain', None) if w % 2 == 0 else ('guarded', guard)
        for t, s in zip((tr.W.master, tr.W.mom, tr.W.work, tr.Bv.master, tr.Bv.mom), state0):       # every window starts from the same weights
            t.copy_(s)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.per_window):
            tr.update()
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / a.per_window)
    tr.guard = None
med = lambda v: sorted(v)[len(v) // 2]
n_stats = sum(b_ - a_ for buf in (tr.W, tr.Bv) for a_, b_ in tr._trainable_ranges(buf))
res = {'batch': B, 'updates_per_window': a.per_window, 'plain_ms_windows': [round(x, 4) for x in ms['plain']],
       'guarded_ms_windows': [round(x, 4) for x in ms['guarded']], 'plain_ms_median': round(med(ms['plain']), 4),
       'guarded_ms_median': round(med(ms['guarded']), 4), 'guard_cost_ms': round(med(ms['guarded']) - med(ms['plain']), 4),
       'statistics_megabytes': round(4e-6 * n_stats, 1), 'report': guard.report()}
print('GUARD_COST ' + json.dumps(res), flush=True)
