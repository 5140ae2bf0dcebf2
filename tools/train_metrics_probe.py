"""Replay time of the captured training step (learn-NMS preset, 600 x 1000, anchor targets on the device) with and without
metric.TrainMetrics -> profiles/r07_notes/train_metrics.txt.

    python tools/train_metrics_probe.py --metrics 0|1 --batch 8|1 [--tree DIR] [--label NAME]

One variant per process: 2 eager steps, train.CapturedStep, >= 1 s of untimed replays, then --windows windows of --per-window
replays between device synchronisations; prints one `AB {json}` line (the metric values the run ended with included).
--tree: the checkout to import the package from (default: this one); a checkout of an earlier commit with its own built library
gives the "parent" rows (it has no `metrics=` argument: use --metrics 0).  For an A/B, alternate the variants in fresh processes.
The kernels' own times: `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/train_metrics_probe.py --metrics 1
--batch 8 --windows 1 --per-window 10`."""
import argparse, json, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')); ap.add_argument('--metrics', type=int, default=0); ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--windows', type=int, default=5); ap.add_argument('--per-window', type=int, default=20); ap.add_argument('--label', default='')
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
import numpy as np
import torch
import relnet_amd  # noqa
from relnet_amd import backbone, train
assert os.path.abspath(train.__file__).startswith(os.path.abspath(a.tree)), train.__file__
H, W, G, B = 600, 1000, 8, a.batch
params = backbone.init_params(seed=1)
cfg = train.TrainConfig.from_experiment('rcnn_end2end_relation_learn_nms_8epoch', train=True)
kw = {}
tm = None
if a.metrics:
    from relnet_amd import metric as M
    tm = M.TrainMetrics(cfg)
    kw['metrics'] = tm
tr = train.Trainer(params, cfg, im_hw=(H, W), **kw)
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
with torch.no_grad():
    for _ in range(2):
        tr.step(*batch)
    graph = train.CapturedStep(tr, batch)
    t_end = time.perf_counter() + 1.0
    n = 0
    while time.perf_counter() < t_end or n < 3:
        graph.replay(); n += 1
        if n % 8 == 0:
            torch.cuda.synchronize()
    per = []
    for _ in range(a.windows):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.per_window):
            graph.replay()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / a.per_window * 1e3)
res = {'label': a.label, 'batch': B, 'metrics': a.metrics, 'ms_windows': [round(x, 4) for x in per], 'ms_median': round(sorted(per)[len(per) // 2], 4)}
if tm is not None:
    res['values'] = dict(zip(*tm.get()))
print('AB ' + json.dumps(res), flush=True)
