"""PSROIPooling, one MI355X, one process -> profiles/r23_notes/psroi.txt.
  1. the worst error / bound of every path over the case table of tests/psroi_cases.py (float32 and bf16 forward, backward written and
     accumulated), against the float64 restatement and the bounds derived there;
  2. one timing of forward and backward at an R-FCN-like shape: one 38 x 63 map with 49 x 81 channels, 300 rois, P = g = 7, in
     channels-last bf16 and in NCHW fp32; 20 samples of 20 calls each between device events (median, min, max), with the bytes each
     kernel must move and the fraction of the measured HBM copy rate (6.29 TB/s) that makes.
    python tools/psroi_probe.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import relnet_amd  # noqa: F401,E402
from relnet_amd import ops  # noqa: E402
import psroi_cases as PC  # noqa: E402

res = {}
worst = {'fwd_f32': 0, 'fwd_bf16': 0, 'bwd': 0, 'bwd_acc': 0}
for name in PC.CASE_NAMES:
    c = PC.case(name)
    if c['R'] == 0: continue
    x = torch.as_tensor(c['data']).cuda(); rois = torch.as_tensor(c['rois']).cuda(); go = torch.as_tensor(c['grad_out']).cuda()
    a = (c['scale'], c['output_dim'], c['P'], c['g'])
    def ratio(err, bound):
        m = bound > 0
        assert np.all(err[~m] == 0)
        return float((err[m] / bound[m]).max()) if m.any() else 0.0
    o = ops.psroi_pool(x, rois, *a)
    worst['fwd_f32'] = max(worst['fwd_f32'], ratio(np.abs(o.double().cpu().numpy() - c['ref64']['out']), PC.fwd_bound(c['ref64'])))
    o = ops.psroi_pool(x.bfloat16(), rois, *a)
    worst['fwd_bf16'] = max(worst['fwd_bf16'], ratio(np.abs(o.double().cpu().numpy() - c['ref64']['out']), PC.fwd_bound(c['ref64'], True)))
    shape = (c['B'], c['C'], c['H'], c['W'])
    g = ops.psroi_pool_bwd(go, rois, shape, *a)
    worst['bwd'] = max(worst['bwd'], ratio(np.abs(g.double().cpu().numpy() - c['ref64']['grad_in']), PC.bwd_bound(c['ref64'])))
    g = ops.psroi_pool_bwd(go, rois, shape, *a, accumulate_into=torch.as_tensor(c['grad_in0']).cuda())
    worst['bwd_acc'] = max(worst['bwd_acc'], ratio(np.abs(g.double().cpu().numpy() - c['ref64_acc']['grad_in']), PC.bwd_bound(c['ref64_acc'])))
res['worst_error_over_bound'] = worst
print(json.dumps(worst))

# R-FCN-like shape: one 38 x 63 map, 49 x 81 channels bf16 channels-last, 300 rois, P = g = 7
torch.manual_seed(0)
H, W, OD, P = 38, 63, 81, 7
C = OD * P * P
x = torch.randn(1, C, H, W, device='cuda').bfloat16().contiguous(memory_format=torch.channels_last)
rng = np.random.RandomState(3)
x1 = rng.uniform(0, 800, 300); y1 = rng.uniform(0, 450, 300)
w = rng.uniform(40, 400, 300); h = rng.uniform(40, 300, 300)
rois = torch.as_tensor(np.stack([np.zeros(300), x1, y1, np.minimum(x1 + w, 1007), np.minimum(y1 + h, 607)], 1).astype(np.float32)).cuda()
go = torch.randn(300, P, P, OD, device='cuda').bfloat16().permute(0, 3, 1, 2)
fwd = lambda: ops.psroi_pool(x, rois, 0.0625, OD, P, P, channels_last_out=True)
bwd = lambda: ops.psroi_pool_bwd(go, rois, (1, C, H, W), 0.0625, OD, P, P, channels_last=True)
def timeit(f, reps=20, inner=20):
    for _ in range(5): f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner): f()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner * 1e3)
    ts = np.array(ts)
    return dict(median_us=float(np.median(ts)), min_us=float(ts.min()), max_us=float(ts.max()))
bytes_fwd = x.numel() * 2 + 300 * OD * P * P * 2 + 300 * 20
bytes_bwd = 300 * OD * P * P * 2 + C * H * W * 4 + 300 * 20
for name, f, nb in (('fwd', fwd, bytes_fwd), ('bwd', bwd, bytes_bwd)):
    t = timeit(f)
    t['bytes'] = nb
    t['hbm_fraction_of_6.29TBps'] = nb / (t['median_us'] * 1e-6) / 6.29e12
    res[name] = t
    print(name, json.dumps(t))
# also the NCHW fp32 form
xf = x.float().contiguous(); gof = go.float().contiguous()
res['fwd_nchw_f32'] = timeit(lambda: ops.psroi_pool(xf, rois, 0.0625, OD, P, P))
res['bwd_nchw_f32'] = timeit(lambda: ops.psroi_pool_bwd(gof, rois, (1, C, H, W), 0.0625, OD, P, P))
print(json.dumps(res))
