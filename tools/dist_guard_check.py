"""Two-rank check of the guarded optimizer step on a ONE-GPU box (both ranks on cuda:0, gloo):
    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29512 tools/dist_guard_check.py
Both ranks run the SAME batch.  Step 1: rank 1 alone writes a NaN into its local gradient before the all-reduce -- the sum carries it to
both ranks, the statistics read the buffers AFTER the exchange, so both must skip and keep their (equal) weights bit for bit.  Step 2 is
clean: both move, and stay equal.  This is the bucketed branch of Trainer.update() with a guard: statistics of a bucket right after its
wait, one decide, then the guarded SGD launches."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.distributed as dist
import __graft_entry__ as ge
ge.build()
import relnet_amd  # noqa: F401
from relnet_amd import backbone, train, dist as D

torch.cuda.set_device(0)
rank, world, _ = D.init(backend='gloo')
B, H, W, G = 1, 256, 320, 4
params = backbone.init_params(seed=1)
cfg = train.TrainConfig(); cfg.learn_nms = True
cfg.rank_in_anchor_seed = False        # identical batches AND identical anchor subsets on both ranks
guard = train.GradGuard(max_norm=1e9)
tr = train.Trainer(params, cfg, im_hw=(H, W), guard=guard)
g = torch.Generator().manual_seed(7)
data = torch.randn(B, 3, H, W, generator=g).cuda()
im_info = torch.tensor([[float(H), float(W), 1.0]] * B).cuda()
rng = np.random.default_rng(3)
gt = np.zeros((B, G, 5), np.float32)
for b in range(B):
    bw, bh = rng.uniform(32, 150, G), rng.uniform(32, 150, G)
    x1, y1 = rng.uniform(0, W - 1 - bw), rng.uniform(0, H - 1 - bh)
    gt[b] = np.stack([x1, y1, x1 + bw, y1 + bh, rng.integers(1, 81, G)], 1)
batch = (data, im_info, torch.as_tensor(gt).cuda())


def fingerprint():
    """(all ranks hold the same bits, a copy of this rank's buffers): every buffer as int32 words, summed in int64 -- exact -- and compared
    through MIN / MAX all-reduces."""
    bufs = [tr.W.master, tr.W.mom, tr.Bv.master, tr.Bv.mom]
    chk = torch.stack([b.view(torch.int32).to(torch.int64).sum() for b in bufs] +
                      [(b.view(torch.int32).to(torch.int64) * (torch.arange(b.numel(), device=b.device) % 8191 + 1)).sum() for b in bufs]).cpu()
    lo, hi = chk.clone(), chk.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    return bool((lo == hi).all()), [b.clone() for b in bufs] + [tr.W.work.clone()]


def flags_on_all_ranks(flag):
    t = torch.tensor([1 if flag else 0])
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(t.item())


res = {}
with torch.no_grad():
    tr.guard = None
    tr.forward_backward(*batch); tr.all_reduce(); torch.cuda.synchronize()          # warm-up without an update
    tr.guard = guard
    equal0, before = fingerprint()
    # ---- step 1: poisoned on rank 1 only
    tr.forward_backward(*batch)
    torch.cuda.synchronize()
    # the backward pass has announced its buckets (their collectives may be in flight): the poison goes into the BIAS buffer, which is
    # exchanged only from all_reduce() / update()
    if rank == 1:
        tr.Bv.grad[tr.Bv.slices['cls_bbox'][0] + 3] = float('nan')
    order = tr.all_reduce(wait=False)
    tr.update(); torch.cuda.synchronize()
    rep1 = guard.report()
    equal1, after1 = fingerprint()
    unchanged = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                                b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16)) for a, b in zip(before, after1))
    res['launch_order'] = order
    res['update_order'] = [i for i, _ in tr.update_order]
    res['step1_skipped_on_all_ranks'] = flags_on_all_ranks(rep1['skipped'] == 1 and rep1['steps'] == 1 and rep1['last_nonfinite'] >= 1)
    res['step1_weights_unchanged_on_all_ranks'] = flags_on_all_ranks(unchanged)
    res['step1_equal_across_ranks'] = equal0 and equal1
    # ---- step 2: clean
    tr.forward_backward(*batch)
    tr.all_reduce(wait=False)
    tr.update(); torch.cuda.synchronize()
    rep2 = guard.report()
    equal2, after2 = fingerprint()
    moved = (not torch.equal(after2[0], after1[0])) and (not torch.equal(after2[2], after1[2])) and bool(torch.isfinite(tr.W.master).all())
    res['step2_applied_on_all_ranks'] = flags_on_all_ranks(rep2['skipped'] == 1 and rep2['steps'] == 2 and rep2['last_nonfinite'] == 0
                                                           and np.isfinite(rep2['last_norm']) and rep2['last_norm'] > 0)
    res['step2_weights_moved_on_all_ranks'] = flags_on_all_ranks(moved)
    res['step2_equal_across_ranks'] = equal2
    norm = torch.tensor([rep2['last_norm']], dtype=torch.float64)
    lo, hi = norm.clone(), norm.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    res['step2_same_norm_on_all_ranks'] = bool((lo == hi).all())
    res['work_copy_is_rounded_master'] = flags_on_all_ranks(torch.equal(tr.W.work, tr.W.master.to(torch.bfloat16)))
    res['step_count'] = tr.step_count
if rank == 0:
    print('DIST_GUARD_CHECK', res)
dist.barrier(); dist.destroy_process_group()
