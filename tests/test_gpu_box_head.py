"""The box head as one module (relation.BoxHead): the train branch (relation.BoxHeadTrain on a Trainer's flat buffers) and the test
branch (relation.RelationHead) run one forward, bit for bit; the trainer's head reads VIEWS of the flat buffers; and the persistent
buffers of the step (VW^T, the backward's transposed / packed operands) never leak rows or columns from a larger call into a smaller one
of the same padded widths.  Synthetic pooled features and rois: no image goes through the trunk."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

B, HW = 2, (128, 160)
#: name -> (N keys = non-gt rows, R rows, key_count | None, relation).  'a': three non-key gt rows, pad32(N) = 64 != N; 'b': N an exact
#: multiple of 32 with a per-image key count; 'plain': the 2FC head without relation modules
FORWARD_CASES = {'a': (40, 43, None, True), 'b': (64, 65, [64, 50], True), 'plain': (40, 43, None, False)}
#: name -> ((N, R) of the first call, (N, R) of the second): the same padded widths both times.  ops.relation_bwd_small_ok switches the
#: backward at 128 rows: 'small' is the one-kernel form (packed a3 scratch), 'large' the two-kernel form (kt / qt / dyt scratch, Mpad = Npad = 160)
LEAK_CASES = {'small': ((48, 51), (40, 43)), 'large': ((140, 143), (132, 135))}
GRAD_SLICES = ('fc_new_1', 'fc_new_2', 'cls_bbox', 'qk_1', 'qk_2', 'linear_out_1', 'linear_out_2', 'pair_pos_fc1_1', 'pair_pos_fc1_2')


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib, backbone, relation, train, detector
    lib.load()
    return SimpleNamespace(ops=ops, backbone=backbone, relation=relation, train=train, detector=detector, params=backbone.init_params(seed=5))


def _trainer(rn, relation=True, deterministic=False):
    cfg = rn.train.TrainConfig()
    cfg.relation, cfg.deterministic = relation, deterministic
    return rn.train.Trainer(rn.params, cfg, im_hw=HW)


@pytest.fixture(scope='module')
def trainers(rn):
    return {True: _trainer(rn), False: _trainer(rn, relation=False)}


def _inputs(N, R, seed):
    """pooled2 [B*R, 12544] bf16 (non-negative, as pooled ReLU outputs are), rois_t [B,R,5] inside the 128 x 160 image."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    u = lambda *s: torch.rand(s, device='cuda', generator=g)
    pooled2 = torch.randn((B * R, 12544), device='cuda', generator=g).abs().to(torch.bfloat16)
    x1, y1 = u(B, R) * 100.0, u(B, R) * 70.0
    rois = torch.stack([torch.arange(B, device='cuda', dtype=torch.float32).view(B, 1).expand(B, R), x1, y1,
                        x1 + 8.0 + u(B, R) * 50.0, y1 + 8.0 + u(B, R) * 48.0], 2).contiguous()
    return pooled2, rois


def _same(a, b):
    if a.dtype == torch.bfloat16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    elif a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 1. one forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(FORWARD_CASES))
def test_train_and_test_branch_run_one_forward(rn, trainers, name):
    N, R, kc, relation = FORWARD_CASES[name]
    pooled2, rois = _inputs(N, R, 11)
    kc = None if kc is None else torch.tensor(kc, dtype=torch.int32, device='cuda')
    want = rn.relation.BoxHeadTrain(trainers[relation]).forward(pooled2, rois, N, kc)
    head = rn.relation.RelationHead(rn.params, torch.bfloat16, 'cuda', fc1_perm=rn.detector.fc1_channels_last_perm(), use_relation=relation)
    pooled = pooled2.view(B, R, -1)
    if relation:
        # the float32 geometry of the train branch handed to the test branch: everything else is the same code on the same bits
        assert want.bias.dtype == torch.float32 and want.bias.shape == (2, B, 16, R, rn.ops.pad32(N))
        got = head.forward(pooled, rois, nongt_dim=N, return_intermediates=True, key_count=kc, bias=want.bias)
        got = SimpleNamespace(f1=got['fc_new_1'], x1=got['fc_all_1_relu'], f2=got['fc_new_2'], x2=got['fc_all_2_relu'],
                              cls_score=got['cls_score'], bbox_pred=got['bbox_pred'])
        assert not _same(want.f1, want.x1) and not _same(want.f2, want.x2)
    else:
        cls_score, bbox_pred, x2 = head.forward(pooled, rois, nongt_dim=N)
        got = head.run(pooled2, B)          # (the public tuple does not carry fc_new_1's output)
        assert _same(cls_score, got.cls_score) and _same(bbox_pred, got.bbox_pred) and _same(x2, got.x2)
        assert want.f1 is want.x1 and want.f2 is want.x2
    torch.cuda.synchronize()
    for k in ('f1', 'x1', 'f2', 'x2', 'cls_score', 'bbox_pred'):
        a, b = getattr(got, k), getattr(want, k)
        assert a.shape[:2] == (B, R) and torch.isfinite(b.float()).all() and float(b.float().abs().max()) > 0, k
        assert _same(a.contiguous(), b), k


# ---------------------------------------------------------------------------------------------------------------------
# 2. views, not copies
# ---------------------------------------------------------------------------------------------------------------------
def test_trainer_head_reads_views_of_the_flat_buffers(rn, trainers):
    tr = trainers[True]
    N, R = 40, 43
    pooled2, rois = _inputs(N, R, 12)
    head = rn.relation.BoxHeadTrain(tr)
    first = head.forward(pooled2, rois, N)
    assert float(first.cls_score.abs().max()) > 0
    w, b = tr.w('cls_bbox'), tr.b('cls_bbox')
    saved = w.clone(), b.clone()
    try:
        w.zero_()                                                   # in place, as the optimizer writes: nothing is rebuilt
        b.copy_(torch.arange(b.numel(), device='cuda', dtype=torch.float32) * 0.25 - 3.0)
        s = head.forward(pooled2, rois, N)
        torch.cuda.synchronize()
        assert _same(torch.cat([s.cls_score, s.bbox_pred], 2), b.view(1, 1, -1).expand(B, R, -1).contiguous())
    finally:
        w.copy_(saved[0]); b.copy_(saved[1])
    again = head.forward(pooled2, rois, N)
    assert _same(again.cls_score, first.cls_score) and _same(again.bbox_pred, first.bbox_pred)


# ---------------------------------------------------------------------------------------------------------------------
# 3. persistent buffers never leak rows
# ---------------------------------------------------------------------------------------------------------------------
def _head_step(tr, N, R, seed):
    """One Trainer._head_forward_backward on synthetic targets -> name -> tensor (clones) of everything the leak test compares."""
    pooled2, rois = _inputs(N, R, seed)
    g = torch.Generator(device='cuda').manual_seed(seed + 1)
    label = torch.randint(0, 81, (B, R), device='cuda', generator=g).float()
    label[:, ::3] = 0.0                                             # background rows
    bbox_target = torch.randn((B, R, 8), device='cuda', generator=g) * 0.2
    bbox_weight = torch.zeros((B, R, 8), device='cuda')
    bbox_weight[:, :, 4:] = (label > 0).float().unsqueeze(2)
    im_info = torch.tensor([[float(HW[0]), float(HW[1]), 1.0]] * B, device='cuda')
    gt = torch.cat([rois[:, N:, 1:], torch.ones((B, R - N, 1), device='cuda')], 2).contiguous()
    num_gt = torch.full((B,), R - N, dtype=torch.int32, device='cuda')
    tr.W.grad.zero_(); tr.Bv.grad.zero_()
    tr._relayout.run()
    d_pool, hs = tr._head_forward_backward(pooled2, rois, N, label, bbox_target, bbox_weight, im_info, gt, num_gt, {})
    tr._flush_wgrads()
    torch.cuda.synchronize()
    r = {'cls_score': hs[2].clone(), 'x2': hs[0].clone(), 'd_pool': d_pool.clone()}
    for n in GRAD_SLICES:
        r['W.grad:' + n] = tr.W.view(tr.W.grad, n).clone()
        r['Bv.grad:' + n] = tr.Bv.view(tr.Bv.grad, n).clone()
    return r


@pytest.mark.parametrize('name', sorted(LEAK_CASES))
def test_persistent_buffers_never_leak_rows(rn, name):
    (n_big, r_big), (n, r) = LEAK_CASES[name]
    assert rn.ops.pad32(n_big) == rn.ops.pad32(n) and rn.ops.pad_to(r_big, 32) == rn.ops.pad_to(r, 32)
    assert rn.ops.relation_bwd_small_ok(torch.bfloat16, r_big, rn.ops.pad32(n_big)) == (name == 'small')
    assert rn.ops.relation_bwd_small_ok(torch.bfloat16, r, rn.ops.pad32(n)) == (name == 'small')
    used = _trainer(rn, deterministic=True)
    _head_step(used, n_big, r_big, 21)
    got = _head_step(used, n, r, 22)
    want = _head_step(_trainer(rn, deterministic=True), n, r, 22)
    for k in sorted(want):
        assert torch.isfinite(want[k].float()).all() and float(want[k].float().abs().max()) > 0, k
        assert _same(got[k], want[k]), k
