"""The trunk is written once (backbone.walk_units / bottleneck_unit / fpn_neck / rpn_head) and its training adjoint stands beside it
(backbone.TrunkTrain): the training trunk and the inference trunk are one computation, the activations the training forward keeps are the
forward's own buffers, and the neck's adjoint matches float64 autograd.  The first two tests use names that older trees have too."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('hw,fpn', [((104, 136), False), ((128, 160), True)])
def test_train_trunk_and_inference_trunk_are_one_computation(hw, fpn):
    """Backbone(dtype=float32) (impl 'hip32', all stages) against a cfg.trunk_fp32 trainer's _trunk_forward on the same two images: both run
    relnet_conv2d_nhwc_f32 on the same folded weights in the same [Cout, R*S*Cin] packing with the same folded bias, through the same walk
    and the same unit, so conv4 and conv5 are EQUAL.  104 x 136 gives 26 x 34, 13 x 17 and 7 x 9 maps: every stride-2 unit sees an odd
    extent.  FPN (128 x 160, stride-2 res5 without dilation): Backbone.forward does not return the stage ends that feed its laterals, so
    conv4 and conv5 are compared, and the trainer's ends[4] / ends[5] must BE those two maps."""
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, train
    H, W = hw
    p = backbone.init_params(seed=71, fpn=fpn)
    data = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(72)).cuda()
    bb = backbone.Backbone(p, dtype=torch.float32, device='cuda', fpn=fpn)
    assert bb.impl == 'hip32' and not bb.frozen_only
    out = bb.forward(data)
    cfg = train.TrainConfig()
    cfg.trunk_fp32 = True
    tr = train.FPNTrainer(p, cfg) if fpn else train.Trainer(p, cfg, im_hw=hw)
    conv5, conv4, saved, ends = tr._trunk_forward(data)
    torch.cuda.synchronize()
    assert conv4.dtype == torch.float32 and len(saved) == 30 and float(conv5.abs().max()) > 0
    for name, got in (('conv4', conv4), ('conv5', conv5)):
        want = out[name].permute(0, 2, 3, 1)
        diff = float((got - want).abs().max())
        print('%s %s fpn=%s: max |train - inference| %.3e' % (name, tuple(got.shape), fpn, diff))
        assert torch.equal(got, want), (name, diff)
    if fpn:
        assert ends[4] is conv4 and ends[5] is conv5 and ends[3].shape[3] == 512 and ends[2].shape[3] == 256
        assert ends[3].data_ptr() == saved[4][5].data_ptr()                  # res3's end is the tensor res4a read


def test_kept_activations_are_the_forwards_own(monkeypatch):
    """bf16 trainer, chain thresholds lowered to 1 (every res3 .. res5 boundary on the chain kernels), 2 x 128 x 160.  Inside a stage a
    unit's kept output IS the next unit's kept input; the kept reduce output of a unit whose predecessor's chain kernel produced it IS
    that kernel's second output, and no second reduce convolution was launched for it: the forward's relnet_conv2d* calls are the frozen
    part's own plus 38 = 3 projections + 30 3x3 layers + the 5 reduce layers no chain kernel precedes with a second product (res3a,
    res4a: first of a stage; res5a, b, c: mid 512 has the expand-only form)."""
    import relnet_amd as rn
    from relnet_amd import backbone, ops, train
    monkeypatch.setattr(ops, 'CHAIN_MIN_PIXELS', {k: 1 for k in ops.CHAIN_MIN_PIXELS})
    chained = []
    real_chain = ops.bottleneck_chain

    def chain(*a, **kw):
        chained.append(real_chain(*a, **kw))
        return chained[-1]
    monkeypatch.setattr(ops, 'bottleneck_chain', chain)
    calls = []

    def recorder(name):
        calls.append(name)
        return contextlib.nullcontext()
    p = backbone.init_params(seed=73)
    data = torch.randn(2, 3, 128, 160, generator=torch.Generator().manual_seed(74)).cuda()
    tr = train.Trainer(p, train.TrainConfig(), im_hw=(128, 160))
    assert len(tr.chain_units) == 30
    tr._fragpack.run()
    monkeypatch.setattr(rn.lib, 'timing_hook', recorder)
    tr._frozen_backbone.forward_res2(data)
    frozen_convs = sum(c.startswith('relnet_conv2d') for c in calls)
    del calls[:], chained[:]
    conv5, conv4, saved, ends = tr._trunk_forward(data)
    monkeypatch.setattr(rn.lib, 'timing_hook', None)
    torch.cuda.synchronize()
    convs = sum(c.startswith('relnet_conv2d') for c in calls)
    print('relnet_conv2d* calls of _trunk_forward: %d (frozen part %d)' % (convs, frozen_convs))
    assert convs == frozen_convs + 38, calls
    assert [s[1] for s in saved] == [u[1] for u in tr.units if u[0] > 2]
    for a, b in zip(saved, saved[1:]):
        if a[0] == b[0]:
            assert a[8].data_ptr() == b[5].data_ptr(), (a[1], b[1])
    assert saved[-1][8] is conv5 and conv4.data_ptr() == saved[26][8].data_ptr()
    by_out = {s[8].data_ptr(): i for i, s in enumerate(saved)}
    handed_over = 0
    for xn, m1 in [c for c in chained if c[0].data_ptr() in by_out]:        # (the frozen part's chain calls keep nothing)
        i = by_out[xn.data_ptr()]
        assert (m1 is not None) == tr.chain_units[saved[i][1]][0]
        if m1 is not None:
            assert saved[i + 1][6].data_ptr() == m1.data_ptr(), saved[i + 1][1]
            handed_over += 1
    assert handed_over == 3 + 22


def test_neck_adjoint_matches_float64_autograd():
    """TrunkTrain.neck_forward / neck_backward on random bf16 stage ends of the smallest pyramid (2 x 64 x 96: 16 x 24 .. 2 x 3) against
    float64 autograd of F.conv2d / F.interpolate(mode='nearest') on the same bf16-rounded operands: d_c5, inject['4b22'], inject['3b3'] and
    the eight fpn_ft* weight-gradient slices with cosine >= 0.999 and norm within 1 % (tighter than the end-to-end bounds of
    test_gpu_train_step.py:375 for the same tensors, 0.97 / 8 %, which include ~100 layers of forward error)."""
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, train
    g = torch.Generator().manual_seed(75)
    p = backbone.init_params(seed=76, fpn=True)
    for lvl in (4, 8, 16, 32):
        for k in ('1x1', '3x3'):
            p['fpn_ft%d_%s_bias' % (lvl, k)] = torch.rand(256, generator=g) * 0.1
    cfg = train.TrainConfig()
    cfg.trunk_fp32 = False
    tr = train.FPNTrainer(p, cfg)
    bf = torch.bfloat16
    B, H, W = 2, 64, 96
    ends = {s: torch.randn(B, H // st, W // st, c, generator=g).to(bf).cuda() for s, st, c in ((2, 4, 256), (3, 8, 512), (4, 16, 1024), (5, 32, 2048))}
    tr._grad_buckets().reset()
    tr.W.grad.zero_(); tr.Bv.grad.zero_()
    tr._relayout.run()
    feats, ctx = tr._trunk.neck_forward(ends)
    d_feats = {lvl: (torch.randn(feats[lvl].shape, generator=g) * 0.01).to(bf).cuda() for lvl in (4, 8, 16, 32)}
    d_c5, inject = tr._trunk.neck_backward(ctx, d_feats)
    tr._flush_wgrads()
    torch.cuda.synchronize()
    assert sorted(inject) == ['3b3', '4b22']
    # ---- float64 autograd on the bf16-rounded operands
    nchw = lambda t: t.permute(0, 3, 1, 2)
    x = {s: nchw(ends[s]).double().cpu().requires_grad_(s > 2) for s in ends}
    wt = {}
    for lvl in (4, 8, 16, 32):
        for k, ks in (('1x1', 1), ('3x3', 3)):
            n = 'fpn_ft%d_%s' % (lvl, k)
            w = tr.w(n).double().cpu()
            wt[n] = (w.view(256, ks, ks, -1).permute(0, 3, 1, 2).contiguous().requires_grad_(True), tr.b(n).double().cpu())
    tops = {32: F.conv2d(x[5], *wt['fpn_ft32_1x1'])}
    for lvl, s in ((16, 4), (8, 3), (4, 2)):
        tops[lvl] = F.conv2d(x[s], *wt['fpn_ft%d_1x1' % lvl]) + F.interpolate(tops[lvl * 2], scale_factor=2, mode='nearest')
    loss = sum((F.conv2d(tops[lvl], *wt['fpn_ft%d_3x3' % lvl], padding=1) * nchw(d_feats[lvl]).double().cpu()).sum() for lvl in (4, 8, 16, 32))
    loss.backward()
    pairs = [('d_c5', d_c5, x[5].grad.permute(0, 2, 3, 1)), ("inject['4b22']", inject['4b22'], x[4].grad.permute(0, 2, 3, 1)),
             ("inject['3b3']", inject['3b3'], x[3].grad.permute(0, 2, 3, 1))]
    for n, (w, _) in wt.items():
        pairs.append((n, tr.W.view(tr.W.grad, n), w.grad.permute(0, 2, 3, 1).reshape(256, -1)))
    bad = []
    for name, got, want in pairs:
        got = got.double().cpu().reshape(want.shape)
        ng, nw = float(got.norm()), float(want.norm())
        cos = float((got * want).sum() / max(ng * nw, 1e-300))
        print('%-16s |want| %.3e |got| %.3e cos %.6f' % (name, nw, ng, cos))
        if not (nw > 0 and cos >= 0.999 and abs(ng / nw - 1) <= 0.01):
            bad.append((name, cos, ng / max(nw, 1e-300)))
    assert len(pairs) == 11 and not bad, bad
