"""Training and inference through ROIAlign (cfg.roi_align): the C4 Trainer and the FPNTrainer pool with ops.roi_align_fpn and
backpropagate with ops.roi_align_fpn_bwd, and every gradient matches float64 autograd of the train graph restated with the definition's
ROIAlign (a sparse sample matrix, tests/test_gpu_roi_align_levels.py:sample_matrix) in place of ROIPooling.  The FPN detector pools the
same way; graph capture and the checkpoint round trip keep the operator."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import network as ON, train_graph as OT, roi_align as ORA  # noqa: E402
from oracle.losses import smooth_l1  # noqa: E402
from test_gpu_roi_align_levels import sample_matrix  # noqa: E402

pytestmark = pytest.mark.gpu

FPN_SCALES = (1 / 4.0, 1 / 8.0, 1 / 16.0, 1 / 32.0)


def _feat_size(n):
    n = (n + 2 * 3 - 7) // 2 + 1
    n = -(-(n - 3) // 2) + 1
    n = (n - 1) // 2 + 1
    return (n - 1) // 2 + 1


def _setup(H, W, G, seed):
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, train
    p = backbone.init_params(seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    p['conv_new_1_bias'] = torch.rand(256, generator=g) * 0.1 + 0.05
    cfg = train.TrainConfig()
    cfg.rpn_post_nms_top_n = 40
    cfg.roi_align = True
    data = torch.randn(1, 3, H, W, generator=g)
    rng = np.random.default_rng(seed + 2)
    gt = np.zeros((1, G, 5), np.float32)
    x1 = rng.uniform(0, W - 70, G); y1 = rng.uniform(0, H - 70, G)
    gt[0, :, 0], gt[0, :, 1] = x1, y1
    gt[0, :, 2], gt[0, :, 3] = x1 + rng.uniform(30, 69, G), y1 + rng.uniform(30, 69, G)
    gt[0, :, 4] = rng.integers(1, 81, G)
    L, Tg, Wg = train.assign_anchor((_feat_size(H), _feat_size(W)), gt[0], (H, W), cfg, seed=seed)
    return p, cfg, data, gt, L, Tg, Wg, train


def _unsaturate_lnms(p, seed=77):
    g_ = torch.Generator().manual_seed(seed)
    p['nms_logit_bias'] = torch.zeros(5)
    for k in ('nms_logit_weight', 'nms_rank_weight', 'roi_feat_embedding_weight', 'nms_query_1_weight', 'nms_key_1_weight',
              'nms_linear_out_1_weight', 'nms_pair_pos_fc1_1_weight'):
        p[k] = torch.randn(p[k].shape, generator=g_) * 0.05


def _align(feats, rois, level, scales, sampling_ratio):
    """Differentiable float64 ROIAlign of [1,C,H,W] maps: the sample matrix times the flattened maps -> [R,C,7,7]."""
    M = sample_matrix(rois, level, [tuple(f.shape) for f in feats], scales, (7, 7), sampling_ratio)
    x = torch.cat([f.permute(0, 2, 3, 1).reshape(-1, f.shape[1]) for f in feats], 0)
    R = len(rois)
    return torch.sparse.mm(M, x).reshape(R, 7, 7, -1).permute(0, 3, 1, 2)


def _f64(p):
    return {k: (v.double() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v), dtype=torch.float64)) for k, v in p.items()}


def _cast64(x):
    return x.double() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.float64)


def total_loss_align(data, p, rois, labels_ohem, bbox_target, bbox_weight_ohem, rpn_label, rpn_bbox_target, rpn_bbox_weight, nongt_dim,
                     sampling_ratio, rpn_batch_size=256, batch_rois_ohem=128, lnms=None):
    """oracle/train_graph.py:total_loss (relation head, no DCN) with ROIAlign on conv_new_1_relu in place of ROIPooling."""
    pd = _f64(p)
    old = ON._t
    ON._t = _cast64
    try:
        conv4, conv5 = ON.backbone(torch.as_tensor(np.asarray(data), dtype=torch.float64), pd)
        cls, box, feat = ON.rpn_and_feat(conv4, conv5, pd)
    finally:
        ON._t = old
    logits = cls.reshape(1, 2, -1)[0].t()
    lab = torch.as_tensor(np.asarray(rpn_label, np.int64))
    valid = lab >= 0
    logp = torch.log_softmax(logits, dim=1)
    l_rpn_cls = -(logp[torch.arange(len(lab)), lab.clamp(min=0)] * valid.double()).sum() / max(int(valid.sum()), 1)
    l_rpn_box = (torch.as_tensor(np.asarray(rpn_bbox_weight), dtype=torch.float64)
                 * smooth_l1(box[0] - torch.as_tensor(np.asarray(rpn_bbox_target), dtype=torch.float64), 3.0)).sum() / rpn_batch_size
    rois = np.asarray(rois, np.float32)
    pooled = _align([feat], rois, None, (0.0625,), sampling_ratio)
    cls_score, bbox_pred, x2, f1, l_cls, l_box = OT._head_losses(pooled, rois, pd, labels_ohem, bbox_target, bbox_weight_ohem, nongt_dim,
                                                                 batch_rois_ohem)
    l_nms, multi = 0.0, None
    if lnms is not None:
        l_nms, multi = OT.learn_nms_loss(cls_score[:nongt_dim], x2[:nongt_dim], pd, lnms['rank_idx'], lnms['class_boxes'], lnms['target'],
                                         lnms['first_n'])
    return l_rpn_cls + l_rpn_box + l_cls + l_box + l_nms, dict(nms_multi=None if multi is None else multi.detach(),
                                                                cls_score=cls_score.detach(), pooled=pooled.detach(), feat=feat.detach())


def total_loss_fpn_align(data, p, rois, level, labels_ohem, bbox_target, bbox_weight_ohem, nongt_dim, sampling_ratio, batch_rois_ohem=128,
                         lnms=None):
    """oracle/train_graph.py:total_loss_fpn with ROIAlign on fpn_ft4 .. fpn_ft32 in place of the four ROIPooling calls."""
    from oracle import fpn as OF
    pd = _f64(p)
    old_n, old_f = ON._t, OF._t
    ON._t = OF._t = _cast64
    try:
        c2, c3, c4, c5 = ON.backbone(torch.as_tensor(np.asarray(data), dtype=torch.float64), pd, fpn=True)
        feats = OF.fpn_neck(c2, c3, c4, c5, pd)
    finally:
        ON._t, OF._t = old_n, old_f
    rois = np.asarray(rois, np.float32)
    pooled = _align(list(feats[:4]), rois, level, FPN_SCALES, sampling_ratio)
    cls_score, bbox_pred, x2, f1, l_cls, l_box = OT._head_losses(pooled, rois, pd, labels_ohem, bbox_target, bbox_weight_ohem, nongt_dim,
                                                                 batch_rois_ohem, ('roi_pool_fc1', 'roi_pool_fc2'))
    l_nms = 0.0
    if lnms is not None:
        l_nms, _ = OT.learn_nms_loss(cls_score[:nongt_dim], x2[:nongt_dim], pd, lnms['rank_idx'], lnms['class_boxes'], lnms['target'],
                                     lnms['first_n'])
    return l_cls + l_box + l_nms, dict(cls_score=cls_score.detach(), pooled=pooled.detach())


def _compare(tr, want, wb, bounds):
    report, bad = [], []
    for name, w in list(want.items()) + [('bias:' + k, v) for k, v in wb.items()]:
        got = (tr.Bv.view(tr.Bv.grad, name[5:]) if name.startswith('bias:') else tr.W.view(tr.W.grad, name)).cpu().double().reshape(w.shape)
        nw, ng = float(w.norm()), float(got.norm())
        cos = float((w * got).sum() / max(nw * ng, 1e-300))
        report.append('%-22s |want| %.3e |got| %.3e cos %.4f' % (name, nw, ng, cos))
        cmin, nmax = bounds(name)
        if nw > 1e-9 and (cos < cmin or abs(ng / nw - 1) > nmax):
            bad.append(report[-1])
    assert not bad, '\n'.join(bad) + '\n--- all ---\n' + '\n'.join(report)


def _packed(pt, name):
    g_ = pt[name + '_weight'].grad
    return g_.permute(0, 2, 3, 1).reshape(g_.shape[0], -1)


@pytest.mark.parametrize('learn_nms', [False, True])
def test_c4_training_step_through_roi_align_matches_autograd(learn_nms):
    H, W, G = 128, 160, 4
    p, cfg, data, gt, L, Tg, Wg, train = _setup(H, W, G, 31)
    cfg.learn_nms, cfg.first_n = learn_nms, 24
    if learn_nms:
        _unsaturate_lnms(p)
    tr = train.Trainer(p, cfg, im_hw=(H, W))
    d = lambda a: torch.as_tensor(a).cuda()
    info = torch.tensor([[H, W, 1.0]]).cuda()
    out = tr.forward_backward(data.cuda(), info, d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
    if learn_nms:          # gt boxes ON some proposals, so that positive NMS targets exist
        props = out['rois'][0, :cfg.rpn_post_nms_top_n, 1:5].cpu().numpy()
        gt[0, :, :4] = props[[0, 7, 14, 21]]
        L, Tg, Wg = train.assign_anchor((_feat_size(H), _feat_size(W)), gt[0], (H, W), cfg, seed=31)
        out = tr.forward_backward(data.cuda(), info, d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
    g_align = tr.W.view(tr.W.grad, 'conv_new_1').double().cpu().clone()
    rois = out['rois'][0].cpu().numpy()
    N = cfg.rpn_post_nms_top_n
    assert rois.shape[0] == N + G and int((out['label'] >= 0).sum()) > 0
    pt = {k: v.double().clone().requires_grad_(not any(f in k for f in ('conv1', 'bn', 'res2'))) for k, v in p.items()}
    lnms = None
    if learn_nms:
        lnms = dict(rank_idx=out['nms_rank_idx'][0].cpu().numpy(), class_boxes=out['nms_class_boxes'][0].cpu().numpy(),
                    target=out['nms_multi_target'][0].cpu().numpy(), first_n=cfg.first_n)
        assert out['nms_multi_target'].sum() > 0
    loss, parts = total_loss_align(data.numpy(), pt, rois, out['label'][0].cpu().numpy(), out['bbox_target'][0].cpu().numpy(),
                                   out['bbox_weight'][0].cpu().numpy(), L, Tg, Wg, N, cfg.roi_align_sampling, lnms=lnms)
    loss.backward()
    if learn_nms:
        ms = out['nms_multi_score'][0].cpu().double()
        assert (ms - parts['nms_multi']).abs().max() <= 0.05 * parts['nms_multi'].abs().max()
    e_cs = float((out['cls_score'][0].cpu().double() - parts['cls_score']).abs().max() / parts['cls_score'].abs().max())
    assert e_cs <= 0.08, e_cs
    want, wb = {}, {}
    for name in tr.W.slices:
        if name.startswith('res'):
            want[name] = _packed(pt, name) * tr.bn_scale[name].cpu().double().view(-1, 1)
    want['rpn_conv_3x3'] = _packed(pt, 'rpn_conv_3x3')
    want['rpn_out'] = torch.cat([_packed(pt, 'rpn_cls_score'), _packed(pt, 'rpn_bbox_pred')], 0)
    want['conv_new_1'] = _packed(pt, 'conv_new_1')
    want['fc_new_1'] = pt['fc_new_1_weight'].grad[:, tr.fc1_perm]
    want['fc_new_2'] = pt['fc_new_2_weight'].grad
    want['cls_bbox'] = torch.cat([pt['cls_score_weight'].grad, pt['bbox_pred_weight'].grad], 0)
    wb.update({'rpn_conv_3x3': pt['rpn_conv_3x3_bias'].grad, 'conv_new_1': pt['conv_new_1_bias'].grad,
               'rpn_out': torch.cat([pt['rpn_cls_score_bias'].grad, pt['rpn_bbox_pred_bias'].grad]),
               'fc_new_1': pt['fc_new_1_bias'].grad, 'fc_new_2': pt['fc_new_2_bias'].grad,
               'cls_bbox': torch.cat([pt['cls_score_bias'].grad, pt['bbox_pred_bias'].grad])})
    for i in (1, 2):
        want['qk_%d' % i] = torch.cat([pt['query_%d_weight' % i].grad, pt['key_%d_weight' % i].grad], 0)
        want['linear_out_%d' % i] = pt['linear_out_%d_weight' % i].grad.reshape(1024, 1024)
        want['pair_pos_fc1_%d' % i] = pt['pair_pos_fc1_%d_weight' % i].grad
        wb['linear_out_%d' % i] = pt['linear_out_%d_bias' % i].grad
        wb['pair_pos_fc1_%d' % i] = pt['pair_pos_fc1_%d_bias' % i].grad
    if learn_nms:
        for n in ('nms_rank', 'roi_feat_embedding', 'nms_pair_pos_fc1_1', 'nms_logit'):
            want[n] = pt[n + '_weight'].grad; wb[n] = pt[n + '_bias'].grad
        want['nms_qk_1'] = torch.cat([pt['nms_query_1_weight'].grad, pt['nms_key_1_weight'].grad], 0)
        want['nms_linear_out_1'] = pt['nms_linear_out_1_weight'].grad.reshape(128, 128)
        wb['nms_linear_out_1'] = pt['nms_linear_out_1_bias'].grad
    assert len(want) == len(tr.W.slices)
    # the bounds of test_gpu_train_step.py::test_training_step_gradients_match_autograd
    _compare(tr, want, wb, lambda n: (0.995, 0.03) if (not n.startswith('res') and 'pair_pos' not in n) else (0.98, 0.08))
    # and the flag is not dropped: the same trainer with ROIPooling gives another conv_new_1 gradient
    cfg.roi_align = False
    tr_pool = train.Trainer(p, cfg, im_hw=(H, W))
    tr_pool.forward_backward(data.cuda(), info, d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
    g_pool = tr_pool.W.view(tr_pool.W.grad, 'conv_new_1').double().cpu()
    cos = float((g_align * g_pool).sum() / (g_align.norm() * g_pool.norm()))
    assert cos < 0.99, cos


@pytest.mark.parametrize('padded', [False, True])
def test_fpn_training_step_through_roi_align_matches_autograd(padded):
    """padded: a batched step's num_proposals -- the padding rows (zero box, label -1) are pooled but carry no loss and are no relation
    keys; the restated graph sees only the real rows."""
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, train
    from test_gpu_fpn import _proposals
    H, W, G, N = 128, 160, 4, 60
    p = backbone.init_params(seed=41, fpn=True)
    g = torch.Generator().manual_seed(42)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    for lvl in (4, 8, 16, 32):
        p['fpn_ft%d_1x1_weight' % lvl] = p['fpn_ft%d_1x1_weight' % lvl] * 2
        p['fpn_ft%d_3x3_weight' % lvl] = p['fpn_ft%d_3x3_weight' % lvl] * 2
        p['fpn_ft%d_3x3_bias' % lvl] = torch.rand(256, generator=g) * 0.1
    _unsaturate_lnms(p)
    cfg = train.TrainConfig()
    cfg.learn_nms, cfg.first_n, cfg.roi_align = not padded, 24, True
    data = torch.randn(1, 3, H, W, generator=g)
    props = _proposals(N, 43, H, W)[None]
    gt = np.zeros((1, G, 5), np.float32)
    gt[0, :, :4] = props[0, [8, 17, 29, 44]]
    gt[0, :, 4] = [3, 17, 17, 60]
    n_real = N - 9 if padded else N
    tr = train.FPNTrainer(p, cfg)
    d = lambda a: torch.as_tensor(a).cuda()
    kw = dict(num_proposals=torch.tensor([n_real], dtype=torch.int32).cuda()) if padded else {}
    out = tr.forward_backward(data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), d(gt), d(props), **kw)
    rois, level = out['rois'][0].cpu().numpy(), out['roi_level'][0].cpu().numpy()
    assert rois.shape[0] == N + G and int((out['label'] >= 1).sum()) > 0
    keep = np.r_[np.arange(n_real), np.arange(N, N + G)]                 # real non-gt rows first, padding behind them, then the gt rows
    if padded:
        assert (out['label'][0, n_real:N] == -1).all()
    pt = {k: v.double().clone().requires_grad_(not any(f in k for f in ('conv1', 'bn', 'res2'))) for k, v in p.items()}
    lnms = None
    if cfg.learn_nms:
        lnms = dict(rank_idx=out['nms_rank_idx'][0].cpu().numpy(), class_boxes=out['nms_class_boxes'][0].cpu().numpy(),
                    target=out['nms_multi_target'][0].cpu().numpy(), first_n=cfg.first_n)
    sel = lambda t: t[0].cpu().numpy()[keep]
    loss, parts = total_loss_fpn_align(data.numpy(), pt, rois[keep], level[keep], sel(out['label']), sel(out['bbox_target']),
                                       sel(out['bbox_weight']), n_real, cfg.roi_align_sampling, lnms=lnms)
    loss.backward()
    po = parts['pooled'].permute(0, 2, 3, 1).reshape(len(keep), -1)
    assert float((out['intermediates']['pooled'].double().cpu()[keep] - po).norm() / po.norm()) <= 0.03
    e_cs = float((out['cls_score'][0].cpu().double()[keep] - parts['cls_score']).abs().max() / parts['cls_score'].abs().max())
    assert e_cs <= 0.08, e_cs
    want, wb = {}, {}
    for name in tr.W.slices:
        if name.startswith('res'):
            want[name] = _packed(pt, name) * tr.bn_scale[name].cpu().double().view(-1, 1)
        elif name.startswith('fpn_'):
            want[name] = _packed(pt, name); wb[name] = pt[name + '_bias'].grad
    want['fc_new_1'] = pt['roi_pool_fc1_weight'].grad[:, tr.fc1_perm]; wb['fc_new_1'] = pt['roi_pool_fc1_bias'].grad
    want['fc_new_2'] = pt['roi_pool_fc2_weight'].grad; wb['fc_new_2'] = pt['roi_pool_fc2_bias'].grad
    want['cls_bbox'] = torch.cat([pt['cls_score_weight'].grad, pt['bbox_pred_weight'].grad], 0)
    wb['cls_bbox'] = torch.cat([pt['cls_score_bias'].grad, pt['bbox_pred_bias'].grad])
    for i in (1, 2):
        want['qk_%d' % i] = torch.cat([pt['query_%d_weight' % i].grad, pt['key_%d_weight' % i].grad], 0)
        want['linear_out_%d' % i] = pt['linear_out_%d_weight' % i].grad.reshape(1024, 1024)
        want['pair_pos_fc1_%d' % i] = pt['pair_pos_fc1_%d_weight' % i].grad
        wb['linear_out_%d' % i] = pt['linear_out_%d_bias' % i].grad
        wb['pair_pos_fc1_%d' % i] = pt['pair_pos_fc1_%d_bias' % i].grad
    if cfg.learn_nms:
        for n in ('nms_rank', 'roi_feat_embedding', 'nms_pair_pos_fc1_1', 'nms_logit'):
            want[n] = pt[n + '_weight'].grad; wb[n] = pt[n + '_bias'].grad
        want['nms_qk_1'] = torch.cat([pt['nms_query_1_weight'].grad, pt['nms_key_1_weight'].grad], 0)
        want['nms_linear_out_1'] = pt['nms_linear_out_1_weight'].grad.reshape(128, 128)
        wb['nms_linear_out_1'] = pt['nms_linear_out_1_bias'].grad
    # the bounds of test_gpu_train_step.py::test_fpn_training_step_gradients_match_autograd at N = 60, except the norm of the first relation
    # module's query / key gradient: through the bf16 pyramid and attention logits it came out 3.4 % and 5.0 % off (cosine 0.998) -- it
    # does not pass through the pooling backward, whose products (fpn_ft*, trunk) sit at cosine >= 0.999 / 0.98
    def bounds(n):
        if n.startswith('qk_'):
            return 0.995, 0.08
        return (0.995, 0.03) if (not n.startswith('res') and 'pair_pos' not in n and 'fpn' not in n) else (0.97, 0.08)
    _compare(tr, want, wb, bounds)


def test_fpn_detector_pools_with_roi_align():
    """The features that reach roi_pool_fc1 are the oracle ROIAlign of this run's fpn_ft4 .. fpn_ft32 (float32 arithmetic on the bf16 maps,
    rounded to bf16), in the dispatch's row order, padded rows included."""
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, detector
    from test_gpu_fpn import _proposals
    H, W, N = 128, 160, 40
    p = backbone.init_params(seed=3, fpn=True)
    cfg = detector.Config()
    cfg.roi_align = True
    det = detector.FPNDetector(p, cfg=cfg)
    seen = {}
    bb, hd = det.backbone.forward, det.head.forward
    det.backbone.forward = lambda *a, **k: seen.setdefault('f', bb(*a, **k))
    det.head.forward = lambda pooled, *a, **k: (seen.setdefault('pooled', pooled.clone()), hd(pooled, *a, **k))[1]
    data = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    props = torch.as_tensor(_proposals(N, 5, H, W)[None]).cuda()
    out = det.forward(data, props, torch.tensor([[H, W, 1.0]]).cuda(), post=False,
                      num_proposals=torch.tensor([N - 3], dtype=torch.int32).cuda())
    rois, level = out['rois'][0].cpu().numpy(), out['roi_level'][0].cpu().numpy()
    f = seen['f']
    maps = [f[k].float().permute(0, 3, 1, 2).cpu().numpy() if f[k].shape[-1] == 256 else f[k].float().cpu().numpy()
            for k in ('fpn_ft4', 'fpn_ft8', 'fpn_ft16', 'fpn_ft32')]
    got = seen['pooled'][0].float().cpu().view(len(rois), 7, 7, -1).permute(0, 3, 1, 2)
    for l in range(4):
        sel = np.where(level == l)[0]
        if not len(sel):
            continue
        want = torch.as_tensor(ORA.roi_align(maps[l], rois[sel], (7, 7), FPN_SCALES[l], cfg.roi_align_sampling))
        assert torch.equal(got[sel], want.to(torch.bfloat16).float()), l
    # and it is not ROIPooling
    cfg2 = detector.Config()
    det2 = detector.FPNDetector(p, cfg=cfg2)
    out2 = det2.forward(data, props, torch.tensor([[H, W, 1.0]]).cuda(), post=False,
                        num_proposals=torch.tensor([N - 3], dtype=torch.int32).cuda())
    assert not torch.equal(out['cls_score'], out2['cls_score'])


def test_captured_roi_align_step_equals_eager():
    H, W, G = 128, 160, 4
    p, cfg, data, gt, L, Tg, Wg, train = _setup(H, W, G, 41)
    cfg.learn_nms, cfg.first_n = True, 24
    tr = train.Trainer(p, cfg, im_hw=(H, W))
    d = lambda a: torch.as_tensor(a).cuda()
    batch = (data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), d(gt))
    with torch.no_grad():
        eager = tr.forward_backward(*batch)
        g_eager = tr.W.grad.clone()
        tr._anchor_step.zero_()
        step = train.CapturedStep(tr, batch, segments=True)
        tr._anchor_step.zero_()
        out = step.replay()
        torch.cuda.synchronize()
        for k in ('bbox_loss', 'rpn_bbox_loss', 'nms_pos_loss', 'nms_neg_loss'):
            assert abs(float(out[k]) - float(eager[k])) <= 1e-3 * max(abs(float(eager[k])), 1e-6), k
        num = (tr.W.grad - g_eager).norm().item()
        assert num <= 1e-3 * g_eager.norm().item(), num


def test_roi_align_checkpoint_round_trip_into_detector(tmp_path):
    """A ROIAlign trainer's checkpoint in Detector(roi_align = True): its pooled features are ROIAlign of its own conv_new_1_relu, and its
    scores those of a detector built from the trainer's exported parameters."""
    import relnet_amd  # noqa: F401
    from relnet_amd import detector, ops
    H, W, G = 128, 160, 4
    p, cfg, data, gt, L, Tg, Wg, train = _setup(H, W, G, 61)
    tr = train.Trainer(p, cfg, im_hw=(H, W))
    d = lambda a: torch.as_tensor(a).cuda()
    info = torch.tensor([[H, W, 1.0]]).cuda()
    tr.step(data.cuda(), info, d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
    prefix = str(tmp_path / 'align')
    tr.save_checkpoint(prefix, 0)
    dcfg = detector.Config(); dcfg.rpn_post_nms_top_n = 40; dcfg.roi_align = True
    det = detector.Detector.from_checkpoint(prefix, 1, im_hw=(H, W), cfg=dcfg)
    out = det.forward(data.cuda(), info, post=False, keep_features=True)
    feat, rois = out['features']['conv_new_1_relu'], out['rois'].view(-1, 5)
    want = ops.roi_align(feat, rois, (7, 7), 1 / 16.0, dcfg.roi_align_sampling, channels_last_out=True)
    assert torch.equal(out['pooled'].reshape(-1), want.permute(0, 2, 3, 1).reshape(-1))
    assert not torch.equal(want, ops.roi_pool(feat, rois, (7, 7), 1 / 16.0, channels_last_out=True))
    # the exported trainer weights (the fixed ones from the source parameters) give the same scores
    params = dict(p)
    params.update(tr.export_params())
    params['bbox_pred_weight'] = params['bbox_pred_weight'] * torch.tensor(cfg.bbox_stds * 2)[:, None]
    params['bbox_pred_bias'] = params['bbox_pred_bias'] * torch.tensor(cfg.bbox_stds * 2) + torch.tensor(cfg.bbox_means * 2)
    ref = detector.Detector(params, im_hw=(H, W), cfg=dcfg).forward(data.cuda(), info, post=False)
    assert torch.equal(out['rois'], ref['rois'])
    assert float((out['cls_score'].float() - ref['cls_score'].float()).abs().max()) <= 1e-2 * float(ref['cls_score'].float().abs().max())
