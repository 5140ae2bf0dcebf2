"""GPU tests of the sampled ROI minibatch (TRAIN.BATCH_ROIS > 0): relnet_proposal_target_sample against the reference's own sample_rois
(tests/golden/sampled_rois.npz, cases of tests/sampled_rois_cases.py), its seeds, the CustomOp forms, and the plain C4 / FPN training steps
that draw such a minibatch inside the step."""
import os
import sys

import numpy as np
import pytest
import torch

import sampled_rois_cases as SC

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import train_graph as OT  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'sampled_rois.npz'))


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, operator_py, lib
    lib.load()
    return ops, operator_py


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _run(ops, c, seed, seed_dev=None):
    o = ops.proposal_target(_d(c['rois']), _d(c['gt']), _d(c['num_gt']), c['num_reg'], c['class_agnostic'], c['bg_thresh_hi'], c['means'],
                            c['stds'], c['weights'], num_rois=None if c['num_rois'] is None else _d(c['num_rois']), batch_rois=c['R'],
                            fg_fraction=c['fg_fraction'], fg_thresh=c['fg_thresh'], bg_thresh_lo=c['bg_thresh_lo'], append_gt=c['append_gt'],
                            seed=seed, seed_dev=seed_dev, want_index=True)
    return dict(zip(('rois_out', 'label', 'bbox_target', 'bbox_weight', 'keep_index'), (t.cpu().numpy() for t in o)))


@pytest.mark.parametrize('name', list(SC.CASES))
def test_kernel_matches_the_reference_run(rn, gold, name):
    """Labels, weights, keep_index and rois_out equal; targets within 2e-6 (float64 -> float32 store against numpy's float32 log, the bound
    tests/test_gpu_targets.py holds the all-rows kernel to) -- and bit-equal to the restatement, whose log is the correctly rounded one."""
    c = SC.case(name)
    got = _run(rn[0], c, SC.SEEDS[0])
    for k in ('rois_out', 'label', 'bbox_weight', 'keep_index'):
        assert got[k].dtype == gold[name + '/' + k].dtype
        np.testing.assert_array_equal(got[k], gold[name + '/' + k], err_msg=k)
    err = float(np.abs(got['bbox_target'].astype(np.float64) - gold[name + '/bbox_target']).max())
    print('%s: max |target - golden| %.3e' % (name, err))
    assert err <= 2e-6
    np.testing.assert_array_equal(got['bbox_target'], SC.sample(c, SC.SEEDS[0])['bbox_target'])


def test_seeds(rn):
    ops = rn[0]
    for name in ('both', 'batch', 'large'):
        c = SC.case(name)
        a, a2, b = _run(ops, c, SC.SEEDS[0]), _run(ops, c, SC.SEEDS[0]), _run(ops, c, SC.SEEDS[1])
        for k in a:
            assert a[k].tobytes() == a2[k].tobytes(), k                         # same seed: same bits
        assert not np.array_equal(a['keep_index'], b['keep_index'])             # the pair the host test shows to differ
        np.testing.assert_array_equal(b['keep_index'], SC.sample(c, SC.SEEDS[1])['keep_index'])
        dev = torch.tensor([5], dtype=torch.int64).cuda()
        s = _run(ops, c, SC.SEEDS[0] - 5, seed_dev=dev)                         # seed + *seed_dev is what counts
        for k in a:
            assert a[k].tobytes() == s[k].tobytes(), k
    c = SC.case('tiny')                                                         # seed 2 - 5 wraps below zero: 64-bit sum
    a, s = _run(ops, c, 2), _run(ops, c, 2 - 5, seed_dev=torch.tensor([5], dtype=torch.int64).cuda())
    np.testing.assert_array_equal(a['keep_index'], s['keep_index'])


def test_no_candidates_and_limit(rn):
    ops = rn[0]
    c = SC.case('tiny')
    c['num_rois'], c['num_gt'] = np.zeros(1, np.int32), np.zeros(1, np.int32)
    got = _run(ops, c, 1)
    assert (got['keep_index'] == -1).all() and (got['label'] == -1).all() and not got['bbox_weight'].any() and not got['rois_out'].any()
    from relnet_amd import lib
    with pytest.raises(lib.RelnetError, match='limit'):
        ops.proposal_target(torch.zeros((1, SC.LIMIT, 5)).cuda(), torch.zeros((1, 1, 5)).cuda(), batch_rois=8)


@pytest.mark.parametrize('batch_rois', [128, -128, -2])
def test_custom_op_forward(rn, batch_rois):
    ops, operator_py = rn
    c = SC.case('large')
    rois, gt = c['rois'][0], c['gt'][0]
    r, lab, bt, bw = operator_py.Custom(rois=_d(rois), gt_boxes=_d(gt), op_type='proposal_target', num_classes=2, batch_images=1,
                                        batch_rois=batch_rois, fg_fraction=0.25, cfg={'seed': SC.SEEDS[0]})
    r, lab, bt, bw = (t.cpu().numpy() for t in (r, lab, bt, bw))
    if batch_rois == -2:            # every proposal, no gt rows: the first N rows of the all-rows kernel
        a = [t[0, :len(rois)].cpu().numpy() for t in ops.proposal_target(_d(rois[None]), _d(gt[None]))]
        assert r.shape == (len(rois), 5) and np.array_equal(r[:, 1:], rois[:, 1:])
    else:
        c['R'], c['append_gt'] = 128, batch_rois > 0
        w = SC.sample(c, SC.SEEDS[0])
        a = [w[k][0] for k in ('rois_out', 'label', 'bbox_target', 'bbox_weight')]
        assert r.shape == (128, 5) and int((lab > 0).sum()) == 32
    for got, want in zip((r, lab, bt, bw), a):
        np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------------------
# training steps
# ---------------------------------------------------------------------------------------
def _compare_gradients(tr, want, wb, res, fpn=None):
    """tests/test_gpu_train_step.py's comparison and bounds: cosine >= 0.995 and norm within 3 % for the head tensors, `res` / `fpn` =
    (minimum cosine, norm tolerance) of the trunk's and the neck's tensors."""
    report, bad = [], []
    for name, w in list(want.items()) + [('bias:' + k, v) for k, v in wb.items()]:
        got = (tr.Bv.view(tr.Bv.grad, name[5:]) if name.startswith('bias:') else tr.W.view(tr.W.grad, name)).cpu().double().reshape(w.shape)
        nw, ng = float(w.norm()), float(got.norm())
        cos = float((w * got).sum() / max(nw * ng, 1e-300))
        report.append('%-22s |want| %.3e |got| %.3e cos %.4f' % (name, nw, ng, cos))
        cmin, nmax = res if name.startswith('res') else fpn if 'fpn' in name else (0.995, 0.03)
        if nw > 1e-9 and (cos < cmin or abs(ng / nw - 1) > nmax):
            bad.append(report[-1])
    print('\n'.join(report))
    assert not bad, '\n'.join(bad) + '\n--- all ---\n' + '\n'.join(report)
    assert set(want) == set(tr.W.slices)


def test_plain_trainer_step_draws_a_sampled_minibatch():
    from test_gpu_train_step import _setup
    from relnet_amd import ops
    H, W, G, R = 128, 160, 4, 16
    p, cfg, data, gt, L, Tg, Wg, train = _setup(H, W, G, 31)
    cfg.relation, cfg.enable_ohem, cfg.batch_rois = False, False, R
    tr = train.Trainer(p, cfg, im_hw=(H, W))
    im_info = torch.tensor([[H, W, 1.0]]).cuda()
    batch = (data.cuda(), im_info, _d(gt), _d(L[None]), _d(Tg[None]), _d(Wg[None]))
    k0 = int(tr._anchor_step)
    out = tr.forward_backward(*batch)
    assert int(tr._anchor_step) == k0 + 1                   # host-made anchor targets: the sampler advanced the step counter itself
    assert out['rois'].shape == (1, R, 5) and out['label'].shape == (1, R) and out['cls_score'].shape[:2] == (1, R)
    # ---- the step's rows are the ops-level call on the step's own proposals
    want = ops.proposal_target(out['proposals'], _d(gt), None, batch_rois=R, fg_fraction=cfg.fg_fraction, fg_thresh=cfg.fg_thresh,
                               bg_thresh_lo=cfg.bg_thresh_lo, seed=0, seed_dev=torch.tensor([k0], dtype=torch.int64).cuda(), want_index=True,
                               **train.box_target_layout(cfg))
    for k, w in zip(('rois', 'label', 'bbox_target', 'bbox_weight', 'keep_index'), want):
        assert torch.equal(out[k], w), k
    assert int((out['label'] > 0).sum()) > 0 and int((out['label'] == 0).sum()) > 0
    keep1 = out['keep_index'].clone()
    # ---- gradients: float64 autograd of the plain-head loss on those rows, box loss / R
    pt = {k: v.double().clone().requires_grad_(not any(f in k for f in ('conv1', 'bn', 'res2'))) for k, v in p.items()}
    loss, parts = OT.total_loss(data.numpy(), pt, out['rois'][0].cpu().numpy(), out['label'][0].cpu().numpy(), out['bbox_target'][0].cpu().numpy(),
                                out['bbox_weight'][0].cpu().numpy(), L, Tg, Wg, R, relation=False, batch_rois_ohem=R)
    loss.backward()
    e_cs = float((out['cls_score'][0].cpu().double() - parts['cls_score']).abs().max() / parts['cls_score'].abs().max())
    assert e_cs <= 0.08, e_cs

    def packed(name):
        g_ = pt[name + '_weight'].grad
        return g_.permute(0, 2, 3, 1).reshape(g_.shape[0], -1)
    wg = {n: packed(n) * tr.bn_scale[n].cpu().double().view(-1, 1) for n in tr.W.slices if n.startswith('res')}
    wg.update({'rpn_conv_3x3': packed('rpn_conv_3x3'), 'rpn_out': torch.cat([packed('rpn_cls_score'), packed('rpn_bbox_pred')], 0),
               'conv_new_1': packed('conv_new_1'), 'fc_new_1': pt['fc_new_1_weight'].grad[:, tr.fc1_perm], 'fc_new_2': pt['fc_new_2_weight'].grad,
               'cls_bbox': torch.cat([pt['cls_score_weight'].grad, pt['bbox_pred_weight'].grad], 0)})
    wb = {'rpn_conv_3x3': pt['rpn_conv_3x3_bias'].grad, 'conv_new_1': pt['conv_new_1_bias'].grad,
          'rpn_out': torch.cat([pt['rpn_cls_score_bias'].grad, pt['rpn_bbox_pred_bias'].grad]),
          'fc_new_1': pt['fc_new_1_bias'].grad, 'fc_new_2': pt['fc_new_2_bias'].grad,
          'cls_bbox': torch.cat([pt['cls_score_bias'].grad, pt['bbox_pred_bias'].grad])}
    _compare_gradients(tr, wg, wb, (0.98, 0.08))            # that file's bounds for the bf16 C4 trunk
    # ---- the next step draws another sample from the same proposals
    out2 = tr.forward_backward(*batch)
    assert torch.equal(out2['proposals'], out['proposals']) and not torch.equal(out2['keep_index'], keep1)
    # ---- captured, with the anchor targets made on the device (rpn_targets advances the counter, the sampler reads it after that)
    dev_batch = batch[:3]
    with torch.no_grad():
        tr.forward_backward(*dev_batch)
        step = train.CapturedStep(tr, dev_batch)
        k = int(tr._anchor_step)
        keeps = []
        for _ in range(2):
            o = step.replay()
            torch.cuda.synchronize()
            keeps.append((o['keep_index'].clone(), o['label'].clone(), o['rois'].clone()))
        assert int(tr._anchor_step) == k + 2
        assert not torch.equal(keeps[0][0], keeps[1][0])            # every replay draws a new sample
        for i in range(2):                                          # ... the one the eager step draws for the same counter
            tr._anchor_step.fill_(k + i)
            e = tr.forward_backward(*dev_batch)
            torch.cuda.synchronize()
            assert torch.equal(e['keep_index'], keeps[i][0]) and torch.equal(e['label'], keeps[i][1]) and torch.equal(e['rois'], keeps[i][2])


def _fpn_plain_loss(data, p, rois, level, label, bbox_target, bbox_weight, R):
    """oracle/train_graph.py:total_loss_fpn with the plain 2FC head (its _head_losses, relation=False) and the box loss / R."""
    from oracle import fpn as OF
    pd = {k: v.double() for k, v in p.items()}
    cast = lambda x: x.double() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.float64)
    old_n, old_f = OT.ON._t, OF._t
    OT.ON._t = OF._t = cast
    try:
        c2, c3, c4, c5 = OT.ON.backbone(torch.as_tensor(np.asarray(data), dtype=torch.float64), pd, fpn=True)
        feats = OF.fpn_neck(c2, c3, c4, c5, pd)
    finally:
        OT.ON._t, OF._t = old_n, old_f
    C = feats[0].shape[1]
    pooled = torch.zeros(R, C, 7, 7, dtype=torch.float64)
    for l, sc in enumerate((1 / 4.0, 1 / 8.0, 1 / 16.0, 1 / 32.0)):
        sel = np.where(level == l)[0]
        if not len(sel):
            continue
        _, arg = OT.ORP.roi_pooling(feats[l].detach().numpy().astype(np.float32), rois[sel], (7, 7), sc, return_argmax=True)
        idx = torch.as_tensor(arg.astype(np.int64))
        flat = feats[l][0].reshape(C, -1)
        g = torch.gather(flat, 1, idx.clamp(min=0).permute(1, 0, 2, 3).reshape(C, -1)).reshape(C, len(sel), 7, 7).permute(1, 0, 2, 3)
        pooled[torch.as_tensor(sel)] = g * (idx >= 0).double()
    cls_score, _, _, _, l_cls, l_box = OT._head_losses(pooled, rois, pd, label, bbox_target, bbox_weight, R, R, ('roi_pool_fc1', 'roi_pool_fc2'),
                                                       relation=False)
    return l_cls + l_box, cls_score.detach()


def test_fpn_trainer_step_samples_real_rows_only():
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, train
    from test_gpu_fpn import _proposals
    H, W, G, N, R, real = 128, 160, 4, 60, 16, 25
    p = backbone.init_params(seed=41, fpn=True)
    g = torch.Generator().manual_seed(42)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    for lvl in (4, 8, 16, 32):              # pyramid features of ~0.1, as tests/test_gpu_train_step.py sets them
        p['fpn_ft%d_1x1_weight' % lvl] = p['fpn_ft%d_1x1_weight' % lvl] * 2
        p['fpn_ft%d_3x3_weight' % lvl] = p['fpn_ft%d_3x3_weight' % lvl] * 2
        p['fpn_ft%d_3x3_bias' % lvl] = torch.rand(256, generator=g) * 0.1
    cfg = train.TrainConfig()
    cfg.relation, cfg.learn_nms, cfg.enable_ohem, cfg.batch_rois = False, False, False, R
    # float32 conv1 .. res5 (same wiring code), the form tests/test_gpu_train_step.py pins the FPN trunk's wiring with: what reaches the trunk's
    # tensors is then the bf16 neck's / heads' error, not ~100 layers of rounding on a gradient that only 16 rois feed (with the bf16 trunk two
    # of its 100 tensors came out at cosine 0.968 / 0.969, all others above 0.97; the sampler does not touch the trunk)
    cfg.trunk_fp32 = True
    data = torch.randn(1, 3, H, W, generator=g)
    props = _proposals(N, 43, H, W)[None].copy()
    gt = np.zeros((1, G, 5), np.float32)
    gt[0, :, :4] = props[0, [8, 17, 19, 23]]
    gt[0, :, 4] = [3, 17, 17, 60]
    # rows past num_proposals: would-be foreground (a gt box moved by one pixel) that must never be drawn
    props[0, real:] = gt[0, np.arange(N - real) % G, :4] + 1.0
    padded = {tuple(b) for b in props[0, real:]}
    from relnet_amd import metric
    tm = metric.TrainMetrics(cfg)
    tr = train.FPNTrainer(p, cfg, metrics=tm)
    batch = (data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), _d(gt), _d(props))
    npr = torch.tensor([real], dtype=torch.int32).cuda()
    keeps = []
    for it in range(3):
        out = tr.forward_backward(*batch, num_proposals=npr)
        rois, perm, keep = out['rois'][0].cpu().numpy(), out['perm'][0].cpu().numpy(), out['keep_index'][0].cpu().numpy()
        assert rois.shape == (R, 5) and np.array_equal(np.sort(perm), np.arange(R)) and (np.diff(out['roi_level'][0].cpu().numpy()) >= 0).all()
        assert keep.min() >= 0 and keep.max() < real + G
        cand = np.vstack((props[0, :real], gt[0, :, :4]))
        np.testing.assert_array_equal(rois[:, 1:], cand[keep][perm])            # level-major rows = the drawn candidates
        assert not ({tuple(b) for b in rois[:, 1:]} & padded)
        assert int((out['label'] > 0).sum()) > 0 and int((out['label'] == 0).sum()) > 0 and not int((out['label'] < 0).sum())
        keeps.append(keep)
    assert not np.array_equal(keeps[0], keeps[1]) and not np.array_equal(keeps[1], keeps[2])
    counts = dict(zip(tm.names(), tm.get_counts()))
    assert counts['RCNNAcc'][1] == 3 * R and counts['RCNNLogLoss'][1] == 3 * R          # the device metrics count the R sampled rows of every step
    # ---- gradients of the last step
    pt = {k: v.double().clone().requires_grad_(not any(f in k for f in ('conv1', 'bn', 'res2'))) for k, v in p.items()}
    loss, cs = _fpn_plain_loss(data.numpy(), pt, rois, out['roi_level'][0].cpu().numpy(), out['label'][0].cpu().numpy(),
                               out['bbox_target'][0].cpu().numpy(), out['bbox_weight'][0].cpu().numpy(), R)
    loss.backward()
    e_cs = float((out['cls_score'][0].cpu().double() - cs).abs().max() / cs.abs().max())
    assert e_cs <= 0.08, e_cs

    def packed(name):
        g_ = pt[name + '_weight'].grad
        return g_.permute(0, 2, 3, 1).reshape(g_.shape[0], -1)
    wg, wb = {}, {}
    for name in tr.W.slices:
        if name.startswith('res'):
            wg[name] = packed(name) * tr.bn_scale[name].cpu().double().view(-1, 1)
        elif name.startswith('fpn_'):
            wg[name] = packed(name); wb[name] = pt[name + '_bias'].grad
    wg['fc_new_1'] = pt['roi_pool_fc1_weight'].grad[:, tr.fc1_perm]; wb['fc_new_1'] = pt['roi_pool_fc1_bias'].grad
    wg['fc_new_2'] = pt['roi_pool_fc2_weight'].grad; wb['fc_new_2'] = pt['roi_pool_fc2_bias'].grad
    wg['cls_bbox'] = torch.cat([pt['cls_score_weight'].grad, pt['bbox_pred_weight'].grad], 0)
    wb['cls_bbox'] = torch.cat([pt['cls_score_bias'].grad, pt['bbox_pred_bias'].grad])
    # that file's bounds for its float32-trunk case: trunk 0.99 / 4 %, neck 0.97 / 8 %, heads 0.995 / 3 %
    _compare_gradients(tr, wg, wb, (0.99, 0.04), (0.97, 0.08))
