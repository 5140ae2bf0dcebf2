"""The trainers with a metric.TrainMetrics attached: the device accumulator after a step equals metric.py's host classes
applied to that step's own output tensors (counts equal; float64 sums within n * 2^-52 * sum|x|, see test_gpu_metrics.py),
metrics=None changes nothing, and a CapturedStep keeps counting on every replay without a host synchronisation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metric_cases as MC  # noqa: E402
from test_gpu_train_step import _setup  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, G = 128, 160, 4
LOSSES = ('bbox_loss', 'rpn_bbox_loss', 'nms_pos_loss', 'nms_neg_loss')
NEW_KEYS = {'rpn_cls_prob', 'rpn_label', 'cls_prob', 'nms_conditional_score', 'rpn_bbox_loss_map', 'bbox_loss_map', 'nms_pos_loss_map',
            'nms_neg_loss_map'}


def _lnms_params(p, seed):
    g = torch.Generator().manual_seed(seed)
    p['nms_logit_bias'] = torch.zeros(5)
    for k in ('nms_logit_weight', 'nms_rank_weight', 'roi_feat_embedding_weight', 'nms_query_1_weight', 'nms_key_1_weight',
              'nms_linear_out_1_weight', 'nms_pair_pos_fc1_1_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    return p


def _tensors(out, rpn=True, nms=True):
    """The step's own outputs as the host classes' input dictionary."""
    cpu = lambda t: t.detach().float().cpu().numpy()
    d = {'cls_prob': cpu(out['cls_prob']), 'rcnn_label': cpu(out['label']), 'bbox_loss': cpu(out['bbox_loss_map'])}
    if rpn:
        d.update(rpn_cls_prob=cpu(out['rpn_cls_prob']), rpn_label=cpu(out['rpn_label']), rpn_bbox_loss=cpu(out['rpn_bbox_loss_map']))
    if nms:
        d.update(nms_multi_target=cpu(out['nms_multi_target']), nms_conditional_score=cpu(out['nms_conditional_score']),
                 nms_pos_loss=cpu(out['nms_pos_loss_map']), nms_neg_loss=cpu(out['nms_neg_loss_map']))
    return d


def _check(tm, d, images):
    rpn, nms = 'rpn_cls_prob' in d, 'nms_multi_target' in d
    host = MC.host_counts(d, rpn=rpn, nms=nms)
    got = dict(zip(tm.names(), tm.get_counts()))
    assert sorted(got) == sorted(host)
    for name, (s, n) in got.items():
        hs, hn = host[name]
        if name.startswith('NMSLoss'):
            hn = images
        assert n == hn, (name, n, hn)
        if name in MC.INTEGER:
            assert s == hs, (name, s, hs)
        else:
            tol = MC.n_terms(d, name) * 2.0 ** -52 * abs(hs)
            print('%s: device %.17g host %.17g diff %.3g tol %.3g' % (name, s, hs, abs(s - hs), tol))
            assert abs(s - hs) <= tol, (name, s, hs, tol)
    return got


def _trainer(seed, learn_nms=True, metrics=True):
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M
    p, cfg, data, gt, L, Tg, Wg, train = _setup(H, W, G, seed)
    if learn_nms:
        _lnms_params(p, seed + 7)
        cfg.learn_nms, cfg.first_n = True, 24
    tm = M.TrainMetrics(cfg) if metrics else None
    tr = train.Trainer(p, cfg, im_hw=(H, W), metrics=tm)
    d = lambda a: torch.as_tensor(a).cuda()
    batch = (data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
    return tr, tm, batch, train


def test_eager_step_accumulates_what_the_host_classes_compute():
    tr, tm, batch, _ = _trainer(61)
    assert tm.names() == MC.ORDER
    with torch.no_grad():
        out = tr.forward_backward(*batch)
    torch.cuda.synchronize()
    assert NEW_KEYS <= set(out) and out['cls_prob'].dim() == 3 and out['nms_conditional_score'].shape == out['nms_multi_target'].shape
    d = _tensors(out)
    got = _check(tm, d, images=1)
    s, n = got['RPNL1Loss']
    assert n == int((d['rpn_label'] != -1).sum()) and n > 0
    assert abs(s - float(out['rpn_bbox_loss'])) <= 1e-3 * max(abs(s), 1e-6)          # the step's own loss scalar is this sum (one image)
    assert got['RPNAcc'][1] > 0 and got['RCNNAcc'][1] > 0 and got['NMSAcc_neg'][1] > 0
    names, values = tm.get()
    assert names == MC.ORDER and values[MC.ORDER.index('NMSLoss_pos')] == got['NMSLoss_pos'][0] / 1
    # a second step adds to the same accumulator; reset clears it
    with torch.no_grad():
        tr.forward_backward(*batch)
    assert dict(zip(tm.names(), tm.get_counts()))['NMSLoss_pos'][1] == 2
    tm.reset()
    assert all(np.isnan(v) for v in tm.get()[1])


def test_metrics_none_is_the_step_as_it_was():
    tr, tm, batch, _ = _trainer(61)
    tr0, _, batch0, _ = _trainer(61, metrics=False)
    with torch.no_grad():
        out, out0 = tr.forward_backward(*batch), tr0.forward_backward(*batch0)
    torch.cuda.synchronize()
    assert set(out) - set(out0) == NEW_KEYS and not (set(out0) & NEW_KEYS) and set(out0) <= set(out)
    for k in LOSSES:
        assert abs(float(out[k]) - float(out0[k])) <= 1e-3 * max(abs(float(out0[k])), 1e-6), k
    assert int(out['num_ohem']) == int(out0['num_ohem'])


def test_captured_step_counts_on_every_replay():
    tr, tm, full, train = _trainer(41)
    batch = full[:3]                                     # no host anchor targets: computed on the device inside the step, as bench.py's
    with torch.no_grad():
        tr.forward_backward(*batch)                      # warm-up (counts: thrown away below)
        tr._anchor_step.zero_()
        step = train.CapturedStep(tr, batch)
        assert len(step.segments) == 1
        torch.cuda.synchronize()
        tm.reset()                                       # (the capture itself launched nothing)
        tr._anchor_step.zero_()
        out = step.replay()
        one = tm.acc.clone()
        one_counts = dict(zip(tm.names(), tm.get_counts()))
        _check(tm, _tensors(out), images=1)
        tm.reset()
        for _ in range(3):                               # no host synchronisation between the replays
            tr._anchor_step.zero_()
            step.replay()
        three = tm.acc.clone()
    torch.cuda.synchronize()
    c1, c3 = one[:16].cpu().numpy(), three[:16].cpu().numpy()
    assert c1[1] > 0 and c1[4] > 0 and c1[6] == 1 and (c3 == 3 * c1).all(), (c1, c3)
    s1, s3 = one[16:].view(torch.float64).cpu().numpy(), three[16:].view(torch.float64).cpu().numpy()
    assert (s1[[0, 2, 5]] > 0).all() and (s1 >= 0).all() and (s3 == (s1 + s1) + s1).all(), (s1, s3)      # the same double added three times
    assert one_counts['NMSLoss_pos'][1] == 1


def test_learn_nms_only_experiment_reports_all_ten():
    """The learn-NMS-only step (detector fixed, the step returns right after the learn-NMS head, the side stream is joined whole):
    the same ten metrics as the joint experiment -- a deliberate difference from the reference, which registers no RPN metric there."""
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M
    p, _, data, gt, L, Tg, Wg, train = _setup(H, W, G, 57)
    _lnms_params(p, 58)
    cfg = train.TrainConfig.from_experiment('rcnn_end2end_learn_nms_3epoch', train=True)
    cfg.rpn_post_nms_top_n, cfg.first_n = 40, 24
    tm = M.TrainMetrics(cfg)
    tr = train.Trainer(p, cfg, im_hw=(H, W), metrics=tm)
    assert tr.lnms_only and tm.names() == MC.ORDER
    d = lambda a: torch.as_tensor(a).cuda()
    batch = (data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
    with torch.no_grad():
        out = tr.forward_backward(*batch)
        got = _check(tm, _tensors(out), images=1)
        assert got['RPNAcc'][1] > 0 and got['RCNNAcc'][1] > 0
        step = train.CapturedStep(tr, batch)                # (runs its own eager warm-up: no update has been made yet)
        torch.cuda.synchronize()
        tm.reset()
        out = step.replay()
        _check(tm, _tensors(out), images=1)


def test_plain_head_without_learn_nms_has_six_metrics():
    tr, tm, batch, _ = _trainer(63, learn_nms=False)
    assert tm.names() == MC.ORDER[:6]
    with torch.no_grad():
        out = tr.forward_backward(*batch)
    torch.cuda.synchronize()
    assert 'nms_conditional_score' not in out and {'rpn_cls_prob', 'rpn_label', 'cls_prob'} <= set(out)
    _check(tm, _tensors(out, nms=False), images=1)
    c = tm.counts.cpu().numpy()
    assert (c[6:] == 0).all() and (tm.sums.cpu().numpy()[4:] == 0).all()               # the NMS kernels were not launched


def test_fpn_trainer_has_no_rpn_metrics_and_skips_padded_rows():
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, metric as M, train
    from test_gpu_fpn import _proposals
    N, n_real = 60, 47
    p = backbone.init_params(seed=41, fpn=True)
    g = torch.Generator().manual_seed(42)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    for lvl in (4, 8, 16, 32):
        p['fpn_ft%d_1x1_weight' % lvl] = p['fpn_ft%d_1x1_weight' % lvl] * 2
        p['fpn_ft%d_3x3_weight' % lvl] = p['fpn_ft%d_3x3_weight' % lvl] * 2
        p['fpn_ft%d_3x3_bias' % lvl] = torch.rand(256, generator=g) * 0.1
    _lnms_params(p, 44)
    cfg = train.TrainConfig()
    cfg.learn_nms, cfg.first_n, cfg.batch_rois_ohem = True, 24, 128
    data = torch.randn(1, 3, H, W, generator=g)
    props = _proposals(N, 43, H, W)[None].copy()
    gt = np.zeros((1, G, 5), np.float32)
    gt[0, :, :4] = props[0, [8, 17, 29, 44]]
    gt[0, :, 4] = [3, 17, 17, 60]
    props[0, n_real:] = 0.0
    tm = M.TrainMetrics(cfg)
    tr = train.FPNTrainer(p, cfg, metrics=tm)
    assert tm.names() == MC.ORDER[3:]
    d = lambda a: torch.as_tensor(a).cuda()
    with torch.no_grad():
        out = tr.forward_backward(data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), d(gt), d(props),
                                  num_proposals=torch.tensor([n_real], dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    assert 'rpn_cls_prob' not in out and 'cls_prob' in out
    got = _check(tm, _tensors(out, rpn=False), images=1)
    label = out['label'].cpu().numpy().reshape(-1)
    assert got['RCNNAcc'][1] == int((label != -1).sum()) <= min(n_real + G, cfg.batch_rois_ohem) and got['RCNNAcc'][1] > 0
    assert (tm.counts.cpu().numpy()[:3] == 0).all()                                    # no RPN slot was touched


def test_speedometer_reads_the_device_accumulator(capsys):
    from relnet_amd import metric as M
    tr, tm, batch, _ = _trainer(61)
    sp = M.Speedometer(batch_size=1, frequent=2)
    lines = []
    with torch.no_grad():
        for n in range(3):
            tr.forward_backward(*batch)
            lines.append(sp(M.BatchEndParam(epoch=0, nbatch=n, eval_metric=tm)))
    assert lines[0] is None and lines[1] is None and lines[2] is not None
    assert capsys.readouterr().out.splitlines() == [lines[2]]
    head, rest = lines[2].split('\tTrain-')
    assert head.startswith('Epoch[0] Batch [2]\tSpeed: ') and head.endswith(' samples/sec')
    fields = rest.split(',\t')
    assert fields[-1] == '' and [f.split('=')[0] for f in fields[:-1]] == MC.ORDER
    vals = dict(f.split('=') for f in fields[:-1])
    assert 0.0 <= float(vals['RPNAcc']) <= 1.0 and float(vals['RPNLogLoss']) > 0
