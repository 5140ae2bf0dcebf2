"""csrc/metrics.hip through the C-ABI against metric.py's host classes (which tests/test_metric_host.py pins to the reference).

Every integer slot must be bit-identical to the host class.  Every double slot must be within n * 2^-52 * sum|x| of the host
class's float64 value: reordering n double additions moves a sum by at most (n - 1) * 2^-53 * sum|x|, plus one ulp per term for
each of the two `log` implementations (numpy's and the device library's double log are both documented at <= 1 ulp).  The same
call into a fresh accumulator must give the same BITS; two calls into one accumulator exactly twice the counts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metric_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

_, CASES = MC.load()


def _large_case(seed):
    """RPN at 38 x 63 x 9 anchors x 2 images, head at 2 x 309 rois, learn-NMS at [2, 100, 80, 5]; ties, exact 0 / 0.5 values
    and a fully ignored tail are planted in it."""
    r = np.random.RandomState(seed)
    B, P, R = 2, 38 * 63 * 9, 309
    sm = lambda x, ax: (lambda e: (e / e.sum(axis=ax, keepdims=True)).astype(np.float32))(np.exp(x - x.max(axis=ax, keepdims=True)))
    d = {}
    d['rpn_cls_prob'] = sm(r.randn(B, 2, P) * 3, 1)
    d['rpn_label'] = r.choice([-1.0, 0.0, 1.0], size=(B, P), p=[0.9, 0.07, 0.03]).astype(np.float32)
    d['rpn_cls_prob'][:, :, 100:164] = 0.5
    d['rpn_label'][:, 100:164] = np.tile([0.0, 1.0], 32)
    d['rpn_cls_prob'][0, 0, 200:204] = [0.0, 1e-20, 1e-10, 1.0]
    d['rpn_label'][0, 200:204] = 0.0
    d['rpn_label'][1, P // 2:] = -1.0
    d['rpn_bbox_loss'] = (np.abs(r.randn(B, 38, 63, 36)) * (r.rand(B, 38, 63, 36) < 0.02)).astype(np.float32)
    d['cls_prob'] = sm(r.randn(B, R, 81) * 3, 2)
    lab = r.randint(0, 81, size=(B, R)).astype(np.float32)
    hit = r.rand(B, R) < 0.5
    lab[hit] = d['cls_prob'].argmax(2)[hit]
    lab[r.rand(B, R) < 0.55] = -1.0
    d['cls_prob'][0, 5] = 0.0; d['cls_prob'][0, 5, [7, 70]] = 0.5; lab[0, 5] = 70.0          # a tie that contains the label, second place
    d['cls_prob'][0, 6] = 0.0; d['cls_prob'][0, 6, [7, 70, 80]] = 1.0 / 3; lab[0, 6] = 7.0   # ... first place
    d['rcnn_label'] = lab
    d['bbox_loss'] = (np.abs(r.randn(B, R, 8)) * (lab[..., None] > 0)).astype(np.float32)
    d['nms_multi_target'] = (r.rand(B, 100, 80, 5) < 0.01).astype(np.float32)
    d['nms_conditional_score'] = r.rand(B, 100, 80, 5).astype(np.float32)
    d['nms_conditional_score'][0, :3] = 0.5
    d['nms_multi_target'][1, :2] = 0.5
    d['nms_pos_loss'] = (np.abs(r.randn(B, 100, 80, 5)) * d['nms_multi_target']).astype(np.float32)
    d['nms_neg_loss'] = (np.abs(r.randn(B, 100, 80, 5)) * 0.01).astype(np.float32)
    return d


def _odd_case():
    """Shapes that take the scalar kernels: inner not a multiple of 4, element counts with a tail, unaligned views."""
    d = {k: v.copy() for k, v in CASES['random'].items() if k != 'golden'}
    d['rpn_cls_prob'] = np.ascontiguousarray(d['rpn_cls_prob'][:, :, :253])
    d['rpn_label'] = np.ascontiguousarray(d['rpn_label'][:, :253])
    d['rpn_bbox_loss'] = np.ascontiguousarray(d['rpn_bbox_loss'].reshape(2, -1)[:, :717])
    for k in ('nms_multi_target', 'nms_conditional_score', 'nms_pos_loss', 'nms_neg_loss'):
        d[k] = np.ascontiguousarray(d[k].reshape(2, -1)[:, :399])
    return d


def _device_run(d, tm=None, images=None, offset=0):
    """The three trainer-side calls on one set of tensors -> the TrainMetrics.  offset: elements by which every device tensor is
    shifted off its 16-byte alignment."""
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M
    import types
    tm = tm or M.TrainMetrics(types.SimpleNamespace(learn_nms=True), device='cuda')

    def dev(a):
        flat = torch.zeros(a.size + offset, device='cuda', dtype=torch.float32)
        flat[offset:] = torch.as_tensor(a).reshape(-1).cuda()
        return flat[offset:].view(a.shape)
    t = {k: dev(d[k]) for k in MC.INPUTS}
    tm.add_rpn(t['rpn_cls_prob'].view(t['rpn_cls_prob'].shape[0], 2, -1), t['rpn_label'], t['rpn_bbox_loss'])
    tm.add_rcnn(t['cls_prob'].view(-1, t['cls_prob'].shape[-1]), t['rcnn_label'].view(-1), t['bbox_loss'])
    tm.add_nms(t['nms_multi_target'], t['nms_conditional_score'], t['nms_pos_loss'], t['nms_neg_loss'],
               d['nms_pos_loss'].shape[0] if images is None else images)
    return tm


def _check(d, tm, label, times=1, images=None):
    host = MC.host_counts(d)
    images = d['nms_pos_loss'].shape[0] if images is None else images
    got = dict(zip(tm.names(), tm.get_counts()))
    for name in MC.ORDER:
        (s, n), (hs, hn) = got[name], host[name]
        if name.startswith('NMSLoss'):
            hn = images                    # one image = one executor: the device counts images, a host update counts 1
        assert n == times * hn and isinstance(n, int), (label, name, n, hn)
        if name in MC.INTEGER:
            assert s == times * hs and isinstance(s, int), (label, name, s, hs)
        else:
            terms = MC.n_terms(d, name)
            tol = terms * 2.0 ** -52 * abs(hs)
            print('%s/%s: device %.17g host %.17g diff %.3g tol %.3g (n %d)' % (label, name, s, hs, abs(s - times * hs), times * tol, terms))
            assert abs(s - times * hs) <= times * tol, (label, name, s, hs, tol)


@pytest.mark.parametrize('case', sorted(CASES))
def test_kernels_match_the_host_classes_on_the_golden_inputs(case):
    d = CASES[case]
    tm = _device_run(d)
    _check(d, tm, case)
    again = _device_run(d)
    assert torch.equal(tm.acc, again.acc)                                 # the same bits into a fresh accumulator


@pytest.mark.parametrize('offset', [0, 1])
def test_kernels_match_the_host_classes_on_step_sized_inputs(offset):
    d = _large_case(5)
    tm = _device_run(d, offset=offset)
    _check(d, tm, 'large+%d' % offset)
    again = _device_run(d, offset=offset)
    assert torch.equal(tm.acc, again.acc)
    if offset == 0:                          # a second time into the same accumulator
        _device_run(d, tm)
        _check(d, tm, 'large twice', times=2)
        c1, c2 = again.acc[:16].cpu().numpy(), tm.acc[:16].cpu().numpy()
        assert (c2 == 2 * c1).all()


def _rpn_case(B, inner, seed):
    r = np.random.RandomState(seed)
    x = r.randn(B, 2, inner) * 3
    e = np.exp(x - x.max(axis=1, keepdims=True))
    prob = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    label = r.choice([-1.0, 0.0, 1.0], size=(B, inner), p=[0.9, 0.07, 0.03]).astype(np.float32)
    prob[:, :, 10:74] = 0.5                                  # exact ties under every label value
    label[:, 10:74] = np.tile([0.0, 1.0, -1.0, 1.0], 16)
    prob[0, 0, 80:84] = [0.0, 1e-20, 1e-10, 1.0]
    label[0, 80:84] = 0.0
    label[:, inner - 5:] = np.array([1.0, 0.0, -1.0, 1.0, 0.0], np.float32)        # the last positions of every image are kept ones
    label[B - 1, inner // 2:inner - 5] = -1.0
    loss = (np.abs(r.randn(B, inner, 4)) * (label[..., None] == 1)).astype(np.float32)
    return {'rpn_cls_prob': prob, 'rpn_label': label, 'rpn_bbox_loss': loss}


# which instantiation of metric_softmax_inner_kernel a shape takes is decided by relnet_metric_softmax from `inner` alone (operands from
# the allocator are 16-byte aligned): inner % 4 == 0 -> 16-byte loads, inner % 2 == 0 -> 8-byte loads, otherwise scalar.  All of these
# shapes run on more than one workgroup (grid-stride loop + the cross-workgroup fold).
@pytest.mark.parametrize('B,inner,loads', [(2, 40 * 64 * 9, 16), (8, 38 * 63 * 12, 16), (2, 38 * 63 * 9, 8), (8, 38 * 63 * 9, 8),
                                           (2, 37 * 63 * 9, 4), (1, 50 * 84 * 12, 16)])
def test_rpn_kernel_on_every_load_width_and_many_workgroups(B, inner, loads):
    import types
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M
    assert {16: inner % 4 == 0, 8: inner % 4 == 2, 4: inner % 2 == 1}[loads] and B * inner // (loads // 4) > 4 * 256
    d = _rpn_case(B, inner, 11 + B)
    labels, preds = [d['rpn_label']], [d['rpn_cls_prob'], d['rpn_bbox_loss']]
    host = {}
    for m in (M.RPNAccMetric(), M.RPNLogLossMetric(), M.RPNL1LossMetric()):
        m.update(labels, preds)
        host[m.name] = (m.sum_metric, m.num_inst)
    accs = []
    for _ in range(2):
        tm = M.TrainMetrics(types.SimpleNamespace(learn_nms=False), device='cuda')
        t = {k: torch.as_tensor(v).cuda() for k, v in d.items()}
        tm.add_rpn(t['rpn_cls_prob'], t['rpn_label'], t['rpn_bbox_loss'])
        accs.append(tm.acc.clone())
    assert torch.equal(accs[0], accs[1])                                  # bitwise equal to itself
    got = dict(zip(tm.names(), tm.get_counts()))
    kept = int((d['rpn_label'].astype('int32') != -1).sum())
    assert got['RPNAcc'] == host['RPNAcc'] and got['RPNAcc'][1] == kept > 0
    for name, terms in (('RPNLogLoss', kept), ('RPNL1Loss', d['rpn_bbox_loss'].size)):
        (s, n), (hs, hn) = got[name], host[name]
        tol = terms * 2.0 ** -52 * abs(hs)
        print('%dx%d %s: device %.17g host %.17g diff %.3g tol %.3g' % (B, inner, name, s, hs, abs(s - hs), tol))
        assert n == hn and abs(s - hs) <= tol, (name, s, hs, tol)


def test_scalar_paths_and_tails():
    d = _odd_case()
    for offset in (0, 3):
        tm = _device_run(d, offset=offset)
        _check(d, tm, 'odd+%d' % offset)
        assert torch.equal(tm.acc, _device_run(d, offset=offset).acc)


def test_all_ignored_input_leaves_the_slots_untouched():
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M
    d = CASES['all_ignored']
    tm = _device_run(d)
    c = tm.counts.cpu().numpy()
    assert c[M.C_RPN_CORRECT] == c[M.C_RPN_INST] == c[M.C_RPN_L1_INST] == c[M.C_RCNN_CORRECT] == c[M.C_RCNN_INST] == c[M.C_RCNN_L1_INST] == 0
    s = tm.sums.cpu().numpy()
    assert s[M.S_RPN_LOG].tobytes() == s[M.S_RCNN_LOG].tobytes() == np.float64(0.0).tobytes()
    got = dict(zip(*tm.get()))
    for n in ('RPNAcc', 'RPNLogLoss', 'RPNL1Loss', 'RCNNAcc', 'RCNNLogLoss', 'RCNNL1Loss'):
        assert np.isnan(got[n]), n
    assert not np.isnan(got['NMSLoss_pos'])
    # no positive target: NMSAcc_pos has no instance
    got = dict(zip(*_device_run(CASES['ignored']).get()))
    assert np.isnan(got['NMSAcc_pos']) and got['NMSAcc_neg'] == 404.0 / 800
    tm.reset()
    assert int(tm.acc.abs().sum()) == 0


def test_entries_refuse_bad_operands():
    import relnet_amd  # noqa: F401
    from relnet_amd import lib, metric as M, ops
    import types
    tm = M.TrainMetrics(types.SimpleNamespace(learn_nms=True), device='cuda')
    x = torch.zeros(8, device='cuda')
    with pytest.raises(lib.RelnetError, match='null operand'):
        lib.call('relnet_metric_softmax', x.data_ptr(), 0, 4, 2, 1, tm.counts.data_ptr(), tm.counts.data_ptr() + 8, tm.sums.data_ptr(),
                 tm._ws['main'].data_ptr(), ops._stream())
    with pytest.raises(lib.RelnetError, match='8-byte aligned'):
        lib.call('relnet_metric_nms_acc', x.data_ptr(), x.data_ptr(), 8, tm.counts.data_ptr() + 4, ops._stream())
    with pytest.raises(lib.RelnetError, match='count slot'):
        lib.call('relnet_metric_sum_count', x.data_ptr(), 0, 8, 0, 0, 2, tm.sums.data_ptr(), 0, 0, tm._ws['main'].data_ptr(), ops._stream())
    with pytest.raises(ValueError, match='label has'):
        ops.metric_softmax(torch.zeros(4, 2, device='cuda'), torch.zeros(3, device='cuda'), tm.counts, tm.sums, 0, 1, 0, tm._ws['main'])
    torch.cuda.synchronize()
    assert int(tm.acc.abs().sum()) == 0 and int(tm._ws['main'].abs().sum()) == 0
