"""metric.py's host classes and lr_scheduler.py against tests/golden/metrics.npz, which was produced by running the
reference's own relation_rcnn/core/metric.py and lib/utils/lr_scheduler.py (tests/golden/gen_golden_metrics.py).

Integer-valued quantities (Acc sums, every num_inst, the NMSAcc counts) must be EQUAL.  Float sums: the reference adds float32
terms in float32, the host classes in float64; any summation order of n non-negative float32 terms is within n * 2^-24 * sum|x|
of the exact sum (n >= 2), and that -- derived, not tuned -- is the tolerance.  Scheduler outputs must be equal (==)."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metric_cases as MC  # noqa: E402

Z, CASES = MC.load()


def test_golden_has_the_cases_the_definitions_hinge_on():
    t = CASES['ties']
    assert (t['rpn_cls_prob'][:, 0, :32] == t['rpn_cls_prob'][:, 1, :32]).all()               # p0 == p1
    row = t['cls_prob'][0, 0]
    assert (row == row.max()).sum() == 2 and (t['cls_prob'][0, 6] == t['cls_prob'][0, 6].max()).sum() == 3
    assert int(t['rcnn_label'][0, 0]) == int(np.argmax(row)) and int(t['rcnn_label'][0, 1]) != int(np.argmax(t['cls_prob'][0, 1]))
    th = CASES['thresholds']
    assert (th['nms_conditional_score'] == 0.5).any() and (th['nms_multi_target'] == 0.5).any()
    ig = CASES['ignored']
    assert (ig['rpn_label'][1] == -1).all() and ig['golden']['NMSAcc_pos'][1] == 0
    assert CASES['all_ignored']['golden']['RPNAcc'][1] == 0 and CASES['all_ignored']['golden']['RCNNLogLoss'][1] == 0
    zc = CASES['zeros']
    assert zc['rpn_cls_prob'][0, 0, 0] == 0.0 and 0 < zc['rpn_cls_prob'][0, 0, 1] < 1e-14 and zc['rpn_label'][0, 0] == 0


@pytest.mark.parametrize('case', sorted(CASES))
def test_host_classes_match_the_reference(case):
    d = CASES[case]
    got = MC.host_counts(d)
    assert sorted(got) == sorted(d['golden']) == sorted(MC.ORDER)
    for name in MC.ORDER:
        (s, n), (rs, rn) = got[name], d['golden'][name]
        assert n == rn and isinstance(n, int), (name, n, rn)
        if name in MC.INTEGER:
            assert s == rs, (name, s, rs)
        else:
            assert isinstance(s, float)
            terms = MC.n_terms(d, name)
            tol = terms * 2.0 ** -24 * abs(s)               # (terms are non-negative: sum|x| = the sum)
            print('%s/%s: host %.17g reference %.9g diff %.3g tol %.3g (n %d)' % (case, name, s, rs, abs(s - rs), tol, terms))
            assert abs(s - rs) <= tol, (name, s, rs, tol)


def test_get_is_nan_without_instances_and_reset_clears():
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M
    d = CASES['ignored']
    labels, preds = MC.preds_labels(d)
    a = M.NMSAccMetric(MC.RefCfg())
    a.update(labels, preds)
    names, values = a.get()
    assert names == ['NMSAcc_pos', 'NMSAcc_neg'] and np.isnan(values[0]) and values[1] == 404.0 / 800
    a.reset()
    assert a.num_inst == [0, 0] and a.sum_metric == [0.0, 0.0] and all(np.isnan(v) for v in a.get()[1])
    m = M.RPNAccMetric()
    assert np.isnan(m.get()[1])
    m.update(*MC.preds_labels(CASES['all_ignored']))
    assert m.num_inst == 0 and np.isnan(m.get()[1])
    m.update(labels, preds); m.update(labels, preds)
    assert (m.sum_metric, m.num_inst) == (120, 270) and m.get() == ('RPNAcc', 120 / 270)
    with pytest.raises(NotImplementedError, match='INSTANCE_WEIGHT'):
        M.NMSAccValidMetric(MC.RefCfg())
    with pytest.raises(AssertionError):
        M.NMSLossMetric(MC.RefCfg(), 'both')


def test_host_classes_take_torch_and_facade_arrays():
    import torch
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M, mx
    d = CASES['random']
    labels, preds = MC.preds_labels(d)
    for wrap in (torch.as_tensor, lambda a: mx.nd.array(a)):
        m = M.RCNNLogLossMetric(MC.RefCfg())
        m.update([None if l is None else wrap(l) for l in labels], [wrap(p) for p in preds])
        assert (m.sum_metric, m.num_inst) == MC.host_counts(d)['RCNNLogLoss']


def test_train_metrics_names_follow_the_configuration():
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M
    cfg = types.SimpleNamespace(learn_nms=True, fpn=False)
    tm = M.TrainMetrics(cfg, device='cpu')
    assert tm.names() == MC.ORDER                                  # train_end2end.py:133-145
    assert M.TrainMetrics(types.SimpleNamespace(learn_nms=False), device='cpu').names() == MC.ORDER[:6]
    assert M.TrainMetrics(types.SimpleNamespace(learn_nms=True, fpn=True), device='cpu').names() == MC.ORDER[3:]
    names, values = tm.get()
    assert names == MC.ORDER and all(np.isnan(v) for v in values)
    tm.counts[M.C_RCNN_CORRECT], tm.counts[M.C_RCNN_INST], tm.sums[M.S_NMS_POS], tm.counts[M.C_NMS_IMAGES] = 3, 4, 1.5, 2
    got = dict(zip(*tm.get()))
    assert got['RCNNAcc'] == 0.75 and got['NMSLoss_pos'] == 0.75 and got['NMSLoss_neg'] == 0.0 and np.isnan(got['RPNAcc'])
    assert tm.get_counts()[3] == (3, 4) and isinstance(tm.get_counts()[3][0], int)
    tm.reset()
    assert all(np.isnan(v) for v in tm.get()[1])


def test_speedometer_prints_the_reference_line(capsys):
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M
    tm = M.TrainMetrics(types.SimpleNamespace(learn_nms=False), device='cpu')
    tm.counts[M.C_RPN_CORRECT], tm.counts[M.C_RPN_INST] = 1, 4
    sp = M.Speedometer(batch_size=8, frequent=2)
    lines = [sp(M.BatchEndParam(epoch=3, nbatch=n, eval_metric=tm)) for n in range(5)]
    assert [l is not None for l in lines] == [False, False, True, False, True]
    out = capsys.readouterr().out.splitlines()
    assert out == [lines[2], lines[4]]
    head, rest = lines[2].split('\tTrain-')
    assert head.startswith('Epoch[3] Batch [2]\tSpeed: ') and head.endswith(' samples/sec')
    assert rest == 'RPNAcc=0.250000,\tRPNLogLoss=0.000000,\tRPNL1Loss=nan,\tRCNNAcc=nan,\tRCNNLogLoss=nan,\tRCNNL1Loss=nan,\t'
    assert M.Speedometer(1, 1)(M.BatchEndParam(0, 0, None)) is None


# ---- the schedule ------------------------------------------------------------------------------------------------------------
def _train_cfg(name):
    lr, factor, warmup, warmup_lr, warmup_step, begin, n_img, batch = Z['sched/%s/config' % name]
    t = types.SimpleNamespace(lr=float(lr), lr_step=str(Z['sched/%s/lr_step' % name]), lr_factor=float(factor), warmup=bool(warmup),
                              warmup_lr=float(warmup_lr), warmup_step=int(warmup_step), begin_epoch=int(begin))
    return t, int(n_img), int(batch)


@pytest.mark.parametrize('name', [str(n) for n in Z['schedules']])
def test_scheduler_equals_the_reference(name):
    """WarmupMultiFactorScheduler: every output and every base_lr equal to what the reference's own class returned for the same
    num_update sequence.  schedule_from_config is NOT pinned that way: train_end2end.py:154-159 sits inside train_net and cannot be run
    on its own, so the npz's `steps` / `start_lr` come from the generator's restatement of those lines -- the comparison here is
    between two restatements and guards against drift, no more."""
    import relnet_amd  # noqa: F401
    from relnet_amd import lr_scheduler as L
    t, n_img, batch = _train_cfg(name)
    start, steps = L.schedule_from_config(t, n_img, batch)
    assert steps == Z['sched/%s/steps' % name].tolist() and start == float(Z['sched/%s/start_lr' % name])
    if not steps:                       # nothing left after begin_epoch: the reference's class asserts on an empty list
        with pytest.raises(AssertionError):
            L.from_config(t, n_img, batch)
        return
    s = L.from_config(t, n_img, batch, begin_epoch=t.begin_epoch)
    assert s.base_lr == start
    outs, bases = Z['sched/%s/out' % name], Z['sched/%s/base_lr' % name]
    for k, nu in enumerate(Z['sched/%s/num_update' % name].tolist()):
        got = s(nu)
        assert got == outs[k] and s.base_lr == bases[k], (name, nu, got, outs[k])
    assert len(set(outs.tolist())) >= 2


def test_scheduler_settings_cover_the_yaml_and_the_edges():
    t, n_img, batch = _train_cfg('yaml_warmup')
    assert (t.lr, t.lr_step, t.warmup_lr, t.warmup_step, t.warmup) == (0.0005, '5.33', 0.00005, 1000, True)
    assert not _train_cfg('yaml')[0].warmup
    assert len(Z['sched/two_steps/steps']) == 2 and _train_cfg('resumed')[0].begin_epoch == 5
    nu, base = Z['sched/jump/num_update'].tolist(), Z['sched/jump/base_lr'].tolist()
    k = nu.index(250)
    assert base[k] == base[k - 1] * 0.25                      # two steps passed in one call


def test_scheduler_refuses_what_the_reference_refuses():
    import relnet_amd  # noqa: F401
    from relnet_amd.lr_scheduler import WarmupMultiFactorScheduler as S
    with pytest.raises(ValueError, match='increasing'):
        S([10, 10])
    with pytest.raises(ValueError, match='greater or equal than 1'):
        S([0, 5])
    with pytest.raises(ValueError, match='no more than 1'):
        S([5], factor=1.5)
    with pytest.raises(AssertionError):
        S([])
    with pytest.raises(AssertionError):
        S((5, 6))
    s = S([5], 0.1)
    assert s.base_lr == 0.01 and s(5) == 0.01 and s(6) == 0.01 * 0.1 and s.count == 5 and s.cur_step_ind == 1
