#!/usr/bin/env python
"""Generate tests/golden/metrics.npz by EXECUTING THE REFERENCE'S OWN `relation_rcnn/core/metric.py` and
`lib/utils/lr_scheduler.py`.

Run in the build container only (needs the reference tree; tests read the committed .npz):

    python tests/golden/gen_golden_metrics.py [--ref /root/reference]

Both files are read from where they lie and imported unchanged.  `mxnet` is a few-line in-memory stub installed here
(tests/golden/refshim is not used): `metric.EvalMetric` with name / num_inst / sum_metric / reset, `ndarray.argmax_channel` =
argmax over axis 1 (first maximum -- a stand-in for the MXNet primitive, not a pin), `lr_scheduler.LRScheduler` with base_lr, and
arrays with .asnumpy() / .shape.

The npz holds seeded synthetic inputs and, per case and per metric, `sum_metric` and `num_inst` after ONE `update` call on a
fresh metric (the reference's `sum_metric += float32` accumulates in whatever type numpy promotes to, so accumulation across
updates is not pinned).  For the scheduler: per setting, the `num_update` sequence fed to one scheduler object and, after every
call, its return value and `base_lr`.  Only data goes into the npz.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NUM_CLASSES = 81


class _Arr(object):
    def __init__(self, a):
        self.a = np.asarray(a)

    def asnumpy(self):
        return self.a.copy()

    @property
    def shape(self):
        return self.a.shape


def install_stub():
    mx = types.ModuleType('mxnet')
    mx.metric = types.ModuleType('mxnet.metric')
    mx.ndarray = types.ModuleType('mxnet.ndarray')
    mx.lr_scheduler = types.ModuleType('mxnet.lr_scheduler')

    class EvalMetric(object):
        def __init__(self, name, num=None):
            self.name, self.num = name, num
            self.reset()

        def reset(self):
            self.num_inst, self.sum_metric = 0, 0.0

    class LRScheduler(object):
        def __init__(self, base_lr=0.01):
            self.base_lr = base_lr

    mx.metric.EvalMetric = EvalMetric
    mx.ndarray.argmax_channel = lambda x: _Arr(np.argmax(x.asnumpy(), axis=1).astype(np.float32))
    mx.lr_scheduler.LRScheduler = LRScheduler
    for m in (mx, mx.metric, mx.ndarray, mx.lr_scheduler):
        sys.modules[m.__name__] = m
    return mx


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Cfg(object):
    class TRAIN(object):
        END2END = True
        ENABLE_OHEM = True
        LEARN_NMS = True


# ---- synthetic cases --------------------------------------------------------------------------------------------------
def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return (e / e.sum(axis=axis, keepdims=True)).astype(np.float32)


def random_case(seed, B=2, P=256, R=24, F=10, C=8, T=5):
    r = np.random.RandomState(seed)
    d = {}
    d['rpn_cls_prob'] = _softmax(r.randn(B, 2, P) * 2, 1)
    d['rpn_label'] = r.choice([-1.0, 0.0, 1.0], size=(B, P), p=[0.5, 0.35, 0.15]).astype(np.float32)
    d['rpn_bbox_loss'] = (np.abs(r.randn(B, 36, 4, 5)) * (r.rand(B, 36, 4, 5) < 0.1)).astype(np.float32)
    d['cls_prob'] = _softmax(r.randn(B, R, NUM_CLASSES) * 3, 2)
    lab = r.randint(0, NUM_CLASSES, size=(B, R)).astype(np.float32)
    lab[r.rand(B, R) < 0.4] = -1.0
    hit = r.rand(B, R) < 0.5                       # half of the kept rows: the label is the arg max
    lab[hit & (lab >= 0)] = d['cls_prob'].argmax(2)[hit & (lab >= 0)]
    d['rcnn_label'] = lab
    d['bbox_loss'] = (np.abs(r.randn(B, R, 8)) * (lab[..., None] > 0)).astype(np.float32)
    d['nms_multi_target'] = (r.rand(B, F, C, T) < 0.05).astype(np.float32)
    d['nms_conditional_score'] = r.rand(B, F, C, T).astype(np.float32)
    d['nms_pos_loss'] = (np.abs(r.randn(B, F, C, T)) * d['nms_multi_target']).astype(np.float32)
    d['nms_neg_loss'] = (np.abs(r.randn(B, F, C, T)) * 0.01 * (1 - d['nms_multi_target'])).astype(np.float32)
    return d


def ties_case():
    d = random_case(11)
    p, l = d['rpn_cls_prob'], d['rpn_label']
    p[:, :, :32] = 0.5                              # p0 == p1 exactly, under every label value
    l[0, :32] = np.tile([0.0, 1.0, -1.0, 1.0], 8)
    l[1, :32] = np.tile([1.0, 0.0, 0.0, -1.0], 8)
    c, rl = d['cls_prob'], d['rcnn_label']
    c[0, :12] = 0.0
    # two equal maxima: (label = first of them, label = second, label = neither, ignored)
    for row, (a, b, lab) in enumerate([(3, 40, 3.0), (3, 40, 40.0), (3, 40, 7.0), (3, 40, -1.0), (0, 80, 0.0), (0, 80, 80.0)]):
        c[0, row, a] = c[0, row, b] = 0.4
        c[0, row, 5] = 0.2
        rl[0, row] = lab
    # three equal maxima
    for row, (a, b, e, lab) in enumerate([(10, 20, 30, 10.0), (10, 20, 30, 20.0), (10, 20, 30, 30.0), (0, 1, 2, 1.0), (78, 79, 80, 78.0),
                                          (63, 64, 65, 64.0)], start=6):
        c[0, row, a] = c[0, row, b] = c[0, row, e] = 0.25
        c[0, row, 50] = 0.125
        rl[0, row] = lab
    c[1, 0] = np.float32(1.0 / NUM_CLASSES)         # all 81 equal
    rl[1, 0] = 0.0
    c[1, 1] = np.float32(1.0 / NUM_CLASSES)
    rl[1, 1] = 80.0
    return d


def thresholds_case():
    d = random_case(12)
    t, s = d['nms_multi_target'], d['nms_conditional_score']
    s[0, 0] = 0.5                                   # cond == 0.5 under positive and negative targets
    t[0, 0, :, 0] = 1.0
    t[0, 1] = 0.5                                   # target == 0.5: neither side, whatever cond is
    s[0, 1, :, :2] = 0.9
    s[0, 1, :, 2:] = 0.1
    t[1, 0] = 1.0
    s[1, 0, :, 0] = np.nextafter(np.float32(0.5), np.float32(1.0))
    s[1, 0, :, 1] = np.nextafter(np.float32(0.5), np.float32(0.0))
    return d


def ignored_case():
    d = random_case(13)
    d['rpn_label'][1] = -1.0                        # an image whose labels are all -1
    d['rcnn_label'][1] = -1.0
    d['nms_multi_target'][:] = 0.0                  # no positive target: NMSAcc_pos num_inst == 0
    d['nms_pos_loss'][:] = 0.0
    return d


def all_ignored_case():
    d = random_case(14, B=1)
    d['rpn_label'][:] = -1.0
    d['rcnn_label'][:] = -1.0
    return d


def zeros_case():
    d = random_case(15)
    p, l = d['rpn_cls_prob'], d['rpn_label']
    tiny = np.array([0.0, 1e-20, 1e-14, 1e-10, 5.9e-8, 1.2e-7, 1e-45, 1e-38], np.float32)     # 0, below 1e-14, around float32 epsilon, denormal
    p[0, 0, :8] = tiny; p[0, 1, :8] = 1.0 - tiny; l[0, :8] = 0.0
    p[1, 1, :8] = tiny; p[1, 0, :8] = 1.0 - tiny; l[1, :8] = 1.0
    c, rl = d['cls_prob'], d['rcnn_label']
    for k in range(8):
        c[0, k] = 0.0
        c[0, k, 17] = 1.0 - tiny[k]
        c[0, k, 60] = tiny[k]
        rl[0, k] = 60.0
    return d


CASES = [('random', lambda: random_case(10)), ('ties', ties_case), ('thresholds', thresholds_case), ('ignored', ignored_case),
         ('all_ignored', all_ignored_case), ('zeros', zeros_case)]
INPUTS = ('rpn_cls_prob', 'rpn_label', 'rpn_bbox_loss', 'cls_prob', 'rcnn_label', 'bbox_loss', 'nms_multi_target',
          'nms_conditional_score', 'nms_pos_loss', 'nms_neg_loss')


def run_metrics(M, d):
    """One update of every reference metric on a fresh object -> {name: (sum_metric, num_inst)}."""
    preds = [_Arr(d[k]) for k in ('rpn_cls_prob', 'rpn_bbox_loss', 'cls_prob', 'bbox_loss', 'rcnn_label', 'nms_multi_target',
                                  'nms_conditional_score', 'nms_pos_loss', 'nms_neg_loss')]
    labels = [_Arr(d['rpn_label']), None, None]
    cfg = _Cfg()
    out = {}
    for m in (M.RPNAccMetric(), M.RPNLogLossMetric(), M.RPNL1LossMetric(), M.RCNNAccMetric(cfg), M.RCNNLogLossMetric(cfg),
              M.RCNNL1LossMetric(cfg), M.NMSLossMetric(cfg, 'pos'), M.NMSLossMetric(cfg, 'neg')):
        m.update(labels, preds)
        out[m.name] = (float(m.sum_metric), int(m.num_inst))
    acc = M.NMSAccMetric(cfg)
    acc.update(labels, preds)
    for k, suf in enumerate(('pos', 'neg')):
        out['NMSAcc_' + suf] = (float(acc.sum_metric[k]), int(acc.num_inst[k]))
    return out


# ---- scheduler settings: (name, lr, lr_step, lr_factor, warmup, warmup_lr, warmup_step, begin_epoch, num_images, batch_size, num_updates)
def _dense(n):
    return list(range(n + 1))


SCHEDULES = [
    ('yaml', 0.0005, '5.33', 0.1, False, 0.00005, 1000, 0, 200, 1, _dense(1300)),            # the learn-NMS yaml as shipped
    ('yaml_warmup', 0.0005, '5.33', 0.1, True, 0.00005, 1000, 0, 200, 1, _dense(1300)),
    ('two_steps', 0.01, '4,6', 0.1, False, 0, 0, 0, 100, 2, _dense(400)),
    ('resumed', 0.01, '4,6', 0.1, False, 0, 0, 5, 100, 2, _dense(120)),                       # begin_epoch past the first step
    ('resumed_past_all', 0.01, '4,6', 0.5, False, 0, 0, 6, 100, 2, _dense(20)),               # no step left (the reference's assert: see the test)
    ('jump', 0.02, '1,2', 0.5, False, 0, 0, 0, 100, 1, [0, 1, 50, 250, 251, 10, 300]),        # one call jumps over two steps
    ('warmup_over_step', 0.02, '0.1,0.2', 0.1, True, 0.001, 15, 0, 100, 1, _dense(40)),       # warm-up ends after the first step
]


def schedule_steps(lr, lr_step, lr_factor, begin_epoch, num_images, batch_size):
    """The iteration list and start value a training script hands to the scheduler: epochs after begin_epoch, in iterations.
    A restatement of train_end2end.py:154-159 (inline in train_net, not runnable on its own): NOT reference output, unlike the
    scheduler sequences below."""
    epochs = [float(e) for e in lr_step.split(',')]
    left = [e - begin_epoch for e in epochs if e > begin_epoch]
    return lr * lr_factor ** (len(epochs) - len(left)), [int(e * num_images / batch_size) for e in left]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    ap.add_argument('--out', default=os.path.join(HERE, 'metrics.npz'))
    a = ap.parse_args()
    install_stub()
    M = _load('ref_metric', os.path.join(a.ref, 'relation_rcnn/core/metric.py'))
    S = _load('ref_lr_scheduler', os.path.join(a.ref, 'lib/utils/lr_scheduler.py'))
    z = {'cases': np.array([n for n, _ in CASES]), 'schedules': np.array([s[0] for s in SCHEDULES])}
    for name, make in CASES:
        d = make()
        for k in INPUTS:
            assert d[k].dtype == np.float32
            z['%s/%s' % (name, k)] = d[k]
        res = run_metrics(M, d)
        z['%s/metric_names' % name] = np.array(sorted(res))
        z['%s/sum_metric' % name] = np.array([res[k][0] for k in sorted(res)], np.float64)
        z['%s/num_inst' % name] = np.array([res[k][1] for k in sorted(res)], np.int64)
        print(name, {k: res[k] for k in sorted(res)})
    for name, lr, lr_step, factor, warmup, warmup_lr, warmup_step, begin, n_img, batch, nus in SCHEDULES:
        base, steps = schedule_steps(lr, lr_step, factor, begin, n_img, batch)
        z['sched/%s/config' % name] = np.array([lr, factor, float(warmup), warmup_lr, warmup_step, begin, n_img, batch], np.float64)
        z['sched/%s/lr_step' % name] = np.array(lr_step)
        z['sched/%s/steps' % name] = np.array(steps, np.int64)
        z['sched/%s/start_lr' % name] = np.array(base, np.float64)
        z['sched/%s/num_update' % name] = np.array(nus, np.int64)
        if not steps:                                # the reference class asserts len(step) >= 1
            z['sched/%s/out' % name] = np.zeros(0); z['sched/%s/base_lr' % name] = np.zeros(0)
            continue
        s = S.WarmupMultiFactorScheduler(steps, factor, warmup, warmup_lr, warmup_step)
        s.base_lr = base                             # (what mx.optimizer does with `learning_rate` when a scheduler is given)
        outs, bases = [], []
        for nu in nus:
            outs.append(s(nu)); bases.append(s.base_lr)
        z['sched/%s/out' % name] = np.array(outs, np.float64)
        z['sched/%s/base_lr' % name] = np.array(bases, np.float64)
        print(name, steps, base, sorted(set(outs)))
    np.savez_compressed(a.out, **z)
    print('wrote', a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
