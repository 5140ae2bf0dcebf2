"""Training metrics of the reference (relation_rcnn/core/metric.py, wired in train_end2end.py:128-148, printed by
core/callback.py:Speedometer): RPNAcc, RPNLogLoss, RPNL1Loss, RCNNAcc, RCNNLogLoss, RCNNL1Loss, NMSLoss_pos, NMSLoss_neg,
NMSAcc_pos, NMSAcc_neg.

Two forms of the same definitions:

  * host classes with the reference's names, constructor arguments and update(labels, preds) / get() / reset() protocol, on
    numpy / torch-CPU / facade NDArray values.  `preds` is the output list of the bound train graph in get_rcnn_names order
    ([rpn_cls_prob, rpn_bbox_loss,] cls_prob, bbox_loss, rcnn_label [, nms_multi_target, nms_conditional_score, nms_pos_loss,
    nms_neg_loss]), `labels` the loader's label list (rpn_label first).  Float sums are float64 here (the reference adds
    float32 sums); counts are exact.
  * `TrainMetrics`: the same ten numbers accumulated ON THE DEVICE by the trainers (csrc/metrics.hip), with no host
    synchronisation and inside a captured step; integer counts bit-identical to the host classes, float sums in float64 and
    bitwise reproducible.  `Speedometer` is the only reader: one device-to-host copy of 192 bytes per `frequent` steps.

One image = one executor.  The reference binds one image per executor and calls `update` once per executor, so a step of B
images adds B to the num_inst of NMSLoss_pos / NMSLoss_neg (`self.num_inst += 1` per update) and the sum over the B images of
the loss tensors to their sum_metric.  TrainMetrics does exactly that for a batched step; for every other metric num_inst
counts elements, and the per-image and the batched view coincide.  A host NMSLossMetric fed a batched tensor in ONE update
counts 1, as the reference's class would.
"""
import logging
import time

import numpy as np
import torch

from .mx import metric as _mxm


def get_rpn_names():
    return ['rpn_cls_prob', 'rpn_bbox_loss'], ['rpn_label', 'rpn_bbox_target', 'rpn_bbox_weight']


def get_rcnn_names(cfg):
    pred, label = ['rcnn_cls_prob', 'rcnn_bbox_loss'], ['rcnn_label', 'rcnn_bbox_target', 'rcnn_bbox_weight']
    if cfg.TRAIN.ENABLE_OHEM or cfg.TRAIN.END2END:
        pred.append('rcnn_label')
    if cfg.TRAIN.END2END:
        rpn_pred, rpn_label = get_rpn_names()
        pred, label = rpn_pred + pred, rpn_label
    return pred, label


def _np(x):
    if hasattr(x, 'asnumpy'):
        return x.asnumpy()
    if torch.is_tensor(x):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _acc(pred_label, label):
    """(#correct, #kept) of int predictions against float labels cast like .astype('int32'); -1 = ignore."""
    label = label.astype('int32').reshape(-1)
    keep = label != -1
    return int(np.sum(pred_label.reshape(-1)[keep] == label[keep])), int(keep.sum())


def _log_loss(pred2d, label):
    """pred2d [n, C] float32, label [n]: (float64 sum of -log(float32(p[label] + 1e-14)), #kept)."""
    label = label.astype('int32').reshape(-1)
    keep = np.where(label != -1)[0]
    cls = pred2d[keep, label[keep]].astype(np.float32) + np.float32(1e-14)            # a float32 add, as the reference's `cls += 1e-14`
    return float(np.sum(-np.log(cls.astype(np.float64)))), int(len(keep))


def _sum64(x):
    return float(np.sum(_np(x).astype(np.float64)))


class RPNAccMetric(_mxm.EvalMetric):
    def __init__(self):
        super(RPNAccMetric, self).__init__('RPNAcc')
        self.pred, self.label = get_rpn_names()

    def update(self, labels, preds):
        pred = _np(preds[self.pred.index('rpn_cls_prob')])
        label = _np(labels[self.label.index('rpn_label')])
        # argmax_channel: first maximum over axis 1 (numpy's rule; the MXNet primitive is not in the reference tree)
        s, n = _acc(np.argmax(pred.reshape(pred.shape[0], pred.shape[1], -1), axis=1), label)
        self.sum_metric += s
        self.num_inst += n


class _RCNNMetric(_mxm.EvalMetric):
    def __init__(self, name, cfg):
        super(_RCNNMetric, self).__init__(name)
        self.e2e, self.ohem = cfg.TRAIN.END2END, cfg.TRAIN.ENABLE_OHEM
        self.pred, self.label = get_rcnn_names(cfg)

    def _label(self, labels, preds):
        if self.ohem or self.e2e:
            return _np(preds[self.pred.index('rcnn_label')])
        return _np(labels[self.label.index('rcnn_label')])


class RCNNAccMetric(_RCNNMetric):
    def __init__(self, cfg):
        super(RCNNAccMetric, self).__init__('RCNNAcc', cfg)

    def update(self, labels, preds):
        pred = _np(preds[self.pred.index('rcnn_cls_prob')])
        s, n = _acc(pred.reshape(-1, pred.shape[-1]).argmax(axis=1), self._label(labels, preds))
        self.sum_metric += s
        self.num_inst += n


class RPNLogLossMetric(_mxm.EvalMetric):
    def __init__(self):
        super(RPNLogLossMetric, self).__init__('RPNLogLoss')
        self.pred, self.label = get_rpn_names()

    def update(self, labels, preds):
        pred = _np(preds[self.pred.index('rpn_cls_prob')])
        label = _np(labels[self.label.index('rpn_label')])
        pred = pred.reshape(pred.shape[0], pred.shape[1], -1).transpose(0, 2, 1).reshape(-1, pred.shape[1])      # (b, c, p) -> (b p, c)
        s, n = _log_loss(pred, label)
        self.sum_metric += s
        self.num_inst += n


class RCNNLogLossMetric(_RCNNMetric):
    def __init__(self, cfg):
        super(RCNNLogLossMetric, self).__init__('RCNNLogLoss', cfg)

    def update(self, labels, preds):
        pred = _np(preds[self.pred.index('rcnn_cls_prob')])
        s, n = _log_loss(pred.reshape(-1, pred.shape[-1]), self._label(labels, preds))
        self.sum_metric += s
        self.num_inst += n


class RPNL1LossMetric(_mxm.EvalMetric):
    def __init__(self):
        super(RPNL1LossMetric, self).__init__('RPNL1Loss')
        self.pred, self.label = get_rpn_names()

    def update(self, labels, preds):
        label = _np(labels[self.label.index('rpn_label')])
        self.sum_metric += _sum64(preds[self.pred.index('rpn_bbox_loss')])
        self.num_inst += int(np.sum(label != -1))             # (no int cast here: metric.py:154)


class RCNNL1LossMetric(_RCNNMetric):
    def __init__(self, cfg):
        super(RCNNL1LossMetric, self).__init__('RCNNL1Loss', cfg)

    def update(self, labels, preds):
        self.sum_metric += _sum64(preds[self.pred.index('rcnn_bbox_loss')])
        self.num_inst += int(np.sum(self._label(labels, preds) != -1))


class NMSLossMetric(_mxm.EvalMetric):
    def __init__(self, cfg, name):
        assert cfg.TRAIN.LEARN_NMS, 'config set learn nms to be false'
        assert name in ['pos', 'neg'], 'only for nms_pos/neg_loss'
        super(NMSLossMetric, self).__init__('NMSLoss_' + name)
        self._offset = ['pos', 'neg'].index(name)

    def update(self, labels, preds):
        self.sum_metric += _sum64(preds[-2 + self._offset])
        self.num_inst += 1


class NMSAccMetric(_mxm.EvalMetric):
    def __init__(self, cfg):
        assert cfg.TRAIN.LEARN_NMS, 'config set learn nms to be false'
        self._suffixes = ['pos', 'neg']
        super(NMSAccMetric, self).__init__('NMSAcc')

    def reset(self):
        self.num_inst = [0, 0]
        self.sum_metric = [0.0, 0.0]

    def get(self):
        name = [self.name + '_' + s for s in self._suffixes]
        value = [float('nan') if n == 0 else s / n for s, n in zip(self.sum_metric, self.num_inst)]
        return name, value

    def update(self, labels, preds):
        target, score = _np(preds[-4]), _np(preds[-3])
        for k, side in enumerate((np.greater, np.less)):      # strict: an element equal to 0.5 is on neither side
            mask = side(target, 0.5)
            self.sum_metric[k] += int(np.sum(mask & side(score, 0.5)))
            self.num_inst[k] += int(np.sum(mask))


class NMSAccValidMetric(_mxm.EvalMetric):
    def __init__(self, cfg):
        raise NotImplementedError("NMSAccValidMetric needs TRAIN.INSTANCE_WEIGHT, which no graph of this project builds")


# ---- the device accumulator -------------------------------------------------------------------------------------------------
# slot numbers: include/relnet_hip.h, "Training metrics"
N_COUNTS, N_SUMS = 16, 8
C_RPN_CORRECT, C_RPN_INST, C_RPN_L1_INST, C_RCNN_CORRECT, C_RCNN_INST, C_RCNN_L1_INST, C_NMS_IMAGES = 0, 1, 2, 3, 4, 5, 6
C_NMS_ACC = 7            # .. 10: pos true, pos inst, neg true, neg inst
S_RPN_LOG, S_RPN_L1, S_RCNN_LOG, S_RCNN_L1, S_NMS_POS, S_NMS_NEG = 0, 1, 2, 3, 4, 5

RPN_NAMES = ['RPNAcc', 'RPNLogLoss', 'RPNL1Loss']
RCNN_NAMES = ['RCNNAcc', 'RCNNLogLoss', 'RCNNL1Loss']
NMS_NAMES = ['NMSLoss_pos', 'NMSLoss_neg', 'NMSAcc_pos', 'NMSAcc_neg']
# name -> (sum slot, is the sum an integer count, num_inst slot)
_SLOTS = {'RPNAcc': (C_RPN_CORRECT, True, C_RPN_INST), 'RPNLogLoss': (S_RPN_LOG, False, C_RPN_INST), 'RPNL1Loss': (S_RPN_L1, False, C_RPN_L1_INST),
          'RCNNAcc': (C_RCNN_CORRECT, True, C_RCNN_INST), 'RCNNLogLoss': (S_RCNN_LOG, False, C_RCNN_INST),
          'RCNNL1Loss': (S_RCNN_L1, False, C_RCNN_L1_INST), 'NMSLoss_pos': (S_NMS_POS, False, C_NMS_IMAGES),
          'NMSLoss_neg': (S_NMS_NEG, False, C_NMS_IMAGES), 'NMSAcc_pos': (C_NMS_ACC, True, C_NMS_ACC + 1),
          'NMSAcc_neg': (C_NMS_ACC + 2, True, C_NMS_ACC + 3)}


class TrainMetrics(object):
    """The device accumulator of one trainer: `Trainer(params, cfg, metrics=TrainMetrics(cfg))`.

    cfg: the trainer's TrainConfig.  The RPN metrics exist only with an RPN in the graph (rpn: default = not cfg.fpn, the FPN
    graphs take proposals as an input), the NMS metrics only with cfg.learn_nms; `names()` lists them in the order train_end2end.py:133-145
    registers them.  One deliberate difference from the reference: it registers the RPN metrics only when JOINT_TRAINING or not LEARN_NMS
    (train_end2end.py:134), so its learn-NMS-only experiment logs 7 names; here that experiment reports all 10, like the joint one (its
    step runs the same RPN forward, and whether the fixed RPN still fits the data is worth seeing).
    NMSLoss_pos / _neg: num_inst counts images and sum_metric sums the loss tensors over them (module docstring, "one image =
    one executor").

    The accumulator is ONE buffer of 16 int64 counts and 8 float64 sums; the step's kernels add into it (RPN slots on the
    trainer's side stream, the others on the main stream, each branch with its own fold workspace), `get` / `get_counts` read it
    with one device-to-host copy, `reset` zeroes it on the current stream.  Eager steps count like replays, including the warm-up step
    a CapturedStep runs when the trainer has not stepped yet: call reset() after building one."""

    def __init__(self, cfg, device='cuda', rpn=None):
        self.device = device
        self.has_rpn = (not getattr(cfg, 'fpn', False)) if rpn is None else bool(rpn)
        self.has_nms = bool(getattr(cfg, 'learn_nms', False))
        self.acc = torch.zeros(N_COUNTS + N_SUMS, device=device, dtype=torch.int64)
        self.counts = self.acc[:N_COUNTS]
        self.sums = self.acc[N_COUNTS:].view(torch.float64)
        self._ws = {}
        if torch.device(device).type == 'cuda':     # made here, never inside a capture
            from . import ops
            self._ws = {'rpn': ops.metric_workspace(device), 'main': ops.metric_workspace(device)}

    def names(self):
        return (RPN_NAMES if self.has_rpn else []) + RCNN_NAMES + (NMS_NAMES if self.has_nms else [])

    def reset(self):
        self.acc.zero_()

    # ---- the trainers' launches (current stream) ----
    def add_rpn(self, rpn_cls_prob, rpn_label, rpn_bbox_loss):
        """rpn_cls_prob [B, 2, A h w], rpn_label [B, A h w] float, rpn_bbox_loss: the smooth-L1 loss tensor."""
        from . import ops
        ops.metric_softmax(rpn_cls_prob, rpn_label, self.counts, self.sums, C_RPN_CORRECT, C_RPN_INST, S_RPN_LOG, self._ws['rpn'])
        ops.metric_sum_count(rpn_bbox_loss, self.counts, self.sums, S_RPN_L1, self._ws['rpn'], label=rpn_label, count_slot=C_RPN_L1_INST)

    def add_rcnn(self, cls_prob, label, bbox_loss):
        """cls_prob [B R, 81], label [B R] (the OHEM labels), bbox_loss: the smooth-L1 loss tensor."""
        from . import ops
        ops.metric_softmax(cls_prob, label, self.counts, self.sums, C_RCNN_CORRECT, C_RCNN_INST, S_RCNN_LOG, self._ws['main'])
        ops.metric_sum_count(bbox_loss, self.counts, self.sums, S_RCNN_L1, self._ws['main'], label=label, count_slot=C_RCNN_L1_INST)

    def add_nms(self, nms_multi_target, nms_conditional_score, nms_pos_loss, nms_neg_loss, images):
        from . import ops
        ops.metric_sum_count(nms_pos_loss, self.counts, self.sums, S_NMS_POS, self._ws['main'], count_slot=C_NMS_IMAGES, inst_inc=images,
                             x2=nms_neg_loss, sum2_slot=S_NMS_NEG)
        ops.metric_nms_acc(nms_multi_target, nms_conditional_score, self.counts, C_NMS_ACC)

    # ---- reading ----
    def _read(self, reduce=False):
        """-> (counts int64 [16], sums float64 [8]) on the host.  reduce: SUM over the ranks of an initialised process group first
        (int64 and float64 sums of a COPY: exact, and the local accumulator keeps counting its own rank).  Tested over gloo on host
        copies (tests/test_dist_metrics.py); the nccl branch -- the same two all_reduce calls on views of a device clone -- has not run
        in any test (the GPU tests are single-process)."""
        import torch.distributed as dist
        if reduce and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            a = self.acc.clone() if dist.get_backend() == 'nccl' else self.acc.cpu().clone()
            c, s = a[:N_COUNTS], a[N_COUNTS:].view(torch.float64)
            dist.all_reduce(c, op=dist.ReduceOp.SUM)
            dist.all_reduce(s, op=dist.ReduceOp.SUM)
            a = a.cpu()
        else:
            a = self.acc.cpu()                      # the one device-to-host copy
        a = a.numpy()
        return a[:N_COUNTS].copy(), a[N_COUNTS:].view(np.float64).copy()

    def get_counts(self, reduce=False):
        """-> [(sum_metric, num_inst)] in names() order: Python ints for counts, floats for the float64 sums."""
        c, s = self._read(reduce)
        out = []
        for n in self.names():
            slot, is_int, inst = _SLOTS[n]
            out.append((int(c[slot]) if is_int else float(s[slot]), int(c[inst])))
        return out

    def get(self, reduce=False):
        """-> (names, values): sum_metric / num_inst, nan where num_inst == 0 (metric.py:225-226, mx.metric.EvalMetric.get)."""
        return self.names(), [float('nan') if n == 0 else s / n for s, n in self.get_counts(reduce)]

    def get_name_value(self):
        return list(zip(*self.get()))


class BatchEndParam(object):
    """What a batch-end callback receives (mx.model.BatchEndParam): epoch, nbatch, eval_metric."""

    def __init__(self, epoch, nbatch, eval_metric, locals=None):
        self.epoch, self.nbatch, self.eval_metric, self.locals = epoch, nbatch, eval_metric, locals


class Speedometer(object):
    """core/callback.py:Speedometer: called after every batch with a BatchEndParam; the first call starts the clock, then every
    `frequent`-th batch logs and prints

        Epoch[e] Batch [n]\\tSpeed: x samples/sec\\tTrain-RPNAcc=0.9,\\tRPNLogLoss=0.1,\\t...

    and returns that line (None otherwise).  `param.eval_metric` is a TrainMetrics or any metric with get(): this is the only
    place the device accumulator is read."""

    def __init__(self, batch_size, frequent=50):
        self.batch_size, self.frequent = batch_size, frequent
        self.init, self.tic, self.last_count = False, 0, 0

    def __call__(self, param):
        count = param.nbatch
        if self.last_count > count:
            self.init = False
        self.last_count = count
        if not self.init:
            self.init, self.tic = True, time.time()
            return None
        if count % self.frequent != 0:
            return None
        speed = self.frequent * self.batch_size / (time.time() - self.tic)
        if param.eval_metric is not None:
            name, value = param.eval_metric.get()
            s = "Epoch[%d] Batch [%d]\tSpeed: %.2f samples/sec\tTrain-" % (param.epoch, count, speed)
            for n, v in zip(name, value):
                s += "%s=%f,\t" % (n, v)
        else:
            s = "Iter[%d] Batch [%d]\tSpeed: %.2f samples/sec" % (param.epoch, count, speed)
        logging.info(s)
        print(s)
        self.tic = time.time()
        return s
