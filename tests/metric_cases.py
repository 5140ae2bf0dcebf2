"""Shared by the metric tests: tests/golden/metrics.npz (produced by running the reference's core/metric.py, see
tests/golden/gen_golden_metrics.py), the facade-order output list, and the host classes applied to one set of tensors."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metrics.npz')
INPUTS = ('rpn_cls_prob', 'rpn_label', 'rpn_bbox_loss', 'cls_prob', 'rcnn_label', 'bbox_loss', 'nms_multi_target',
          'nms_conditional_score', 'nms_pos_loss', 'nms_neg_loss')
ORDER = ['RPNAcc', 'RPNLogLoss', 'RPNL1Loss', 'RCNNAcc', 'RCNNLogLoss', 'RCNNL1Loss', 'NMSLoss_pos', 'NMSLoss_neg', 'NMSAcc_pos', 'NMSAcc_neg']
INTEGER = ('RPNAcc', 'RCNNAcc', 'NMSAcc_pos', 'NMSAcc_neg')


class RefCfg(object):
    """The three switches the reference's metric classes read (end2end yamls)."""
    class TRAIN(object):
        END2END = True
        ENABLE_OHEM = True
        LEARN_NMS = True


def load():
    z = np.load(GOLDEN)
    cases = {}
    for name in z['cases']:
        name = str(name)
        d = {k: z['%s/%s' % (name, k)] for k in INPUTS}
        names = [str(n) for n in z['%s/metric_names' % name]]
        d['golden'] = {n: (float(s), int(i)) for n, s, i in zip(names, z['%s/sum_metric' % name], z['%s/num_inst' % name])}
        cases[name] = d
    return z, cases


def preds_labels(d, rpn=True, nms=True):
    """(labels, preds) in the order of the train graph's outputs (get_rcnn_names + the four learn-NMS outputs)."""
    preds = ([d['rpn_cls_prob'], d['rpn_bbox_loss']] if rpn else []) + [d['cls_prob'], d['bbox_loss'], d['rcnn_label']]
    if nms:
        preds += [d['nms_multi_target'], d['nms_conditional_score'], d['nms_pos_loss'], d['nms_neg_loss']]
    return [d.get('rpn_label'), None, None], preds


def host_counts(d, rpn=True, nms=True):
    """{name: (sum_metric, num_inst)} of the package's host classes after one update on fresh objects."""
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M

    class Cfg(RefCfg):
        class TRAIN(RefCfg.TRAIN):
            END2END = rpn
    cfg = Cfg()
    labels, preds = preds_labels(d, rpn, nms)
    ms = ([M.RPNAccMetric(), M.RPNLogLossMetric(), M.RPNL1LossMetric()] if rpn else []) + \
        [M.RCNNAccMetric(cfg), M.RCNNLogLossMetric(cfg), M.RCNNL1LossMetric(cfg)]
    if nms:
        ms += [M.NMSLossMetric(cfg, 'pos'), M.NMSLossMetric(cfg, 'neg')]
    out = {}
    for m in ms:
        m.update(labels, preds)
        out[m.name] = (m.sum_metric, m.num_inst)
    if nms:
        a = M.NMSAccMetric(cfg)
        a.update(labels, preds)
        for k, suf in enumerate(('pos', 'neg')):
            out['NMSAcc_' + suf] = (a.sum_metric[k], a.num_inst[k])
    return out


def n_terms(d, name):
    """(number of added terms, at least 2) of a float sum: the `n` of the reordering bounds."""
    if name == 'RPNLogLoss':
        n = int((d['rpn_label'].astype('int32') != -1).sum())
    elif name == 'RCNNLogLoss':
        n = int((d['rcnn_label'].astype('int32') != -1).sum())
    else:
        n = {'RPNL1Loss': 'rpn_bbox_loss', 'RCNNL1Loss': 'bbox_loss', 'NMSLoss_pos': 'nms_pos_loss', 'NMSLoss_neg': 'nms_neg_loss'}[name]
        n = int(np.asarray(d[n]).size)
    return max(n, 2)
