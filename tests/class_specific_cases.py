"""Inputs and host restatements for class-specific box regression (CLASS_AGNOSTIC false), shared by
tests/golden/gen_golden_class_specific.py, the host tests and the GPU tests.

The inputs are the generators of tests/golden/cases.py with ONE change: bbox_pred is [n, 4 * (c + 1)] (one box per class,
background included) instead of [n, 8]; the wider deltas are seeded here.  The expected outputs of the reference's own
Python on these inputs are in tests/golden/class_specific.npz.
"""
import numpy as np

import cases

F32 = np.float32

#: learn-NMS operator cases: name -> (n_rois, num_fg_classes, first_n, seed, (means, stds) or None)
LNMS_CASES = {
    'cs_n60_c6_f20': (60, 6, 20, 21, None),                                              # the test graph passes None
    'cs_n60_c6_f20_norm': (60, 6, 20, 21, ((0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2))),  # the training graph's means / stds
    'cs_n120_c80_f30': (120, 80, 30, 24, None),                                          # more than 64 foreground classes
}

#: post-processing case: (n_rois, num_classes incl. background, seed)
POST_CASE = (150, 5, 33)
#: regression-target case of cases.targets_case: (n_rois, n_gt, seed, num_fg)
TARGETS_CASE = (90, 7, 61, 4)


def wide_deltas(n, num_classes, seed, sigma):
    """bbox_pred [n, 4 * num_classes] fp32."""
    return np.random.default_rng(seed + 7000).normal(0, sigma, (n, 4 * num_classes)).astype(F32)


def lnms_case(n, num_fg, seed):
    """cases.learn_nms_case with bbox_pred [n, 4 * (num_fg + 1)]; with the [n, 8] form's N(0, 0.1) spread."""
    cls_score, _, rois, im_info, feat, p = cases.learn_nms_case(n, num_fg, seed)
    return cls_score, wide_deltas(n, num_fg + 1, seed, 0.1), rois, im_info, feat, p


def post_case(n, num_classes, seed):
    """rois [n, 5], scores [n, C] fp32 (softmax rows), deltas [n, 4 C] fp32 N(0, 0.5): a sizeable share of boxes is clipped."""
    rng = np.random.default_rng(seed)
    rois = np.hstack((np.zeros((n, 1), F32), cases.random_boxes(n, seed + 1))).astype(F32)
    z = rng.normal(0, 2.5, (n, num_classes))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    scores = (e / e.sum(axis=1, keepdims=True)).astype(F32)
    return rois, scores, wide_deltas(n, num_classes, seed, 0.5)


def softmax_f32(z):
    z = np.asarray(z, F32)
    e = np.exp((z - z.max(axis=1, keepdims=True)).astype(np.float64))
    return (e / e.sum(axis=1, keepdims=True)).astype(F32)


def refine_boxes(rois, bbox_pred, im_info, means=None, stds=None):
    """The box path of the learn-NMS operator with class_agnostic false, in float32 (operator_py/learn_nms.py:175-217,283-287):
    bbox_pred[:, 4:] is [N, C-1, 4], every foreground class refines the roi by its own four deltas, clipped to the image.
    -> [N, C-1, 4]."""
    rois, d = np.asarray(rois, F32), np.asarray(bbox_pred, F32)
    d = d[:, 4:].reshape(len(d), -1, 4)
    x1, y1, x2, y2 = (rois[:, k:k + 1] for k in (1, 2, 3, 4))
    one, half = F32(1.0), F32(0.5)
    w, h = x2 - x1 + one, y2 - y1 + one
    cx, cy = half * (x1 + x2), half * (y1 + y2)
    dx, dy, dw, dh = (d[:, :, k] for k in range(4))
    if means is not None and stds is not None:
        dx, dy, dw, dh = (v * F32(s) + F32(m) for v, s, m in zip((dx, dy, dw, dh), stds, means))
    rcx, rcy = cx + w * dx, cy + h * dy
    rw = w * np.exp(dw.astype(np.float64)).astype(F32)
    rh = h * np.exp(dh.astype(np.float64)).astype(F32)
    wo, ho = half * (rw - one), half * (rh - one)
    out = np.stack((rcx - wo, rcy - ho, rcx + wo, rcy + ho), axis=2).astype(F32)
    info = np.asarray(im_info, F32).reshape(-1, 3)[0]
    lim = np.array([info[1] - one, info[0] - one, info[1] - one, info[0] - one], F32)
    return np.maximum(np.minimum(out, lim), F32(0.0))


def sort_and_pick(cls_score, refined, first_n):
    """learn_nms.py:289-321: per foreground class the first_n rois by descending probability (ties: smaller roi index first),
    sorted_bbox[r, k] = refined[idx[r, k], k].  -> rank_idx [F, C-1], sorted_score [F, C-1], sorted_bbox [F, C-1, 4]."""
    prob = softmax_f32(cls_score)[:, 1:]
    idx = np.argsort(-prob, axis=0, kind='stable')[:first_n]
    k = np.arange(prob.shape[1])[None, :]
    return idx, prob[idx, k], refined[idx, k]


def head_losses(x2, pd, labels_ohem, bbox_target, bbox_weight_ohem, batch_rois_ohem=128):
    """cls_score / bbox_pred FCs on fc_all_2_relu and the two head losses of ONE image as torch float64 autograd sees them
    (symbols/...:262-300: SoftmaxOutput normalization='valid' with ignore label -1, MakeLoss(w * smooth_l1) / BATCH_ROIS_OHEM);
    width-generic: bbox_pred_weight is [4 * num_reg, 1024], targets / weights [R, 4 * num_reg].  x2 [R, 1024] float64, pd: the four
    parameter tensors (differentiable).  -> (l_cls, l_box, cls_score, bbox_pred)."""
    import torch
    from oracle.losses import smooth_l1
    cls_score = x2 @ pd['cls_score_weight'].t() + pd['cls_score_bias']
    bbox_pred = x2 @ pd['bbox_pred_weight'].t() + pd['bbox_pred_bias']
    lo = torch.as_tensor(np.asarray(labels_ohem, np.int64))
    v = lo >= 0
    lp = torch.log_softmax(cls_score, dim=1)
    l_cls = -(lp[torch.arange(len(lo)), lo.clamp(min=0)] * v.double()).sum() / max(int(v.sum()), 1)
    w = torch.as_tensor(np.asarray(bbox_weight_ohem), dtype=torch.float64)
    t = torch.as_tensor(np.asarray(bbox_target), dtype=torch.float64)
    l_box = (w * smooth_l1(bbox_pred - t, 1.0)).sum() / batch_rois_ohem
    return l_cls, l_box, cls_score, bbox_pred
