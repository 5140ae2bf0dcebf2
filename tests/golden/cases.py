"""Seeded synthetic inputs shared by the golden generator and the tests
(fixed seeds, tie-free scores, boxes inside a 600x1000 image).

Large tensors (features, weights) are regenerated from the seed instead of being
stored in the fixtures; only the reference-side OUTPUTS are committed as .npz.
"""
import numpy as np

F32 = np.float32
IM_H, IM_W = 600, 1000


def random_boxes(n, seed, im_h=IM_H, im_w=IM_W, min_size=16, max_size=400):
    """n boxes (x1,y1,x2,y2) fp32, integer-free uniform, clipped to the image."""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(0, im_w - min_size - 1, n)
    y1 = rng.uniform(0, im_h - min_size - 1, n)
    w = rng.uniform(min_size, max_size, n)
    h = rng.uniform(min_size, max_size, n)
    x2 = np.minimum(x1 + w, im_w - 1)
    y2 = np.minimum(y1 + h, im_h - 1)
    return np.stack((x1, y1, x2, y2), axis=1).astype(F32)


def relation_case(n, m, seed, std, feat_dim=1024, dim=(1024, 1024, 1024), fc_dim=16, emb=64,
                  index=1, prefix=''):
    """boxes [n,4], feat [n,feat_dim], relation weights N(0,std) (biases small non-zero so
    bias handling is exercised; the reference initialises them to 0 but trains them)."""
    rng = np.random.default_rng(seed)
    boxes = random_boxes(n, seed + 1000)
    feat = rng.normal(0, 1, (n, feat_dim)).astype(F32)
    p = {}
    def nrm(*shape, s=std):
        return rng.normal(0.0, s, size=shape).astype(F32)
    p['%spair_pos_fc1_%d_weight' % (prefix, index)] = nrm(fc_dim, emb)
    p['%spair_pos_fc1_%d_bias' % (prefix, index)] = nrm(fc_dim, s=std)
    p['%squery_%d_weight' % (prefix, index)] = nrm(dim[0], feat_dim)
    p['%squery_%d_bias' % (prefix, index)] = nrm(dim[0], s=std)
    p['%skey_%d_weight' % (prefix, index)] = nrm(dim[1], feat_dim)
    p['%skey_%d_bias' % (prefix, index)] = nrm(dim[1], s=std)
    p['%slinear_out_%d_weight' % (prefix, index)] = nrm(dim[2], feat_dim, 1, 1)
    p['%slinear_out_%d_bias' % (prefix, index)] = nrm(dim[2], s=std)
    return boxes, feat, p


RELATION_CASES = {
    # name: (n, m, seed, std)
    'rel_n48_m48_std01': (48, 48, 11, 0.01),
    'rel_n40_m32_std05': (40, 32, 12, 0.05),     # keys = first 32 rois (nongt_dim < N)
}


def learn_nms_case(n, num_fg, seed, std=0.05):
    """Inputs of the learn_nms operator (operator_py/learn_nms.py:437-441 argument order)."""
    rng = np.random.default_rng(seed)
    boxes = random_boxes(n, seed + 2000)
    rois = np.hstack((np.zeros((n, 1), F32), boxes)).astype(F32)
    cls_score = rng.normal(0, 2.0, (n, num_fg + 1)).astype(F32)
    bbox_pred = rng.normal(0, 0.1, (n, 8)).astype(F32)
    im_info = np.array([[IM_H, IM_W, 1.0]], dtype=F32)
    feat = np.maximum(rng.normal(0, 1, (n, 1024)), 0).astype(F32)
    def nrm(*shape, s=std):
        return rng.normal(0.0, s, size=shape).astype(F32)
    p = {
        'nms_rank_weight': nrm(128, 1024), 'nms_rank_bias': nrm(128),
        'roi_feat_embedding_weight': nrm(128, 1024), 'roi_feat_embedding_bias': nrm(128),
        'nms_pair_pos_fc1_1_weight': nrm(16, 64), 'nms_pair_pos_fc1_1_bias': nrm(16),
        'nms_query_1_weight': nrm(1024, 128), 'nms_query_1_bias': nrm(1024),
        'nms_key_1_weight': nrm(1024, 128), 'nms_key_1_bias': nrm(1024),
        'nms_linear_out_1_weight': nrm(128, 128, 1, 1), 'nms_linear_out_1_bias': nrm(128),
        'nms_logit_weight': nrm(5, 128), 'nms_logit_bias': np.full(5, -3.0, F32),
    }
    return cls_score, bbox_pred, rois, im_info, feat, p


LEARN_NMS_ARG_ORDER = ['nms_rank_weight', 'nms_rank_bias', 'roi_feat_embedding_weight',
                       'roi_feat_embedding_bias', 'nms_pair_pos_fc1_1_weight',
                       'nms_pair_pos_fc1_1_bias', 'nms_query_1_weight', 'nms_query_1_bias',
                       'nms_key_1_weight', 'nms_key_1_bias', 'nms_linear_out_1_weight',
                       'nms_linear_out_1_bias', 'nms_logit_weight', 'nms_logit_bias']

#: full-size cases (tests/golden/relation_large.npz keeps a SUBSET of query rows: the logits of one N = 1000 case are 64 MB)
RELATION_LARGE_CASES = {
    # name: (n, m, seed, std, rows kept)
    'rel_n300_m300_std01': (300, 300, 13, 0.01, 48),
    'rel_n333_m300_std05': (333, 300, 14, 0.05, 48),      # training shape: 300 proposals + gt rows, keys = first 300
    'rel_n1000_m1000_std02': (1000, 1000, 15, 0.02, 24),  # FPN configuration (TOP_ROIS 1000)
}


def kept_rows(n, k, seed):
    """The query rows stored for a large case: first, last and k-2 seeded random ones (sorted)."""
    rng = np.random.default_rng(seed + 5000)
    r = set([0, n - 1]) | set(int(x) for x in rng.choice(n, k, replace=False))
    return np.array(sorted(r)[:k], dtype=np.int64)


LEARN_NMS_LARGE_CASES = {
    'lnms_n300_c80_f100': (300, 80, 100, 22),               # the benchmark's learn-NMS shape
}

LEARN_NMS_CASES = {
    # name: (n_rois, num_fg_classes, first_n, seed)
    'lnms_n60_c6_f20': (60, 6, 20, 21),
}

#: the learn-NMS head AS THE FPN YAML WORDS IT (experiments/relation_rcnn/cfgs/..._rcnn_fpn_relation_learn_nms_8epoch.yaml:141,166-167:
#: TOP_ROIS 1000, FIRST_N 150, LEARN_NMS_CLASS_SCORE_TH 0.05); stored in tests/golden/learn_nms_fpn.npz
LEARN_NMS_FPN_CASES = {
    # name: (n_rois, num_fg_classes, first_n, seed, class_thresh)
    'lnms_n1000_c80_f150_th05': (1000, 80, 150, 23, 0.05),
}


def learn_nms_fpn_case(n, num_fg, seed):
    """learn_nms_case with every fourth class pushed down by 5 logits: 9 of the 80 class maxima fall below 0.01 and another 9
    between 0.01 and 0.05, so the yaml's 0.05 valid-class rule and the default 0.01 give different class sets."""
    cls_score, bbox_pred, rois, im_info, feat, p = learn_nms_case(n, num_fg, seed)
    cls_score[:, 1 + np.arange(0, num_fg, 4)] -= F32(5.0)
    return cls_score, bbox_pred, rois, im_info, feat, p


def dets_case(n, seed):
    """[n,5] fp32 detections with distinct scores for NMS tests."""
    rng = np.random.default_rng(seed)
    boxes = random_boxes(n, seed + 3000, max_size=300)
    scores = rng.permutation(n).astype(np.float64)
    scores = (scores + rng.uniform(0.1, 0.9, n)) / n       # distinct, in (0,1)
    return np.hstack((boxes, scores[:, None].astype(F32))).astype(F32)


def rpn_case(seed, height=38, width=63, num_anchors=12, score_sigma=2.0, delta_sigma=0.5):
    """cls_prob [1,2A,H,W] (softmax pairs), bbox_pred [1,4A,H,W]; fg scores tie-free."""
    rng = np.random.default_rng(seed)
    logit = rng.normal(0, score_sigma, (1, num_anchors, height, width))
    fg = 1.0 / (1.0 + np.exp(-logit))
    fg = fg.astype(F32)
    flat = fg.ravel()
    # break exact fp32 ties deterministically
    order = np.argsort(flat, kind='stable')
    s = flat[order]
    for _ in range(4):
        dup = np.where(s[1:] <= s[:-1])[0]
        if dup.size == 0:
            break
        for d in dup:
            s[d + 1] = np.nextafter(s[d], F32(2.0), dtype=F32)
    flat[order] = s
    fg = flat.reshape(fg.shape)
    cls_prob = np.concatenate((F32(1) - fg, fg), axis=1).astype(F32)
    deltas = rng.normal(0, delta_sigma, (1, 4 * num_anchors, height, width)).astype(F32)
    im_info = np.array([[IM_H, IM_W, 1.0]], dtype=F32)
    return cls_prob, deltas, im_info


def targets_case(n, g, seed, num_fg=80):
    """Training-target inputs: rois [n,5], gt_boxes [g,5] (class ids 1..num_fg), and head outputs."""
    rng = np.random.default_rng(seed)
    gt = random_boxes(g, seed + 4000, min_size=32)
    gt_cls = rng.integers(1, num_fg + 1, g).astype(F32)
    gt_boxes = np.hstack((gt, gt_cls[:, None])).astype(F32)
    rois = random_boxes(n, seed + 4001)
    # a third of the rois are jittered copies of gt boxes so that positives exist
    k = n // 3
    src = rng.integers(0, g, k)
    rois[:k] = np.clip(gt[src] + rng.normal(0, 6, (k, 4)).astype(F32), 0, [IM_W - 1, IM_H - 1, IM_W - 1, IM_H - 1])
    rois[:k, 2:] = np.maximum(rois[:k, 2:], rois[:k, :2] + 4)
    rois = np.hstack((np.zeros((n, 1), F32), rois)).astype(F32)
    cls_score = rng.normal(0, 2, (n + g, num_fg + 1)).astype(F32)
    bbox_pred = rng.normal(0, 0.5, (n + g, 8)).astype(F32)
    return rois, gt_boxes, cls_score, bbox_pred


def nms_target_case(first_n, num_fg, g, seed):
    """bbox [F,C,4], gt_box [1,G,5], score [F,C] (descending per class, like sorted_score)."""
    rng = np.random.default_rng(seed)
    gt = random_boxes(g, seed + 5000, min_size=40)
    gt_cls = rng.integers(1, min(num_fg, 4) + 1, g).astype(F32)      # few classes -> several gts per class
    gt_box = np.hstack((gt, gt_cls[:, None])).astype(F32)[None]
    bbox = np.zeros((first_n, num_fg, 4), F32)
    for c in range(num_fg):
        b = random_boxes(first_n, seed + 6000 + c)
        src = rng.integers(0, g, first_n // 2)
        b[:first_n // 2] = np.clip(gt[src] + rng.normal(0, 8, (first_n // 2, 4)).astype(F32), 0, [IM_W - 1, IM_H - 1, IM_W - 1, IM_H - 1])
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 4)
        bbox[:, c] = b[rng.permutation(first_n)]
    score = np.sort(rng.random((first_n, num_fg)).astype(F32), axis=0)[::-1].copy()
    return bbox, gt_box, score


def fpn_proposals(n, seed, im_h=800, im_w=1024):
    """n float32 proposals spanning all four pyramid levels; the first six sit exactly ON the level boundaries
    (sqrt(w*h) = 112, 224, 448 with w = h and with w = 4h)."""
    rng = np.random.default_rng(seed)
    side = np.exp(rng.uniform(np.log(12), np.log(700), n))
    ar = np.exp(rng.uniform(-0.7, 0.7, n))
    w = np.minimum(side * ar, im_w - 2); h = np.minimum(side / ar, im_h - 2)
    x1 = rng.uniform(0, im_w - 1 - w); y1 = rng.uniform(0, im_h - 1 - h)
    b = np.stack([x1, y1, x1 + w, y1 + h], 1).astype(F32)
    for i, s in enumerate((112, 224, 448)):
        b[i] = [10, 20, 10 + s - 1, 20 + s - 1]
        b[3 + i] = [5, 5, 5 + 2 * s - 1, 5 + s / 2 - 1]
    return b


def rpn_gt_boxes(g, seed, im_h=IM_H, im_w=IM_W):
    """g gt boxes [g,5] (x1,y1,x2,y2,cls) float32 with sides in [40, 400]."""
    rng = np.random.default_rng(seed)
    bw, bh = rng.uniform(40, 400, g), rng.uniform(40, 400, g)
    x1, y1 = rng.uniform(0, im_w - 1 - bw), rng.uniform(0, im_h - 1 - bh)
    return np.stack([x1, y1, x1 + bw, y1 + bh, rng.integers(1, 81, g)], 1).astype(F32)


def cocoeval_case(seed=71, n_images=6, n_cats=4):
    """A synthetic detection problem for the COCO bbox evaluation: ground truth with crowd boxes and every area range, detections
    that hit, miss, duplicate and drift, several per (image, category), distinct scores.  -> (gts, dts) lists of dicts in the
    COCO json layout (bbox = [x, y, w, h])."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    gid = 1
    for img in range(1, n_images + 1):
        for cat in range(1, n_cats + 1):
            ng = int(rng.integers(0, 5))
            for _ in range(ng):
                side = float(np.exp(rng.uniform(np.log(8), np.log(300))))
                ar = float(np.exp(rng.uniform(-0.6, 0.6)))
                w, h = min(side * ar, 590.0), min(side / ar, 390.0)
                x, y = float(rng.uniform(0, 600 - w)), float(rng.uniform(0, 400 - h))
                crowd = int(rng.random() < 0.12)
                gts.append(dict(id=gid, image_id=img, category_id=cat, bbox=[x, y, w, h], area=w * h * float(rng.uniform(0.5, 1.0)),
                                iscrowd=crowd))
                gid += 1
                for k in range(int(rng.integers(0, 4))):        # detections around this gt: jittered copies
                    j = rng.normal(0, 0.08 + 0.1 * k, 4)
                    dts.append(dict(image_id=img, category_id=cat, score=float(rng.random()),
                                    bbox=[x + j[0] * w, y + j[1] * h, w * float(np.exp(j[2])), h * float(np.exp(j[3]))]))
            for _ in range(int(rng.integers(0, 3))):            # false positives
                w, h = float(rng.uniform(5, 200)), float(rng.uniform(5, 200))
                dts.append(dict(image_id=img, category_id=cat, score=float(rng.random()) * 0.7,
                                bbox=[float(rng.uniform(0, 600 - w)), float(rng.uniform(0, 400 - h)), w, h]))
    for i, d in enumerate(dts):
        d['id'] = i + 1
        d['area'] = d['bbox'][2] * d['bbox'][3]
    return gts, dts


# ---------------------------------------------------------------------------------------------------------------------------
# Adversarial inputs: exact ties and threshold equalities (tests/test_gpu_ties.py; tests/test_ties_host.py asserts that every
# generator below really delivers the property it is for).  The tie-free generators above stay as they are.
# ---------------------------------------------------------------------------------------------------------------------------
def round_mantissa(x, bits):
    """float32 -> float32 rounded (nearest, ties to even) to `bits` SIGNIFICANT bits (the implicit leading one included):
    bits = 8 is exactly the bfloat16 grid, bits = 24 the identity."""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    drop = 24 - int(bits)
    if drop > 0:
        u = u + ((1 << (drop - 1)) - 1) + ((u >> drop) & 1)
        u = (u >> drop) << drop
    return u.astype(np.uint32).view(F32).reshape(np.shape(x))


def quantised_scores(n, seed, bits=8, straddle=None, sigma=2.0):
    """n float32 objectness scores in (0, 1) rounded to `bits` significant bits: with bits = 8 the distribution a bf16 trunk hands
    the RPN (a few hundred distinct values over 28 728 anchors, so thousands of anchors share a score).
    straddle = (K, run): additionally the `run` scores around the K-th largest (sorted positions K - run // 2 ... K + run - run // 2 - 1)
    all get the K-th largest value, so that a run of equal scores lies ACROSS the top-K cut."""
    rng = np.random.default_rng(seed)
    s = round_mantissa((1.0 / (1.0 + np.exp(-rng.normal(0, sigma, n)))).astype(F32), bits)
    if straddle is not None:
        K, run = straddle
        order = np.argsort(-s, kind='stable')
        lo = max(K - run // 2, 0)
        s[order[lo:min(lo + run, n)]] = s[order[K - 1]]
    return s


def lattice_boxes(n, seed, stride=16, im_h=IM_H, im_w=IM_W, n_beyond=2):
    """n float32 rois (x1,y1,x2,y2) on the lattice where rounding decides: coordinates are ODD multiples of stride / 2 (8, 24, 40, ...
    for stride 16), which scale to k + 0.5 exactly under spatial_scale = 1 / stride, or integers on the image border (0, im_w - 1,
    im_h - 1: what clip_boxes produces).  Fixed rows first: [8,8,40,40] (pools cells 1..3 with C round(), 0..2 with half-to-even),
    a roi from the border 0 to the border im_w-1 / im_h-1, rois with NEGATIVE odd multiples (round(-0.5) = -1: the window is clamped
    to the map), a one-cell roi, and `n_beyond` rois wholly beyond the map (every bin empty -> 0 / argmax -1).  The rest are seeded
    random lattice boxes, a third of them with x1 = 0 or x2 = im_w - 1; duplicates occur, as they do after clip_boxes."""
    rng = np.random.default_rng(seed)
    h = stride // 2
    kx, ky = (im_w - 1) // h, (im_h - 1) // h                 # lattice points inside the image: h (2 j + 1) <= im - 1
    def odd(lo, hi, size):
        return (2 * rng.integers(lo, hi, size) + 1) * h
    jx, jy = (kx - 1) // 2, (ky - 1) // 2
    x1 = odd(0, jx - 2, n); y1 = odd(0, jy - 2, n)
    x2 = np.minimum(x1 + 2 * h * rng.integers(0, 24, n), (2 * jx - 1) * h)
    y2 = np.minimum(y1 + 2 * h * rng.integers(0, 18, n), (2 * jy - 1) * h)
    b = np.stack((x1, y1, x2, y2), 1).astype(F32)
    third = n // 3
    b[:third:2, 0] = 0
    b[1:third:2, 2] = im_w - 1
    b[2:third:4, 3] = im_h - 1
    fixed = [[8, 8, 40, 40], [0, 0, im_w - 1, im_h - 1], [-h, -h, 5 * h, 7 * h], [-3 * h, h, 3 * h, 9 * h], [3 * h, 3 * h, 3 * h, 3 * h],
             [0, h, im_w - 1, 3 * h]]
    for i in range(n_beyond):
        fixed.append([im_w + (2 * i + 1) * h + 2 * h, im_h + h + 2 * h, im_w + (2 * i + 13) * h, im_h + 11 * h])
    fixed = np.asarray(fixed[:n], dtype=F32)
    b[len(b) - len(fixed):] = fixed                          # (at the END: the first rows keep the seeded border boxes)
    return b


def relu_tied_map(B, C, H, W, seed, levels=8):
    """[B,C,H,W] float32, every value bf16-representable, as a feature map looks after ReLU in the bf16 trunk: about half the cells are
    exactly 0 and the others lie on a grid of `levels` values (multiples of 0.25), so the maximum of a pooling bin is usually held by
    several cells and many bins are all-zero; on top of that every second column copies its left neighbour in three quarters of the cells and
    every second row the row above in half (a duplicated maximum side by side and one below the other: a scan that prefers the
    LAST maximum reports another argmax).  Channel 0 of every image is entirely zero (every bin of it ties at 0)."""
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.normal(0, 1, (B, C, H, W)), 0)
    x = np.minimum(np.ceil(x * 4), levels) / 4                # 0 stays 0; (0, 0.25] -> 0.25 ...
    wp, hp = W // 2, H // 2
    cw = rng.random((B, C, H, wp)) < 0.75
    x[..., 1:2 * wp:2] = np.where(cw, x[..., 0:2 * wp:2], x[..., 1:2 * wp:2])
    ch = rng.random((B, C, hp, W)) < 0.5
    x[:, :, 1:2 * hp:2] = np.where(ch, x[:, :, 0:2 * hp:2], x[:, :, 1:2 * hp:2])
    x[:, 0] = 0
    return x.astype(F32)


def _nested_pair(S, w, hh):
    """B = [0,0,w-1,hh-1] inside A = [0,0,S-1,S-1]: IoU = w hh / S^2 with every float32 operand an exact integer."""
    return np.array([0, 0, S - 1, S - 1], F32), np.array([0, 0, w - 1, hh - 1], F32)


def _dev_iou_nested(S, w, hh):
    """devIoU (nms_kernel.cu:24-32, float32, one rounding per operation) of the pair of _nested_pair."""
    inter = F32(w) * F32(hh)
    return inter / ((F32(S) * F32(S) + inter) - inter)


def iou_boundary_pairs(thresh):
    """Integer box pairs whose IoU sits exactly ON the NMS threshold and one float32 ulp either side of it.
    -> dict(eq=[(a, b), ...], above=(a, b), below=(a, b)), boxes float32 [4]:
      eq     IoU == thresh in float64 AND devIoU (float32, oracle.nms.iou_f32) == float32(thresh): [0,0,9,9] against [0,0,9,k-1] is k/10 and
             [0,0,19,19] against [0,0,19,2k-1] the same ratio at another size (a correctly rounded quotient of exact integers is the float
             nearest the ratio, in either precision); thresh must be a multiple of 0.1;
      above  devIoU == nextafter(float32(thresh), 1), below == nextafter(float32(thresh), 0): nested integer boxes [0,0,S-1,S-1] /
             [0,0,w-1,h-1] with w h / S^2 inside the target float's rounding interval, found by a deterministic search: first over the S with S^2 + w h < 2^24
             (every intermediate of devIoU is then an exact float32 integer), then, where that grid is coarser than the ulp (0.5 from
             below), over larger S with the float32 devIoU itself as the test."""
    k = int(round(thresh * 10))
    assert abs(thresh * 10 - k) < 1e-9 and 0 < k < 10, thresh
    eq = [(np.array([0, 0, 9, 9], F32), np.array([0, 0, 9, k - 1], F32)),
          (np.array([0, 0, 19, 19], F32), np.array([0, 0, 19, 2 * k - 1], F32))]
    out = dict(eq=eq)
    t32 = F32(thresh)
    for name, toward in (('above', F32(1)), ('below', F32(0))):
        target = np.nextafter(t32, toward)
        found = None
        for S in list(range(int(np.sqrt(2.0 ** 24 / (1.0 + thresh + 1e-3))), 2000, -1)) + list(range(4095, 5700)):
            q = S * S
            for prod in range(int(np.floor(float(target) * q)) - 2, int(np.ceil(float(target) * q)) + 3):
                ws = np.arange(-(-prod // S), S + 1)
                ws = ws[prod % ws == 0]
                if ws.size and _dev_iou_nested(S, int(ws[0]), prod // int(ws[0])) == target:
                    found = _nested_pair(S, int(ws[0]), prod // int(ws[0]))
                    break
            if found is not None:
                break
        assert found is not None, (thresh, name)
        out[name] = found
    return out


def saturated_posteriors(B, N, C, seed):
    """Head outputs as a TRAINED detector produces them -> (cls_prob [B,N,C] float32, boxes [B,N,4] float64, info).
      * ordinary rows: float32 softmax of N(0, 2) logits, integer-free boxes;
      * clusters (about a third of the rows): 2-5 DISTINCT overlapping integer boxes (one object seen by several rois) whose softmax
        saturates: the cluster's class holds exactly 1.0f, every other class ~1e-18.  The clusters share the first four foreground
        classes, so a class sees two-way and multi-way ties at 1.0f, between overlapping boxes (one cluster) and disjoint or partly
        overlapping ones (different clusters).  Even clusters occupy consecutive roi indices (one wavefront of the class-NMS
        kernel), odd clusters indices 64 apart (different wavefronts) when N > 64;
      * duplicated posteriors: every seventh ordinary row copies the posterior (not the box) of the row before it: two-way ties in
        every class at generic values;
      * the LAST class is constructed and holds nothing else (ordinary rows are 0 there): P1 (0.9) over A (0.5) and P2 (0.8) over B (0.5),
        the second pair an integer translate of the first and disjoint from it -- A and B are tied, A's rescoring by P1 breaks the tie,
        B's by P2 restores it exactly (a tie that ARISES from rescoring); M1 and M2 (0.25 each) disjoint mirror images either side of P3 (0.7):
        tied before and after their common rescoring; and, on disjoint boxes, three rows at exactly float32(1e-3) (excluded by the
        `> 1e-3` of tester.py), three at nextafter(float32(1e-3), 1) (included, tied), two at nextafter(float32(1e-3), 0).
        The overwritten rows no longer sum to one: the kernels take cls_prob as it is.
    info: dict(clusters=[(class, indices)], constructed=dict(name -> roi index), threshold_rows=dict(eq=[..], up=[..], down=[..]))."""
    rng = np.random.default_rng(seed)
    assert N >= 36 and C >= 6
    boxes = np.stack([random_boxes(N, seed + 7000 + b, max_size=300) for b in range(B)]).astype(np.float64)
    z = rng.normal(0, 2.0, (B, N, C))
    used = np.zeros(N, bool)
    special = 16                                              # the last 16 rois carry the constructed class
    used[N - special:] = True
    clusters = []
    n_clusters = max(4, (N - special) // 12)
    for k in range(n_clusters):
        cls = 1 + k % 4
        m = 2 + k % 4
        idx = None
        if k % 2 == 1 and N - special > 64:                   # members 64 apart: different wavefronts
            for j in range(64):
                cand = [j + 64 * t for t in range(m) if j + 64 * t < N]
                if len(cand) >= 2 and not used[cand].any():
                    idx = cand
                    break
        if idx is None:                                       # consecutive members inside one block of 64
            start = (k * 37) % N
            for off in range(N):
                j = (start + off) % N
                if j // 64 == (j + m - 1) // 64 and j + m <= N and not used[j:j + m].any():
                    idx = list(range(j, j + m))
                    break
        if idx is None:
            continue
        used[idx] = True
        x1, y1 = rng.integers(0, 600), rng.integers(0, 300)
        w, h = rng.integers(60, 300), rng.integers(60, 250)
        for t, i in enumerate(idx):
            boxes[:, i] = [x1 + 3 * t, y1 + 2 * t, x1 + w + 3 * t, y1 + h + 2 * t]
            z[:, i, :] = rng.normal(0, 1.0, (B, C))
            z[:, i, cls] = 42.0
        clusters.append((cls, idx))
    zf = z.astype(F32)
    e = np.exp((zf - zf.max(axis=2, keepdims=True)).astype(np.float64))
    prob = (e / e.sum(axis=2, keepdims=True)).astype(F32)
    free = np.where(~used)[0]
    for i in free[1::7]:
        if not used[i - 1]:
            prob[:, i] = prob[:, i - 1]
    # ---- the constructed class ----------------------------------------------------------------------------------------
    last = C - 1
    prob[:, :, last] = 0
    base = N - special
    names = ['P1', 'A', 'P2', 'B', 'M1', 'P3', 'M2', 'eq0', 'eq1', 'eq2', 'up0', 'up1', 'up2', 'down0', 'down1', 'pad']
    con = {nm: base + i for i, nm in enumerate(names)}
    def put(nm, box, p):
        boxes[:, con[nm]] = box
        prob[:, con[nm], :] = 0
        prob[:, con[nm], last] = p
    put('P1', [10, 10, 109, 89], 0.9); put('A', [40, 30, 139, 109], 0.5)
    put('P2', [410, 10, 509, 89], 0.8); put('B', [440, 30, 539, 109], 0.5)
    put('P3', [200, 300, 299, 379], 0.7); put('M1', [150, 300, 249, 379], 0.25); put('M2', [250, 300, 349, 379], 0.25)
    t = F32(1e-3)
    vals = dict(eq=t, up=np.nextafter(t, F32(1)), down=np.nextafter(t, F32(0)))
    for j, nm in enumerate(names[7:15]):
        put(nm, [600 + 40 * j, 450, 630 + 40 * j, 480], vals[nm[:-1]])
    put('pad', [900, 500, 930, 530], 0.0)
    info = dict(clusters=clusters, constructed=con,
                threshold_rows={k: [con[nm] for nm in names[7:15] if nm[:-1] == k] for k in vals})
    return prob, boxes, info


def tied_image_lists(B, NC, N, seed, counts_hi, levels=16, counts_lo=0):
    """Per-class detection lists as class_nms leaves them -> (dets [B,NC,N,5] float64, counts [B,NC] int32): every list non-increasing,
    scores on a grid of `levels` values (k / levels), so many detections of an image share the max_per_image-th largest score."""
    rng = np.random.default_rng(seed)
    dets = np.zeros((B, NC, N, 5))
    counts = rng.integers(counts_lo, counts_hi + 1, (B, NC)).astype(np.int32)
    for b in range(B):
        for c in range(NC):
            k = counts[b, c]
            s = np.sort(rng.integers(1, levels + 1, k) / float(levels))[::-1]
            dets[b, c, :k, 4] = s
            dets[b, c, :k, :4] = random_boxes(k, seed + 100 * b + c).astype(np.float64) if k else 0
    return dets, counts


def fpn_boundary_rois():
    """float32 rois [n,4] ON and one float32 step either side of every FPN level boundary: for k in (-1, 0, 1) boxes of width 224 2^k whose
    height is stepped through the float32 neighbours of 224 2^k until s = sqrt(w h) / 224 (float32, rcnn.py:56-58) is exactly 2^k, its
    predecessor and its successor; plus both clamps (1 x 1, zero-area x2 = x1 - 1, 4000 x 4000) -> (rois, s values)."""
    rois, svals = [], []
    for k in (-1, 0, 1):
        side = F32(224.0 * 2.0 ** k)
        want = {F32(2.0 ** k): None, np.nextafter(F32(2.0 ** k), F32(0)): None, np.nextafter(F32(2.0 ** k), F32(9)): None}
        y2 = side - F32(1)
        cands = [y2]
        up, dn = y2, y2
        for _ in range(64):
            up = np.nextafter(up, F32(1e9)); dn = np.nextafter(dn, F32(0))
            cands += [up, dn]
        for c in cands:
            w = (side - F32(1)) - F32(0) + F32(1)
            h = F32(c) - F32(0) + F32(1)
            s = F32(np.sqrt(F32(w * h)) / F32(224))
            if s in want and want[s] is None:
                want[s] = [0, 0, side - F32(1), c]
        for s, r in want.items():
            assert r is not None, (k, s)
            rois.append(r); svals.append(s)
    for r in ([5, 5, 5, 5], [7, 7, 6, 9], [0, 0, 3999, 3999], [0, 0, 0.5, 0.25]):
        rois.append(r); svals.append(F32(np.nan))
    return np.asarray(rois, dtype=F32), np.asarray(svals, dtype=F32)
