"""Edge cases of the training-target kernels (csrc/targets.hip: relnet_assign_anchor, relnet_proposal_target_ex, relnet_box_annotator_ohem,
relnet_nms_multi_target, relnet_bbox_overlaps) and of the proposal decode (csrc/proposal.hip: relnet_proposal_decode).  numpy only: the
host test (tests/test_target_edge_cases_host.py) asserts that every case is what it claims, the GPU test (tests/test_gpu_target_edges.py)
compares the kernels with the expected arrays built here.

Expected outputs come from the pinned oracle pieces alone -- oracle/anchors.py, oracle/targets.py, oracle/boxes.py (bbox_pred, clip_boxes,
generate_anchors, bbox_overlaps) and oracle/proposal.py:shifted_anchors -- and from the layouts that relnet_amd/ops.py documents (padding
rows, image index columns).  Where the oracle cannot run (an image without a single inside anchor, an image without gt boxes in
proposal_target, a class-specific gt label past num_reg) the contract of include/relnet_hip.h / ops.py is written out and says so.

  ANCHOR_CASES / anchor_case / anchor_expected        relnet_assign_anchor
  PT_CASES / pt_case / pt_expected                    relnet_proposal_target_ex (all rows, BATCH_ROIS = -1)
  OHEM_CASES / ohem_case / ohem_expected              relnet_box_annotator_ohem
  NMT_CASES / nmt_case / nmt_expected                 relnet_nms_multi_target
  OVERLAP_CASES / overlap_case                        relnet_bbox_overlaps
  DECODE_CASES / decode_case / decode_expected        relnet_proposal_decode
"""
import numpy as np

import cases
from oracle import anchors as OA
from oracle import boxes as OB
from oracle import targets as OT
from oracle.proposal import shifted_anchors

F32 = np.float32
DEFAULT_SCALES, DEFAULT_RATIOS = (4, 8, 16, 32), (0.5, 1, 2)


def _boxes(n, seed, im_h, im_w, lo=0.15, hi=0.7):
    """n float32 boxes inside an im_h x im_w image with sides of lo..hi of the image's."""
    rng = np.random.default_rng(seed)
    bw, bh = rng.uniform(lo, hi, n) * im_w, rng.uniform(lo, hi, n) * im_h
    x1, y1 = rng.uniform(0, im_w - 1 - bw), rng.uniform(0, im_h - 1 - bh)
    return np.stack([x1, y1, x1 + bw, y1 + bh], 1).astype(F32)


def _gts(n, seed, im_h, im_w, num_fg=80, lo=0.15, hi=0.7):
    rng = np.random.default_rng(seed + 9000)
    return np.hstack((_boxes(n, seed, im_h, im_w, lo, hi), rng.integers(1, num_fg + 1, (n, 1)).astype(F32))).astype(F32)


def _pad_gt(gts, fill=None):
    """list of [g_b, 5] -> [B, Gmax, 5] (Gmax >= 1) and the counts.  The slots past an image's count hold `fill` (a box that WOULD match):
    a kernel that read them would show."""
    G = max(1, max(len(g) for g in gts))
    pad = np.zeros((len(gts), G, 5), F32)
    for b, g in enumerate(gts):
        if fill is not None:
            pad[b] = fill
        pad[b, :len(g)] = g
    return pad, np.array([len(g) for g in gts], np.int32)


# =====================================================================================================================
# relnet_assign_anchor
# =====================================================================================================================
# name -> feat_hw, stride, scales, ratios, images [(number of gts or an explicit [g, 5] list, (im_h, im_w))], the settings that differ from
# the defaults of lib/rpn/rpn.py, and what the host test holds image 0 to: cut = which of the two random draws must have to cut.
_ANCHOR_DEFAULTS = dict(feat_stride=16, scales=DEFAULT_SCALES, ratios=DEFAULT_RATIOS, allowed_border=0, rpn_batch_size=256, fg_fraction=0.5,
                        negative_overlap=0.3, positive_overlap=0.7, clobber_positives=False)
_OFF = [[1000, 1000, 1100, 1100, 1]]                                          # a gt box that no anchor of a 208 x 336 image overlaps
_SMALL = dict(feat_hw=(13, 21), images=[(3, (208, 336)), (5, (208, 336))])
ANCHOR_CASES = {
    'defaults_small': dict(_SMALL, cut=('bg',)),
    'border': dict(_SMALL, allowed_border=32, cut=('bg',)),
    'small_batch': dict(_SMALL, rpn_batch_size=16, fg_fraction=0.25, cut=('fg', 'bg')),
    'overlaps_swapped_clobber': dict(_SMALL, positive_overlap=0.3, negative_overlap=0.5, rpn_batch_size=16, clobber_positives=True, cut=('fg', 'bg')),
    'overlaps_swapped_noclobber': dict(_SMALL, positive_overlap=0.3, negative_overlap=0.5, rpn_batch_size=16, clobber_positives=False, cut=('fg', 'bg')),
    'a1_stride8': dict(feat_hw=(17, 19), feat_stride=8, scales=(4,), ratios=(1,), images=[(4, (136, 152)), (1, (136, 152))], gt_seed=10, cut=()),
    'a32': dict(feat_hw=(5, 7), scales=(1, 2, 3, 4, 6, 8, 12, 16), ratios=(0.5, 1, 2, 3), allowed_border=200,
                images=[(3, (80, 112)), (1, (80, 112))], cut=('bg',)),
    'one_cell': dict(feat_hw=(1, 1), allowed_border=600, images=[([[0, 0, 15, 15, 1], [-20, -10, 40, 30, 2]], (16, 16)), ([[2, 2, 12, 12, 3]], (16, 16))], cut=()),
    'no_gt': dict(feat_hw=(13, 21), images=[(0, (208, 336)), (2, (208, 336))], allowed_border=16, cut=('bg',)),
    'gt_off_image': dict(feat_hw=(13, 21), images=[(_OFF, (208, 336)), (2, (208, 336))], allowed_border=16, rpn_batch_size=16, cut=('fg',)),
    'fg_fraction_0': dict(_SMALL, fg_fraction=0.0, cut=('fg', 'bg')),
    'batch_0': dict(_SMALL, rpn_batch_size=0, cut=('fg', 'bg')),
    # anchor totals around the 256-thread grid edge of the label kernels and the 1024-thread stride of anchor_sample_kernel (all exact)
    'total_255': dict(feat_hw=(5, 17), scales=(2,), ratios=(0.5, 1, 2), allowed_border=16, images=[(2, (80, 272)), (3, (80, 272))], total=255, cut=()),
    'total_256': dict(feat_hw=(8, 8), scales=(2, 4), ratios=(1, 2), allowed_border=16, images=[(2, (128, 128)), (1, (128, 128))], total=256, cut=()),
    'total_257': dict(feat_hw=(1, 257), scales=(1,), ratios=(1,), allowed_border=16, rpn_batch_size=64,
                      images=[([[100, 0, 131, 15, 1], [2000, 0, 2040, 15, 2]], (16, 4112)), ([[3000, 2, 3020, 14, 1]], (16, 4112))], total=257, cut=('bg',)),
    'total_1023': dict(feat_hw=(11, 31), scales=(2,), ratios=(0.5, 1, 2), allowed_border=16, rpn_batch_size=32, gt_seed=23, images=[(3, (176, 496)), (2, (176, 496))], total=1023, cut=('fg', 'bg')),
    'total_1024': dict(feat_hw=(16, 16), scales=(2, 4), ratios=(1, 2), allowed_border=16, rpn_batch_size=32, gt_seed=24, images=[(3, (256, 256)), (4, (256, 256))], total=1024, cut=('fg', 'bg')),
    'total_1025': dict(feat_hw=(5, 41), scales=(2,), ratios=(0.5, 1, 2, 3, 0.33), allowed_border=16, rpn_batch_size=32, gt_seed=25, images=[(3, (80, 656)), (1, (80, 656))], total=1025, cut=('fg', 'bg')),
    'partial_frame': dict(feat_hw=(13, 21), allowed_border=16, images=[(3, (208, 336)), (2, (120, 200)), (0, (96, 336))], cut=('bg',)),
    # not one inside anchor (the smallest default anchor is 91 x 45 around a 48 x 80 image's cells): the oracle and the reference stop with
    # "argmax of an empty sequence"; the kernel's contract is asserted directly (anchor_expected)
    'no_inside': dict(feat_hw=(3, 5), images=[(2, (48, 80)), (1, (48, 80))], cut=()),
}
ANCHOR_SEED = 20261021


def anchor_case(name):
    """-> dict(gt [B, Gmax, 5], num_gt [B], im_info [B, 3], gts (list of [g, 5]), hw (list), base [A, 4] float64, feat_hw, total, kw (the
    keyword arguments that oracle.anchors.assign_anchor and ops.assign_anchor share), scales, ratios, seed, cut)."""
    c = dict(_ANCHOR_DEFAULTS, **ANCHOR_CASES[name])
    gts, hw = [], []
    for b, (g, (h, w)) in enumerate(c['images']):
        if isinstance(g, int):
            g = _gts(g, c.get('gt_seed', 0) + b, h, w) if g > 0 else np.zeros((0, 5), F32)       # (one gt_seed: the same boxes in every case that shares it)
        gts.append(np.asarray(g, F32).reshape(-1, 5))
        hw.append((h, w))
    pad, num_gt = _pad_gt(gts, fill=[40, 40, 120, 120, 9])
    base = OB.generate_anchors(c['feat_stride'], c['ratios'], c['scales']).astype(np.float64)
    fh, fw = c['feat_hw']
    kw = {k: c[k] for k in ('feat_stride', 'allowed_border', 'rpn_batch_size', 'fg_fraction', 'negative_overlap', 'positive_overlap', 'clobber_positives')}
    return dict(name=name, gt=pad, num_gt=num_gt, im_info=np.array([[h, w, 1.0] for h, w in hw], F32), gts=gts, hw=hw, base=base,
                feat_hw=(fh, fw), total=base.shape[0] * fh * fw, kw=kw, scales=c['scales'], ratios=c['ratios'], seed=ANCHOR_SEED, cut=c['cut'])


def anchor_inside(c, b):
    """Number of anchors of image b inside the image + border (rpn.py:144-147), from the pinned anchor enumeration."""
    fh, fw = c['feat_hw']
    a = shifted_anchors(fh, fw, c['kw']['feat_stride'], c['base'])
    bd, (h, w) = c['kw']['allowed_border'], c['hw'][b]
    return int(((a[:, 0] >= -bd) & (a[:, 1] >= -bd) & (a[:, 2] < w + bd) & (a[:, 3] < h + bd)).sum())


def anchor_expected(c, b):
    """-> label [total], bbox_target [4A, fh, fw], bbox_weight [4A, fh, fw], label_all [total] of image b."""
    fh, fw = c['feat_hw']
    A = c['base'].shape[0]
    if anchor_inside(c, b) == 0:           # the kernel's contract where rpn.py cannot run: nothing is labelled, nothing is regressed
        return np.full(c['total'], -1, F32), np.zeros((4 * A, fh, fw), F32), np.zeros((4 * A, fh, fw), F32), np.full(c['total'], -1, F32)
    with np.errstate(divide='ignore', invalid='ignore'):       # (the oracle masks the quotients of disjoint pairs afterwards)
        return OA.assign_anchor((fh, fw), c['gts'][b], c['hw'][b], scales=c['scales'], ratios=c['ratios'], sampler='hash', seed=c['seed'],
                                image_index=b, return_all=True, **c['kw'])


def anchor_counts(c, b):
    """inside, fg / bg before sub-sampling, fg / bg after, num_fg, batch: the figures of the per-case summary."""
    lab, _, _, lall = anchor_expected(c, b)
    return dict(inside=anchor_inside(c, b), fg_before=int((lall == 1).sum()), bg_before=int((lall == 0).sum()), fg_after=int((lab == 1).sum()),
                bg_after=int((lab == 0).sum()), num_fg=int(c['kw']['fg_fraction'] * c['kw']['rpn_batch_size']), batch=c['kw']['rpn_batch_size'])


# =====================================================================================================================
# relnet_proposal_target_ex: all rows
# =====================================================================================================================
# N + Gmax of 255 / 256 / 257 (one 256-thread workgroup less one row, exactly one, one row into the second); num_gt = 0 inside a batch;
# num_rois of 0, N and in between; N = 0; class-specific columns with labels on both sides of num_reg
PT_CASES = {
    'rows_255': dict(N=250, num_gt=[5, 3], num_rois=None, num_reg=2, class_agnostic=True),
    'rows_256_one_image_without_gt': dict(N=250, num_gt=[6, 0], num_rois=None, num_reg=2, class_agnostic=True),
    'rows_257_num_rois': dict(N=249, num_gt=[8, 2, 5], num_rois=[249, 100, 0], num_reg=2, class_agnostic=True),
    'no_proposals': dict(N=0, num_gt=[4, 1], num_rois=None, num_reg=2, class_agnostic=True),
    'class_specific_5': dict(N=60, num_gt=[6, 4], num_rois=[60, 37], num_reg=5, class_agnostic=False, num_fg=7),
    'class_specific_5_without_gt': dict(N=33, num_gt=[0, 7], num_rois=[20, 33], num_reg=5, class_agnostic=False, num_fg=7),
}


def pt_case(name):
    """-> dict(rois [B, N, 5] (column 0 = the image index), gt [B, Gmax, 5], num_gt, num_rois (or None), N, Gmax, num_reg, class_agnostic)."""
    c = dict(PT_CASES[name])
    B, N = len(c['num_gt']), c['N']
    seed = 300 + 10 * sorted(PT_CASES).index(name)
    rois = np.zeros((B, N, 5), F32)
    gts = []
    for b in range(B):
        r, g, _, _ = cases.targets_case(N, max(c['num_gt'][b], 1), seed + b, num_fg=c.get('num_fg', 80))
        rois[b] = r
        rois[b, :, 0] = b
        gts.append(g[:c['num_gt'][b]])
    fill = np.append(rois[0, 0, 1:], 3) if N else [10, 10, 200, 200, 3]    # unused gt slots: a box that matches a proposal exactly
    gt, num_gt = _pad_gt(gts, fill=fill)
    c.update(name=name, rois=rois, gt=gt, num_gt=num_gt, Gmax=gt.shape[1], B=B,
             num_rois=None if c['num_rois'] is None else np.array(c['num_rois'], np.int32))
    return c


def pt_expected(c, b):
    """Image b laid out as ops.proposal_target documents -> rois_out [N + Gmax, 5], label, bbox_target, bbox_weight [N + Gmax, 4 num_reg].
    oracle.targets.proposal_target on the first num_rois[b] rows and num_gt[b] gts; padding rows get a zero box, the image index, label -1
    and zero targets and weights; the appended gt rows carry the image index.  An image without gt boxes has no overlaps: every proposal
    is background (csrc/targets.hip: pt_label_targets, G == 0)."""
    N, Gmax, D = c['N'], c['Gmax'], 4 * c['num_reg']
    nr = N if c['num_rois'] is None else int(c['num_rois'][b])
    G = int(c['num_gt'][b])
    R = N + Gmax
    ro, lab = np.zeros((R, 5), F32), np.full(R, -1, F32)
    bt, bw = np.zeros((R, D), F32), np.zeros((R, D), F32)
    ro[:, 0] = b
    src = c['rois'][b, :nr].copy()
    src[:, 0] = 0                                                            # (the oracle is the one-image operator: batch index 0)
    if G == 0:
        ro[:nr, 1:] = src[:, 1:]
        lab[:nr] = 0
        return ro, lab, bt, bw
    g = c['gt'][b, :G]
    # class-specific: bbox_regression.py:134-138 writes columns 4 cls .. 4 cls + 3; a label past num_reg has no such columns here (the head has
    # num_reg column groups), so the oracle runs with enough classes for every label and the columns that exist are kept
    ncls = c['num_reg'] if c['class_agnostic'] else max(c['num_reg'], int(g[:, 4].max()) + 1)
    wr, wl, wt, ww = OT.proposal_target(src, g, num_classes=ncls, class_agnostic=c['class_agnostic'])
    rows = np.concatenate((np.arange(nr), N + np.arange(G)))                 # proposals, then the appended gt rows
    ro[rows, 1:] = wr[:, 1:]
    lab[rows] = wl
    bt[rows] = wt[:, :D]
    bw[rows] = ww[:, :D]
    return ro, lab, bt, bw


# =====================================================================================================================
# relnet_box_annotator_ohem
# =====================================================================================================================
def _ohem_table():
    """R in {1, 2, 3, 1023, 1024, 1025, 2047, 2048} (np2 = 1: no sort stage; one row around the 1024-thread stride; the 2048 keys of LDS), each
    with roi_per_img in {0, 1, R - 1, R, R + 5}; C and D cycle through {2, 5} x {4, 8, 20}.  Seeds are chosen so that the losses on the two
    sides of every cut differ by more than 1e-4 relative (asserted by the host test)."""
    t = {}
    k = 0
    for R in (1, 2, 3, 1023, 1024, 1025, 2047, 2048):
        for rpi in sorted({0, 1, R - 1, R, R + 5}):
            t['R%d_keep%d' % (R, rpi)] = dict(R=R, roi_per_img=rpi, C=(2, 5)[k % 2], D=(4, 8, 20)[k % 3], ignored='none', seed=500 + k)
            k += 1
    # ignored rows (label -1, zero weights: what proposal_target emits for its padding rows)
    t['ignored_tail_inside_the_cut'] = dict(R=300, roi_per_img=256, C=5, D=8, ignored='tail', n_valid=(200, 131), seed=600)
    t['ignored_interleaved_cut_in_valid'] = dict(R=1025, roi_per_img=128, C=5, D=20, ignored='every_third', seed=601)
    t['ignored_all'] = dict(R=65, roi_per_img=16, C=2, D=4, ignored='all', seed=602)
    return t


OHEM_CASES = _ohem_table()
OHEM_B = 2


def ohem_case(name):
    """-> dict(cls_score [B, R, C], bbox_pred / bbox_targets / bbox_weights [B, R, D], labels [B, R], roi_per_img): different data per image."""
    c = dict(OHEM_CASES[name])
    rng = np.random.default_rng(c['seed'])
    B, R, C, D = OHEM_B, c['R'], c['C'], c['D']
    cs = rng.normal(0, 2, (B, R, C)).astype(F32)
    bp = rng.normal(0, 0.5, (B, R, D)).astype(F32)
    bt = rng.normal(0, 1, (B, R, D)).astype(F32)
    lab = rng.integers(0, C, (B, R)).astype(F32)
    bw = np.zeros((B, R, D), F32)
    grp = rng.integers(0, D // 4, (B, R))                                   # weights 1 on one group of four columns of every foreground row
    for q in range(4):
        np.put_along_axis(bw, (4 * grp + q)[..., None], (lab > 0).astype(F32)[..., None], axis=2)
    ign = np.zeros((B, R), bool)
    if c['ignored'] == 'tail':
        for b in range(B):
            ign[b, c['n_valid'][b]:] = True
    elif c['ignored'] == 'every_third':
        ign[0, ::3] = True
        ign[1, 1::3] = True
    elif c['ignored'] == 'all':
        ign[:] = True
    lab[ign] = -1
    bw[ign] = 0
    c.update(name=name, cls_score=cs, bbox_pred=bp, bbox_targets=bt, bbox_weights=bw, labels=lab, ignored_rows=ign)
    return c


def ohem_expected(c, b):
    """-> labels_ohem [R], bbox_weights_ohem [R, D], loss [R] (float32; -inf on ignored rows), and the oracle's loss order of the valid rows.
    oracle.targets.box_annotator_ohem on the non-ignored rows; ignored rows stay ignored whatever their rank."""
    ok = ~c['ignored_rows'][b]
    lo = np.full(c['R'], -1, F32)
    wo = np.zeros((c['R'], c['D']), F32)
    loss = np.full(c['R'], -np.inf, F32)
    order = np.zeros(0, np.int64)
    if ok.any():
        vlo, vwo, vloss = OT.box_annotator_ohem(c['cls_score'][b][ok], c['bbox_pred'][b][ok], c['labels'][b][ok], c['bbox_targets'][b][ok],
                                                c['bbox_weights'][b][ok], c['roi_per_img'])
        lo[ok], wo[ok], loss[ok] = vlo, vwo, vloss
        order = np.flatnonzero(ok)[np.argsort(vloss, kind='stable')[::-1]]
    return lo, wo, loss, order


# =====================================================================================================================
# relnet_nms_multi_target
# =====================================================================================================================
THRESH = {1: (0.5,), 5: (0.5, 0.6, 0.7, 0.8, 0.9), 8: (0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95)}
# F around the wavefront (63 / 64 / 65: one or two entries of the cross-wave reduction) and the workgroup (255 / 256); T of 1, 5 and 8 (all
# of thresh[8]); G per image (0 = an image without gt inside the batch); one_class: every gt is of class 1, so with C = 2 class 2 has none
NMT_CASES = {
    'F1': dict(F=1, C=1, G=[1, 1], T=1),
    'F63': dict(F=63, C=2, G=[3, 1], T=5),
    'F64_T8': dict(F=64, C=1, G=[3, 2], T=8),
    'F65_image_without_gt': dict(F=65, C=2, G=[3, 0], T=5),
    'F255_T1': dict(F=255, C=2, G=[1, 3], T=1),
    'F256_128_gts_of_one_class': dict(F=256, C=2, G=[128, 3], T=5, one_class=True),
    'F256_T8': dict(F=256, C=1, G=[3, 128], T=8),
    'row0_quirk': dict(F=24, C=2, G=[2, 3], T=5, by_hand='row0_quirk'),
    # the winner in the LAST row (the last wavefront's entry of red_v / red_i decides), and equal scores in rows 63 | 64
    'F65_winner_in_the_last_row': dict(F=65, C=2, G=[2, 1], T=5, by_hand='last_row'),
    'F255_winner_in_the_last_row': dict(F=255, C=2, G=[2, 1], T=8, by_hand='last_row'),
    'no_gt_at_all': dict(F=40, C=2, G=[0, 0], T=5),
}


def _row0_quirk():
    """Class 1 has two gts; NO box overlaps the second.  The reference's argmax over that gt's all-zero score column is row 0
    (nms_multi_target.py:67-70), and row 0 is a valid row (it overlaps the FIRST gt by 0.75) -- so row 0 gets a 1 at the thresholds below 0.75,
    although row 5, with the higher score, is the first gt's pick.  The kernel's s_best falls to row 0 the same way."""
    bbox, score = _filler(24, 2)
    gt = np.array([[100, 100, 199, 199, 1], [500, 100, 599, 199, 1], [100, 300, 199, 399, 2]], F32)
    bbox[0, 0] = [100, 100, 199, 174]                                       # overlap with gt 0: 75 / 100
    bbox[5, 0] = [100, 100, 199, 194]; score[5, 0] = 0.9                    # 0.95, and the best score of the class
    bbox[2, 1] = [100, 300, 199, 399]
    return bbox, gt, score


def _filler(F_, C):
    bbox = np.zeros((F_, C, 4), F32)
    f = np.arange(F_)
    for c in range(C):
        bbox[:, c] = np.stack([2000 + 40 * f, np.full(F_, 50 * c), 2009 + 40 * f, np.full(F_, 50 * c + 9)], 1)     # disjoint, far from every gt
    return bbox, np.tile(np.linspace(0.6, 0.05, F_).astype(F32)[:, None], (1, C))


def _last_row(F_):
    """Class 1: the only box on the gt is row F - 1, the row with the lowest score of the last wavefront.  Class 2: exact copies of the gt in
    rows 63 and 64 -- the last lane of one wavefront and the first of the next -- with EQUAL scores: argmax takes the first, row 63."""
    bbox, score = _filler(F_, 2)
    gt = np.array([[100, 100, 199, 199, 1], [100, 300, 199, 399, 2]], F32)
    bbox[F_ - 1, 0] = gt[0, :4]
    bbox[63, 1] = bbox[64, 1] = gt[1, :4]
    score[64, 1] = score[63, 1]
    return bbox, gt, score


def nmt_case(name):
    """-> dict(bbox [B, F, C, 4], gt [B, Gmax, 5], num_gt [B], score [B, F, C], thresh)."""
    c = dict(NMT_CASES[name])
    F_, C, B = c['F'], c['C'], len(c['G'])
    seed = 700 + 10 * sorted(NMT_CASES).index(name)
    bbox, score, gts = np.zeros((B, F_, C, 4), F32), np.zeros((B, F_, C), F32), []
    for b in range(B):
        if c.get('by_hand') == 'row0_quirk':
            bb, g, sc = _row0_quirk()
            if b == 1:                                                      # the second image: the two gts of class 1 swapped
                g = g[[1, 0, 2]]
        elif c.get('by_hand') == 'last_row':
            bb, g, sc = _last_row(F_)
            if b == 1:                                                      # the second image: the class-2 gt alone
                g = g[[1, 0]]
        else:
            bb, g, sc = cases.nms_target_case(F_, C, max(c['G'][b], 1), seed + b)
            g = g[0]
            if c.get('one_class'):
                g[:, 4] = 1
            if F_ < 8:                                                      # too few boxes for a random one to hit: row 0 sits on the first gt of its class
                for k in range(C):
                    m = np.flatnonzero(g[:, 4] == k + 1)
                    if len(m):
                        bb[0, k] = g[m[0], :4] + F32(1.5)
        bbox[b], score[b] = bb, sc
        gts.append(g[:c['G'][b]])
    gt, num_gt = _pad_gt(gts, fill=np.append(bbox[0, 0, 0], 1))             # unused slots: a class-1 gt ON a box
    c.update(name=name, bbox=bbox, gt=gt, num_gt=num_gt, score=score, thresh=THRESH[c['T']], B=B)
    return c


def nmt_expected(c, b):
    G = int(c['num_gt'][b])
    if G == 0:                                                              # no gt: the class loop of nms_multi_target.py:45-49 skips every class
        return np.zeros((c['F'], c['C'], c['T']), F32)
    return OT.nms_multi_target(c['bbox'][b], c['gt'][b, :G][None], c['score'][b], c['thresh'])


# =====================================================================================================================
# relnet_bbox_overlaps
# =====================================================================================================================
OVERLAP_CASES = {'255': (15, 17), '256': (16, 16), '257': (257, 1), '257_wide': (1, 257), 'N0': (0, 5), 'K0': (5, 0)}
# rows 0.. of `boxes` against rows 0.. of `query` by hand: touching (iw = 0 after the +1), one shared pixel row (ih = 1), identical, x2 < x1
_OV_BOXES = [[0, 0, 9, 9], [0, 0, 9, 9], [3, 4, 50, 60], [10, 10, 5, 20]]
_OV_QUERY = [[10, 0, 19, 9], [0, 9, 9, 18], [3, 4, 50, 60], [0, 0, 30, 30]]


def overlap_case(name):
    """-> boxes [N, 4], query [K, 4] float64 (float32-representable values, as every caller passes)."""
    N, K = OVERLAP_CASES[name]
    boxes = cases.random_boxes(N, 800 + N, im_h=200, im_w=300, max_size=150).astype(np.float64)
    query = cases.random_boxes(K, 900 + K, im_h=200, im_w=300, max_size=150).astype(np.float64)
    nb, nq = min(N, len(_OV_BOXES)), min(K, len(_OV_QUERY))
    if nb:
        boxes[:nb] = _OV_BOXES[:nb]
    if nq:
        query[:nq] = _OV_QUERY[:nq]
    return boxes, query


def overlap_expected(boxes, query):
    with np.errstate(divide='ignore', invalid='ignore'):
        return OB.bbox_overlaps(boxes, query)


# =====================================================================================================================
# relnet_proposal_decode
# =====================================================================================================================
# map (H, W), anchors, im_info rows (h, w, scale), the explicit im_hw (None: read from im_info), min_size and the operand layout:
#   contiguous     plain NCHW
#   mixed_views    cls_prob a channels-last permute, bbox_deltas a slice of a larger tensor in all four dimensions
# Raw scores lie on the grid of SCORE_GRID = 2^-10 inside +-30 (the bf16 trunk's scores are coarser still), where the float32 difference
# bg - fg is EXACT -- what the bound on the two-way softmax (tests/test_gpu_target_edges.py) assumes.  The two float32_scores cases take
# unrounded float32 scores; there the float32 softmax (SoftmaxActivation, oracle/network.py:rpn_softmax, the kernel) first rounds
# bg - max and fg - max, and is held to the float64 softmax of THOSE differences (decode_expected(f32_gap=True)).
SCORE_GRID = 2.0 ** -10
_D12 = dict(scales=DEFAULT_SCALES, ratios=DEFAULT_RATIOS)
DECODE_CASES = {
    'a12': dict(_D12, map=(13, 21), info=[(208, 336, 1.0)], im_hw=None, min_size=16),
    'a12_no_filter': dict(_D12, map=(13, 21), info=[(208, 336, 1.0), (208, 336, 1.0)], im_hw=None, min_size=0),
    'a1': dict(scales=(8,), ratios=(1,), map=(13, 21), info=[(208, 336, 1.0)], im_hw=None, min_size=16),
    'a3': dict(scales=(8,), ratios=DEFAULT_RATIOS, map=(13, 21), info=[(208, 336, 1.0)], im_hw=None, min_size=16),
    'n255': dict(scales=(4,), ratios=DEFAULT_RATIOS, map=(5, 17), info=[(80, 272, 1.0)], im_hw=None, min_size=8),
    'n256': dict(scales=(2, 4), ratios=(1, 2), map=(8, 8), info=[(128, 128, 1.0)], im_hw=None, min_size=8),
    'n257': dict(scales=(4,), ratios=(1,), map=(1, 257), info=[(16, 4112, 1.0)], im_hw=None, min_size=8),
    'cropped': dict(_D12, map=(13, 21), info=[(150, 280, 1.0)], im_hw=(150, 280), min_size=8),                  # h = 9, w = 17 with the map's strides
    'strided': dict(_D12, map=(13, 21), info=[(208, 336, 1.0), (200, 330, 1.0)], im_hw=(208, 336), min_size=16, layout='mixed_views'),
    'strided_cropped': dict(_D12, map=(13, 21), info=[(150, 280, 1.0), (150, 280, 1.0)], im_hw=None, min_size=16, layout='mixed_views'),
    'batch_infos': dict(_D12, map=(13, 21), info=[(208, 336, 1.0), (150, 300, 1.5), (100, 200, 0.6)], im_hw=(208, 336), min_size=16),
    'scale_min_size': dict(_D12, map=(13, 21), info=[(208, 336, 1.5), (208, 336, 0.6)], im_hw=(208, 336), min_size=16),
    'all_filtered': dict(_D12, map=(13, 21), info=[(208, 336, 1.0), (208, 336, 2.0)], im_hw=(208, 336), min_size=400),
    # raw score pairs far apart (|bg - fg| up to 60): the softmax of the trained RPN's confident anchors
    'wide_logits': dict(_D12, map=(13, 21), info=[(208, 336, 1.0)], im_hw=None, min_size=16, score_sigma=12.0),
    'float32_scores': dict(_D12, map=(13, 21), info=[(208, 336, 1.0), (208, 336, 1.0)], im_hw=None, min_size=16, score_grid=None),
    'float32_scores_wide': dict(_D12, map=(13, 21), info=[(208, 336, 1.0)], im_hw=None, min_size=16, score_sigma=12.0, score_grid=None),
}
DECODE_STRIDE = 16


def decode_case(name):
    """-> dict(cls [B, 2A, H, W], deltas [B, 4A, H, W] float32, im_info [B, 3], base [A, 4] float64, h, w (the cropped grid), im_hw, min_size,
    layout, stride)."""
    c = dict(DECODE_CASES[name])
    rng = np.random.default_rng(1000 + sorted(DECODE_CASES).index(name))
    base = OB.generate_anchors(DECODE_STRIDE, c['ratios'], c['scales']).astype(np.float64)
    A, (H, W), B = base.shape[0], c['map'], len(c['info'])
    cls = np.clip(rng.normal(0, c.get('score_sigma', 2.0), (B, 2 * A, H, W)), -30, 30)
    grid = c.get('score_grid', SCORE_GRID)
    cls = (cls if grid is None else np.round(cls / grid) * grid).astype(F32)
    deltas = rng.normal(0, 0.5, (B, 4 * A, H, W)).astype(F32)
    im_info = np.array(c['info'], F32)
    hw = c['im_hw'] if c['im_hw'] is not None else c['info'][0][:2]
    h, w = min(int(hw[0] / DECODE_STRIDE), H), min(int(hw[1] / DECODE_STRIDE), W)           # proposal.py:85, ops.proposal_decode
    c.update(name=name, cls=cls, deltas=deltas, im_info=im_info, base=base, A=A, B=B, h=h, w=w, n=h * w * A, stride=DECODE_STRIDE,
             layout=c.get('layout', 'contiguous'), score_grid=grid)
    return c


def decode_expected(cls, deltas, im_info, base, stride, min_size, h, w, softmax_pairs, f32_gap=False):
    """-> boxes [B, n, 4] float32, scores [B, n] float64 (-inf where filtered), n = h w A in (y, x, a) order over the cropped grid.
    proposal.py:75-135: boxes = clip_boxes(bbox_pred(anchors, deltas), im_info[b, :2]) cast to float32; scores = the fg channel, or the
    two-way softmax of (bg, fg) = channels (a, A + a) in float64; -inf where width or height < min_size * im_info[b, 2].
    f32_gap: the differences bg - max and fg - max are taken in float32, as every float32 softmax takes them; all else in float64."""
    B, A = cls.shape[0], base.shape[0]
    anchors = shifted_anchors(h, w, stride, base)
    boxes, scores = np.zeros((B, h * w * A, 4), F32), np.zeros((B, h * w * A), np.float64)
    for b in range(B):
        d = deltas[b, :, :h, :w].transpose(1, 2, 0).reshape(-1, 4)
        p = OB.clip_boxes(OB.bbox_pred(anchors, d), im_info[b, :2].astype(np.float64))
        fg = cls[b, A:, :h, :w].transpose(1, 2, 0).reshape(-1).astype(np.float64)
        if softmax_pairs:
            bg = cls[b, :A, :h, :w].transpose(1, 2, 0).reshape(-1).astype(np.float64)
            m = np.maximum(bg, fg)
            db, df = bg - m, fg - m
            if f32_gap:
                db, df = (bg.astype(F32) - m.astype(F32)).astype(np.float64), (fg.astype(F32) - m.astype(F32)).astype(np.float64)
            fg = np.exp(df) / (np.exp(db) + np.exp(df))
        ms = float(min_size) * float(im_info[b, 2])
        ok = (p[:, 2] - p[:, 0] + 1 >= ms) & (p[:, 3] - p[:, 1] + 1 >= ms)
        boxes[b] = p.astype(F32)
        scores[b] = np.where(ok, fg, -np.inf)
    return boxes, scores
