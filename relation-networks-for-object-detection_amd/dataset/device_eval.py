"""COCO bbox evaluation on the device: dataset/cocoeval.py's matching and accumulation as two HIP launches
(csrc/cocoeval.hip), bit-identical to it.

The ground truth is packed once into a CSR table over (image position, category position), annotation order kept inside each
cell, with `ignore` / `iscrowd` and the area ranges folded into one flag byte per box exactly as COCOeval folds them.
`add` matches one batch of the detector's device outputs against it and writes the batch images' detection slots
[n_images, S]; it launches on the current stream, makes no host synchronisation and can be captured.  `accumulate` sorts every slot
once by (category, -score) on the device and returns the same `eval` dict as `COCOeval.accumulate`; `summarize` is COCOeval's.
"""
import numpy as np
import torch

from .. import ops
from .cocoeval import COCOeval, Params

MAX_SLOTS = 2048          # detection slots per image (csrc/cocoeval.hip: kCocoMaxSlots)
MAX_PAIRS = 64            # area ranges x IoU thresholds


def pack_params(p):
    """Params -> float64 IoU thresholds [T], area ranges [A, 2], recall thresholds [R] and int32 maxDets [M], taken from the
    host arrays (the device never recomputes a linspace)."""
    iou = np.asarray(p.iouThrs, np.float64)
    area = np.asarray(p.areaRng, np.float64).reshape(-1, 2)
    rec = np.asarray(p.recThrs, np.float64)
    max_dets = np.asarray(p.maxDets, np.int32)
    if len(area) * len(iou) > MAX_PAIRS or len(area) > 7 or not 0 < len(max_dets) <= 4:
        raise ValueError("device evaluation handles at most %d (area, IoU) pairs, 7 area ranges and 4 maxDets" % MAX_PAIRS)
    if (np.diff(max_dets) < 0).any():
        raise ValueError("maxDets must be ascending, got %s" % list(p.maxDets))
    return iou, area, rec, max_dets


def pack_ground_truth(gts, img_ids, cat_ids, area_rng):
    """COCOeval's view of the ground truth as a CSR table.  gts: the dict list COCOeval takes; img_ids / cat_ids: the sorted
    evaluated ids.  -> dict(gt_off int32 [n_images * K + 1], gt_box float64 [n, 4] (x, y, w, h), gt_flags uint8 [n] (bit 0
    iscrowd, bit 1 + a: ignored in area range a), npig int64 [K, A], gt_cap = most boxes of one image)."""
    img_pos = {i: k for k, i in enumerate(img_ids)}
    cat_pos = {c: k for k, c in enumerate(cat_ids)}
    K, A = len(cat_ids), len(area_rng)
    cells, boxes, flags = [], [], []
    for i, g in enumerate(gts):
        ip, cp = img_pos.get(g['image_id']), cat_pos.get(g['category_id'])
        if ip is None or cp is None:
            continue
        if g.get('id', i + 1) == 0:
            raise ValueError("ground-truth id 0: COCOeval reads a match to it as no match")
        crowd = int(g.get('iscrowd', 0))
        area = g['area'] if 'area' in g else g['bbox'][2] * g['bbox'][3]
        ignore = int(g.get('ignore', 0) or crowd)
        f = 1 if crowd else 0
        for a, (lo, hi) in enumerate(area_rng):
            if ignore or area < lo or area > hi:
                f |= 2 << a
        cells.append(ip * K + cp)
        boxes.append(np.asarray(g['bbox'], np.float64).reshape(4))
        flags.append(f)
    cells = np.asarray(cells, np.int64)
    order = np.argsort(cells, kind='mergesort')                     # stable: annotation order inside a cell
    gt_box = np.asarray(boxes, np.float64).reshape(-1, 4)[order]
    gt_flags = np.asarray(flags, np.uint8)[order]
    counts = np.bincount(cells, minlength=len(img_ids) * K)
    gt_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    cat_of = cells[order] % K if len(cells) else np.zeros(0, np.int64)
    npig = np.zeros((K, A), np.int64)
    for a in range(A):
        np.add.at(npig[:, a], cat_of[(gt_flags & (2 << a)) == 0], 1)
    per_image = counts.reshape(len(img_ids), K).sum(1) if len(img_ids) else np.zeros(0, np.int64)
    return dict(gt_off=gt_off, gt_box=gt_box, gt_flags=gt_flags, npig=npig, gt_cap=int(per_image.max()) if per_image.size else 0)


def class_to_category(imdb):
    """Detector class index -> position of its COCO category id in sorted(cat_ids) (-1: background)."""
    cat_pos = {c: k for k, c in enumerate(sorted(imdb._coco_ind_to_class_ind))}
    table = np.full(imdb.num_classes, -1, np.int32)
    for c, cls in imdb._coco_ind_to_class_ind.items():
        table[cls] = cat_pos[c]
    return table


def pack_detections(dts, img_ids, cat_ids):
    """COCOeval's view of a detection dict list as the match kernel's input in (x, y, w, h) form: -> (det float64
    [n_images, S, 6] (category position, score, x, y, w, h), num_det int32 [n_images]), rows of an image in list order."""
    img_pos = {i: k for k, i in enumerate(img_ids)}
    cat_pos = {c: k for k, c in enumerate(cat_ids)}
    rows = [[] for _ in img_ids]
    for i, d in enumerate(dts):
        ip, cp = img_pos.get(d['image_id']), cat_pos.get(d['category_id'])
        if ip is None or cp is None:
            continue
        if d.get('id', i + 1) == 0:
            raise ValueError("detection id 0: COCOeval reads a match by it as no match")
        x, y, w, h = (float(v) for v in d['bbox'])
        if 'area' in d and d['area'] != w * h:
            raise ValueError("detection area %r is not bbox w * h (%r): the device evaluator derives it from the box" % (d['area'], w * h))
        rows[ip].append((cp, float(d['score']), x, y, w, h))
    S = max([len(r) for r in rows] + [1])
    if S > MAX_SLOTS:
        raise ValueError("an image has %d detections; the device evaluator takes at most %d per image" % (S, MAX_SLOTS))
    det = np.zeros((len(img_ids), S, 6), np.float64)
    num = np.zeros(len(img_ids), np.int32)
    for k, r in enumerate(rows):
        if r:
            det[k, :len(r)] = r
            num[k] = len(r)
    return det, num


class DeviceCOCOeval(object):
    """Device twin of COCOeval.  DeviceCOCOeval(imdb, slots) scores the detector's outputs against a `coco` imdb's ground
    truth (all annotations, image_set_index, every category; detections as pred_eval reports them: rounded to float32, boxes
    (x1, y1, x2, y2) with w = x2 - x1 + 1).  `slots`: detection rows per image that `add` will be given (<= MAX_SLOTS)."""

    _summarize = COCOeval._summarize
    summarize = COCOeval.summarize

    def __init__(self, imdb, slots=128, device='cuda'):
        gts = [a for anns in imdb._anns.values() for a in anns]         # the list evaluate_detections hands to COCOeval
        self._setup(gts, imdb.image_set_index, sorted(imdb._coco_ind_to_class_ind), class_to_category(imdb), slots, device,
                    round_f32=True, box_xywh=False)

    @classmethod
    def from_lists(cls, gts, dts, img_ids=None, cat_ids=None, device='cuda', slots=None, chunk=1024):
        """The dict lists COCOeval takes; the detections are added at once.  slots: room for more rows per image than `dts`
        has (for later `add` calls)."""
        if img_ids is None:
            img_ids = {g['image_id'] for g in gts} | {d['image_id'] for d in dts}
        if cat_ids is None:
            cat_ids = {g['category_id'] for g in gts} | {d['category_id'] for d in dts}
        img_ids, cat_ids = sorted(img_ids), sorted(cat_ids)
        det, num = pack_detections(dts, img_ids, cat_ids)
        self = cls.__new__(cls)
        self._setup(gts, img_ids, cat_ids, np.arange(len(cat_ids), dtype=np.int32), max(det.shape[1], slots or 0), device,
                    round_f32=False, box_xywh=True)
        for lo in range(0, len(img_ids), chunk):
            n = num[lo:lo + chunk]
            s = max(int(n.max()), 1)
            self.add(torch.as_tensor(det[lo:lo + chunk, :s]).to(device), torch.as_tensor(n).to(device),
                     np.arange(lo, lo + len(n)))
        return self

    def _setup(self, gts, img_ids, cat_ids, class_to_cat, slots, device, round_f32, box_xywh):
        self.params = Params()
        self.img_ids, self.cat_ids = sorted(img_ids), sorted(cat_ids)
        if len(set(self.img_ids)) != len(self.img_ids) or len(set(self.cat_ids)) != len(self.cat_ids):
            raise ValueError("image and category ids must be distinct")
        if not self.img_ids or not self.cat_ids:
            raise ValueError("nothing to evaluate: %d images, %d categories" % (len(self.img_ids), len(self.cat_ids)))
        if not 0 < slots <= MAX_SLOTS:
            raise ValueError("slots per image must be in 1..%d, got %d" % (MAX_SLOTS, slots))
        iou, area, rec, max_dets = pack_params(self.params)
        gt = pack_ground_truth(gts, self.img_ids, self.cat_ids, area)
        dev = lambda a: torch.as_tensor(a).to(device)
        self.device, self.slots, self.round_f32, self.box_xywh = device, int(slots), round_f32, box_xywh
        self.gt_cap, self.max_det = gt['gt_cap'], int(max_dets[-1])
        self.iou_thr, self.area_rng, self.rec_thr, self.max_dets = dev(iou), dev(area), dev(rec), dev(max_dets)
        self.class_to_cat = dev(np.asarray(class_to_cat, np.int32))
        self.gt_off, self.gt_box, self.gt_flags, self.npig = dev(gt['gt_off']), dev(gt['gt_box']), dev(gt['gt_flags']), dev(gt['npig'])
        N, S, AT = len(self.img_ids), self.slots, len(iou) * len(area)
        self.slot_cat = torch.full((N, S), -1, device=device, dtype=torch.int32)
        self.slot_score = torch.zeros((N, S), device=device, dtype=torch.float64)
        self.slot_rank = torch.full((N, S), 2 ** 31 - 1, device=device, dtype=torch.int32)
        self.slot_code = torch.zeros((N, S, AT), device=device, dtype=torch.uint8)
        self.eval, self.stats = None, None

    def add(self, detections, num_detections, image_positions):
        """detections [B, D, 6] (class, score, box) float32 / float64 on the device, num_detections [B], image_positions [B]:
        the images' positions in `img_ids`.  Host positions are checked and uploaded from pinned memory without blocking;
        device positions must be distinct and in range (an out-of-range position is skipped).  Re-adding an image replaces its
        detections."""
        if detections.dim() != 3 or detections.shape[2] != 6:
            raise ValueError("detections must be [B, D, 6], got %s" % (tuple(detections.shape),))
        B, D = detections.shape[:2]
        if D > self.slots:
            raise ValueError("%d detection rows per image, the evaluator was built for %d" % (D, self.slots))
        if not torch.is_tensor(image_positions) or not image_positions.is_cuda:
            pos = np.asarray(image_positions.cpu() if torch.is_tensor(image_positions) else image_positions, np.int64).reshape(-1)
            if len(pos) != B or len(set(pos.tolist())) != B or (pos < 0).any() or (pos >= len(self.img_ids)).any():
                raise ValueError("image positions must be %d distinct values in 0..%d" % (B, len(self.img_ids) - 1))
            image_positions = torch.as_tensor(pos.astype(np.int32)).pin_memory().to(detections.device, non_blocking=True)
        ops.coco_match(detections.contiguous(), num_detections.to(torch.int32), image_positions.to(torch.int32),
                       self.class_to_cat, self.gt_off, self.gt_box, self.gt_flags, self.iou_thr, self.area_rng, self.slot_cat,
                       self.slot_score, self.slot_rank, self.slot_code, self.gt_cap, self.max_det, round_f32=self.round_f32,
                       box_xywh=self.box_xywh)

    def accumulate(self):
        """-> and self.eval: dict(precision [T,R,K,A,M], recall [T,K,A,M] float64 numpy, counts), as COCOeval.accumulate."""
        precision, recall = ops.coco_accumulate(self.slot_cat, self.slot_score, self.slot_rank, self.slot_code, self.npig,
                                                self.rec_thr, self.max_dets, self.max_det)
        T, R, K, A, M = precision.shape
        self.eval = dict(precision=precision.cpu().numpy(), recall=recall.cpu().numpy(), counts=[T, R, K, A, M])
        return self.eval
