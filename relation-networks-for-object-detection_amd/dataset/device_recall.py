"""Proposal recall on the device: dataset/recall.py (the reference's `imdb.evaluate_recall`) as one HIP launch per batch
(csrc/recall.hip), bit-identical to it.

The valid ground truth is packed once into a CSR table over images, roidb order kept, with one area-range bitmask per box
computed here on the host in the roidb's own dtype (coco's uint16 areas wrap as they do in the reference).  `add` covers one
batch of candidate lists on the current stream without a host synchronisation; the kernel accumulates integer counts, so the
batching cannot change them.  `summarize` turns the counts into recalls and AR with recall.py's own numpy expressions and
returns the same log string.  Every image has to be added exactly once before `summarize`.
"""
import numpy as np
import torch

from .. import ops
from . import recall as R


def pack_ground_truth(roidb, num_images):
    """-> dict(gt_off int32 [num_images + 1], gt_box float64 [n, 4], gt_mask uint8 [n] (bit a: area in AREA_RANGES[a]),
    gt_cap = most valid gts of one image)."""
    boxes, masks, counts = [], [], []
    for i in range(num_images):
        gt = R.valid_gt(roidb[i])
        inside = R.area_masks(gt)
        bits = np.zeros(len(gt), np.uint8)
        for a in range(len(R.AREA_RANGES)):
            bits |= (inside[a].astype(np.uint8) << a)
        boxes.append(gt.astype(np.float64).reshape(-1, 4))
        masks.append(bits)
        counts.append(len(gt))
    gt_cap = max(counts + [0])
    if gt_cap > ops.RECALL_MAX_GT:
        raise ValueError("an image has %d valid ground-truth boxes; the device recall takes at most %d" % (gt_cap, ops.RECALL_MAX_GT))
    return dict(gt_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                gt_box=np.concatenate(boxes + [np.zeros((0, 4))]).astype(np.float64),
                gt_mask=np.concatenate(masks + [np.zeros(0, np.uint8)]), gt_cap=gt_cap)


def pack_candidates(candidate_list):
    """Per image float32 [n, 4+] arrays -> (boxes float32 [N, P, 4], num_valid int32 [N]).  Non-empty lists must be float32:
    the reference takes candidate areas in the candidates' own dtype and the kernel in float32."""
    for c in candidate_list:
        if len(c) and c.dtype != np.float32:
            raise ValueError("candidate boxes must be float32 (the _rpn.pkl format), got %s" % c.dtype)
    P = max([len(c) for c in candidate_list] + [1])
    if P > ops.RECALL_MAX_CANDIDATES:
        raise ValueError("an image has %d candidates; the device recall takes at most %d" % (P, ops.RECALL_MAX_CANDIDATES))
    boxes = np.zeros((len(candidate_list), P, 4), np.float32)
    num = np.zeros(len(candidate_list), np.int32)
    for k, c in enumerate(candidate_list):
        if len(c):
            boxes[k, :len(c)] = c[:, :4]
            num[k] = len(c)
    return boxes, num


class DeviceRecall(object):
    """Device twin of IMDB.evaluate_recall.  DeviceRecall(imdb or roidb): an imdb contributes gt_roidb() and num_images, a roidb
    list its length.  thresholds: as evaluate_recall's (None: 0.50:0.95).  record_overlaps: also keep every image's recorded
    values, so that summarize() can return the sorted gt_overlaps arrays as well."""

    def __init__(self, imdb_or_roidb, thresholds=None, device='cuda', record_overlaps=False):
        if isinstance(imdb_or_roidb, (list, tuple)):
            roidb, n = imdb_or_roidb, len(imdb_or_roidb)
        else:
            roidb, n = imdb_or_roidb.gt_roidb(), imdb_or_roidb.num_images
        if n <= 0:
            raise ValueError("nothing to evaluate: 0 images")
        self.num_images, self.device = n, device
        self.thresholds = R.default_thresholds() if thresholds is None else thresholds
        thr = np.asarray(self.thresholds, np.float64).reshape(-1)
        if not 0 < len(thr) <= ops.RECALL_MAX_THRESHOLDS:
            raise ValueError("1..%d thresholds, got %d" % (ops.RECALL_MAX_THRESHOLDS, len(thr)))
        gt = pack_ground_truth(roidb, n)
        dev = lambda a: torch.as_tensor(a).to(device)
        A, T = len(R.AREA_RANGES), len(thr)
        self.gt_cap = gt['gt_cap']
        self._gt_off_host, self._gt_mask_host = gt['gt_off'], gt['gt_mask']
        self.gt_off, self.gt_box, self.gt_mask = dev(gt['gt_off']), dev(gt['gt_box']), dev(gt['gt_mask'])
        self.thr = dev(thr)
        self.area_rng = dev(np.asarray(R.AREA_RANGES, np.float64))
        self.hits = torch.zeros((A, T), device=device, dtype=torch.int64)
        self.num_pos = torch.zeros((A,), device=device, dtype=torch.int64)
        self.area_count = torch.zeros((A - 1,), device=device, dtype=torch.int64)
        self.n_cand = torch.zeros((n,), device=device, dtype=torch.int32)
        self.added = torch.zeros((n,), device=device, dtype=torch.int32)
        self.overlaps = torch.zeros((n, A, self.gt_cap), device=device, dtype=torch.float64) if record_overlaps else None

    @classmethod
    def from_lists(cls, roidb, candidate_boxes=None, thresholds=None, device='cuda', record_overlaps=False, chunk=256):
        """The analogue of evaluate_recall(roidb, candidate_boxes, thresholds) over len(roidb) images: candidate_boxes is a
        per-image list of float32 [n, 4+] arrays, None takes the roidb's non-gt rows."""
        self = cls(list(roidb), thresholds, device, record_overlaps)
        cands = [R.candidates_of(roidb, i, candidate_boxes) for i in range(self.num_images)]
        for lo in range(0, self.num_images, chunk):
            boxes, num = pack_candidates(cands[lo:lo + chunk])
            self.add(torch.as_tensor(boxes).to(device), torch.as_tensor(num).to(device), np.arange(lo, lo + len(num)))
        return self

    def add(self, boxes, num_boxes, image_positions, scores=None, thresh=0.0, scale=None):
        """boxes [B, P, 4] float32 on the device (e.g. rois[:, :, 1:]), num_boxes [B] (None: all P), image_positions [B] (host
        positions are checked and uploaded from pinned memory without blocking).  scores [B, P] with thresh: keep score > thresh
        as tester.generate_proposals does; scale [B] (im_info[:, 2]): boxes / scale in float32 first."""
        if boxes.dim() != 3 or boxes.shape[2] != 4:
            raise ValueError("boxes must be [B, P, 4], got %s" % (tuple(boxes.shape),))
        B, P = boxes.shape[:2]
        if P > ops.RECALL_MAX_CANDIDATES:
            raise ValueError("%d candidates per image; the device recall takes at most %d" % (P, ops.RECALL_MAX_CANDIDATES))
        if not torch.is_tensor(image_positions) or not image_positions.is_cuda:
            pos = np.asarray(image_positions.cpu() if torch.is_tensor(image_positions) else image_positions, np.int64).reshape(-1)
            if len(pos) != B or len(set(pos.tolist())) != B or (pos < 0).any() or (pos >= self.num_images).any():
                raise ValueError("image positions must be %d distinct values in 0..%d" % (B, self.num_images - 1))
            image_positions = torch.as_tensor(pos.astype(np.int32)).pin_memory().to(boxes.device, non_blocking=True)
        if boxes.stride(2) != 1:
            boxes = boxes.contiguous()
        i32 = lambda t: None if t is None else t.to(torch.int32).reshape(-1)
        f32 = lambda t: None if t is None else t.to(torch.float32).reshape(-1).contiguous()
        ops.recall_match(boxes, i32(image_positions), self.gt_off, self.gt_box, self.gt_mask, self.thr,
                         self.area_rng, self.hits, self.num_pos, self.area_count, self.n_cand, self.added, self.gt_cap,
                         num_valid=i32(num_boxes), scores=f32(scores), thresh=float(np.float32(thresh)), scale=f32(scale),
                         overlaps=self.overlaps)

    def summarize(self):
        """-> (all_log_info, result) as dataset/recall.py:evaluate_recall returns them.  Without record_overlaps the result's
        gt_overlaps are None and image_overlaps is absent."""
        added = self.added.cpu().numpy()
        if (added != 1).any():
            bad = np.nonzero(added != 1)[0]
            raise ValueError("every image must be added exactly once: image %d was added %d times" % (bad[0], added[bad[0]]))
        hits, num_pos = self.hits.cpu().numpy(), self.num_pos.cpu().numpy()
        area_counts = [int(c) for c in self.area_count.cpu().numpy()]
        image_overlaps, covered = None, None
        if self.overlaps is not None:
            image_overlaps = self.overlaps.cpu().numpy()
            covered = self.n_cand.cpu().numpy() > 0
        ranges = []
        for a, (name, rng) in enumerate(zip(R.AREA_NAMES, R.AREA_RANGES)):
            gt_overlaps = None
            if image_overlaps is not None:
                off, bit = self._gt_off_host, (self._gt_mask_host >> a) & 1
                parts = [image_overlaps[i, a, :int(bit[off[i]:off[i + 1]].sum())] for i in np.nonzero(covered)[0]]
                gt_overlaps = np.sort(np.concatenate([np.zeros(0)] + parts))
            with np.errstate(invalid='ignore', divide='ignore'):
                recalls, ar = R.recall_from_hits(hits[a], int(num_pos[a]), self.thresholds)
            ranges.append(dict(name=name, range=rng, gt_overlaps=gt_overlaps, recalls=recalls, ar=ar, num_pos=int(num_pos[a]),
                               hits=hits[a].copy()))
        result = dict(thresholds=self.thresholds, num_images=self.num_images, area_counts=area_counts, ranges=ranges)
        if image_overlaps is not None:
            result['image_overlaps'] = image_overlaps
        return R.format_log(result), result
