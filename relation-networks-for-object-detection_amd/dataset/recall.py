"""Proposal recall of `lib/dataset/imdb.py:274-370` (`evaluate_recall`) in numpy, with its result as arrays as well as the log.

Every quirk of the reference is kept, because what it prints is the contract:

  * candidate areas (x2 - x1 + 1) * (y2 - y1 + 1) are taken in the candidates' own dtype (float32 for a `_rpn.pkl` list) and
    counted per half-open range [lo, hi) over the six ranges after 'all';
  * a ground-truth row counts when gt_classes > 0 and its gt_overlaps row has max 1; its area is taken in the roidb's box dtype,
    so the uint16 boxes of a coco roidb wrap areas above 65535 modulo 65536 before the range test.  The IoU itself runs on
    boxes.astype(float64);
  * num_pos counts the valid ground truth of every image, also of images without candidates, which are otherwise skipped;
  * the greedy cover runs min(P, G) rounds.  Each round takes the global maximum overlap: on ties the LOWEST gt index whose
    column maximum equals it, then the LOWEST proposal index of that column; the value is recorded and that row and column set
    to -1.  With P < G the entries of the unfilled rounds stay 0 and are counted as 0;
  * recall(t) = (gt_overlaps >= t).sum() / float(num_pos) (nan when num_pos is 0) and ar = recalls.mean().

The cover below keeps the column maxima of the reference's matrix instead of recomputing them every round: removing proposal p
only changes the columns whose first maximum was p, so those alone are rescanned.  The chosen (gt, proposal) pairs are the
reference's.  Boxes with NaN coordinates are outside this contract (csrc/recall.hip orders NaN differently from numpy's argmax).
"""
import numpy as np

AREA_NAMES = ['all', '0-25', '25-50', '50-100', '100-200', '200-300', '300-inf']
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 25 ** 2], [25 ** 2, 50 ** 2], [50 ** 2, 100 ** 2],
               [100 ** 2, 200 ** 2], [200 ** 2, 300 ** 2], [300 ** 2, 1e5 ** 2]]


def default_thresholds():
    return np.arange(0.5, 0.95 + 1e-5, 0.05)


def bbox_overlaps(boxes, query_boxes):
    """float64 [N, K] IoU in `lib/bbox/bbox.pyx:15-55`'s order of operations: iw = min(x2) - max(x1) + 1, ih only where iw > 0,
    ua = box_area + query_area - iw * ih, result iw * ih / ua (0 where iw or ih <= 0)."""
    b = np.asarray(boxes, np.float64)
    q = np.asarray(query_boxes, np.float64)
    ov = np.zeros((b.shape[0], q.shape[0]), np.float64)
    if ov.size == 0:
        return ov
    q_area = (q[:, 2] - q[:, 0] + 1) * (q[:, 3] - q[:, 1] + 1)
    b_area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    with np.errstate(invalid='ignore', over='ignore'):
        iw = np.minimum(b[:, None, 2], q[None, :, 2]) - np.maximum(b[:, None, 0], q[None, :, 0]) + 1
        ih = np.minimum(b[:, None, 3], q[None, :, 3]) - np.maximum(b[:, None, 1], q[None, :, 1]) + 1
    n, k = np.nonzero((iw > 0) & (ih > 0))
    inter = iw[n, k] * ih[n, k]
    ua = b_area[n] + q_area[k] - inter
    ov[n, k] = inter / ua
    return ov


def candidates_of(roidb, i, candidate_boxes):
    """The candidate rows of image i: candidate_boxes[i], or the roidb's non-gt rows (gt_classes == 0) when it is None."""
    if candidate_boxes is None:
        return roidb[i]['boxes'][np.where(roidb[i]['gt_classes'] == 0)[0], :]
    return candidate_boxes[i]


def valid_gt(rec):
    """Ground-truth rows of one roidb record that evaluate_recall scores (gt_classes > 0, overlap row max == 1), roidb dtype."""
    max_gt_overlaps = rec['gt_overlaps'].max(axis=1)
    return rec['boxes'][np.where((rec['gt_classes'] > 0) & (max_gt_overlaps == 1))[0], :]


def area_masks(boxes):
    """bool [len(AREA_RANGES), n]: box area in [lo, hi), the area taken in the boxes' own dtype."""
    areas = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    return np.stack([(areas >= lo) & (areas < hi) for lo, hi in AREA_RANGES]) if len(boxes) else \
        np.zeros((len(AREA_RANGES), 0), bool)


def greedy_cover(overlaps):
    """The reference's greedy loop on one [P, G] overlap matrix -> float64 [G]: the value recorded in round j at j, 0 after
    round min(P, G).  `overlaps` is modified."""
    P, G = overlaps.shape
    rec = np.zeros(G)
    rounds = min(P, G)
    if rounds == 0:
        return rec
    cols = np.arange(G)
    best_p = overlaps.argmax(axis=0)
    best_v = overlaps[best_p, cols]
    for j in range(rounds):
        gt_ind = best_v.argmax()
        box_ind = best_p[gt_ind]
        rec[j] = overlaps[box_ind, gt_ind]
        overlaps[box_ind, :] = -1
        overlaps[:, gt_ind] = -1
        best_v[gt_ind] = -1
        stale = np.nonzero((best_p == box_ind) & (cols != gt_ind) & (best_v != -1))[0]
        if len(stale):
            best_p[stale] = overlaps[:, stale].argmax(axis=0)
            best_v[stale] = overlaps[best_p[stale], stale]
    return rec


def recall_from_hits(hits, num_pos, thresholds):
    """recalls[i] = hits[i] / float(num_pos) in the reference's expression and dtype (np.zeros_like(thresholds)), ar = mean."""
    recalls = np.zeros_like(thresholds)
    for i in range(len(thresholds)):
        recalls[i] = hits[i] / float(num_pos)
    return recalls, recalls.mean()


def format_log(result):
    """The all_log_info string of evaluate_recall from a result dict (host or device)."""
    all_log_info = ''
    area_counts = [int(c) for c in result['area_counts']]
    total_counts = float(sum(area_counts))
    for area_name, area_count in zip(AREA_NAMES[1:], area_counts):
        all_log_info += 'percentage of {} {}'.format(area_name, area_count / total_counts)
    all_log_info += 'average number of proposal {}'.format(total_counts / result['num_images'])
    for r in result['ranges']:
        all_log_info += 'average recall for {}: {:.3f}'.format(r['name'], r['ar'])
        for threshold, recall in zip(result['thresholds'], r['recalls']):
            all_log_info += 'recall @{:.2f}: {:.3f}'.format(threshold, recall)
    return all_log_info


def evaluate_recall(roidb, num_images, candidate_boxes=None, thresholds=None):
    """-> (all_log_info, result).  result: thresholds, num_images, area_counts [6] (python ints), image_overlaps float64
    [num_images, 7, gt_cap] (image i's recorded values per range in round order, zeros where nothing was recorded), and
    `ranges`: per area range dict(name, range, gt_overlaps (sorted float64), recalls, ar, num_pos, hits int64 [T])."""
    if thresholds is None:
        thresholds = default_thresholds()
    area_counts = [0] * (len(AREA_RANGES) - 1)
    for i in range(num_images):
        boxes = candidates_of(roidb, i, candidate_boxes)
        inside = area_masks(boxes[:, :4])
        for a in range(1, len(AREA_RANGES)):
            area_counts[a - 1] += int(inside[a].sum())
    gts = [valid_gt(roidb[i]) for i in range(num_images)]
    gt_cap = max([len(g) for g in gts] + [0])
    image_overlaps = np.zeros((num_images, len(AREA_RANGES), gt_cap))
    parts = [[] for _ in AREA_RANGES]
    num_pos = [0] * len(AREA_RANGES)
    for i in range(num_images):
        gt_boxes = gts[i]
        inside = area_masks(gt_boxes)
        for a in range(len(AREA_RANGES)):
            num_pos[a] += int(inside[a].sum())
        boxes = candidates_of(roidb, i, candidate_boxes)
        if boxes.shape[0] == 0:
            continue
        ov_all = bbox_overlaps(boxes[:, :4].astype(np.float64), gt_boxes.astype(np.float64))
        for a in range(len(AREA_RANGES)):
            rec = greedy_cover(ov_all[:, inside[a]])
            image_overlaps[i, a, :len(rec)] = rec
            parts[a].append(rec)
    ranges = []
    for a, (name, rng) in enumerate(zip(AREA_NAMES, AREA_RANGES)):
        gt_overlaps = np.sort(np.concatenate([np.zeros(0)] + parts[a]))
        hits = np.array([(gt_overlaps >= t).sum() for t in thresholds], np.int64)
        with np.errstate(invalid='ignore', divide='ignore'):
            recalls, ar = recall_from_hits(hits, num_pos[a], thresholds)
        ranges.append(dict(name=name, range=rng, gt_overlaps=gt_overlaps, recalls=recalls, ar=ar, num_pos=num_pos[a], hits=hits))
    result = dict(thresholds=thresholds, num_images=num_images, area_counts=area_counts, image_overlaps=image_overlaps,
                  ranges=ranges)
    return format_log(result), result
