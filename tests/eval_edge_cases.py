"""Cases for the COCO evaluation kernels (csrc/cocoeval.hip) and the proposal-recall kernel (csrc/recall.hip) at their capacity edges:
builders, plain float64 restatements and defect models.  numpy only, deterministic seeds, no device.

tests/test_eval_edge_cases_host.py checks on the CPU that every case reaches the edge it is named for, that the restatements equal
the package's definitions (dataset/cocoeval.py, dataset/recall.py) bit for bit, and that a numpy model of each plausible defect
changes the expected output.  tests/test_gpu_eval_edges.py compares the kernels with the definitions bit for bit on these cases.

The kernels' constants are written out below with the line of the source they come from; the host test parses the sources and
holds the table to them."""
import functools
import os

import numpy as np

from relnet_amd.dataset import cocoeval, recall as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'relation-networks-for-object-detection_amd', 'csrc')

# name -> (value, file, line)
CONSTANTS = {
    'kCocoMatchThreads': (1024, 'cocoeval.hip', 10),    # stride of the staging, rank and unit loops of coco_match_kernel
    'kCocoMaxSlots': (2048, 'cocoeval.hip', 11),        # detection rows / slots per image
    'kCocoMaxPairs': (64, 'cocoeval.hip', 12),          # A * T, the width of the accumulate workgroup
    'kCocoMaxDetsLen': (4, 'cocoeval.hip', 13),         # M
    'kCocoMaxAreas': (7, 'cocoeval.hip', 14),           # A: the ignore flag of range a is bit 1 + a of a uint8
    'kSortTile': (2048, 'cocoeval.hip', 15),            # slots per workgroup of one radix pass
    'kSortThreads': (256, 'cocoeval.hip', 16),          # = radix: one byte per pass, so a second category pass when K > 255
    'kRecallThreads': (256, 'recall.hip', 26),          # one lane per ground-truth box in a round's argmax: 4 waves
    'kRecallMaxCand': (2048, 'recall.hip', 28),
    'kRecallMaxGt': (256, 'recall.hip', 29),
    'kRecallMaxThr': (256, 'recall.hip', 30),
    'kRecallMaxAreas': (8, 'recall.hip', 31),
}
MATCH_THREADS, MAX_SLOTS, MAX_PAIRS, MAX_DETS_LEN, MAX_AREAS = 1024, 2048, 64, 4, 7
SORT_TILE, RADIX, SCAN_THREADS = 2048, 256, 1024        # coco_scan_kernel: __launch_bounds__(1024), per = ceil(len / 1024)
WAVE, RECALL_THREADS, RECALL_MAX_CAND, RECALL_MAX_GT, CAND_PER_THREAD = 64, 256, 2048, 256, 8
CODE_FP, CODE_TP, CODE_IGNORED = 0, 1, 2                # cocoeval.hip: enum { kCodeFP, kCodeTP, kCodeIgnored }
EMPTY_RANK = 2 ** 31 - 1


# ======================================================================================================================
# The synthetic problem of tests/test_gpu_device_eval.py (moved here unchanged so that the host test can measure it)
# ======================================================================================================================
def synthetic_problem(seed, n_images=24):
    """Crowd and ignored ground truth, areas exactly 32^2 / 96^2, scores tied inside and across images, images without ground
    truth or without detections, a category without detections, one whose ground truth is all ignored, one with nothing,
    150 detections in one (image, category) and 300 ground-truth boxes in another."""
    rng = np.random.default_rng(seed)
    cats = [2, 5, 9, 11, 13]                 # 9: no detections; 11: every box crowd or ignored; 13: nothing at all
    img_ids = [1000 + 3 * i for i in range(n_images)]
    gts, dts = [], []

    def box(scale):
        w, h = float(rng.uniform(0.5, 1.5) * scale), float(rng.uniform(0.5, 1.5) * scale)
        return [float(rng.uniform(0, 500)), float(rng.uniform(0, 400)), w, h]

    def det_near(b, img, cat):
        j = rng.normal(0, 0.12, 4)
        dts.append(dict(image_id=img, category_id=cat, score=float(np.round(rng.random(), 1)),
                        bbox=[b[0] + j[0] * b[2], b[1] + j[1] * b[3], b[2] * float(np.exp(j[2])), b[3] * float(np.exp(j[3]))]))

    for i, img in enumerate(img_ids):
        if i % 7 == 3:                       # no ground truth, detections only
            for _ in range(5):
                det_near(box(40), img, 2)
            continue
        for cat in (2, 5, 9, 11):
            for _ in range(int(rng.integers(0, 6))):
                b = box(float(np.exp(rng.uniform(np.log(10), np.log(200)))))
                gd = dict(image_id=img, category_id=cat, bbox=b)
                r = rng.random()
                if cat == 11:
                    gd['iscrowd' if r < 0.5 else 'ignore'] = 1
                elif r < 0.1:
                    gd['iscrowd'] = 1
                elif r < 0.2:
                    gd['ignore'] = 1
                elif r < 0.3:
                    gd['area'] = float(32 ** 2)
                elif r < 0.4:
                    gd['area'] = float(96 ** 2)
                gts.append(gd)
                if cat != 9 and i % 5 != 1:  # images i % 5 == 1: no detections
                    for _ in range(int(rng.integers(0, 4))):
                        det_near(b, img, cat)
            if cat != 9 and i % 5 != 1:
                for _ in range(int(rng.integers(0, 3))):
                    dts.append(dict(image_id=img, category_id=cat, score=float(np.round(rng.random() * 0.7, 1)), bbox=box(50)))
    # 150 detections in one (image, category): maxDets truncation at 100
    img = img_ids[2]
    base = [g for g in gts if g['image_id'] == img and g['category_id'] == 5 and not g.get('iscrowd') and not g.get('ignore')]
    for k in range(150):
        b = base[k % len(base)]['bbox'] if base and k % 3 == 0 else box(60)
        det_near(b, img, 5)
    # 300 ground-truth boxes in one (image, category)
    img = img_ids[4]
    for k in range(300):
        b = [float(10 * (k % 30)), float(12 * (k // 30)), float(rng.uniform(8, 40)), float(rng.uniform(8, 40))]
        gd = dict(image_id=img, category_id=2, bbox=b)
        if k % 17 == 0:
            gd['iscrowd'] = 1
        gts.append(gd)
        if k % 2 == 0:
            det_near(b, img, 2)
    for i, g in enumerate(gts):
        g['id'] = i + 1
    return gts, dts, img_ids, cats


# ======================================================================================================================
# COCO cases
# ======================================================================================================================
DEFAULT_AREA = cocoeval.Params().areaRng
AREA7 = [[0.0, 1e10], [0.0, 400.0], [400.0, 1600.0], [1600.0, 6400.0], [6400.0, 25600.0], [25600.0, 1e10], [100.0, 10000.0]]
AREA2 = [[0.0, 1e10], [0.0, 1024.0]]


def _side(lo, hi):
    """A box side whose square lies inside [lo, hi]."""
    a, b = np.sqrt(lo), min(np.sqrt(hi), np.sqrt(lo) + 120.0)
    return float(np.round(max(a + 0.4 * (b - a), 6.0) * 2) / 2)


class Case(dict):
    __getattr__ = dict.__getitem__


def make_case(name, seed, K, n_images, full=None, area=None, iou=None, max_dets=None, rec=None, slots=None, chunk=None,
              empty_cats=(), dets_per_gt=(1, 3), extra_fp=(0, 2), rows=None, tie_images=(), heavy=None, edge='', degenerate=False):
    """A problem in which every category except `empty_cats` has one regular ground-truth box inside every area range in each
    image of `full` (default: all), so that no (category, area) cell is without ground truth, and detections that are exact
    copies (IoU 1.0), jittered copies and strays, with scores on a 0.01 grid.  rows: {image index: number of detection rows},
    filled with strays of every category and ordered by ascending score, so that the last rows rank first.  tie_images: every
    detection of these images scores 0.5.  heavy: (image, category, n) adds n strays to one cell."""
    rng = np.random.default_rng(seed)
    area = DEFAULT_AREA if area is None else area
    full = list(range(n_images)) if full is None else list(full)
    img_ids = [10 + 7 * i for i in range(n_images)]
    cat_ids = [3 + 2 * k for k in range(K)]
    sides = [_side(lo, hi) for lo, hi in area]
    gts, dts_by_img = [], {i: [] for i in range(n_images)}
    for i in full:
        for k in range(K):
            if k in empty_cats:
                continue
            for a, s in enumerate(sides):
                x, y = float(rng.integers(0, 800)) / 2, float(rng.integers(0, 600)) / 2
                w, h = (s, s) if rng.random() < 0.5 else (s * 2, s / 2)
                gd = dict(image_id=img_ids[i], category_id=cat_ids[k], bbox=[x, y, w, h])
                r = rng.random()
                if i != full[0] and r < 0.08:
                    gd['iscrowd'] = 1
                elif i != full[0] and r < 0.16:
                    gd['ignore'] = 1
                elif r < 0.3:
                    gd['area'] = float(area[a][0] if area[a][0] > 0 else area[a][1])      # exactly on an area bound
                gts.append(gd)
                for _ in range(int(rng.integers(dets_per_gt[0], dets_per_gt[1] + 1))):
                    r = rng.random()
                    if r < 0.2:
                        bb = [x, y, w, h]                                                 # IoU exactly 1
                    elif r < 0.3:
                        bb = [x, y, w, h / 2]                                             # IoU exactly 0.5 (every term is exact)
                    elif r < 0.8:
                        j = np.round(rng.normal(0, 0.1, 4) * 8) / 8
                        bb = [x + j[0] * w, y + j[1] * h, w * (1 + j[2]), h * (1 + j[3])]
                    else:
                        bb = [x + 3 * w, y + 3 * h, w, h]
                    dts_by_img[i].append(dict(image_id=img_ids[i], category_id=cat_ids[k], bbox=[float(v) for v in bb],
                                              score=float(np.round(0.4 + 0.6 * rng.random(), 2))))
            for _ in range(int(rng.integers(extra_fp[0], extra_fp[1] + 1))):
                s = sides[int(rng.integers(0, len(sides)))]
                dts_by_img[i].append(dict(image_id=img_ids[i], category_id=cat_ids[k], score=float(np.round(0.7 * rng.random(), 2)),
                                          bbox=[float(rng.integers(0, 800)) / 2, float(rng.integers(0, 600)) / 2, s, s]))
    live = [k for k in range(K) if k not in empty_cats]
    if heavy:
        for _ in range(heavy[2]):
            dts_by_img[heavy[0]].append(dict(image_id=img_ids[heavy[0]], category_id=cat_ids[heavy[1]], score=float(np.round(0.9 * rng.random(), 2)),
                                             bbox=[float(rng.integers(0, 800)) / 2, float(rng.integers(0, 600)) / 2, sides[0], sides[0]]))
    for i, n in (rows or {}).items():
        d = dts_by_img[i]
        assert len(d) <= n, (name, i, len(d), n)
        while len(d) < n:
            k = live[len(d) % len(live)]
            s = sides[int(rng.integers(0, len(sides)))]
            d.append(dict(image_id=img_ids[i], category_id=cat_ids[k], score=float(np.round(0.6 * rng.random(), 2)),
                          bbox=[float(rng.integers(0, 800)) / 2, float(rng.integers(0, 600)) / 2, s, s * 1.5]))
        d.sort(key=lambda x: x['score'])                                                   # stable: the best rows come last
    for i in tie_images:
        for d in dts_by_img[i]:
            d['score'] = 0.5
    dts = [d for i in range(n_images) for d in dts_by_img[i]]
    for i, g in enumerate(gts):
        g['id'] = i + 1
    per_img = [len(dts_by_img[i]) for i in range(n_images)]
    return Case(name=name, gts=gts, dts=dts, img_ids=img_ids, cat_ids=cat_ids, area=area, iou=iou, max_dets=max_dets, rec=rec,
                slots=slots or max(per_img + [1]), chunk=chunk, edge=edge, degenerate=degenerate)


IOU8 = [0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95]
IOU9 = [0.25, 0.5, 0.5 + 2.0 ** -40, 0.75, 0.9, 1.0 - 1e-10, 1.0, 1.0 + 2.0 ** -52, 1.5]      # 1.0 and above: clamped to 1 - 1e-10
IOU16 = [float(v) for v in np.linspace(0.2, 0.95, 16)]
SMALL = dict(area=AREA2, iou=[0.5, 0.75], max_dets=[1, 10], rec=[float(v) for v in np.linspace(0, 1, 11)])

COCO_BUILDERS = {
    # ---- unit loop of coco_match_kernel: units = categories present in the image x A x T, stride 1024
    'units1200': lambda: make_case('units1200', 1, 30, 1, dets_per_gt=(1, 1), extra_fp=(0, 0), edge='30 categories x 40 pairs = 1200 units'),
    'units1024': lambda: make_case('units1024', 2, 32, 1, iou=IOU8, edge='32 categories x (A 4 x T 8) = 1024 units'),
    'units1056': lambda: make_case('units1056', 3, 33, 1, iou=IOU8, edge='33 categories x (A 4 x T 8) = 1056 units'),
    # ---- staging and rank loops: S_in at and around 1024 and the cap, the second image has 3 rows
    'rows1024': lambda: _rows_case(1024, 4),
    'rows1025': lambda: _rows_case(1025, 5),
    'rows2047': lambda: _rows_case(2047, 6),
    'rows2048': lambda: _rows_case(2048, 7),
    # ---- slots: tiles of the radix sort and words per thread of the scan
    'slots1': lambda: make_case('slots1', 8, 1, 1, dets_per_gt=(0, 0), extra_fp=(0, 0), rows={0: 1}, slots=1, edge='n_slots 1'),
    'slots2047': lambda: make_case('slots2047', 9, 3, 23, full=[0, 11, 22], slots=89, rows={0: 89, 22: 89}, edge='23 x 89 = 2047 slots: one tile, tail 2047'),
    'slots2048': lambda: make_case('slots2048', 10, 3, 16, full=[0, 7, 15], slots=128, rows={0: 128, 15: 128}, edge='16 x 128 = 2048 slots: one full tile'),
    'slots2049': lambda: make_case('slots2049', 11, 3, 3, slots=683, rows={2: 683}, edge='3 x 683 = 2049 slots: tile tail 1'),
    'slots9k': lambda: make_case('slots9k', 12, 3, 72, full=[0, 15, 16, 40, 71], slots=128, rows={15: 128, 16: 128, 71: 128}, tie_images=(15, 16),
                                 chunk=7, edge='72 x 128 = 9216 slots: 5 tiles, 2 words per scan thread; ties across the tile boundary of images 15 | 16'),
    'slots40k': lambda: make_case('slots40k', 13, 3, 320, full=[0, 15, 16, 17, 160, 319], slots=128, rows={15: 128, 16: 128, 319: 128},
                                  tie_images=(15, 16, 160), edge='320 x 128 = 40960 slots: 20 tiles, 5 words per scan thread'),
    # ---- second category pass of the sort: K at and past one byte
    'K255': lambda: make_case('K255', 14, 255, 2, empty_cats=(100,), heavy=(1, 7, 30), edge='K 255: the not-evaluated digit 255 fits one byte', **SMALL),
    'K256': lambda: make_case('K256', 15, 256, 2, empty_cats=(100,), heavy=(1, 7, 30), edge='K 256: second category pass', **SMALL),
    'K257': lambda: make_case('K257', 16, 257, 2, empty_cats=(100,), heavy=(1, 7, 30), edge='K 257: category 256 has digit (0, 1)', **SMALL),
    'K300': lambda: make_case('K300', 17, 300, 2, empty_cats=(100,), heavy=(1, 7, 30), edge='K 300', **SMALL),
    # ---- Params
    'maxdets1': lambda: make_case('maxdets1', 18, 3, 6, max_dets=[1], edge='M 1, maxDets [1]'),
    'maxdets1237': lambda: make_case('maxdets1237', 19, 3, 6, max_dets=[1, 2, 3, 7], dets_per_gt=(2, 4), edge='M 4, maxDets [1, 2, 3, 7]'),
    'maxdets100': lambda: make_case('maxdets100', 20, 3, 6, max_dets=[1, 10, 100], rows={2: 400}, edge='maxDets [1, 10, 100], 133 rows of one category'),
    'A7T9': lambda: make_case('A7T9', 21, 3, 5, area=AREA7, iou=IOU9, rec=[0.5], edge='A 7 (ignore flag in bit 7), T 9 with thresholds 1.0 and above, R 1'),
    'A4T16': lambda: make_case('A4T16', 22, 3, 5, iou=IOU16, edge='A 4 x T 16 = 64 pairs, R 101'),
}


def _odd_values():
    c = make_case('odd_values', 23, 3, 4, edge='zero-area boxes, +-inf scores, unmatched detections exactly on an area bound')
    img, cat, n = c.img_ids[1], c.cat_ids[0], len(c.gts)
    c.gts.append(dict(image_id=img, category_id=cat, bbox=[50.0, 60.0, 0.0, 0.0], id=n + 1))
    c.gts.append(dict(image_id=img, category_id=cat, bbox=[70.0, 60.0, 0.0, 12.0], iscrowd=1, id=n + 2))
    odd = [([50.0, 60.0, 0.0, 0.0], 0.9), ([70.0, 60.0, 0.0, 12.0], 0.8), ([50.0, 60.0, 10.0, 0.0], float('inf')),
           ([2000.0, 2000.0, 32.0, 32.0], float('-inf')), ([2100.0, 2000.0, 96.0, 96.0], 0.95), ([2300.0, 2000.0, 64.0, 16.0], 0.93),
           ([2400.0, 2000.0, 32.0, float(np.nextafter(32.0, 64.0))], 0.92), ([2500.0, 2000.0, 1e5, 1e5], float('inf'))]
    c.dts.extend(dict(image_id=img, category_id=cat, bbox=b, score=s) for b, s in odd)
    return c


def _no_gt():
    c = make_case('no_gt', 24, 3, 4, edge='gt_cap 0: no ground truth at all', degenerate=True)
    c['gts'] = []
    return c


COCO_BUILDERS['odd_values'] = _odd_values
COCO_BUILDERS['no_gt'] = _no_gt


def _rows_case(n, seed):
    return make_case('rows%d' % n, seed, 4, 2, rows={0: n}, dets_per_gt=(1, 2), extra_fp=(0, 0), slots=n,
                     edge='S_in %d in one image, 3 rows in the other, %d rows of one category' % (n, n // 4))


@functools.lru_cache(maxsize=None)
def coco_case(name):
    c = COCO_BUILDERS[name]()
    if name == 'slots1':                             # the one row is a copy of the first ground-truth box
        g = c.gts[0]
        c['dts'] = [dict(image_id=g['image_id'], category_id=g['category_id'], bbox=list(g['bbox']), score=0.5)]
    if name.startswith('rows'):                      # the second image keeps 3 rows
        img1 = c.img_ids[1]
        keep, out = 0, []
        for d in c.dts:
            if d['image_id'] == img1:
                keep += 1
                if keep > 3:
                    continue
            out.append(d)
        c['dts'] = out
    c['slots'] = max(c['slots'], int(rows_per_image(c).max()))
    return c


def case_params(c):
    p = cocoeval.Params()
    if c.get('iou') is not None:
        p.iouThrs = np.asarray(c['iou'], np.float64)
    if c.get('area') is not None:
        p.areaRng = [list(a) for a in c['area']]
    if c.get('max_dets') is not None:
        p.maxDets = list(c['max_dets'])
    if c.get('rec') is not None:
        p.recThrs = np.asarray(c['rec'], np.float64)
    return p


def host_eval(c, dts=None, iou=None):
    """COCOeval on the case with its Params -> the evaluated and accumulated COCOeval."""
    ev = cocoeval.COCOeval(c['gts'], c['dts'] if dts is None else dts, c['img_ids'], c['cat_ids'])
    ev.params = case_params(c)
    if iou is not None:
        ev.params.iouThrs = np.asarray(iou, np.float64)
    ev.evaluate()
    ev.accumulate()
    return ev


@functools.lru_cache(maxsize=None)
def coco_expected(name):
    return host_eval(coco_case(name))


def rows_per_image(c):
    pos = {i: k for k, i in enumerate(c['img_ids'])}
    n = np.zeros(len(c['img_ids']), np.int64)
    for d in c['dts']:
        n[pos[d['image_id']]] += 1
    return n


def structure(c):
    """The figures the kernels' loops depend on, from the inputs and the constants alone."""
    p = case_params(c)
    A, T = len(p.areaRng), len(p.iouThrs)
    pos = {i: k for k, i in enumerate(c['img_ids'])}
    groups = [set() for _ in c['img_ids']]
    for d in c['dts']:
        groups[pos[d['image_id']]].add(d['category_id'])
    rows = rows_per_image(c)
    n_slots = len(c['img_ids']) * c['slots']
    tiles = -(-n_slots // SORT_TILE)
    return dict(A=A, T=T, K=len(c['cat_ids']), M=len(p.maxDets), R=len(p.recThrs), units=max(len(g) for g in groups) * A * T,
                S_in=int(rows.max()), n_slots=n_slots, tiles=tiles, tail=n_slots - (tiles - 1) * SORT_TILE,
                per=-(-RADIX * tiles // SCAN_THREADS), category_passes=2 if len(c['cat_ids']) > 255 else 1)


# ---- the device's slot layout from the host evaluator ---------------------------------------------------------------
def host_slots(ev, S):
    """The slot tensors coco_match_kernel writes, from an evaluated COCOeval: per image the rows in (category position,
    -score, list order) order; the rows past maxDets[-1] are there with their rank and code 0.  -> slot_cat int32 [N, S], slot_score float64, slot_rank int32,
    slot_code uint8 [N, S, A * T] (pair = a * T + t), npig int64 [K, A]."""
    p = ev.params
    A, T, N, K = len(p.areaRng), len(p.iouThrs), len(ev.img_ids), len(ev.cat_ids)
    cat = np.full((N, S), -1, np.int32)
    score = np.zeros((N, S), np.float64)
    rank = np.full((N, S), EMPTY_RANK, np.int32)
    code = np.zeros((N, S, A * T), np.uint8)
    npig = np.zeros((K, A), np.int64)
    for n, img in enumerate(ev.img_ids):
        at = 0
        for k, c in enumerate(ev.cat_ids):
            es = [ev.eval_imgs[(c, a, img)] for a in range(A)]
            if es[0] is None:
                continue
            for a, e in enumerate(es):
                npig[k, a] += int(np.count_nonzero(e['gtIgnore'] == 0))
            D = len(es[0]['dtScores'])
            every = np.array([d['score'] for d in ev.dts.get((img, c), [])], np.float64)      # the rows past maxDets[-1] keep
            every = every[np.argsort(-every, kind='mergesort')]                                # their place, with code 0
            assert np.array_equal(every[:D], es[0]['dtScores'], equal_nan=True)
            cat[n, at:at + len(every)] = k
            score[n, at:at + len(every)] = every
            rank[n, at:at + len(every)] = np.arange(len(every))
            for a, e in enumerate(es):
                cd = np.where(e['dtIgnore'], CODE_IGNORED, np.where(e['dtMatches'] != 0, CODE_TP, CODE_FP))      # [T, D]
                code[n, at:at + D, a * T:(a + 1) * T] = cd.T
            at += len(every)
    return cat, score, rank, code, npig


def accumulate_slots(slot_cat, slot_score, slot_rank, slot_code, npig, iou, area, rec, max_dets, sequence=None):
    """COCOeval.accumulate restated on slots, the same operations in the same order.  A slot counts for category k at maxDets m
    when slot_cat == k and slot_rank < maxDets[m]; the slots are taken in slot order and sorted by -score with a stable sort.
    sequence: the sorted slot indices to use instead (for the defect models).  -> precision [T, R, K, A, M], recall [T, K, A, M]."""
    T, R, A, M = len(iou), len(rec), len(area), len(max_dets)
    K = npig.shape[0]
    cat, score, rank = slot_cat.reshape(-1), slot_score.reshape(-1), slot_rank.reshape(-1)
    code = slot_code.reshape(len(cat), A * T)
    rec = np.asarray(rec, np.float64)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    if sequence is None:
        live = np.nonzero((cat >= 0) & (cat < K) & (rank < max_dets[-1]))[0]
        with np.errstate(invalid='ignore'):
            sequence = live[np.argsort(-score[live], kind='mergesort')]
    sequence = sequence[np.argsort(cat[sequence], kind='mergesort')]
    starts = np.searchsorted(cat[sequence], np.arange(K + 1))
    for k in range(K):
        mine = sequence[starts[k]:starts[k + 1]]
        for a in range(A):
            if npig[k, a] == 0:
                continue
            for m, max_det in enumerate(max_dets):
                sel = mine[rank[mine] < max_det]
                cd = code[sel][:, a * T:(a + 1) * T].T                                  # [T, n]
                tps, fps = cd == CODE_TP, cd == CODE_FP
                tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(float), np.cumsum(fps, axis=1).astype(float)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig[k, a]
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(R)
                    idx = np.searchsorted(rc, rec, side='left')
                    for ri, pi in enumerate(idx):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return precision, recall


def accumulate_case_slots(c, slots, **kw):
    p = case_params(c)
    return accumulate_slots(slots[0], slots[1], slots[2], slots[3], slots[4], p.iouThrs, p.areaRng, p.recThrs, p.maxDets, **kw)


# ---- defect models ----------------------------------------------------------------------------------------------------
def desc_score_key(s):
    """cocoeval.hip:desc_score_key in numpy: uint64 keys whose ascending order is numpy's argsort(-s, kind='mergesort')."""
    s = np.where(s == 0, 0.0, np.asarray(s, np.float64))
    u = s.view(np.uint64)
    u = np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))
    return np.where(np.isnan(s), np.uint64(2 ** 64 - 1), ~u)


def radix_sort_model(slot_cat, slot_score, slot_rank, K, max_det, scan='full', category_bytes=None, full=False):
    """The LSD radix sort of relnet_coco_accumulate in numpy: 8 byte passes over the score key, then the category digit in one
    or two byte passes, every pass a per-tile histogram, one exclusive scan over [digit, tile] and a stable scatter.
    scan='first_word': the scan adds only the first of each thread's `per` words to the thread sums.  category_bytes: passes
    over the category digit (default: 2 when K > 255).  -> the sorted slot indices, without the not-evaluated slots and the
    positions that no element was scattered to (full: every position, and its category digit)."""
    cat, rank = slot_cat.reshape(-1), slot_rank.reshape(-1)
    n = len(cat)
    catd = np.where((cat >= 0) & (cat < K) & (rank < max_det), cat, K).astype(np.uint64)
    tiles = -(-n // SORT_TILE)
    tile = np.arange(n) // SORT_TILE
    key, val = desc_score_key(slot_score.reshape(-1)), np.arange(n)

    def one_pass(key, val, shift):
        digit = ((key >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
        flat = digit * tiles + tile
        hist = np.bincount(flat, minlength=RADIX * tiles)
        right = np.concatenate([[0], np.cumsum(hist)[:-1]])
        if scan == 'full':
            off = right
        else:
            per = -(-len(hist) // SCAN_THREADS)
            first = np.zeros(SCAN_THREADS, np.int64)
            lo = np.arange(SCAN_THREADS) * per
            first[lo < len(hist)] = hist[lo[lo < len(hist)]]
            run0 = np.concatenate([[0], np.cumsum(first)[:-1]])
            pad = np.concatenate([hist, np.zeros(SCAN_THREADS * per - len(hist), np.int64)]).reshape(SCAN_THREADS, per)
            inner = np.concatenate([np.zeros((SCAN_THREADS, 1), np.int64), np.cumsum(pad, axis=1)[:, :-1]], axis=1)
            off = (run0[:, None] + inner).reshape(-1)[:len(hist)]
        order = np.argsort(flat, kind='mergesort')
        within = np.arange(n) - right[flat[order]]
        dst = off[flat[order]] + within
        k2, v2 = np.zeros(n, np.uint64), np.full(n, -1, np.int64)
        k2[dst], v2[dst] = key[order], val[order]
        return k2, v2

    for shift in range(0, 64, 8):
        key, val = one_pass(key, val, shift)
    key = np.where(val >= 0, catd[np.maximum(val, 0)], np.uint64(K))
    for b in range(category_bytes if category_bytes is not None else (2 if K > 255 else 1)):
        key, val = one_pass(key, val, 8 * b)
    if full:                                       # every position with its category digit (K: not evaluated or never written)
        return val, key.astype(np.int64)
    return val[(val >= 0) & (catd[np.maximum(val, 0)] < K)]


def drop_units_from(c, slots, first=MATCH_THREADS):
    """Slots as a unit loop that stops at `first` units would leave them: the groups of an image are taken in category order,
    unit = group * A * T + pair, and the codes of the units past `first` keep their initial 0."""
    p = case_params(c)
    AT = len(p.areaRng) * len(p.iouThrs)
    cat, code = slots[0], slots[3].copy()
    for n in range(cat.shape[0]):
        present = np.unique(cat[n][cat[n] >= 0])
        for g, k in enumerate(present):
            pairs = np.arange(AT)[g * AT + np.arange(AT) >= first]
            if len(pairs):
                rows = np.nonzero(cat[n] == k)[0]
                code[np.ix_([n], rows, pairs)] = 0
    return slots[0], slots[1], slots[2], code, slots[4]


def drop_rows_from(c, first=MATCH_THREADS):
    """The detection list without each image's rows at index >= first."""
    seen, out = {}, []
    for d in c['dts']:
        seen[d['image_id']] = seen.get(d['image_id'], 0) + 1
        if seen[d['image_id']] <= first:
            out.append(d)
    return out


def strictly_above(thr):
    """Thresholds t' with (x >= t') == (x > t) for every float64 x: the model of `>` in place of `>=`."""
    return np.nextafter(np.asarray(thr, np.float64), np.inf)


# ---- hand-built slots ---------------------------------------------------------------------------------------------------
def hand_slots(seed, n_slots, K, A, T, max_dets, empty_every=3):
    """Slots that no matching produced: categories from -2 to K + 1, ranks at and past every maxDets value and the empty rank,
    every code value, NaN / -0.0 / 0.0 / +-inf scores among tied ones, and category 1 with npig == 0."""
    rng = np.random.default_rng(seed)
    cat = rng.integers(-2, K + 2, n_slots).astype(np.int32)
    cat[rng.random(n_slots) < 1.0 / empty_every] = -1
    score = np.round(rng.random(n_slots), 1)
    special = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf])
    pick = rng.random(n_slots) < 0.15
    score[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    md = np.asarray(max_dets)
    ranks = np.unique(np.concatenate([[0], md - 1, md, md + 1, [EMPTY_RANK]]))
    ranks = ranks[ranks >= 0]
    rank = np.where(rng.random(n_slots) < 0.5, rng.integers(0, max(int(md[-1]), 1), n_slots),
                    ranks[rng.integers(0, len(ranks), n_slots)]).astype(np.int32)
    code = rng.integers(0, 3, (n_slots, A * T)).astype(np.uint8)
    npig = rng.integers(1, 40, (K, A)).astype(np.int64)
    if K > 1:
        npig[1] = 0
    npig[0, A - 1] = 0
    return cat, score, rank, code, npig


HAND_CASES = {   # name: (seed, n_slots, K, iou, area, rec, maxDets)
    'hand_default': (1, 3000, 4, list(cocoeval.Params().iouThrs), DEFAULT_AREA, list(cocoeval.Params().recThrs), [1, 10, 100]),
    'hand_M4_tail1': (2, 2049, 3, [0.5, 0.75], AREA2, [0.0, 0.5, 1.0], [1, 2, 3, 7]),
    'hand_M1_one_slot': (3, 1, 1, [0.5], AREA2, [0.5], [1]),
    'hand_64pairs_K257': (4, 9 * 1024, 257, IOU16, DEFAULT_AREA, [0.0, 0.3, 1.0], [2, 5]),
    'hand_A7_tail2047': (5, 2047, 5, [0.5, 0.9], AREA7, [0.1, 0.9], [1, 10, 100]),
}


@functools.lru_cache(maxsize=None)
def hand_case(name):
    seed, n, K, iou, area, rec, md = HAND_CASES[name]
    slots = hand_slots(seed, n, K, len(area), len(iou), md)
    if name == 'hand_M1_one_slot':
        slots[0][:] = 0; slots[2][:] = 0; slots[1][:] = 0.5; slots[4][:] = 1
    return dict(slots=slots, iou=np.asarray(iou, np.float64), area=area, rec=np.asarray(rec, np.float64), max_dets=md)


@functools.lru_cache(maxsize=None)
def hand_expected(name):
    h = hand_case(name)
    return accumulate_slots(*h['slots'], h['iou'], h['area'], h['rec'], h['max_dets'])


# ---- detection rows as the entry point takes them ----------------------------------------------------------------------
def surviving_rows(det, num_det, class_to_cat, img_ids, cat_ids):
    """The rows of det [N, S, 6] (class, score, x, y, w, h) that coco_match_kernel keeps, as COCOeval's detection dicts: the
    first clamp(num_det, 0, S) rows whose class is an integer in [0, n_classes) that the table maps to a category."""
    out = []
    for n, img in enumerate(img_ids):
        for r in det[n, :min(max(int(num_det[n]), 0), det.shape[1])]:
            cv = r[0]
            if not (cv >= 0 and cv < len(class_to_cat)) or int(cv) != cv or class_to_cat[int(cv)] < 0:
                continue
            out.append(dict(image_id=img, category_id=cat_ids[class_to_cat[int(cv)]], score=float(r[1]),
                            bbox=[float(r[2]), float(r[3]), float(r[4]), float(r[5])]))
    return out


def dirty_rows(c, seed):
    """The case's detections as rows behind a class -> category table with background and an unused class, between rows
    that must be dropped: class NaN / -1 / 0.5 / n_classes / 1e30 / the unmapped classes, and rows past num_det.
    -> det float64 [N, S, 6], num_det, class_to_cat."""
    rng = np.random.default_rng(seed)
    K, N = len(c['cat_ids']), len(c['img_ids'])
    class_to_cat = np.concatenate([[-1], np.arange(K), [-1]]).astype(np.int32)           # class 0 background, class K + 1 unused
    bad = [np.nan, -1.0, 0.5, float(K + 2), 1e30, 0.0, float(K + 1), -np.inf, np.inf, K + 0.999]
    pos = {i: k for k, i in enumerate(c['img_ids'])}
    cpos = {i: k for k, i in enumerate(c['cat_ids'])}
    rows = [[] for _ in range(N)]
    for d in c['dts']:
        r = rows[pos[d['image_id']]]
        r.append([cpos[d['category_id']] + 1.0, d['score']] + list(d['bbox']))
        if rng.random() < 0.3:
            r.append([bad[int(rng.integers(0, len(bad)))], 0.99, 10.0, 10.0, 30.0, 30.0])
    S = max(len(r) for r in rows) + 4
    det = np.zeros((N, S, 6))
    num = np.zeros(N, np.int32)
    for n, r in enumerate(rows):
        det[n, :len(r)] = r
        det[n, len(r):] = [1.0, 0.97, 5.0, 5.0, 40.0, 40.0]                                # valid-looking rows behind num_det
        num[n] = len(r)
    return det, num, class_to_cat


# ======================================================================================================================
# Recall cases
# ======================================================================================================================
def recall_reference(gts, cands, thresholds, area_rng, cover=None, argmax_width=None):
    """dataset/recall.py:evaluate_recall for any area ranges, through its own bbox_overlaps and greedy_cover.  gts: per image
    [G, 4] in the roidb's dtype; cands: per image float32 [n, 4].  -> dict(hits int64 [A, T], num_pos [A], area_count [A - 1],
    n_cand int32 [N], overlaps float64 [N, A, gt_cap])."""
    cover = cover or R.greedy_cover
    thr = np.asarray(thresholds, np.float64)
    A, N = len(area_rng), len(gts)
    gt_cap = max([len(g) for g in gts] + [0])
    out = dict(hits=np.zeros((A, len(thr)), np.int64), num_pos=np.zeros(A, np.int64), area_count=np.zeros(A - 1, np.int64),
               n_cand=np.zeros(N, np.int32), overlaps=np.zeros((N, A, gt_cap)))
    for i in range(N):
        g, c = gts[i], cands[i]
        inside = range_masks(g, area_rng)
        out['num_pos'] += inside.sum(1)
        if len(c):
            cin = range_masks(c[:, :4], area_rng)
            out['area_count'] += cin[1:].sum(1)
        out['n_cand'][i] = len(c)
        if len(c) == 0:
            continue
        ov = R.bbox_overlaps(c[:, :4].astype(np.float64), g.astype(np.float64))
        for a in range(A):
            rec = cover(ov[:, inside[a]])
            out['overlaps'][i, a, :len(rec)] = rec
            out['hits'][a] += np.array([(rec >= t).sum() for t in thr], np.int64)
    return out


def range_masks(boxes, area_rng):
    """recall.py:area_masks for any ranges: area in the boxes' own dtype, half-open [lo, hi)."""
    if len(boxes) == 0:
        return np.zeros((len(area_rng), 0), bool)
    areas = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    return np.stack([(areas >= lo) & (areas < hi) for lo, hi in area_rng])


def cover_variant(gt_first=None, gt_last=False, box_last=False):
    """Defect models of the greedy cover: the round's argmax over the first `gt_first` columns only (while one of them is
    unused), the LAST column among equal maxima, the LAST proposal among equal maxima of a column."""
    def last_argmax(v, axis=None):
        if axis is None:
            return len(v) - 1 - v[::-1].argmax()
        return v.shape[0] - 1 - v[::-1].argmax(axis=0)

    def cover(overlaps):
        P, G = overlaps.shape
        rec = np.zeros(G)
        for j in range(min(P, G)):
            colmax = overlaps.max(axis=0)
            w = gt_first if gt_first and (colmax[:gt_first] > -1).any() else G
            gt_ind = last_argmax(colmax[:w]) if gt_last else colmax[:w].argmax()
            col = overlaps[:, gt_ind]
            box_ind = last_argmax(col) if box_last else col.argmax()
            rec[j] = overlaps[box_ind, gt_ind]
            overlaps[box_ind, :] = -1
            overlaps[:, gt_ind] = -1
        return rec
    return cover


RANGES8 = [[0.0, 1e10], [0.0, 625.0], [625.0, 2500.0], [2500.0, 10000.0], [10000.0, 40000.0], [40000.0, 90000.0], [90000.0, 1e10],
           [1681.0, 1682.0]]                                          # the last holds the 41 x 41 boxes
RANGES2 = [[0.0, 1e10], [900.0, 1e10]]
T256 = np.linspace(0.0, 1.0, 256)


def _random_gt(rng, G, dtype=np.uint16):
    x1 = rng.integers(0, 900, G); y1 = rng.integers(0, 700, G)
    side = rng.choice([12, 30, 70, 150, 250, 380], G)
    return np.stack([x1, y1, x1 + side + rng.integers(0, 9, G), y1 + side + rng.integers(0, 9, G)], 1).astype(dtype)


def _near(rng, gt, P):
    """float32 proposals: copies of the gts (IoU 1.0), jittered on a 0.5 grid so that overlaps tie, and strays."""
    b = gt[rng.integers(0, len(gt), P)].astype(np.float64) + np.round(rng.uniform(-8, 8, (P, 4)) * 2) / 2
    exact = rng.random(P) < 0.1
    b[exact] = gt[rng.integers(0, len(gt), int(exact.sum()))]
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2])
    return b.astype(np.float32)


def _tie_clusters(n, y0=1200):
    """n clusters of two ground-truth boxes mirrored about one proposal p (both overlap it 36 x 40 / (2 x 1600 - 1440)), and a
    second proposal q that overlaps the left box more than the right.  Taken with the lowest index first the left box gets p
    and the right one q at 0.4286; the other way round the left one gets q at 0.6667.  -> (left [n,4], right [n,4], p, q)"""
    y = y0 + 60 * np.arange(n)
    z = np.zeros(n)
    left = np.stack([z + 96, y, z + 135, y + 39], 1)
    right = np.stack([z + 104, y, z + 143, y + 39], 1)
    p = np.stack([z + 100, y, z + 139, y + 39], 1)
    q = np.stack([z + 88, y, z + 127, y + 39], 1)
    return left, right, p, q


def recall_gt_case(G, seed, far):
    """One image with G ground-truth boxes.  Boxes i and i + far (i < 20) are a tie cluster; 40 boxes in the middle are identical
    and share one best proposal; the rest are random.  A second image has 3 boxes, a third none."""
    rng = np.random.default_rng(seed)
    gt = _random_gt(rng, G).astype(np.float64)
    nc = min(20, G - far)
    left, right, p, q = _tie_clusters(nc)
    gt[:nc] = left
    gt[far:far + nc] = right
    same = np.arange(22, 22 + min(40, far - 22))
    gt[same] = [300, 1200, 340, 1240]                         # (41 x 41: alone in the last of RANGES8)
    free = np.setdiff1d(np.arange(G), np.concatenate([np.arange(nc), far + np.arange(nc), same]))
    cands = _near(rng, gt[free].astype(np.uint16), 280)                # (nothing random near the clusters)
    cands = np.concatenate([cands[:140], q.astype(np.float32), cands[140:], p.astype(np.float32),
                            np.array([[301, 1200, 341, 1240], [300, 1201, 340, 1241]], np.float32)])
    gt2 = _random_gt(rng, 3)
    return [gt.astype(np.uint16), gt2, np.zeros((0, 4), np.uint16)], [cands, _near(rng, gt2, 50), _near(rng, gt2, 10)]


def recall_cand_case(P, seed):
    """P candidates for 70 ground-truth boxes: mirrored pairs at i and i + 64 (equal overlaps in one lane of column_best), exact
    duplicates at i and i + 64, and the LAST row the only exact copy of ground-truth box 5."""
    rng = np.random.default_rng(seed)
    gt = _random_gt(rng, 70).astype(np.float64)
    n = 12
    y = 1200 + 60 * np.arange(n)
    z = np.zeros(n)
    gt[:n] = np.stack([z + 100, y, z + 139, y + 39], 1)               # A: p_a and p_b overlap it equally
    gt[n:2 * n] = np.stack([z + 108, y, z + 147, y + 39], 1)          # B: prefers p_b
    gt[5 + 2 * n] = [700, 900, 760, 990]
    c = _near(rng, gt[2 * n + 6:].astype(np.uint16), P)               # (nothing random near the pairs or box 5 + 2 n)
    c[200:200 + n] = np.stack([z + 96, y, z + 135, y + 39], 1)       # p_a at i
    c[264:264 + n] = np.stack([z + 104, y, z + 143, y + 39], 1)      # p_b at i + 64
    c[400 + 64:400 + 64 + 30] = c[400:430]                            # duplicates at i and i + 64
    c[P - 1] = gt[5 + 2 * n]
    return [gt.astype(np.uint16)], [c]


def recall_filter_case(seed):
    """Raw rows with scores: the score filter leaves 0, 1 and G - 1 candidates, and one image has num_valid 0.
    -> gts, raw [4, P, 4] float32, scores [4, P] float32, thresh, num_valid"""
    rng = np.random.default_rng(seed)
    G, P = 9, 40
    gts = [_random_gt(rng, G) for _ in range(4)]
    raw = np.stack([_near(rng, g, P) for g in gts])
    scores = np.full((4, P), 0.25, np.float32)                     # == thresh: not kept (score > thresh)
    scores[1, 17] = 0.75
    scores[2, rng.permutation(P)[:G - 1]] = np.float32(0.25) + np.float32(2.0 ** -25) * 2
    scores[3] = 0.9
    return gts, raw, scores, 0.25, np.array([P, P, P, 0], np.int32)


def filtered(raw, scores, thresh, num_valid):
    return [raw[i][:num_valid[i]][scores[i][:num_valid[i]] > np.float32(thresh)] for i in range(len(raw))]


RECALL_CASES = {   # name: (builder, thresholds, area ranges, edge)
    'G64': (lambda: recall_gt_case(64, 1, 32), None, R.AREA_RANGES, 'G 64: one wave of the argmax full'),
    'G65': (lambda: recall_gt_case(65, 2, 64), None, R.AREA_RANGES, 'G 65: box 64 alone in wave 1, tied with box 0'),
    'G255': (lambda: recall_gt_case(255, 3, 64), None, RANGES2, 'G 255, A 2; tie clusters at i and i + 64'),
    'G256': (lambda: recall_gt_case(256, 4, 128), T256, RANGES8, 'G 256 (cap), A 8, T 256 with 0.0 and 1.0; tie clusters at i and i + 128'),
    'P2047': (lambda: recall_cand_case(2047, 5), np.array([0.6]), RANGES2, 'P 2047, T 1, A 2'),
    'P2048': (lambda: recall_cand_case(2048, 6), None, R.AREA_RANGES, 'P 2048 (cap): the last register of the last thread'),
}


@functools.lru_cache(maxsize=None)
def recall_case(name):
    build, thr, ranges, edge = RECALL_CASES[name]
    gts, cands = build()
    return dict(gts=gts, cands=cands, thr=R.default_thresholds() if thr is None else thr, ranges=[list(r) for r in ranges], edge=edge)


@functools.lru_cache(maxsize=None)
def recall_expected(name):
    c = recall_case(name)
    return recall_reference(c['gts'], c['cands'], c['thr'], c['ranges'])
