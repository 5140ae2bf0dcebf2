"""Cases and a numpy restatement of the sampled ROI minibatch (TRAIN.BATCH_ROIS > 0; relnet_proposal_target_sample, the contract is in
include/relnet_hip.h).  numpy only: the golden generator (tests/golden/gen_golden_sampled_rois.py), the host tests and the GPU tests share it.

  key32 / words / choose   the selection rule that stands in for npr.choice: the `take` members with the smallest 64-bit word
                           (key32(seed, image, stream, i) << 32) | i, returned in ascending order
  sample_image             core/rcnn.py:329-397 (sample_rois) + operator_py/proposal_target.py:64-67 restated for one image, with that rule
  CASES                    name -> inputs and settings; `case(name)` builds the arrays
"""
import numpy as np

F32 = np.float32
LIMIT = 8192                     # candidates per image the kernel accepts
SEEDS = (20240917, 77)           # the seed of the golden, and a second one (the seed tests)
MEANS, STDS, WEIGHTS = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2), (1.0, 1.0, 1.0, 1.0)
M32 = 0xffffffff


def key32(seed, b, stream, idx):
    """The avalanche hash of the anchor sampler (csrc/targets.hip anchor_key) with stream * 0x27D4EB2F xor-ed into its input.
    seed: 64-bit, b / stream: ints, idx: int array -> uint32 array."""
    seed = int(seed) & (2 ** 64 - 1)
    x = (np.asarray(idx, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(M32)
    c = (seed & M32) ^ ((b * 0x85EBCA77) & M32) ^ (((seed >> 32) * 0xC2B2AE3D) & M32) ^ ((stream * 0x27D4EB2F) & M32)
    x = x ^ np.uint64(c)
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7feb352d)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846ca68b)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    return x.astype(np.uint32)


def words(seed, b, stream, idx):
    idx = np.asarray(idx, dtype=np.int64)
    return (key32(seed, b, stream, idx).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)


def choose(members, take, seed, b, stream):
    """The `take` members with the smallest words of `stream`, ascending."""
    members = np.asarray(members, dtype=np.int64)
    w = words(seed, b, stream, members)
    return np.sort(members[np.argsort(w, kind='stable')[:int(take)]])


def fg_rois_per_image(fg_fraction, R):
    return int(np.round(fg_fraction * R))          # proposal_target.py:58,61 (round half to even)


def overlaps(boxes, gt):
    """lib/bbox/bbox.pyx:33-55 in float64: [n, k]."""
    b = np.asarray(boxes, np.float64)[:, None, :]
    q = np.asarray(gt, np.float64)[None, :, :4]
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0]) + 1
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1]) + 1
    ua = (b[..., 2] - b[..., 0] + 1) * (b[..., 3] - b[..., 1] + 1) + (q[..., 2] - q[..., 0] + 1) * (q[..., 3] - q[..., 1] + 1) - iw * ih
    return np.where((iw > 0) & (ih > 0), iw * ih / ua, 0.0)


def _transform_f32(ex, gt):
    """bbox_transform.py:74-100 on float32 arrays; the log correctly rounded (what the kernel computes; numpy's own float32 log is within 1 ulp)."""
    one, half = F32(1.0), F32(0.5)
    ew = ex[:, 2] - ex[:, 0] + one; eh = ex[:, 3] - ex[:, 1] + one
    ecx = ex[:, 0] + half * (ew - one); ecy = ex[:, 1] + half * (eh - one)
    gw = gt[:, 2] - gt[:, 0] + one; gh = gt[:, 3] - gt[:, 1] + one
    gcx = gt[:, 0] + half * (gw - one); gcy = gt[:, 1] + half * (gh - one)
    dx = (gcx - ecx) / (ew + F32(1e-14)); dy = (gcy - ecy) / (eh + F32(1e-14))
    dw = np.log((gw / ew).astype(np.float64)).astype(F32); dh = np.log((gh / eh).astype(np.float64)).astype(F32)
    return np.vstack((dx, dy, dw, dh)).T.astype(F32)


def sample_image(c, b, seed):
    """One image of case dict c -> dict(rois_out, label, bbox_target, bbox_weight, keep_index, fg, bg, picks, n_choice).
    picks: [(stream, members, take, chosen)] of every draw that had to choose (the npr.choice calls of the reference)."""
    R, D = c['R'], 4 * c['num_reg']
    nr = c['N'] if c['num_rois'] is None else int(c['num_rois'][b])
    G = int(c['num_gt'][b])
    gt = c['gt'][b, :G]
    cand = c['rois'][b, :nr]
    if c['append_gt']:
        cand = np.vstack((cand, np.hstack((np.full((G, 1), b, F32), gt[:, :4]))))
    M = cand.shape[0]
    out = dict(rois_out=np.zeros((R, 5), F32), label=np.full((R,), -1, F32), bbox_target=np.zeros((R, D), F32),
               bbox_weight=np.zeros((R, D), F32), keep_index=np.full((R,), -1, np.int32), fg=np.zeros(0, np.int64),
               bg=np.zeros(0, np.int64), picks=[], n_choice=0)
    if M == 0:
        out['rois_out'][:, 0] = b
        return out
    if G > 0:
        ov = overlaps(cand[:, 1:], gt)
        assign, mx = ov.argmax(axis=1), ov.max(axis=1)
    else:
        assign, mx = np.zeros(M, np.int64), np.zeros(M)
    fg = np.where(mx >= c['fg_thresh'])[0]
    bg = np.where((mx < c['bg_thresh_hi']) & (mx >= c['bg_thresh_lo']))[0]
    picks = []

    def draw(stream, members, take):
        if len(members) > take:
            chosen = choose(members, take, seed, b, stream)
            picks.append((stream, np.asarray(members), int(take), chosen))
            return chosen
        return np.asarray(members, np.int64)
    fg_take = min(fg_rois_per_image(c['fg_fraction'], R), len(fg))
    keep = draw(0, fg, fg_take)
    bg_take = min(R - fg_take, len(bg))
    keep = np.append(keep, draw(1, bg, bg_take))
    t = 0
    while len(keep) < R:
        gap = min(M, R - len(keep))
        keep = np.append(keep, draw(2 + t, np.arange(M), gap))
        t += 1
    keep = keep.astype(np.int64)
    rows = cand[keep]
    label = gt[assign[keep], 4].copy() if G > 0 else np.zeros(R, F32)
    label[mx[keep] < c['bg_thresh_hi']] = 0
    out.update(rois_out=rows, label=label.astype(F32), keep_index=keep.astype(np.int32), fg=fg, bg=bg, picks=picks, n_choice=len(picks))
    if G > 0:
        tg = (_transform_f32(rows[:, 1:], gt[assign[keep], :4]) - np.array(c['means'])) / np.array(c['stds'])      # float64
        for r in np.where(label > 0)[0]:
            start = 4 if c['class_agnostic'] else 4 * int(label[r])
            if start + 4 <= D:
                out['bbox_target'][r, start:start + 4] = tg[r]
                out['bbox_weight'][r, start:start + 4] = c['weights']
    return out


def sample(c, seed):
    """Every image of the case: the five outputs stacked [B, ...], plus the per-image dicts."""
    per = [sample_image(c, b, seed) for b in range(c['B'])]
    o = {k: np.stack([p[k] for p in per]) for k in ('rois_out', 'label', 'bbox_target', 'bbox_weight', 'keep_index')}
    o['per_image'] = per
    return o


# ---------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------
GT3 = np.array([[10, 12, 57, 63, 2], [110, 20, 171, 83, 4], [24, 120, 95, 171, 3]], F32)       # three separate boxes, classes < 5


def _roi(kind, gt, rng):
    """fg: the gt box jittered by < 2 px (IoU > 0.8); bg: shifted by half its width (IoU 1/3 up to the jitter); far: a box in the corner
    x, y >= 200 that no gt box reaches (IoU 0)."""
    x1, y1, x2, y2 = gt[:4]
    j = rng.uniform(-1.5, 1.5, 4)
    if kind == 'fg':
        return np.array([x1, y1, x2, y2]) + j
    if kind == 'bg':
        s = 0.5 * (x2 - x1 + 1)
        return np.array([x1 + s, y1, x2 + s, y2]) + j * 0.5
    x, y = rng.uniform(200, 260, 2)
    return np.array([x, y, x + rng.uniform(10, 40), y + rng.uniform(10, 40)])


def _image(kinds, gt, seed, b=0):
    rng = np.random.default_rng(seed)
    boxes = np.stack([_roi(k, gt[i % max(len(gt), 1)] if len(gt) else np.zeros(5), rng) for i, k in enumerate(kinds)])
    return np.hstack((np.full((len(kinds), 1), b), np.maximum(boxes, 0))).astype(F32)


def _random_image(n, g, seed, num_fg=80, size=1000.0):
    """n rois, g gt boxes; a third of the rois are jittered copies of gt boxes, a third shifted ones, the rest anywhere."""
    rng = np.random.default_rng(seed)
    x1 = rng.uniform(0, size - 120, g); y1 = rng.uniform(0, size - 120, g)
    gt = np.stack((x1, y1, x1 + rng.uniform(30, 110, g), y1 + rng.uniform(30, 110, g), rng.integers(1, num_fg + 1, g)), 1).astype(F32)
    x1 = rng.uniform(0, size - 120, n); y1 = rng.uniform(0, size - 120, n)
    rois = np.stack((x1, y1, x1 + rng.uniform(16, 110, n), y1 + rng.uniform(16, 110, n)), 1)
    k = n // 3
    src = rng.integers(0, g, 2 * k)
    rois[:k] = gt[src[:k], :4] + rng.normal(0, 4, (k, 4))
    rois[k:2 * k] = gt[src[k:], :4] + rng.normal(0, 4, (k, 4)) + (0.4 * (gt[src[k:], 2] - gt[src[k:], 0]))[:, None] * np.array([1, 0, 1, 0])
    rois[:, 2:] = np.maximum(rois[:, 2:], rois[:, :2] + 4)
    rois = rng.permutation(np.maximum(rois, 0))
    return np.hstack((np.zeros((n, 1)), rois)).astype(F32), gt


def _one(kinds, num_gt=3, seed=1, **kw):
    gt = GT3.copy()
    return dict(rois=_image(kinds, gt[:num_gt], seed)[None], gt=gt[None], num_gt=[num_gt], **kw)


def _edges():
    gt = np.array([[0, 0, 9, 9, 4]], F32)
    rois = _image(['far'] * 12, gt, 7)
    rois[3, 1:] = [0, 0, 9, 4]          # 50 / 100: exactly fg_thresh -> foreground, and not below bg_thresh_hi
    rois[8, 1:] = [0, 0, 9, 0]          # 10 / 100: exactly bg_thresh_lo -> background
    return dict(rois=rois[None], gt=gt[None], num_gt=[1], bg_thresh_lo=0.1, append_gt=False)


def _batch():
    kinds = ['fg', 'bg', 'bg', 'fg', 'bg', 'bg', 'fg', 'bg', 'bg', 'bg', 'fg', 'bg']
    gt = np.stack([GT3, GT3[[1, 0, 2]] + np.array([3, 5, 3, 5, 0], F32), np.zeros((3, 5), F32)])
    rois = np.stack([_image(kinds, GT3, 21, 0), _image(kinds, gt[1, :1], 22, 1), _image(kinds, GT3, 23, 2)])
    return dict(rois=rois, gt=gt, num_gt=[3, 1, 0], num_rois=[12, 7, 12])


def _large(n, g, seed):
    rois, gt = _random_image(n, g, seed)
    return dict(rois=rois[None], gt=gt[None], num_gt=[g], R=512)


CASES = {
    # |fg| = 2 (the gt rows), |bg| = 6, six rows in neither set: the reference makes no random call -- order and values are its own
    'exact-fit': lambda: _one(['bg', 'far'] * 6, num_gt=2, seed=11, bg_thresh_lo=0.1),
    'many-fg': lambda: _one(['fg', 'bg'] * 6, seed=12),                                  # |fg| 9 > 2, |bg| 6 = 8 - 2
    'many-bg': lambda: _one(['fg'] + ['bg'] * 11, num_gt=1, seed=13),                    # |fg| 2, |bg| 11 > 6
    'both': lambda: _one(['fg'] * 5 + ['bg'] * 7, seed=14),                              # |fg| 8 > 2, |bg| 7 > 6
    'short': lambda: _one(['bg'] * 3 + ['far'] * 9, seed=15, bg_thresh_lo=0.1),          # 2 + 3 rows, then one padding round of 3 out of 15
    'tiny': lambda: dict(rois=_image(['bg'], GT3[:1], 16)[None], gt=GT3[None, :1], num_gt=[1]),      # M = 2: three padding rounds of 2
    'edges': _edges,
    'no-append': lambda: _one(['fg', 'bg'] * 6, seed=17, append_gt=False),               # the BATCH_ROIS < -10 form
    'class-specific': lambda: _one(['fg'] * 5 + ['bg'] * 7, seed=18, num_reg=5, class_agnostic=False),
    'batch': _batch,
    'large': lambda: _large(2000, 100, 19),
    'limit': lambda: _large(LIMIT - 100, 100, 20),
}
SAMPLED = ('many-fg', 'many-bg', 'both', 'short', 'edges', 'no-append', 'class-specific', 'batch', 'large', 'limit')      # cases whose result depends on the seed


def case(name):
    c = dict(R=8, fg_fraction=0.25, fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0.0, append_gt=True, num_reg=2, class_agnostic=True,
             num_rois=None, means=MEANS, stds=STDS, weights=WEIGHTS)
    c.update(CASES[name]())
    c['rois'] = np.ascontiguousarray(c['rois'], F32); c['gt'] = np.ascontiguousarray(c['gt'], F32)
    c['num_gt'] = np.asarray(c['num_gt'], np.int32)
    if c['num_rois'] is not None:
        c['num_rois'] = np.asarray(c['num_rois'], np.int32)
    c['B'], c['N'] = c['rois'].shape[:2]
    c['name'] = name
    return c
