"""Host side of the uint8 image path: resize_plan against resize(), and the loaders with raw_images=True against the default
float batches (same im_info / boxes / proposals; the shipped sources, pre-processed in numpy, give the default `data`)."""
import os

import numpy as np
import pytest

import relnet_amd  # noqa: F401
from relnet_amd import config as C
from relnet_amd.dataset import image as IMG, loader as LD


@pytest.mark.parametrize('stride', [0, 32])
def test_resize_plan_reproduces_resize(stride):
    for h, w in ((150, 200), (480, 640), (37, 53), (600, 1000), (123, 457), (801, 399), (17, 29), (1000, 100)):
        for target, cap in ((600, 1000), (800, 1333), (300, 500), (120, 200), (128, 192)):
            im = np.zeros((h, w, 3), np.uint8)
            out, s = IMG.resize(im, target, cap, stride=stride)
            ps, nh, nw, ph, pw = IMG.resize_plan(h, w, target, cap, stride)
            assert ps == s and (ph, pw) == out.shape[:2], (h, w, target, cap)
            assert (nh, nw) == IMG.resize(im, target, cap, stride=0)[0].shape[:2]
            if stride:
                assert ph % stride == 0 and pw % stride == 0 and 0 <= ph - nh < stride and 0 <= pw - nw < stride
            else:
                assert (ph, pw) == (nh, nw)


def _roidb(root, n=5, seed=0):
    """uint8 .npy images of mixed orientation and odd sizes, each also flipped; gt rows and precomputed proposal rows."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = ((97, 143), (151, 88), (120, 161), (75, 75), (133, 190))[i % 5]
        path = os.path.join(root, 'im%d.npy' % i)
        np.save(path, rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        ng, npr = 3, 7
        x1, y1 = rng.uniform(0, w - 30, ng + npr), rng.uniform(0, h - 30, ng + npr)
        boxes = np.stack([x1, y1, x1 + rng.uniform(5, 29, ng + npr), y1 + rng.uniform(5, 29, ng + npr)], 1).astype(np.uint16)
        cls = np.concatenate([rng.integers(1, 81, ng), np.zeros(npr, np.int64)]).astype(np.int32)
        rec = dict(image=path, height=h, width=w, boxes=boxes, gt_classes=cls, max_classes=cls,
                   is_gt=np.concatenate([np.ones(ng), np.zeros(npr)]).astype(np.int32), flipped=False)
        out.append(rec)
        f = dict(rec, flipped=True)
        b = boxes.astype(np.int64)
        f['boxes'] = np.stack([w - b[:, 2] - 1, b[:, 1], w - b[:, 0] - 1, b[:, 3]], 1).astype(np.uint16)
        out.append(f)
    return out


def _data_from_raw(batch, cfg):
    """numpy resize + transform + tensor_vstack of the sources a raw batch ships, driven by its table alone."""
    src, table, scale = batch['image_src'].numpy(), batch['image_table'].numpy(), batch['image_scale'].numpy()
    ims = []
    for (off, h, w, flip, nh, nw), s in zip(table, scale):
        im = src[off:off + h * w * 3].reshape(h, w, 3)
        if flip:
            im = im[:, ::-1, :]
        target, cap = cfg.SCALES[0]
        out, s2 = IMG.resize(im, target, cap, stride=cfg.network.IMAGE_STRIDE)
        assert s2 == s and out.shape[0] >= nh and out.shape[1] >= nw
        ims.append(IMG.transform(out, cfg.network.PIXEL_MEANS))
    return IMG.tensor_vstack(ims)


def _same_batch(a, b, cfg):
    assert 'data' not in b and set(a) - {'data'} == set(b) - {'image_src', 'image_table', 'image_scale', 'canvas_hw'}
    for k in a:
        if k != 'data':
            va, vb = a[k], b[k]
            assert (va == vb) if not hasattr(va, 'numpy') else np.array_equal(va.numpy(), vb.numpy()), k
    assert b['canvas_hw'] == tuple(a['data'].shape[2:])
    assert tuple(b['canvas_hw']) == (int(b['im_info'][:, 0].max()), int(b['im_info'][:, 1].max()))
    d = _data_from_raw(b, cfg)
    assert d.dtype == a['data'].numpy().dtype and np.array_equal(d, a['data'].numpy())


def test_test_loader_raw_images(tmp_path):
    cfg = C.experiment('rcnn_end2end_relation_8epoch')
    cfg.SCALES[0] = (120, 200)
    roidb = _roidb(str(tmp_path))
    for has_rpn in (True, False):
        ref = list(LD.TestLoader(roidb, cfg, batch_size=3, has_rpn=has_rpn))
        raw = list(LD.TestLoader(roidb, cfg, batch_size=3, has_rpn=has_rpn, raw_images=True))
        assert len(ref) == len(raw) == 4
        for a, b in zip(ref, raw):
            _same_batch(a, b, cfg)


def test_anchor_loader_raw_images(tmp_path):
    cfg = C.experiment('rcnn_end2end_relation_8epoch')
    cfg.SCALES[0] = (120, 200)
    roidb = _roidb(str(tmp_path))
    for device_targets in (False, True):
        kw = dict(batch_size=2, shuffle=True, aspect_grouping=True, seed=5, device_targets=device_targets)
        ref = list(LD.AnchorLoader(roidb, cfg, **kw))
        raw = list(LD.AnchorLoader(roidb, cfg, raw_images=True, **kw))
        assert len(ref) == len(raw) == 5
        for a, b in zip(ref, raw):
            _same_batch(a, b, cfg)


def test_roi_iter_raw_images(tmp_path):
    cfg = C.experiment('rcnn_fpn_relation_learn_nms_8epoch')
    cfg.SCALES[0] = (128, 192)
    cfg.TRAIN.TOP_ROIS = 6
    assert cfg.network.IMAGE_STRIDE == 32
    roidb = _roidb(str(tmp_path))
    ref = list(LD.ROIIter(roidb, cfg, batch_size=2))
    raw = list(LD.ROIIter(roidb, cfg, batch_size=2, raw_images=True))
    assert len(ref) == len(raw) == 5
    for a, b in zip(ref, raw):
        _same_batch(a, b, cfg)
        assert b['canvas_hw'][0] % 32 == 0 and b['canvas_hw'][1] % 32 == 0
