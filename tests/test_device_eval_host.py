"""Host side of the device COCO evaluator (dataset/device_eval.py): how the ground truth, the parameters and the detections are
packed for the match kernel.  No GPU."""
import os
import sys

import numpy as np
import pytest

import relnet_amd  # noqa: F401
from relnet_amd.dataset import cocoeval
from relnet_amd.dataset import device_eval as DE

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _area():
    return np.asarray(cocoeval.Params().areaRng, np.float64)


def test_params_tables_are_the_host_arrays():
    p = cocoeval.Params()
    iou, area, rec, max_dets = DE.pack_params(p)
    assert iou.dtype == np.float64 and np.array_equal(iou, p.iouThrs) and len(iou) == 10
    assert rec.dtype == np.float64 and np.array_equal(rec, p.recThrs) and len(rec) == 101
    assert area.shape == (4, 2) and area.dtype == np.float64 and area[2].tolist() == [32 ** 2, 96 ** 2]
    assert max_dets.dtype == np.int32 and max_dets.tolist() == [1, 10, 100]
    p.maxDets = [100, 10]
    with pytest.raises(ValueError):
        DE.pack_params(p)
    p = cocoeval.Params()
    p.iouThrs = np.linspace(0.05, 0.95, 19)             # 4 x 19 pairs > 64 lanes
    with pytest.raises(ValueError):
        DE.pack_params(p)


def test_ground_truth_csr_keeps_annotation_order_and_folds_ignore():
    g = lambda i, img, cat, b, **kw: dict(id=i, image_id=img, category_id=cat, bbox=b, **kw)
    gts = [g(1, 20, 7, [0, 0, 10, 10]),
           g(2, 10, 7, [1, 1, 40, 40], area=32 ** 2),                    # exactly 32^2: small and medium
           g(3, 20, 3, [2, 2, 5, 5], iscrowd=1),
           g(4, 20, 7, [3, 3, 200, 200], ignore=1),
           g(5, 20, 7, [4, 4, 96, 96], area=96 ** 2),                    # exactly 96^2: medium and large
           g(6, 30, 7, [5, 5, 1, 1]),                                    # image not evaluated
           g(7, 20, 9, [6, 6, 1, 1]),                                    # category not evaluated
           g(8, 20, 3, [7, 7, 20, 20])]
    img_ids, cat_ids = [10, 20], [3, 7]
    t = DE.pack_ground_truth(gts, img_ids, cat_ids, _area())
    # cells (image position, category position): (0,0) -, (0,1) [2], (1,0) [3, 8], (1,1) [1, 4, 5]
    assert t['gt_off'].dtype == np.int32 and t['gt_off'].tolist() == [0, 0, 1, 3, 6]
    assert t['gt_box'].dtype == np.float64 and t['gt_box'][:, 0].tolist() == [1, 2, 7, 0, 3, 4]
    all_, small, medium, large = 2, 4, 8, 16
    f = t['gt_flags'].tolist()
    assert f[0] == large                                    # area 1024: inside small [0, 1024] and medium [1024, 9216]
    assert f[1] == 1 | all_ | small | medium | large        # crowd: ignored everywhere
    assert f[2] == medium | large                           # 400: small only
    assert f[3] == medium | large                           # 100
    assert f[4] == all_ | small | medium | large            # ignore flag
    assert f[5] == small                                    # area 9216: medium and large
    # non-ignored boxes per (category, area): cat 3 has the 20x20 box only, cat 7 three regular boxes
    assert t['npig'].dtype == np.int64 and t['npig'].tolist() == [[1, 1, 0, 0], [3, 2, 2, 1]]
    assert t['gt_cap'] == 5
    with pytest.raises(ValueError):
        DE.pack_ground_truth([g(0, 10, 7, [0, 0, 1, 1])], img_ids, cat_ids, _area())


def test_ground_truth_defaults_follow_cocoeval():
    gts = [dict(image_id=1, category_id=1, bbox=[0, 0, 40, 40]),         # area from the box, id from the position
           dict(image_id=1, category_id=1, bbox=[0, 0, 4, 4], iscrowd=True, area=5000.0)]
    t = DE.pack_ground_truth(gts, [1], [1], _area())
    ev = cocoeval.COCOeval(gts, [])
    want = []
    for gg in ev.gts[(1, 1)]:
        f = 1 if gg['iscrowd'] else 0
        for a, (lo, hi) in enumerate(ev.params.areaRng):
            f |= (2 << a) if (gg['ignore'] or gg['area'] < lo or gg['area'] > hi) else 0
        want.append(f)
    assert t['gt_flags'].tolist() == want == [4 | 16, 1 | 2 | 4 | 8 | 16]           # 1600: all and medium


def test_class_table_follows_sorted_category_ids(tmp_path):
    from test_dataset import make_dataset
    db = make_dataset(str(tmp_path))
    table = DE.class_to_category(db)
    # classes: background, person (1), car (3), train (7): category positions in sorted(cat_ids)
    assert table.dtype == np.int32 and table.tolist() == [-1, 0, 1, 2]
    db._coco_ind_to_class_ind = {1: 3, 3: 1, 7: 2}
    assert DE.class_to_category(db).tolist() == [-1, 1, 2, 0]


def test_detection_slots_layout():
    d = lambda img, cat, s, b, **kw: dict(image_id=img, category_id=cat, score=s, bbox=b, **kw)
    dts = [d(2, 5, 0.5, [1, 2, 3, 4]), d(1, 5, 0.9, [0, 0, 1, 1]), d(2, 8, 0.7, [5, 6, 7, 8]), d(2, 9, 0.1, [0, 0, 1, 1])]
    det, num = DE.pack_detections(dts, [1, 2, 3], [5, 8])
    assert det.dtype == np.float64 and det.shape == (3, 2, 6) and num.tolist() == [1, 2, 0]
    assert det[1].tolist() == [[0, 0.5, 1, 2, 3, 4], [1, 0.7, 5, 6, 7, 8]]           # list order kept inside the image
    assert det[0, 0].tolist() == [0, 0.9, 0, 0, 1, 1] and not det[2].any()
    with pytest.raises(ValueError):                                                  # area must be the box's w * h
        DE.pack_detections([d(1, 5, 0.5, [0, 0, 2, 2], area=5.0)], [1], [5])
    with pytest.raises(ValueError):
        DE.pack_detections([d(1, 5, 0.5, [0, 0, 2, 2], id=0)], [1], [5])
    with pytest.raises(ValueError):
        DE.pack_detections([d(1, 5, 0.5, [0, 0, 2, 2])] * (DE.MAX_SLOTS + 1), [1], [5])


def test_evaluator_rejects_bad_setup_before_touching_the_device():
    with pytest.raises(ValueError):
        DE.DeviceCOCOeval.from_lists([], [], img_ids=[1, 1], cat_ids=[1])
    with pytest.raises(ValueError):
        DE.DeviceCOCOeval.from_lists([], [], img_ids=[], cat_ids=[1])
