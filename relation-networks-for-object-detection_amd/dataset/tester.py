"""Test-time drivers of `relation_rcnn/core/tester.py` on the HIP detector.

  pred_eval            :163-307  loop over a TestLoader, collect all_boxes[cls][image] = [k,5], `imdb.evaluate_detections`.
                                 device_eval=True: the detections stay on the device, are matched per batch by
                                 dataset/device_eval.py:DeviceCOCOeval and copied to the host once at the end.
                                 The per-class threshold / (soft-)NMS / max_per_image steps (:244-277) run in the detector's
                                 post-processing kernels (relnet_class_nms / relnet_image_topk); learn-NMS outputs are
                                 thresholded as :231-242.
  generate_proposals   :63-126   RPN-only pass, boxes mapped back to the original image scale, written as the
                                 `<name>_rpn.pkl` list the precomputed-proposal training reads (imdb.load_rpn_data).
                                 device_recall=True: the rois stay on the device and are scored per batch by
                                 dataset/device_recall.py:DeviceRecall; one device-to-host copy at the end builds the list.
  test_rpn             function/test_rpn.py:25-76  generate_proposals + imdb.evaluate_recall (or DeviceRecall).
"""
import os
import pickle
import time

import numpy as np
import torch


def _class_lists(out, b, num_classes, scale):
    """detections [n,6] (class, score, x1,y1,x2,y2) of image b -> list over classes of [k,5] (x1,y1,x2,y2,score)."""
    n = int(out['num_detections'][b])
    return _split_classes(out['detections'][b, :n].detach().float().cpu().numpy(), num_classes)


def _split_classes(det, num_classes):
    """float32 rows [n,6] (class, score, x1,y1,x2,y2) -> list over classes of [k,5] (x1,y1,x2,y2,score)."""
    res = [np.zeros((0, 5), np.float32) for _ in range(num_classes)]
    for c in range(1, num_classes):
        rows = det[det[:, 0] == c]
        if len(rows):
            res[c] = np.hstack((rows[:, 2:6], rows[:, 1:2])).astype(np.float32)
    return res


def pred_eval(detector, test_data, imdb, vis=False, thresh=1e-3, logger=None, device='cuda', device_eval=False):
    """Returns (info_str, stats, all_boxes).  `detector`: relnet_amd.detector.Detector (HAS_RPN graphs) or FPNDetector
    (precomputed proposals from the loader).  The detector divides boxes by im_info[2] itself (tester.py:156).
    device_eval: score on the device (DeviceCOCOeval): no explicit synchronisation and no device-to-host copy of the detections
    per batch (the loader's own host-to-device uploads may still wait); all_boxes, the detections pickle, the results json, info
    and stats are identical to the default path's."""
    if device_eval:
        return _pred_eval_device(detector, test_data, imdb, logger, device)
    num_images = imdb.num_images
    all_boxes = [[[] for _ in range(num_images)] for _ in range(imdb.num_classes)]
    t_net = []
    with torch.no_grad():
        for batch in test_data:
            t0 = time.time()
            out = _run_detector(detector, batch, device)
            torch.cuda.synchronize()
            t_net.append(time.time() - t0)
            for b, idx in enumerate(batch['index']):
                per_cls = _class_lists(out, b, imdb.num_classes, float(batch['im_info'][b, 2]))
                for c in range(1, imdb.num_classes):
                    all_boxes[c][idx] = per_cls[c]
    _dump_detections(imdb, all_boxes)
    info, stats = imdb.evaluate_detections(all_boxes)
    if logger:
        logger.info('evaluate detections: \n{}'.format(info))
        logger.info('net time per batch: %.4f s' % (float(np.mean(t_net)) if t_net else 0.0))
    return info, stats, all_boxes


def _dump_detections(imdb, all_boxes):
    for c in range(imdb.num_classes):
        for i in range(imdb.num_images):
            if len(all_boxes[c][i]) == 0:
                all_boxes[c][i] = np.zeros((0, 5), np.float32)
    det_file = os.path.join(imdb.result_path, imdb.name + '_detections.pkl')
    with open(det_file, 'wb') as f:
        pickle.dump(all_boxes, f, protocol=pickle.HIGHEST_PROTOCOL)


def _run_detector(detector, batch, device):
    data, im_info = batch['data'].to(device), batch['im_info'].to(device)
    if 'proposals' in batch:
        nprop = batch.get('num_proposals')                       # TestLoader pads the images' proposal lists to one length
        return detector.forward(data, batch['proposals'].to(device), im_info,
                                num_proposals=None if nprop is None else nprop.to(device=device, dtype=torch.int32))
    detector.im_hw = (int(data.shape[2]), int(data.shape[3]))
    return detector.forward(data, im_info)


def _pred_eval_device(detector, test_data, imdb, logger, device):
    """pred_eval(device_eval=True): each batch's detections are matched on the device as they come (no torch.cuda.synchronize,
    no copy to the host) and kept there as float32 (pred_eval's .float()); one device-to-host copy at the end builds all_boxes."""
    from .device_eval import DeviceCOCOeval
    scoring = 'test' not in imdb.image_set                 # test sets only write results
    ev, kept = None, []
    t0 = time.time()
    with torch.no_grad():
        for batch in test_data:
            out = _run_detector(detector, batch, device)
            det, num = out['detections'], out['num_detections']
            if scoring:
                if ev is None:
                    ev = DeviceCOCOeval(imdb, slots=det.shape[1], device=device)
                ev.add(det, num, batch['index'])
            kept.append((list(batch['index']), det.to(torch.float32, copy=True), num.to(torch.int32, copy=True)))
    all_boxes = [[[] for _ in range(imdb.num_images)] for _ in range(imdb.num_classes)]
    if kept:
        width = max(d.shape[1] for _, d, _ in kept)
        dets = torch.cat([torch.nn.functional.pad(d, (0, 0, 0, width - d.shape[1])) for _, d, _ in kept]).cpu().numpy()
        nums = torch.cat([n for _, _, n in kept]).cpu().numpy()
        row = 0
        for idx, _, _ in kept:
            for i in idx:
                per_cls = _split_classes(dets[row, :nums[row]], imdb.num_classes)
                for c in range(1, imdb.num_classes):
                    all_boxes[c][i] = per_cls[c]
                row += 1
    t_net = time.time() - t0
    _dump_detections(imdb, all_boxes)
    if ev is None:
        info, stats = imdb.evaluate_detections(all_boxes)
    else:
        info, stats = imdb.evaluate_detections_device(ev, all_boxes)
    if logger:
        logger.info('evaluate detections: \n{}'.format(info))
        logger.info('net time per batch: %.4f s' % (t_net / max(len(kept), 1)))
    return info, stats, all_boxes


def _proposal_values(cfg, proposal_settings):
    """(pre_nms_top_n, post_nms_top_n, nms_thresh, min_size) handed to propose_batch: the detector's rpn_* values, or with
    proposal_settings the proposal_* ones (TEST.PROPOSAL_*; ValueError naming the first that is not set)."""
    if not proposal_settings:
        return cfg.rpn_pre_nms_top_n, cfg.rpn_post_nms_top_n, cfg.rpn_nms_thresh, cfg.rpn_min_size
    names = ('proposal_pre_nms_top_n', 'proposal_post_nms_top_n', 'proposal_nms_thresh', 'proposal_min_size')
    for name in names:
        if getattr(cfg, name, None) is None:
            raise ValueError("proposal_settings=True needs cfg.%s (TEST.%s; Config.from_experiment fills it)" % (name, name.upper()))
    return tuple(getattr(cfg, name) for name in names)


def generate_proposals(detector, test_data, imdb, thresh=0.0, device='cuda', save=True, device_recall=False, proposal_settings=False):
    """tester.py:63-126: per image [n,5] = (x1,y1,x2,y2 at the ORIGINAL scale, rpn score); returns the list and writes
    `<rpn_path>/rpn_data/<name>_rpn.pkl` (+ `_full_rpn.pkl` when thresh > 0).
    device_recall=True: returns (list, DeviceRecall) -- every batch's rois are scored on the device as they come (scaled and
    thresholded there as below, no copy to the host) and copied to the host once at the end; the list is the same.
    proposal_settings=True: the proposals are cut with cfg.proposal_* (TEST.PROPOSAL_PRE_NMS_TOP_N 20000 -> PROPOSAL_POST_NMS_TOP_N 2000,
    the values the reference's tester.py:78-79 symbol is built with and the rcnn_fpn_* experiments are defined on) instead of the
    detector's cfg.rpn_* (6000 -> 300); ValueError before any device work if one of the four is None."""
    pre, post, nms_thresh, min_size = _proposal_values(detector.cfg, proposal_settings)
    if device_recall:
        return _generate_proposals_device(detector, test_data, imdb, thresh, device, save, proposal_settings=proposal_settings)
    from ..operator_py.proposal import propose_batch
    imdb_boxes, original = [None] * imdb.num_images, [None] * imdb.num_images
    c = detector.cfg
    with torch.no_grad():
        for batch in test_data:
            data, im_info = batch['data'].to(device), batch['im_info'].to(device)
            f = detector.backbone.forward(data)
            rois, scores = propose_batch(f['rpn_cls_score'].float(), f['rpn_bbox_pred'].float(), im_info, detector.anchors,
                                         c.feat_stride, pre, post, nms_thresh, min_size,
                                         im_hw=(int(data.shape[2]), int(data.shape[3])), softmax_pairs=True)
            for b, idx in enumerate(batch['index']):
                boxes = rois[b, :, 1:].cpu().numpy() / float(batch['im_info'][b, 2])
                dets = np.hstack((boxes, scores[b].cpu().numpy().reshape(-1, 1))).astype(np.float32)
                original[idx] = dets
                imdb_boxes[idx] = dets[np.where(dets[:, 4] > thresh)[0], :]
    assert all(x is not None for x in imdb_boxes), 'calculations not complete'
    if save:
        imdb.save_rpn_data(imdb_boxes)
        if thresh > 0:
            imdb.save_rpn_data(original, full=True)
    return imdb_boxes


def _rpn_batch(detector, batch, device, proposal_settings=False):
    from ..operator_py.proposal import propose_batch
    c = detector.cfg
    pre, post, nms_thresh, min_size = _proposal_values(c, proposal_settings)
    data, im_info = batch['data'].to(device), batch['im_info'].to(device)
    f = detector.backbone.forward(data)
    return propose_batch(f['rpn_cls_score'].float(), f['rpn_bbox_pred'].float(), im_info, detector.anchors, c.feat_stride,
                         pre, post, nms_thresh, min_size,
                         im_hw=(int(data.shape[2]), int(data.shape[3])), softmax_pairs=True), im_info


def _generate_proposals_device(detector, test_data, imdb, thresh, device, save, proposal_settings=False):
    """generate_proposals(device_recall=True): the proposal list is built from one device-to-host copy of every batch's rois
    and scores with the default path's numpy expressions, so it is identical to it.  proposal_settings: as generate_proposals."""
    from .device_recall import DeviceRecall
    _proposal_values(detector.cfg, proposal_settings)          # (refuse unset values before the evaluator touches the device)
    ev = DeviceRecall(imdb, device=device)
    kept = []
    with torch.no_grad():
        for batch in test_data:
            (rois, scores), im_info = _rpn_batch(detector, batch, device, proposal_settings)
            scores = scores.reshape(rois.shape[0], rois.shape[1])
            ev.add(rois[:, :, 1:], None, batch['index'], scores=scores, thresh=thresh, scale=im_info[:, 2])
            kept.append((list(batch['index']), [float(batch['im_info'][b, 2]) for b in range(len(batch['index']))],
                         rois[:, :, 1:].to(torch.float32, copy=True), scores.to(torch.float32, copy=True)))
    imdb_boxes, original = [None] * imdb.num_images, [None] * imdb.num_images
    if kept:
        width = max(r.shape[1] for _, _, r, _ in kept)
        rois = torch.cat([torch.nn.functional.pad(r, (0, 0, 0, width - r.shape[1])) for _, _, r, _ in kept]).cpu().numpy()
        scores = torch.cat([torch.nn.functional.pad(s, (0, width - s.shape[1])) for _, _, _, s in kept]).cpu().numpy()
        row = 0
        for idx, scales, r, _ in kept:
            n = r.shape[1]
            for i, scale in zip(idx, scales):
                boxes = rois[row, :n] / scale
                dets = np.hstack((boxes, scores[row, :n].reshape(-1, 1))).astype(np.float32)
                original[i] = dets
                imdb_boxes[i] = dets[np.where(dets[:, 4] > thresh)[0], :]
                row += 1
    assert all(x is not None for x in imdb_boxes), 'calculations not complete'
    if save:
        imdb.save_rpn_data(imdb_boxes)
        if thresh > 0:
            imdb.save_rpn_data(original, full=True)
    return imdb_boxes, ev


def test_rpn(detector, test_data, imdb, thresh=0.0, device='cuda', device_eval=False, logger=None, proposal_settings=False):
    """function/test_rpn.py:25-76: proposals of every test image (generate_proposals, which writes `<name>_rpn.pkl`) scored by
    imdb.evaluate_recall against imdb.gt_roidb(); returns all_log_info.  device_eval=True scores them on the device
    (DeviceRecall) and returns the same string.
    The reference builds its network with sym.get_symbol_rpn, which none of its shipped symbol files defines; the RPN here is
    the detector's backbone RPN head + propose_batch, as generate_proposals uses it.  `test_data` is a non-shuffled
    TestLoader(imdb.gt_roidb(), cfg, has_rpn=True).  proposal_settings: as generate_proposals (TEST.PROPOSAL_*, 20000 -> 2000)."""
    if device_eval:
        _, ev = generate_proposals(detector, test_data, imdb, thresh=thresh, device=device, device_recall=True,
                                   proposal_settings=proposal_settings)
        all_log_info = ev.summarize()[0]
    else:
        imdb_boxes = generate_proposals(detector, test_data, imdb, thresh=thresh, device=device, proposal_settings=proposal_settings)
        all_log_info = imdb.evaluate_recall(imdb.gt_roidb(), candidate_boxes=imdb_boxes)
    if logger:
        logger.info(all_log_info)
    return all_log_info
