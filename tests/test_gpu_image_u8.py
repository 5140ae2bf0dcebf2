"""uint8 image input on the GPU: the batched resize (relnet_resize_u8) against dataset/image.py:resize, the unfused transform
(relnet_image_transform_u8) against transform + tensor_vstack, the uint8 fused stem (relnet_stem_fused_u8) against the fp32 fused
stem, and the detector / captured step / trainer / float32 backbone on the uint8 canvas against the same on the host-preprocessed
fp32 tensor.  Everything after the first layer gets identical bits, so the comparisons are exact -- except where a downstream
kernel is not bit-reproducible from run to run (named at the comparison)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEANS = (103.06, 115.90, 123.15)


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib, backbone, detector, train
    from relnet_amd.dataset import image as IMG
    lib.load()
    return ops, backbone, detector, train, IMG


# (h, w, target, cap, flip): up- and downscaling, the max_size cap, odd sizes, mirrored sources
SOURCES = [(48, 64, 60, 100, False), (37, 53, 64, 96, True), (123, 457, 120, 160, False), (201, 99, 50, 80, True),
           (17, 29, 40, 200, False), (90, 90, 90, 90, True)]


def _batch(IMG, sources, stride, seed=0):
    """-> (sources, the host-side table, im_info, float batch of get_image + tensor_vstack, padded uint8 images)."""
    rng = np.random.default_rng(seed)
    raws, info, ts, padded = [], [], [], []
    for h, w, target, cap, flip in sources:
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        s, nh, nw, ph, pw = IMG.resize_plan(h, w, target, cap, stride)
        raws.append((im, flip, s, nh, nw))
        out, s2 = IMG.resize(im[:, ::-1, :] if flip else im, target, cap, stride=stride)
        assert s2 == s and out.shape[:2] == (ph, pw)
        padded.append(out)
        ts.append(IMG.transform(out, np.array(MEANS)))
        info.append([ph, pw, s])
    return IMG.pack_raw(raws, info), np.array(info, np.float32), IMG.tensor_vstack(ts), padded


def _device(pk):
    return dict(image_src=torch.as_tensor(pk['image_src']).cuda(), image_table=torch.as_tensor(pk['image_table']).cuda(),
                image_scale=torch.as_tensor(pk['image_scale']).cuda(), canvas_hw=pk['canvas_hw'])


def _canvas(rn, pk):
    from relnet_amd.dataset import device_images
    return device_images(_device(pk))


@pytest.mark.parametrize('stride', [0, 32])
def test_resize_u8_bit_identical_to_numpy(rn, stride):
    ops, backbone, detector, train, IMG = rn
    pk, info, data, padded = _batch(IMG, SOURCES, stride)
    canvas = _canvas(rn, pk).cpu().numpy()
    Hc, Wc = pk['canvas_hw']
    assert canvas.shape == (len(SOURCES), Hc, Wc, 3) and canvas.dtype == np.uint8
    for b, out in enumerate(padded):
        want = np.zeros((Hc, Wc, 3), np.uint8)
        want[:out.shape[0], :out.shape[1]] = out.astype(np.uint8)       # stride padding and the rest of the slot: 0
        bad = np.argwhere(canvas[b] != want)
        assert bad.size == 0, (b, bad[:5], canvas[b][tuple(bad[0])], want[tuple(bad[0])])


def test_image_transform_u8_equals_transform_and_vstack(rn):
    ops, backbone, detector, train, IMG = rn
    pk, info, data, _ = _batch(IMG, SOURCES, 32, seed=1)
    canvas = _canvas(rn, pk)
    im_info = torch.as_tensor(info).cuda()
    assert (info[:, 0] < canvas.shape[1]).any() and (info[:, 1] < canvas.shape[2]).any()      # extents smaller than the canvas
    x = ops.image_transform_u8(canvas, MEANS, im_info)
    assert x.dtype == torch.float32 and torch.equal(x.cpu(), torch.as_tensor(data))
    xb = ops.image_transform_u8(canvas, MEANS, im_info, dtype=torch.bfloat16)
    assert torch.equal(xb.cpu(), torch.as_tensor(data).to(torch.bfloat16))


def _stem_weights(backbone, ops, seed):
    p = backbone.init_params(seed=seed)
    w1, b1 = backbone.fold_bn(p['conv1_weight'], p['bn_conv1_gamma'], p['bn_conv1_beta'], p['bn_conv1_moving_mean'],
                              p['bn_conv1_moving_var'])
    return ops.pack_stem_weight(w1, torch.bfloat16, 'cuda'), b1.float().cuda().contiguous()


def test_stem_fused_u8_bit_identical_to_fp32_stem(rn):
    ops, backbone, detector, train, IMG = rn
    w, b = _stem_weights(backbone, ops, 3)
    # mixed-extent batch from the resize kernel
    pk, info, data, _ = _batch(IMG, SOURCES, 32, seed=2)
    canvas = _canvas(rn, pk)
    im_info = torch.as_tensor(info).cuda()
    want = ops.stem_fused(torch.as_tensor(data).cuda(), w, b)
    got = ops.stem_fused(canvas, w, b, im_info, MEANS)
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(ops.stem_fused(ops.image_transform_u8(canvas, MEANS, im_info), w, b), want)
    # 600 x 1000 canvas, the second image with a smaller extent; and im_info=None: the whole canvas is the image
    g = torch.Generator().manual_seed(5)
    big = torch.randint(0, 256, (2, 600, 1000, 3), generator=g, dtype=torch.uint8).cuda()
    im_info = torch.tensor([[600, 1000, 1.0], [576, 800, 1.0]]).cuda()
    ref = ops.image_transform_u8(big, MEANS, im_info)
    assert float(ref[1, :, 576:].abs().max()) == 0 and float(ref[1, :, :, 800:].abs().max()) == 0
    assert torch.equal(ops.stem_fused(big, w, b, im_info, MEANS), ops.stem_fused(ref, w, b))
    assert torch.equal(ops.stem_fused(big, w, b, None, MEANS), ops.stem_fused(ops.image_transform_u8(big, MEANS), w, b))


DET_SOURCES = [(150, 200, 128, 192, False), (160, 120, 128, 192, True)]       # two images of different sizes


def _det_inputs(rn, stride=0):
    ops, backbone, detector, train, IMG = rn
    pk, info, data, _ = _batch(IMG, DET_SOURCES, stride, seed=3)
    return _canvas(rn, pk), torch.as_tensor(info).cuda(), torch.as_tensor(data).cuda()


@pytest.mark.parametrize('learn_nms', [False, True])         # configs[1] (relation, soft-NMS), configs[2] (relation + learn-NMS)
def test_detector_on_uint8_equals_fp32(rn, learn_nms):
    ops, backbone, detector, train, IMG = rn
    canvas, im_info, data = _det_inputs(rn)
    p = backbone.init_params(seed=4)
    cfg = detector.Config(); cfg.rpn_post_nms_top_n = 64
    assert cfg.softnms and cfg.pixel_means == MEANS
    if learn_nms:
        cfg.learn_nms, cfg.first_n = True, 50
    det = detector.Detector(p, dtype=torch.bfloat16, im_hw=tuple(data.shape[2:]), cfg=cfg)
    with torch.no_grad():
        a = det.forward(data, im_info, keep_features=True)
        b = det.forward(canvas, im_info, keep_features=True)
    assert torch.equal(a['features']['conv4'], b['features']['conv4'])
    keys = ['rois', 'cls_score', 'bbox_pred', 'detections', 'num_detections']
    keys += ['nms_final_score', 'sorted_bbox'] if learn_nms else ['cls_prob', 'pred_boxes']
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    if not learn_nms:
        # the per-class lists of relnet_class_nms_topk stop once a pick cannot reach the image's top max_per_image scores, and when
        # that is known depends on the order the classes finish in: their LENGTHS are not deterministic from run to run (the
        # detections are).  Every list is a prefix of the full per-class list, so the common prefixes agree.
        n = torch.minimum(a['class_counts'], b['class_counts'])
        live = torch.arange(a['class_dets'].shape[2], device='cuda')[None, None, :] < n[..., None]
        assert torch.equal(a['class_dets'][live], b['class_dets'][live])
    assert int(a['num_detections'].min()) > 0


def test_captured_steps_on_uint8_inputs(rn):
    """InFlight with uint8 resident canvases, refreshed in place between replays: every replay is the eager forward."""
    ops, backbone, detector, train, IMG = rn
    canvas, im_info, data = _det_inputs(rn)
    p = backbone.init_params(seed=4)
    cfg = detector.Config(); cfg.rpn_post_nms_top_n = 64
    dets = [detector.Detector(p, dtype=torch.bfloat16, im_hw=tuple(data.shape[2:]), cfg=cfg) for _ in range(2)]
    for d in dets:
        d.overlap_rpn = False
    g = torch.Generator().manual_seed(9)
    canv = [canvas.clone(), torch.flip(canvas, [2]).contiguous()]
    keys = ('rois', 'cls_prob', 'pred_boxes', 'detections', 'num_detections')
    with torch.no_grad():
        fl = detector.InFlight([lambda i=i: dets[i].forward(canv[i], im_info) for i in range(2)])
        for rnd in range(2):
            if rnd == 1:
                for c in canv:
                    c.copy_(torch.randint(0, 256, c.shape, generator=g, dtype=torch.uint8).cuda())
                torch.cuda.synchronize()
            ref = [{k: v.clone() for k, v in dets[i].forward(canv[i], im_info).items() if k in keys} for i in range(2)]
            fp = dets[0].forward(ops.image_transform_u8(canv[0], MEANS, im_info), im_info)
            assert torch.equal(fp['rois'], ref[0]['rois'])
            torch.cuda.synchronize()
            assert [fl.submit() for _ in range(2)] == [0, 1]
            for i in range(2):
                out = fl.result(i)
                for k in keys:
                    assert torch.equal(out[k], ref[i][k]), (rnd, i, k)


def test_trainer_step_on_uint8_equals_fp32(rn):
    """configs[2] (relation + learn-NMS end2end), the setup of test_gpu_train_step.py's gradient test on a uint8 image whose stride
    padding (u8 0 -> -mean) is part of the canvas: the same stem output, losses and decisions as on the fp32 tensor, the same
    gradients up to the backward pass's run-to-run last-bit differences."""
    ops, backbone, detector, train, IMG = rn
    pk, info, data, _ = _batch(IMG, [(120, 150, 120, 200, True)], 32, seed=6)
    canvas, im_info, data = _canvas(rn, pk), torch.as_tensor(info).cuda(), torch.as_tensor(data).cuda()
    H, W = ops.image_hw(canvas)
    assert (H, W) == (128, 160) == tuple(data.shape[2:])
    p = backbone.init_params(seed=31)
    g = torch.Generator().manual_seed(32)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    p['conv_new_1_bias'] = torch.rand(256, generator=g) * 0.1 + 0.05
    g_ = torch.Generator().manual_seed(77)
    p['nms_logit_bias'] = torch.zeros(5)
    for k in ('nms_logit_weight', 'nms_rank_weight', 'roi_feat_embedding_weight', 'nms_query_1_weight', 'nms_key_1_weight',
              'nms_linear_out_1_weight', 'nms_pair_pos_fc1_1_weight'):
        p[k] = torch.randn(p[k].shape, generator=g_) * 0.05
    cfg = train.TrainConfig()
    cfg.rpn_post_nms_top_n, cfg.learn_nms, cfg.first_n = 40, True, 24
    rng = np.random.default_rng(33)
    G = 4
    gt = np.zeros((1, G, 5), np.float32)
    x1, y1 = rng.uniform(0, W - 70, G), rng.uniform(0, H - 70, G)
    gt[0, :, 0], gt[0, :, 1], gt[0, :, 2], gt[0, :, 3] = x1, y1, x1 + rng.uniform(30, 69, G), y1 + rng.uniform(30, 69, G)
    gt[0, :, 4] = rng.integers(1, 81, G)
    from relnet_amd.dataset.loader import _conv4_size
    L, Tg, Wg = train.assign_anchor((_conv4_size(H), _conv4_size(W)), gt[0], (H, W), cfg, seed=31)
    d = lambda a: torch.as_tensor(a).cuda()
    tr = train.Trainer(p, cfg, im_hw=(H, W))
    # gt boxes ON some proposals (they do not depend on gt), so that the learn-NMS head has positive targets (as in the gradient test)
    out = tr.forward_backward(data, im_info, d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
    gt[0, :, :4] = out['rois'][0, :cfg.rpn_post_nms_top_n, 1:5].cpu().numpy()[[0, 7, 14, 21]]
    L, Tg, Wg = train.assign_anchor((_conv4_size(H), _conv4_size(W)), gt[0], (H, W), cfg, seed=31)
    assert tr._frozen_backbone is not None
    assert torch.equal(tr._frozen_backbone.forward_res2(canvas, im_info), tr._frozen_backbone.forward_res2(data, im_info))
    res = []
    for x in (data, canvas):
        out = tr.forward_backward(x, im_info, d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
        torch.cuda.synchronize()
        res.append(({k: v.clone() for k, v in out.items() if torch.is_tensor(v)}, tr.W.grad.clone(), tr.Bv.grad.clone()))
    (oa, wa, ba), (ob, wb, bb) = res
    losses = [k for k in oa if 'loss' in k]
    assert 'rpn_bbox_loss' in losses and 'bbox_loss' in losses
    for k in losses + ['rois', 'label', 'cls_score', 'bbox_pred']:
        assert torch.equal(oa[k], ob[k]), k
    for a, b, kind in ((wa, wb, 'weights'), (ba, bb, 'biases')):
        # The backward pass is not bit-reproducible from run to run (its gradient sums differ in the last bit between two runs on the
        # SAME input), so the gradients are compared at 1e-5 after the bit-exact stem / losses / decisions above.  This one-image
        # learn-NMS step also leaves non-finite entries in the flat gradient buffer on the fp32 input; they must sit at the same places.
        fa, fb = torch.isfinite(a), torch.isfinite(b)
        assert torch.equal(fa, fb), kind
        da, db = a[fa].double(), b[fb].double()
        assert float(da.norm()) > 0 and float((da - db).norm() / da.norm()) < 1e-5, kind


@pytest.mark.parametrize('impl,stem', [('hip32', 'hip'), ('hip', 'hip3'), ('hip', 'library')])
def test_backbone_paths_without_fused_stem_take_uint8(rn, impl, stem):
    """impl 'hip32' (float32 parity trunk) and the bf16 trunk with the three-launch / library stem convert the canvas on the device
    (relnet_image_transform_u8) and give what they give on the fp32 tensor."""
    ops, backbone, detector, train, IMG = rn
    canvas, im_info, data = _det_inputs(rn)
    p = backbone.init_params(seed=8)
    dt = torch.float32 if impl == 'hip32' else torch.bfloat16
    bb = backbone.Backbone(p, dtype=dt, impl=impl, stem=stem)
    with torch.no_grad():
        a = bb.forward(data)
        b = bb.forward(canvas, im_info=im_info)
    for k in ('conv4', 'conv5', 'conv_new_1_relu', 'rpn_cls_score', 'rpn_bbox_pred'):
        assert torch.equal(a[k], b[k]), k
