"""The learn-NMS head as one module: learn_nms.rank_stage is the ranking of the test branch (LearnNMS.forward) and of the train branch
(Trainer._lnms_forward_backward -> learn_nms.LearnNMSTrain) bit for bit; the front ends ops.lnms_* refuse a wrong operand on the host,
before any launch; and each of them issues exactly the launch the hand-marshalled call issued (argument order, strides, delta_off,
Npad / Fpad)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import cases
import class_specific_cases as CS

pytestmark = pytest.mark.gpu

NORM = ((0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2))
#: name -> (rois N, foreground classes C, first_n F, seed, n_valid of the two images).  'f20' is class_specific_cases.LNMS_CASES['cs_n60_c6_f20_norm'];
#: 'f33': pad32(F) = 64 differs from F and F is no multiple of 32
RANK_CASES = {'f20': CS.LNMS_CASES['cs_n60_c6_f20_norm'][:4] + ([60, 53],), 'f33': (40, 6, 33, 25, [40, 36])}


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib, backbone, learn_nms, train
    from types import SimpleNamespace
    lib.load()
    return SimpleNamespace(ops=ops, lib=lib, backbone=backbone, learn_nms=learn_nms, train=train)


def _d(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _inputs(name):
    """Two images of the case: cls_score [2,N,C+1], bbox_pred [2,N,4(C+1)] (its first 8 columns are the class-agnostic head), rois, im_info, feat, params."""
    n, c, first_n, seed, nv = RANK_CASES[name]
    ins = [CS.lnms_case(n, c, seed + b) for b in range(2)]
    cls_score, bbox_pred, rois = (_d(np.stack([i[k] for i in ins])) for k in (0, 1, 2))
    im_info = _d(np.concatenate([i[3] for i in ins]))
    feat = _d(np.stack([i[4] for i in ins]))
    return cls_score, bbox_pred, rois, im_info, feat, ins[0][5], _d(np.array(nv, np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# 1. one ranking
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('class_agnostic', [True, False])
@pytest.mark.parametrize('name', sorted(RANK_CASES))
def test_train_and_test_branch_rank_as_rank_stage(rn, name, class_agnostic):
    n, c, first_n, seed, nv_host = RANK_CASES[name]
    cls_score, bbox_pred, rois, im_info, feat, p, nv = _inputs(name)
    if class_agnostic:
        bbox_pred = bbox_pred[:, :, :8].contiguous()
    want = rn.learn_nms.rank_stage(cls_score, bbox_pred, rois, im_info, first_n, class_agnostic, NORM[0], NORM[1], nv)
    assert want.rank_idx.shape == (2, c, first_n) and int(want.rank_idx[1].max()) < nv_host[1] < n       # image 1's padding rows are never ranked
    assert want.boxes.shape == ((2, n, 4) if class_agnostic else (2, n, c, 4))
    # the test branch
    m = rn.learn_nms.LearnNMS({k: torch.as_tensor(v) for k, v in p.items()}, c, first_n, bbox_means=NORM[0], bbox_stds=NORM[1],
                              class_agnostic=class_agnostic)
    r = m.forward(cls_score, bbox_pred, rois, im_info, feat, n_valid=nv)
    assert torch.equal(r['sorted_score'], want.sorted_score) and torch.equal(r['sorted_bbox'], want.sorted_bbox)
    # the train branch
    tp = rn.backbone.init_params(seed=3, num_classes=c + 1, num_reg_classes=2 if class_agnostic else c + 1)
    cfg = rn.train.TrainConfig()
    cfg.learn_nms, cfg.first_n, cfg.num_classes, cfg.class_agnostic = True, first_n, c + 1, class_agnostic
    cfg.bbox_means, cfg.bbox_stds = NORM
    tr = rn.train.Trainer(tp, cfg, im_hw=(600, 1000))
    gt = torch.zeros((2, 2, 5), device='cuda')
    gt[:, :, :4] = rois[:, :2, 1:]
    gt[:, :, 4] = 1.0
    tr.W.grad.zero_(); tr.Bv.grad.zero_()
    tr._relayout.run()
    _, _, lo = tr._lnms_forward_backward(cls_score, bbox_pred, rois, im_info, feat.to(torch.bfloat16), gt,
                                         torch.full((2,), 2, dtype=torch.int32, device='cuda'), n_valid=nv)
    tr._flush_wgrads()
    torch.cuda.synchronize()
    assert torch.equal(lo['sorted_score'], want.sorted_score) and torch.equal(lo['nms_rank_idx'], want.rank_idx)
    assert torch.equal(lo['nms_class_boxes'], want.class_boxes)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the front ends refuse on the host
# ---------------------------------------------------------------------------------------------------------------------
def _valid_operands(B=2, N=40, C=6, F=20, T=5):
    """name -> keyword arguments every front end accepts (shapes only matter here: nothing is launched)."""
    z = lambda *s, dt=torch.float32: torch.zeros(s, device='cuda', dtype=dt)
    bf, i32 = torch.bfloat16, torch.int32
    ranks = z(B, C, F, dt=i32)
    return {
        'lnms_prepare': dict(cls_score=z(B, N, C + 1), bbox_pred=z(B, N, 8), rois=z(B, N, 5), im_info=z(B, 3), n_valid=z(B, dt=i32)),
        'lnms_sort': dict(prob=z(B, N, C), boxes=z(B, N, 4), first_n=F),
        'lnms_embed': dict(roi_emb=z(B * N, 128, dt=bf), rank_feat=z(F, 128), rank_idx=ranks),
        'lnms_score': dict(x=z(B, C, F, 128, dt=bf), att=z(B * C, F, 1024, dt=bf), w_logit=z(5, 128), b_logit=z(5), sorted_score=z(B, F, C),
                           sorted_bbox=z(B, F, C, 4), class_max=z(B, C), im_info=z(B, 3)),
        'lnms_pad_params': dict(wo=z(128, 128, dt=bf), bo=z(128), wl=z(T, 128, dt=bf), bl=z(T), wout_pad=z(1024, 128, dt=bf), bout_pad=z(1024),
                                wl_pad=z(64, 128, dt=bf), bl_pad=z(64)),
        'lnms_gather_bias': dict(img=z(B, 16, N, 64), rank_idx=ranks),
        'lnms_residual_relu': dict(att=z(B * C, F, 1024, dt=bf), x=z(B * C, F, 128, dt=bf)),
        'lnms_cond_multi': dict(logit=z(B * C * F, 64), sorted_score=z(B, F, C), T=T),
        'lnms_cond_bwd': dict(d_multi=z(B, F, C, T), cond=z(B, F, C, T), sorted_score=z(B, F, C)),
        'lnms_take_bwd': dict(d_x=z(B, C, F, 128, dt=bf), rank_idx=ranks, N=N),
        'lnms_softmax_bwd': dict(prob=z(B, N, C), d_prob=z(B, N, C), d_cls=z(B, N + 3, C + 1)),
    }


def _wrong_operands(B=2, N=40, C=6, F=20, T=5):
    """(front end, what is wrong, the replaced keyword arguments)."""
    z = lambda *s, dt=torch.float32: torch.zeros(s, device='cuda', dtype=dt)
    bf, i32, i64 = torch.bfloat16, torch.int32, torch.int64
    return [
        ('lnms_prepare', 'n_valid of length B + 1', dict(n_valid=z(B + 1, dt=i32))),
        ('lnms_prepare', 'int64 n_valid', dict(n_valid=z(B, dt=i64))),
        ('lnms_prepare', 'float64 scores', dict(cls_score=z(B, N, C + 1, dt=torch.float64))),
        ('lnms_prepare', 'rois of another N', dict(rois=z(B, N + 1, 5))),
        ('lnms_prepare', 'transposed bbox_pred', dict(bbox_pred=z(B, 8, N).permute(0, 2, 1))),
        ('lnms_prepare', 'three means', dict(means=(0.0, 0.0, 0.0))),
        ('lnms_prepare', 'class-specific head of 8 columns', dict(class_agnostic=False)),
        ('lnms_prepare', 'delta_off past the row', dict(delta_off=8)),
        ('lnms_sort', 'first_n > N', dict(first_n=N + 1)),
        ('lnms_sort', 'permuted prob', dict(prob=z(B, C, N).permute(0, 2, 1))),
        ('lnms_sort', 'boxes of another N', dict(boxes=z(B, N - 1, 4))),
        ('lnms_embed', 'int64 rank_idx', dict(rank_idx=z(B, C, F, dt=i64))),
        ('lnms_embed', 'fewer rows than ranks (N < F)', dict(roi_emb=z(B * (F - 1), 128, dt=bf))),
        ('lnms_embed', 'rank_feat of another F', dict(rank_feat=z(F + 1, 128))),
        ('lnms_score', 'fp32 att beside a bf16 x', dict(att=z(B * C, F, 1024))),
        ('lnms_score', 'sorted_score in rank_idx layout', dict(sorted_score=z(B, C, F))),
        ('lnms_score', 'six thresholds', dict(w_logit=z(6, 128), b_logit=z(6))),
        ('lnms_pad_params', 'T = 65', dict(wl=z(65, 128, dt=bf), bl=z(65))),
        ('lnms_pad_params', 'fp32 nms_linear_out_1 where bf16 is read', dict(wo=z(128, 128))),
        ('lnms_pad_params', 'a 128-row padded operand', dict(wout_pad=z(128, 128, dt=bf))),
        ('lnms_gather_bias', 'int64 rank_idx', dict(rank_idx=z(B, C, F, dt=i64))),
        ('lnms_gather_bias', 'first_n > N', dict(img=z(B, 16, F - 1, 32))),
        ('lnms_gather_bias', 'permuted table', dict(img=z(B, 16, 64, N).permute(0, 1, 3, 2))),
        ('lnms_residual_relu', 'fp32 att where bf16 is read', dict(att=z(B * C, F, 1024))),
        ('lnms_residual_relu', 'permuted x', dict(x=z(F, B * C, 128, dt=bf).permute(1, 0, 2))),
        ('lnms_cond_multi', 'T = 9', dict(T=9)),
        ('lnms_cond_multi', 'logit rows of another F', dict(logit=z(B * C * (F - 1), 64))),
        ('lnms_cond_multi', 'bf16 logit', dict(logit=z(B * C * F, 64, dt=bf))),
        ('lnms_cond_bwd', 'T = 9', dict(d_multi=z(B, F, C, 9), cond=z(B, F, C, 9))),
        ('lnms_cond_bwd', 'permuted d_multi', dict(d_multi=z(B, C, F, T).permute(0, 2, 1, 3))),
        ('lnms_take_bwd', 'int64 rank_idx', dict(rank_idx=z(B, C, F, dt=i64))),
        ('lnms_take_bwd', 'fp32 d_x where bf16 is read', dict(d_x=z(B, C, F, 128))),
        ('lnms_take_bwd', 'non-contiguous d_x (a permuted view)', dict(d_x=z(B, F, C, 128, dt=bf).permute(0, 2, 1, 3))),
        ('lnms_take_bwd', 'C = 129', dict(d_x=z(B, 129, F, 128, dt=bf), rank_idx=z(B, 129, F, dt=i32))),
        ('lnms_take_bwd', 'first_n > N', dict(N=F - 1)),
        ('lnms_softmax_bwd', 'd_cls_out whose last dimension is not C + 1', dict(d_cls=z(B, N + 3, C + 2))),
        ('lnms_softmax_bwd', 'd_cls_out with R < N', dict(d_cls=z(B, N - 1, C + 1))),
        ('lnms_softmax_bwd', 'bf16 d_cls_out', dict(d_cls=z(B, N + 3, C + 1, dt=bf))),
        ('lnms_softmax_bwd', 'd_prob of another C', dict(d_prob=z(B, N, C + 1))),
    ]


def test_front_ends_reject_before_they_launch(rn):
    launched = []

    def recorder(name):
        launched.append(name)
        return contextlib.nullcontext()
    valid, wrong = _valid_operands(), _wrong_operands()
    assert {w[0] for w in wrong} == set(valid)             # every front end is tried
    accepted = []
    saved = rn.lib.timing_hook
    rn.lib.timing_hook = recorder
    try:
        for fn, what, repl in wrong:
            kw = dict(valid[fn])
            kw.update(repl)
            try:
                getattr(rn.ops, fn)(**kw)
                accepted.append('%s accepted %s' % (fn, what))
            except Exception:
                pass
    finally:
        rn.lib.timing_hook = saved
    assert not accepted, accepted
    assert not launched, launched


# ---------------------------------------------------------------------------------------------------------------------
# 3. the front ends issue the hand-marshalled launches
# ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    if a.dtype == torch.bfloat16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def test_front_ends_equal_the_raw_calls(rn):
    ops, call, s = rn.ops, rn.lib.call, rn.ops._stream()
    n, c, first_n, seed, _ = RANK_CASES['f20']
    cls_score, bbox_pred, rois, im_info, _, _, nv = _inputs('f20')
    B, N, C1, C, F, T = 2, n, c + 1, c, first_n, 5
    BC = B * C
    dev, f32, bf = cls_score.device, torch.float32, torch.bfloat16
    g = torch.Generator(device='cuda').manual_seed(11)
    rnd = lambda *shape, dt=f32: torch.randn(shape, device=dev, generator=g).to(dt)
    e = lambda *shape, dt=f32: torch.empty(shape, device=dev, dtype=dt)
    means, stds = [(ctypes.c_float * 4)(*v) for v in NORM]
    cs2, bp2 = cls_score.view(B * N, C1), bbox_pred.view(B * N, 4 * C1)
    # prepare: class-agnostic at two delta_off (the second one is class 1's columns of the wide head), class-specific
    for off in (4, 8):
        prob, boxes = ops.lnms_prepare(cls_score, bbox_pred, rois, im_info, True, NORM[0], NORM[1], nv, delta_off=off)
        prob_r, boxes_r = e(B, N, C), e(B, N, 4)
        call('relnet_lnms_prepare_ex', cs2.data_ptr(), cs2.stride(0), bp2.data_ptr(), bp2.stride(0), rois.data_ptr(), im_info.data_ptr(),
             prob_r.data_ptr(), boxes_r.data_ptr(), B, N, C1, off, means, stds, nv.data_ptr(), s)
        assert _same(prob, prob_r) and _same(boxes, boxes_r), off
    assert not _same(ops.lnms_prepare(cls_score, bbox_pred, rois, im_info, True, NORM[0], NORM[1], nv)[1], boxes)       # delta_off matters
    prob_c, boxes_c = ops.lnms_prepare(cls_score, bbox_pred, rois, im_info, False, NORM[0], NORM[1], nv)
    prob_r, boxes_cr = e(B, N, C), e(B, N, C, 4)
    call('relnet_lnms_prepare_cs', cs2.data_ptr(), cs2.stride(0), bp2.data_ptr(), bp2.stride(0), rois.data_ptr(), im_info.data_ptr(),
         prob_r.data_ptr(), boxes_cr.data_ptr(), B, N, C1, means, stds, nv.data_ptr(), s)
    assert _same(prob_c, prob_r) and _same(boxes_c, boxes_cr)
    # means / stds None reach the kernel as NULL
    p0, b0 = ops.lnms_prepare(cls_score, bbox_pred, rois, im_info)
    p0_r, b0_r = e(B, N, C), e(B, N, 4)
    call('relnet_lnms_prepare_ex', cs2.data_ptr(), cs2.stride(0), bp2.data_ptr(), bp2.stride(0), rois.data_ptr(), im_info.data_ptr(),
         p0_r.data_ptr(), b0_r.data_ptr(), B, N, C1, 4, None, None, 0, s)
    assert _same(p0, p0_r) and _same(b0, b0_r) and not _same(b0, boxes)
    # sort, both box layouts
    for bx, entry in ((boxes, 'relnet_lnms_sort'), (boxes_c, 'relnet_lnms_sort_cs')):
        got = ops.lnms_sort(prob, bx, F)
        raw = (e(B, C, F, dt=torch.int32), e(B, F, C), e(B, F, C, 4), e(B, C, F, 4), e(B, C))
        call(entry, prob.data_ptr(), bx.data_ptr(), *[t.data_ptr() for t in raw], B, N, C, F, s)
        assert all(_same(a, b) for a, b in zip(got, raw)), entry
    rank_idx, sorted_score, sorted_bbox, class_boxes, class_max = got
    # embed
    roi_emb, rank_feat = rnd(B * N, 128, dt=bf), rnd(F, 128)
    x = ops.lnms_embed(roi_emb, rank_feat, rank_idx)
    x_r = e(B, C, F, 128, dt=bf)
    call('relnet_lnms_embed', roi_emb.data_ptr(), rank_feat.data_ptr(), rank_idx.data_ptr(), x_r.data_ptr(), B, N, C, F, 128, ops._dt(x_r), s)
    assert x.dtype == bf and _same(x, x_r)
    # score (test-branch tail)
    att, w_logit, b_logit = rnd(BC, F, 1024, dt=bf), rnd(T, 128) * 0.1, rnd(T)
    multi, final, dets, counts = ops.lnms_score(x, att, w_logit, b_logit, sorted_score, sorted_bbox, class_max, im_info, -1, 0.01, 1e-3)
    multi_r, final_r = e(B, F, C, T), e(B, F, C)
    dets_r, counts_r = torch.zeros((B, C, F, 5), device=dev, dtype=torch.float64), e(B, C, dt=torch.int32)
    call('relnet_lnms_score', x.data_ptr(), att.data_ptr(), w_logit.data_ptr(), b_logit.data_ptr(), sorted_score.data_ptr(), sorted_bbox.data_ptr(),
         class_max.data_ptr(), im_info.data_ptr(), multi_r.data_ptr(), final_r.data_ptr(), dets_r.data_ptr(), counts_r.data_ptr(), B, C, F, 128, T, 16, 8, 64,
         -1, 0.01, 1e-3, ops._dt(x), s)
    assert _same(multi, multi_r) and _same(final, final_r) and _same(dets, dets_r) and _same(counts, counts_r) and int(counts.sum()) > 0
    assert ops.lnms_score(x, att, w_logit, b_logit, sorted_score, sorted_bbox, class_max, im_info, want_detections=False)[2:] == (None, None)
    # pad_params
    wo, bo, wl, bl = rnd(128, 128, dt=bf), rnd(128), rnd(T, 128, dt=bf), rnd(T)
    pads = [tuple(torch.zeros(sh, device=dev, dtype=dt) for sh, dt in (((1024, 128), bf), ((1024,), f32), ((64, 128), bf), ((64,), f32))) for _ in range(2)]
    ops.lnms_pad_params(wo, bo, wl, bl, *pads[0])
    call('relnet_lnms_pad_params', wo.data_ptr(), bo.data_ptr(), wl.data_ptr(), bl.data_ptr(), *[t.data_ptr() for t in pads[1]], T, s)
    assert all(_same(a, b) for a, b in zip(*pads)) and _same(pads[0][2][:T], wl) and not pads[0][2][T:].any()
    # gather_bias: N = 60 -> Npad 64, F = 20 -> Fpad 32 (the pad columns are unwritten)
    img = rnd(B, 16, N, ops.pad32(N))
    bias = ops.lnms_gather_bias(img, rank_idx)
    bias_r = e(BC, 16, F, ops.pad32(F))
    call('relnet_lnms_gather_bias', img.data_ptr(), rank_idx.data_ptr(), bias_r.data_ptr(), B, C, N, img.shape[-1], F, bias_r.shape[-1], s)
    assert bias.shape == bias_r.shape and _same(bias[..., :F], bias_r[..., :F])
    # residual_relu
    xr = x.view(BC, F, 128)
    allf = ops.lnms_residual_relu(att, xr)
    allf_r = e(BC, F, 128, dt=bf)
    call('relnet_lnms_residual_relu', att.data_ptr(), xr.data_ptr(), allf_r.data_ptr(), BC * F, s)
    assert _same(allf, allf_r)
    # cond_multi on the T real of 64 columns, cond_bwd
    logit = rnd(BC * F, 64)
    cond, multi = ops.lnms_cond_multi(logit, sorted_score, T)
    cond_r, multi_r = e(B, F, C, T), e(B, F, C, T)
    call('relnet_lnms_cond_multi', logit.data_ptr(), logit.stride(0), sorted_score.data_ptr(), cond_r.data_ptr(), multi_r.data_ptr(), B, C, F, T, s)
    assert _same(cond, cond_r) and _same(multi, multi_r)
    d_multi = rnd(B, F, C, T)
    d_sorted, d_logit = ops.lnms_cond_bwd(d_multi, cond, sorted_score)
    d_sorted_r, d_logit_r = e(B, F, C), e(BC * F, 64, dt=bf)
    call('relnet_lnms_cond_bwd', d_multi.data_ptr(), cond.data_ptr(), sorted_score.data_ptr(), d_sorted_r.data_ptr(), d_logit_r.data_ptr(), B, C, F, T, s)
    assert _same(d_sorted, d_sorted_r) and _same(d_logit, d_logit_r)
    # take_bwd
    d_x = rnd(B, C, F, 128, dt=bf)
    d_emb = ops.lnms_take_bwd(d_x, rank_idx, N)
    d_emb_r = e(B * N, 128, dt=bf)
    call('relnet_lnms_take_bwd', d_x.data_ptr(), rank_idx.data_ptr(), d_emb_r.data_ptr(), B, N, C, F, s)
    assert _same(d_emb, d_emb_r)
    # softmax_bwd accumulates into the first N of R rows
    R = N + 3
    base, d_prob = rnd(B, R, C1), rnd(B, N, C)
    acc, acc_r = base.clone(), base.clone()
    ops.lnms_softmax_bwd(prob, d_prob, acc)
    call('relnet_lnms_softmax_bwd', prob.data_ptr(), d_prob.data_ptr(), acc_r.data_ptr(), acc_r.stride(1), acc_r.stride(0), B, N, C, s)
    torch.cuda.synchronize()
    assert _same(acc, acc_r) and _same(acc[:, N:], base[:, N:]) and not _same(acc[:, :N], base[:, :N])
