"""GPU tests of the trainable stem and res2 (train.check_fixed_params: a network.FIXED_PARAMS list that leaves conv1 / res2 trainable): the two
new kernels against the restatements of tests/stem_train_cases.py (tests/test_stem_train_cases_host.py asserts on the same inputs that the tie
rule and the accumulation order decide something), the wiring of all 104 trunk gradients against float64 autograd on the float32 trunk, one
bf16 step with its checkpoint, and the deterministic / captured step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stem_train_cases as SC  # noqa: E402
import deterministic_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().contiguous().view(torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------
# relnet_stem_pool_bwd
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [True, False], ids=['bf16', 'f32'])
@pytest.mark.parametrize('hw', SC.POOL_CASES, ids=['%dx%d' % hw for hw in SC.POOL_CASES])
def test_stem_pool_bwd_equals_the_restatement_bit_for_bit(hw, bf16):
    """Every case of SC.POOL_CASES (B = 2, C = 64; placed ties inside one window, on a pixel of two and of four windows, an all-negative
    window, four gradients that cancel differently in another order), bf16 and float32: the forward kernels give the restatement's pooled
    map, the adjoint is bit-equal to the restatement in its defined order and over three calls, and written into the middle of a poisoned
    buffer it leaves every word around its output alone."""
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib
    c = SC.pool_case(*hw)
    dt = torch.bfloat16 if bf16 else torch.float32
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda().to(dt).contiguous()
    conv, d_out, bias = dev(c['conv']), dev(c['d_out']), torch.as_tensor(c['bias']).cuda()
    assert np.array_equal(conv.float().cpu().numpy(), c['conv']) and np.array_equal(d_out.float().cpu().numpy(), c['d_out'])
    out_np = SC.pool_forward(c['conv'], c['bias'], bf16)
    out = ops.stem_bias_relu_pool(conv, bias) if bf16 else torch.relu(ops.maxpool_nhwc_f32(conv, 3, 2) + bias)
    assert np.array_equal(out.float().cpu().numpy(), out_np)
    want = SC.pool_backward(c['conv'], out_np, c['d_out'], bf16)
    calls = [ops.stem_pool_bwd(conv, out, d_out) for _ in range(3)]
    torch.cuda.synchronize()
    got = calls[0].float().cpu().numpy()
    assert got.dtype == np.float32 and calls[0].dtype == dt and calls[0].shape == conv.shape
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), '%d words differ, first at %s' % (int(bad.sum()), tuple(np.argwhere(bad)[0]))
    assert _same_bits(calls[0], calls[1]) and _same_bits(calls[0], calls[2])
    if min(SC.pooled_hw(*hw)) >= 2:
        assert (got[0, 2, 2, 48:] == 1.0).all()                    # 2^27 + 1 - 2^27 + 1 in ascending (ph, pw)
    assert not got[1, 0:2, 0:2].any()                               # the all-negative window
    # poison around the output: 64 elements (a multiple of 16 bytes) on either side
    n, guard = conv.numel(), 64
    poison = -7.0
    buf = torch.full((n + 2 * guard,), poison, device='cuda', dtype=dt)
    B, Hc, Wc, C = conv.shape
    lib.call('relnet_stem_pool_bwd', conv.data_ptr(), out.data_ptr(), d_out.data_ptr(), buf[guard:].data_ptr(), B, Hc, Wc, C, 1 if bf16 else 0,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _same_bits(buf[guard:guard + n].view(conv.shape), calls[0])
    assert bool((buf[:guard] == poison).all()) and bool((buf[guard + n:] == poison).all())


def test_stem_pool_bwd_refuses_operands_that_do_not_belong_together():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops
    conv = torch.zeros(1, 5, 5, 64, device='cuda', dtype=torch.bfloat16)
    with pytest.raises(AssertionError):
        ops.stem_pool_bwd(conv, torch.zeros(1, 3, 3, 64, device='cuda', dtype=torch.bfloat16), torch.zeros(1, 3, 3, 64, device='cuda', dtype=torch.bfloat16))
    with pytest.raises(AssertionError):
        ops.stem_pool_bwd(conv, torch.zeros(1, 2, 2, 64, device='cuda'), torch.zeros(1, 2, 2, 64, device='cuda'))


# ---------------------------------------------------------------------------------------------------------
# relnet_stem_wgrad
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SC.WGRAD_CASES, ids=[c[0] for c in SC.WGRAD_CASES])
def test_stem_wgrad_within_the_summation_bound_and_reproducible(case):
    """Images 2 x 3 x 8 x 8 (conv map 4 x 4: every tap crosses the padding), 2 x 3 x 37 x 53 and 1 x 3 x 34 x 482 (4097 pixels: one chunk and one
    pixel).  Every word within the n-term float32 summation bound (deterministic_cases.sum_bound on the bf16 operands, n = B Hc Wc) of the
    float64 restatement; three calls bit-equal; `+=` into a non-zero dW is one float32 addition per word; row_scale multiplies by its square;
    the columns past 147 of a wider gradient row keep their poison."""
    import relnet_amd  # noqa: F401
    from relnet_amd import ops
    id_, B, H, W = case
    img_np, d_np = SC.wgrad_case(*case)
    img = torch.as_tensor(img_np).cuda()
    d = torch.as_tensor(d_np).cuda().to(torch.bfloat16).contiguous()
    assert np.array_equal(d.float().cpu().numpy(), d_np)
    w0 = torch.zeros(64, 256, device='cuda', dtype=torch.bfloat16)
    conv, packed = ops.stem_conv7(img, w0, None, relu=False, want_packed=True)
    assert tuple(conv.shape) == d.shape and packed.shape[3] == 4
    want, ab, n = SC.wgrad_float64(img_np, d_np)
    bound = DC.sum_bound(ab, n)
    calls = []
    for _ in range(3):
        wide = torch.full((64, 160), -7.0, device='cuda')
        dw = wide[:, :147]
        dw.zero_()
        ops.stem_wgrad(packed, d, dw)
        calls.append(wide)
    torch.cuda.synchronize()
    got = calls[0][:, :147].double().cpu().numpy()
    err = np.abs(got - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print('stem_wgrad %s: n = %d, max |err| %.3e, max err / bound %.4f' % (id_, n, float(err.max()), worst))
    assert np.abs(want).max() > 0 and (err <= bound).all(), worst
    assert bool((calls[0][:, 147:] == -7.0).all())
    assert _same_bits(calls[0], calls[1]) and _same_bits(calls[0], calls[2])
    r0 = calls[0][:, :147].contiguous()
    base = torch.as_tensor(DC.order_sensitive(np.random.default_rng(SC.seed('stem-wgrad-base')), (64, 147))).cuda()
    acc = base.clone()
    ops.stem_wgrad(packed, d, acc)
    assert _same_bits(acc, base + r0)                                # one IEEE addition per word
    scale = torch.as_tensor(np.random.default_rng(SC.seed('stem-wgrad-scale')).uniform(0.5, 2.0, 64).astype(np.float32)).cuda()
    scaled = torch.zeros(64, 147, device='cuda')
    ops.stem_wgrad(packed, d, scaled, scale)
    assert _same_bits(scaled, (scale * scale).view(-1, 1) * r0)


# ---------------------------------------------------------------------------------------------------------
# wiring: every trunk gradient against float64 autograd, on the float32 trunk
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fixed,slices', [(['gamma', 'beta'], 104), (['conv1', 'bn_conv1', 'gamma', 'beta'], 103)], ids=['conv1+res2', 'res2'])
def test_float32_trunk_with_trainable_stem_matches_float64_autograd_tightly(fixed, slices):
    """tests/test_gpu_train_step.py's test_float32_trunk_forward_and_gradients_match_float64_autograd_tightly with network.FIXED_PARAMS =
    ['gamma', 'beta'] (104 slices: its 93, conv1 and the ten res2 weights) and with conv1 still fixed (103, no conv1 slice): 2 images of
    128 x 160, the same inject / backward / flush sequence, the same bars (stage outputs within 2e-5 of scale, every weight gradient with
    cosine >= 0.9999 and norm within 0.5 % of float64 autograd of oracle.network.backbone)."""
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, train
    from oracle import network as ON
    H, W = 128, 160
    p = backbone.init_params(seed=61)
    cfg = train.TrainConfig()
    cfg.trunk_fp32 = True
    cfg.fixed_params = fixed
    g = torch.Generator().manual_seed(62)
    data = torch.randn(2, 3, H, W, generator=g)
    tr = train.Trainer(p, cfg, im_hw=(H, W))
    assert tr.trunk_fp32 and tr.res2_trainable and tr.stem_trainable == ('conv1' not in fixed)
    assert ('conv1' in tr.W.slices) == tr.stem_trainable and 'res2a_branch1' in tr.W.slices
    assert tr._grad_buckets() is not None and tr._bucket_names == ('res2', 'res3', 'res4_lo', 'res4_hi', 'res5', 'heads')
    conv5, conv4, saved, ends = tr._trunk_forward(data.cuda())
    assert conv5.dtype == torch.float32 and isinstance(saved[0], backbone.SavedStem) == tr.stem_trainable
    g5 = torch.randn(conv5.shape, generator=g) * 0.01
    g4 = torch.randn(conv4.shape, generator=g) * 0.01
    tr._grad_buckets().reset()
    tr.W.grad.zero_(); tr.Bv.grad.zero_()
    tr._trunk_backward(saved, g5.cuda(), {'4b22': g4.cuda()})
    tr._flush_wgrads()
    torch.cuda.synchronize()
    trainable = lambda k: k.endswith('_weight') and (k.startswith(('res2', 'res3', 'res4', 'res5')) or (k == 'conv1_weight' and tr.stem_trainable))
    pt = {k: v.double().clone().requires_grad_(trainable(k)) for k, v in p.items()}
    old = ON._t
    ON._t = lambda x: x.double() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x), dtype=torch.float64)
    try:
        c4, c5 = ON.backbone(data.double(), pt)
    finally:
        ON._t = old
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    for name, got, want in (('conv4', conv4, c4), ('conv5', conv5, c5)):
        err = float((got.double().cpu() - nhwc(want).detach()).abs().max() / want.detach().abs().max())
        assert err <= 2e-5, (name, err)
    ((nhwc(c5) * g5.double()).sum() + (nhwc(c4) * g4.double()).sum()).backward()
    bad, worst, n_checked = [], 1.0, 0
    for name in tr.W.slices:
        if not (name.startswith('res') or name == 'conv1'):
            continue
        gw = pt[name + '_weight'].grad
        want = gw.permute(0, 2, 3, 1).reshape(gw.shape[0], -1) * tr.bn_scale[name].cpu().double().view(-1, 1)      # s * dL/dw = s^2 dL/dw'
        got = tr.W.view(tr.W.grad, name).cpu().double().reshape(want.shape)
        nw, ng = float(want.norm()), float(got.norm())
        cos = float((want * got).sum() / max(nw * ng, 1e-300))
        worst = min(worst, cos)
        n_checked += 1
        print('%-20s |want| %.3e |got| %.3e cos %.7f' % (name, nw, ng, cos))
        if not (nw > 1e-12) or cos < 0.9999 or abs(ng / nw - 1) > 5e-3:
            bad.append('%-20s |want| %.3e |got| %.3e cos %.6f' % (name, nw, ng, cos))
    assert n_checked == slices and not bad, '\n'.join(bad)
    assert pt['conv1_weight'].grad is None or tr.stem_trainable


# ---------------------------------------------------------------------------------------------------------
# the bf16 step
# ---------------------------------------------------------------------------------------------------------
def _feat_size(n):
    n = (n + 2 * 3 - 7) // 2 + 1
    n = -(-(n - 3) // 2) + 1
    n = (n - 1) // 2 + 1
    return (n - 1) // 2 + 1


def _setup(seed, learn_nms=False):
    """tests/test_gpu_train_step.py's smallest setup: one 128 x 160 image, 4 gt boxes, rpn_post_nms_top_n 40; the plain C4 graph unless learn_nms."""
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, train
    H, W, G = 128, 160, 4
    p = backbone.init_params(seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    p['conv_new_1_bias'] = torch.rand(256, generator=g) * 0.1 + 0.05

    def make_cfg(fixed, deterministic=False):
        cfg = train.TrainConfig()
        cfg.rpn_post_nms_top_n, cfg.first_n = 40, 24
        cfg.learn_nms = learn_nms
        if not learn_nms:
            cfg.relation, cfg.enable_ohem = False, False
        cfg.fixed_params, cfg.deterministic = fixed, deterministic
        return cfg
    data = torch.randn(1, 3, H, W, generator=g)
    rng = np.random.default_rng(seed + 2)
    gt = np.zeros((1, G, 5), np.float32)
    x1 = rng.uniform(0, W - 70, G); y1 = rng.uniform(0, H - 70, G)
    gt[0, :, 0], gt[0, :, 1] = x1, y1
    gt[0, :, 2], gt[0, :, 3] = x1 + rng.uniform(30, 69, G), y1 + rng.uniform(30, 69, G)
    gt[0, :, 4] = rng.integers(1, 81, G)
    L, Tg, Wg = train.assign_anchor((_feat_size(H), _feat_size(W)), gt[0], (H, W), make_cfg(None), seed=seed)
    d = lambda a: torch.as_tensor(a).cuda()
    batch = (data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
    return p, make_cfg, batch, train, (H, W)


BOTTOM = ['conv1'] + ['res2%s_branch%s' % (u, b) for u in 'abc' for b in (('1',) if u == 'a' else ()) + ('2a', '2b', '2c')]


def test_one_bf16_step_moves_conv1_and_res2_and_the_checkpoint_holds_them(tmp_path):
    """One image of 128 x 160, plain C4 graph, FIXED_PARAMS = ['gamma', 'beta'], one step(): conv1 and the ten res2 master weights move
    (finite, non-zero gradients), everything else trains as before; under the shipped list the same tensors come back from the checkpoint
    bit-identical to their initial values.  After save_checkpoint, conv1_weight read back equals export_params()['conv1_weight'] and
    differs from the initial tensor."""
    from relnet_amd import checkpoint as ck, dist as D
    p, make_cfg, batch, train, hw = _setup(71)
    tr = train.Trainer(p, make_cfg(['gamma', 'beta']), im_hw=hw)
    assert tr.stem_trainable and tr.res2_trainable and not tr.frozen_names and len(BOTTOM) == 11
    assert list(tr.W.slices)[:11] == BOTTOM and tr._grad_buckets() is not None and tr._bucket_names[0] == 'res2'
    assert not any(k.startswith(('conv1_', 'res2')) for k in tr._fixed_src) and 'bn_conv1_gamma' in tr._fixed_src
    before = {n: tr.W.view(tr.W.master, n).clone() for n in BOTTOM}
    with torch.no_grad():
        out = tr.step(*batch)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.W.grad).all() and torch.isfinite(tr.W.master).all() and float(out['bbox_loss']) >= 0
    for n in BOTTOM:
        gn = float(tr.W.view(tr.W.grad, n).norm())
        assert gn > 0, n
        assert not torch.equal(tr.W.view(tr.W.master, n), before[n]), n
        assert torch.equal(tr.W.view(tr.W.work, n), tr.W.view(tr.W.master, n).to(torch.bfloat16)), n
    exp = tr.export_params()
    prefix = str(tmp_path / 'stem')
    tr.save_checkpoint(prefix, 0)
    arg, aux = ck.load_param(prefix, 1)
    for k in ('conv1_weight', 'res2a_branch1_weight', 'res2c_branch2b_weight'):
        assert tuple(np.asarray(arg[k]).shape) == tuple(p[k].shape)
        assert np.array_equal(np.asarray(arg[k], np.float32), exp[k].numpy()), k
        assert not np.array_equal(np.asarray(arg[k], np.float32), p[k].numpy()), k
    assert 'bn_conv1_moving_mean' in aux and np.array_equal(np.asarray(arg['bn_conv1_gamma'], np.float32), p['bn_conv1_gamma'].numpy())
    # the shipped list: the same step leaves conv1 / res2 out of the buffers, and the checkpoint holds their initial bits
    ship = train.Trainer(p, make_cfg(list(D.FIXED_PARAMS)), im_hw=hw)
    assert not ship.stem_trainable and not ship.res2_trainable and len(ship.W.slices) == len(tr.W.slices) - 11
    assert ship._grad_buckets() is not None and ship._bucket_names == ('res3', 'res4_lo', 'res4_hi', 'res5', 'heads')
    with torch.no_grad():
        ship.step(*batch)
    arg_s, _ = ship.checkpoint_params()
    for k in ('conv1_weight', 'res2a_branch1_weight', 'res2c_branch2b_weight'):
        assert torch.equal(arg_s[k], p[k].float()), k
    assert not torch.equal(arg_s['res3a_branch1_weight'], p['res3a_branch1_weight'].float())


# ---------------------------------------------------------------------------------------------------------
# determinism and capture
# ---------------------------------------------------------------------------------------------------------
def _three_steps(tr, batch):
    rec = []
    with torch.no_grad():
        for _ in range(3):
            tr.forward_backward(*batch)
            rec.append((tr.W.grad.clone(), tr.Bv.grad.clone()))
            tr.all_reduce(); tr.update()
    torch.cuda.synchronize()
    return rec


def test_two_deterministic_trainers_with_a_trainable_stem_give_the_same_bits():
    p, make_cfg, batch, train, hw = _setup(31, learn_nms=True)
    a = train.Trainer(p, make_cfg(['gamma', 'beta'], True), im_hw=hw)
    assert a.deterministic and a.stem_trainable
    ra = _three_steps(a, batch)
    b = train.Trainer(p, make_cfg(['gamma', 'beta'], True), im_hw=hw)
    rb = _three_steps(b, batch)
    for step, ((wa, ba), (wb, bb)) in enumerate(zip(ra, rb)):
        assert float(a.W.view(wa, 'conv1').abs().max()) > 0 and torch.isfinite(wa).all()
        assert _same_bits(wa, wb), 'W.grad differs in step %d: %d words' % (step, int((_bits(wa) != _bits(wb)).sum()))
        assert _same_bits(ba, bb), step
    assert not _same_bits(ra[0][0], ra[2][0])
    assert _same_bits(a.W.master, b.W.master) and _same_bits(a.W.mom, b.W.mom) and _same_bits(a.Bv.master, b.Bv.master)


def test_captured_step_with_a_trainable_stem_replays_bit_for_bit():
    """CapturedStep of a deterministic trainer with a trainable stem: cut at every bucket, the last segment announces bucket 0 = 'res2'; the
    replay's gradients are bit-equal to the eager pass."""
    p, make_cfg, batch, train, hw = _setup(41, learn_nms=True)
    tr = train.Trainer(p, make_cfg(['gamma', 'beta'], True), im_hw=hw)
    batch = batch[:3]                                       # anchor targets on the device, inside the step
    with torch.no_grad():
        tr.forward_backward(*batch)                        # eager warm-up
        g_eager = tr.W.grad.clone()
        tr._anchor_step.zero_()
        step = train.CapturedStep(tr, batch, segments=True)
        assert [i for _, i in step.segments][:6] == [5, 4, 3, 2, 1, 0] and len(step.segments) == 6
        grads = []
        for _ in range(2):
            tr._anchor_step.zero_()
            step.replay()
            torch.cuda.synchronize()
            grads.append((tr.W.grad.clone(), tr.Bv.grad.clone()))
    assert float(tr.W.view(grads[0][0], 'conv1').abs().max()) > 0
    assert _same_bits(grads[0][0], grads[1][0]) and _same_bits(grads[0][1], grads[1][1])
    assert _same_bits(grads[0][0], g_eager)
