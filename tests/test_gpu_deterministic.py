"""GPU tests of the deterministic training mode (train.TrainConfig.deterministic): every ordered kernel against the
float32 restatement of its defined order (bit for bit) or the n-term float32 summation bound (tests/deterministic_cases.py says where each
comes from), reruns bit for bit, and the whole step: two trainers built from the same parameters give the same bits, step after step.
The inputs make the order matter (tests/test_deterministic_cases_host.py asserts that on the same inputs)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import deterministic_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().contiguous()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _np_bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


# ---------------------------------------------------------------------------------------------------------
# ROI pooling backward
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', DC.ROI_CASES, ids=[c[0] for c in DC.ROI_CASES])
def test_roi_pool_bwd_ordered_equals_the_restatement_bit_for_bit(case):
    """ops.roi_pool_bwd(deterministic=True): 6 x 8 maps, B = 2, R = 24 rois (whole-map, sub-cell with 49 bins on one cell, corner rois with
    empty bins, exact duplicates; in two cases every roi on image 1), argmax from the forward on a random map.  Bit-equal to the ascending
    (roi, ph, pw) restatement and over three calls; the existing kernel's result (the default path, left alone) and the ordered one are both
    within the n-term bound of the float64 sum, and within it of each other."""
    import relnet_amd  # noqa: F401
    from relnet_amd import ops
    id_, C, bf16, base, image1 = case
    B, H, W, R, P = DC.ROI_B, DC.ROI_H, DC.ROI_W, DC.ROI_R, DC.ROI_P
    rng = np.random.default_rng(DC.seed('roi-' + id_))
    rois_np = DC.roi_case_rois(base, image1)
    g_np = DC.order_sensitive(rng, (R, C, P, P), bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    gen = torch.Generator().manual_seed(DC.seed('roi-map-' + id_) % (2 ** 31))
    if bf16:      # NHWC memory, the 8-channel vector path
        data = torch.randn(B, H, W, C, generator=gen).cuda().to(dt).permute(0, 3, 1, 2)
    else:
        data = torch.randn(B, C, H, W, generator=gen).cuda()
    rois = torch.as_tensor(rois_np).cuda()
    out, arg = ops.roi_pool(data, rois, (P, P), DC.ROI_SCALE, channels_last_out=bf16, want_argmax=True, batch_index_base=base)
    grad = torch.empty_strided(out.shape, out.stride(), device='cuda', dtype=dt)
    grad.copy_(torch.as_tensor(g_np).cuda().to(dt))
    assert torch.equal(grad.float().cpu(), torch.as_tensor(g_np))                # the device sees exactly the restatement's values
    calls = [ops.roi_pool_bwd(grad, arg, rois, (B, C, H, W), base, channels_last=bf16, deterministic=True, spatial_scale=DC.ROI_SCALE)
             for _ in range(3)]
    assert calls[0].shape == (B, C, H, W) and calls[0].dtype == torch.float32
    if bf16:
        assert calls[0].permute(0, 2, 3, 1).is_contiguous()
    assert _same_bits(calls[0], calls[1]) and _same_bits(calls[0], calls[2])
    arg_np = arg.cpu().numpy()
    img = (rois_np[:, 0] - base).astype(np.int64)
    want, cnt, s64, a64 = DC.roi_pool_bwd_ordered_ref(g_np, arg_np, img, B, H, W, stats=True)
    assert int(cnt.max()) >= 49 and int((arg_np < 0).sum()) > 0 and int((arg_np[2:6] >= 0).all())
    got = calls[0].contiguous().cpu().numpy().reshape(B, C, H * W)
    assert _np_bits_equal(got, want), 'max |diff| %g' % np.abs(got - want).max()
    if image1:
        assert not got[0].any()
    old = ops.roi_pool_bwd(grad, arg, rois, (B, C, H, W), base, channels_last=bf16).contiguous().cpu().numpy().reshape(B, C, H * W)
    bound = DC.sum_bound(a64, cnt)
    print('roi_pool_bwd %s: max |ordered - f64| %.3e, |atomic - f64| %.3e, |ordered - atomic| %.3e, min slack %.3e' % (
        id_, np.abs(got - s64).max(), np.abs(old - s64).max(), np.abs(got - old).max(), (bound - np.abs(got.astype(np.float64) - old)).min()))
    assert (np.abs(got - s64) <= bound).all() and (np.abs(old - s64) <= bound).all()
    assert (np.abs(got.astype(np.float64) - old) <= bound).all()


# ---------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------
def _colsum_operands(id_, rows, cols, bf16):
    x_np, out0 = DC.colsum_case(id_, rows, cols, bf16)
    x = torch.as_tensor(x_np).cuda().to(torch.bfloat16 if bf16 else torch.float32)
    return x_np, out0, x


@pytest.mark.parametrize('case', DC.COLSUM_CASES, ids=[c[0] for c in DC.COLSUM_CASES])
def test_colsum_ordered_single_shapes(case):
    """4100 x 24 bf16 (nine row chunks, ragged last one), 1 x 8, 257 x 5 fp32 (the scalar body): out pre-filled, within the (rows + 1)-term
    bound of the float64 sum, bit-equal over three calls and to the documented tree; a bf16 operand whose row pitch forbids the 16-byte loads
    gives the same bits (the tree does not depend on alignment)."""
    import relnet_amd  # noqa: F401
    from relnet_amd import train_ops as T
    id_, rows, cols, bf16 = case
    x_np, out0, x = _colsum_operands(id_, rows, cols, bf16)
    res = []
    for _ in range(3):
        out = torch.as_tensor(out0).cuda()
        T.colsum_add(x, out, deterministic=True)
        res.append(out)
    assert _same_bits(res[0], res[1]) and _same_bits(res[0], res[2])
    got = res[0].cpu().numpy()
    want64 = out0.astype(np.float64) + x_np.astype(np.float64).sum(0)
    bound = DC.sum_bound(np.abs(out0).astype(np.float64) + np.abs(x_np).astype(np.float64).sum(0), rows + 1)
    print('colsum %s: max err %.3e, min slack %.3e' % (id_, np.abs(got - want64).max(), (bound - np.abs(got - want64)).min()))
    assert (np.abs(got - want64) <= bound).all()
    assert _np_bits_equal(got, DC.colsum_ordered_ref(x_np, out0))
    if bf16:
        wide = torch.zeros(rows, cols + 1, device='cuda', dtype=torch.bfloat16)
        wide[:, :cols] = x
        out = torch.as_tensor(out0).cuda()
        T.colsum_add(wide[:, :cols], out, deterministic=True)                    # row pitch cols + 1: the scalar bf16 body
        assert _same_bits(out, res[0])
    # the default path still accumulates (left alone)
    out = torch.as_tensor(out0).cuda()
    T.colsum_add(x, out)
    assert (np.abs(out.cpu().numpy() - want64) <= bound).all()


def test_colsum_ordered_group_of_17_equals_the_sums_issued_alone():
    """ColsumQueue(deterministic=True) with 17 problems of differing rows (two grouped launches): every output within the bound, bit-equal over
    three flushes, and bit-equal to the same sum issued alone -- the tree depends on the operand's shape only.  Two queued sums into the SAME
    bias are split into consecutive launches and add up in queue order."""
    import relnet_amd  # noqa: F401
    from relnet_amd import train_ops as T
    rng = np.random.default_rng(DC.seed('colsum-group'))
    ops_ = []
    for rows, cols in zip(DC.COLSUM_GROUP_ROWS, DC.COLSUM_GROUP_COLS):
        x_np = DC.order_sensitive(rng, (rows, cols), True)
        ops_.append((x_np, DC.order_sensitive(rng, (cols,)), torch.as_tensor(x_np).cuda().to(torch.bfloat16)))
    runs = []
    for _ in range(3):
        q = T.ColsumQueue(deterministic=True)
        outs = [torch.as_tensor(o0).cuda() for _, o0, _ in ops_]
        for (_, _, x), o in zip(ops_, outs):
            T.colsum_add(x, o, q)
        assert len(q) == 17
        q.flush()
        assert len(q) == 0
        runs.append(outs)
    for a, b, c in zip(*runs):
        assert _same_bits(a, b) and _same_bits(a, c)
    for (x_np, o0, x), grouped in zip(ops_, runs[0]):
        alone = torch.as_tensor(o0).cuda()
        T.colsum_add(x, alone, deterministic=True)
        assert _same_bits(alone, grouped), x_np.shape
        want64 = o0.astype(np.float64) + x_np.astype(np.float64).sum(0)
        bound = DC.sum_bound(np.abs(o0).astype(np.float64) + np.abs(x_np).astype(np.float64).sum(0), x_np.shape[0] + 1)
        assert (np.abs(grouped.cpu().numpy() - want64) <= bound).all(), x_np.shape
    for i in (3, 5, 6):
        assert _np_bits_equal(runs[0][i].cpu().numpy(), DC.colsum_ordered_ref(ops_[i][0], ops_[i][1])), i
    # the same bias twice in one queue
    q = T.ColsumQueue(deterministic=True)
    out = torch.as_tensor(ops_[3][1]).cuda()
    T.colsum_add(ops_[3][2], out, q); T.colsum_add(ops_[5][2], out, q)
    q.flush()
    want = DC.colsum_ordered_ref(ops_[5][0], DC.colsum_ordered_ref(ops_[3][0], ops_[3][1]))
    assert _np_bits_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------
# scalar reduction
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', DC.SCALAR_NS)
def test_reduce_scalar_ordered_both_modes(n):
    import relnet_amd  # noqa: F401
    from relnet_amd import train_ops as T
    x_np = DC.scalar_case(n)
    x = torch.as_tensor(x_np).cuda()
    s = [T.scalar_sum(x, DC.SCALAR_SCALE, deterministic=True) for _ in range(3)]
    c = [T.scalar_sum(x, count_nonneg=True, deterministic=True) for _ in range(3)]
    assert _same_bits(s[0], s[1]) and _same_bits(s[0], s[2]) and _same_bits(c[0], c[1]) and _same_bits(c[0], c[2])
    want = DC.SCALAR_SCALE * float(x_np.astype(np.float64).sum())
    bound = float(DC.sum_bound(DC.SCALAR_SCALE * np.abs(x_np).astype(np.float64).sum(), n))
    print('reduce_scalar n=%d: err %.3e bound %.3e' % (n, abs(float(s[0]) - want), bound))
    assert abs(float(s[0]) - want) <= bound
    assert float(c[0]) == float((x_np >= 0).sum())
    assert _np_bits_equal(np.float32(float(s[0])), DC.reduce_scalar_ordered_ref(x_np, DC.SCALAR_SCALE, 0))
    assert abs(float(T.scalar_sum(x, DC.SCALAR_SCALE)) - want) <= bound                 # the default path, left alone


# ---------------------------------------------------------------------------------------------------------
# geometry backward dwp / dbp
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,m', [(20, 12), (140, 130)], ids=['small-kernel-path', 'two-kernel-path'])
@pytest.mark.parametrize('fast', [True, False], ids=['matrix-core', 'per-wavefront'])
def test_geometry_bias_bwd_ordered(n, m, fast, monkeypatch):
    """dwp / dbp of pair_pos_fc1 behind both forms of the attention backward: (N, M) = (20, 12) -> Mpad 32, the one-workgroup kernel;
    (140, 130) -> Mpad 160 > 128, the two-kernel form (tests/test_gpu_relation_bwd.py: the switch is N, Mpad <= 128).  B = 2, M < N <= Mpad
    (padded keys), key counts below M.  The second stage adds `slots` partial sums to the pre-filled dwp / dbp: within the (slots + 1)-term
    bound of the float64 sum of the partials the first stage wrote, bit-equal to the documented tree over them, to the wrapper's result and over three
    calls; the atomic wrapper adds the same partials in the hardware's order and meets the same bound."""
    import cases
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib
    B, H, d = 2, 16, 1024
    bt = torch.bfloat16
    g = torch.Generator().manual_seed(n * 7 + m)
    mpad = ops.pad32(m)
    assert ops.relation_bwd_small_ok(bt, n, mpad) == (n == 20)
    qk = (torch.randn(B, n, 2 * d, generator=g) * 0.3).cuda().to(bt)
    q, k = qk[:, :, :d], qk[:, :m, d:]
    vw = (torch.randn(B, m, d, generator=g) * 0.3).cuda().to(bt)
    dy = torch.randn(B, n, d, generator=g).cuda().to(bt)
    y = torch.randn(B, n, d, generator=g).cuda().to(bt)
    bout = torch.randn(d, generator=g).cuda()
    bias = (torch.randn(B, H, n, mpad, generator=g) - 2.0).cuda()
    kt = torch.zeros(B, d, mpad, device='cuda', dtype=bt); ops.transpose_2d(k, out=kt)
    qt = ops.transpose_2d(q, pad_cols_to=32); dyt = ops.transpose_2d(dy, pad_cols_to=32)
    key_count = torch.tensor([m, max(1, m // 2)], dtype=torch.int32).cuda()
    dlog = ops.relation_attention_bwd(q, k, kt, vw, bias, dy, y, bout, qt, dyt, m, key_count=key_count)[4]
    dlog[..., m:] = 0.0                                                       # (pad columns are never read; make them defined anyway)
    boxes = torch.as_tensor(np.stack([cases.random_boxes(n, 5), cases.random_boxes(n, 6)])).cuda()
    rng = np.random.default_rng(DC.seed('geom-%d-%d' % (n, m)))
    w0, b0 = DC.order_sensitive(rng, (16, 64)) * np.float32(1e-3), DC.order_sensitive(rng, (16,)) * np.float32(1e-3)
    L = lib.load()
    nbytes = int(L.relnet_geometry_bias_bwd_workspace_bytes(B, n))
    assert nbytes == B * n * 1040 * 4
    ws = torch.zeros(nbytes // 4, device='cuda')
    div = ops.embedding_divisors().to(torch.float32).cpu().contiguous()
    res = []
    for _ in range(3):
        dwp, dbp = torch.as_tensor(w0).cuda(), torch.as_tensor(b0).cuda()
        lib.call('relnet_geometry_bias_bwd_ordered', boxes.data_ptr(), 4, 0, bias.data_ptr(), dlog.data_ptr(), div.data_ptr(), dwp.data_ptr(),
                 dbp.data_ptr(), B, n, m, mpad, int(fast), ws.data_ptr(), nbytes, ops._stream())
        res.append((dwp, dbp))
    for a, b_ in res[1:]:
        assert _same_bits(a, res[0][0]) and _same_bits(b_, res[0][1])
    slots = min(768, (B * n + 3) // 4) if fast else B * n
    part = ws.cpu().numpy().reshape(B * n, 1040)[:slots]
    assert np.abs(part).max() > 0 and np.isfinite(part).all()
    init = np.concatenate([w0.reshape(-1), b0])
    got = np.concatenate([res[0][0].cpu().numpy().reshape(-1), res[0][1].cpu().numpy()])
    t = np.zeros(1040, np.float32)
    for lane in range(16):                               # the documented tree: 16 slot lanes (slots l, l + 16, ..), then the lanes, ascending from 0
        acc = np.zeros(1040, np.float32)
        for s_ in range(lane, slots, 16):
            acc = acc + part[s_]
        t = t + acc
    assert _np_bits_equal(got, init + t)
    want64 = init.astype(np.float64) + part.astype(np.float64).sum(0)
    bound = DC.sum_bound(np.abs(init).astype(np.float64) + np.abs(part).astype(np.float64).sum(0), slots + 1)
    print('geometry bwd N=%d M=%d fast=%s: %d slots, max err %.3e, min slack %.3e' % (n, m, fast, slots, np.abs(got - want64).max(),
                                                                                   (bound - np.abs(got - want64)).min()))
    assert (np.abs(got - want64) <= bound).all()
    dwp, dbp = torch.as_tensor(w0).cuda(), torch.as_tensor(b0).cuda()
    ops.geometry_bias_bwd(boxes, bias, dlog, m, fast=fast, out=(dwp, dbp), deterministic=True)
    assert _same_bits(dwp, res[0][0]) and _same_bits(dbp, res[0][1])
    dwp, dbp = torch.as_tensor(w0).cuda(), torch.as_tensor(b0).cuda()
    ops.geometry_bias_bwd(boxes, bias, dlog, m, fast=fast, out=(dwp, dbp))           # the atomic form, left alone: the same partials, any order
    old = np.concatenate([dwp.cpu().numpy().reshape(-1), dbp.cpu().numpy()])
    assert (np.abs(old - want64) <= bound).all()


# ---------------------------------------------------------------------------------------------------------
# take adjoint
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_lnms_take_bwd_ordered_equals_the_restatement(bf16):
    """B = 1, N = 12 rois, 5 classes, first_n 8: some rois are ranked by several classes, rois 10 and 11 by none (their rows are written as
    zeros).  Bit-equal to the ascending-flat-index restatement and over three calls."""
    import relnet_amd  # noqa: F401
    from relnet_amd import ops
    d_np, rank = DC.take_case(bf16)
    d_x = torch.as_tensor(d_np).cuda().to(torch.bfloat16 if bf16 else torch.float32)
    rk = torch.as_tensor(rank).cuda()
    res = [ops.lnms_take_bwd_ordered(d_x, rk, DC.TAKE_N) for _ in range(3)]
    assert _same_bits(res[0], res[1]) and _same_bits(res[0], res[2])
    got = res[0].cpu().numpy()
    assert got.shape == (DC.TAKE_N, 128) and not got[10:].any()
    assert _np_bits_equal(got, DC.take_bwd_ordered_ref(d_np, rank, DC.TAKE_N))


# ---------------------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------------------
def test_wgrad_deterministic_group_and_overlapping_writers():
    """One grouped launch of three layers with disjoint gradient slices: bit-equal over three calls in deterministic mode (whole-tile shares)
    and within twice the P-term bound of the float64 product (bf16 x bf16 is exact in float32; the matrix core's own adder tree is not
    documented as round-to-nearest per addition, hence the factor two).  A pair that accumulates into the SAME slice is split into two
    launches in queue order: reproducible, and bit-equal to issuing the two products one after the other."""
    import relnet_amd  # noqa: F401
    from relnet_amd import ops
    rng = np.random.default_rng(DC.seed('wgrad'))
    P = 3000
    layers = []
    for cout, kk in ((24, 72), (40, 136), (136, 264)):
        dy = DC.order_sensitive(rng, (P, cout), True)
        x = DC.order_sensitive(rng, (P, kk), True)
        layers.append((dy, x, DC.order_sensitive(rng, (cout, kk)), torch.as_tensor(dy).cuda().to(torch.bfloat16), torch.as_tensor(x).cuda().to(torch.bfloat16)))
    runs = []
    for _ in range(3):
        q = ops.WgradQueue(deterministic=True)
        outs = [torch.as_tensor(o0).cuda() for _, _, o0, _, _ in layers]
        for (_, _, _, dy, x), o in zip(layers, outs):
            q.add(dy, x, o)
        q.flush()
        runs.append(outs)
    for a, b, c in zip(*runs):
        assert _same_bits(a, b) and _same_bits(a, c)
    for (dy, x, o0, _, _), got in zip(layers, runs[0]):
        want = o0.astype(np.float64) + dy.astype(np.float64).T @ x.astype(np.float64)
        bound = 2 * DC.sum_bound(np.abs(o0).astype(np.float64) + np.abs(dy).astype(np.float64).T @ np.abs(x).astype(np.float64), P + 1)
        assert (np.abs(got.cpu().numpy() - want) <= bound).all(), dy.shape
    # overlapping writers: layers 0 and a second product of the same shape into the same slice
    dy2 = DC.order_sensitive(rng, (P, 24), True); x2 = DC.order_sensitive(rng, (P, 72), True)
    dy2_t, x2_t = torch.as_tensor(dy2).cuda().to(torch.bfloat16), torch.as_tensor(x2).cuda().to(torch.bfloat16)
    both = []
    for _ in range(3):
        q = ops.WgradQueue(deterministic=True)
        o = torch.as_tensor(layers[0][2]).cuda()
        q.add(layers[0][3], layers[0][4], o); q.add(dy2_t, x2_t, o)
        q.flush()
        both.append(o)
    assert _same_bits(both[0], both[1]) and _same_bits(both[0], both[2])
    seq = torch.as_tensor(layers[0][2]).cuda()
    ops.wgrad_tn(layers[0][3], layers[0][4], out=seq, deterministic=True)
    ops.wgrad_tn(dy2_t, x2_t, out=seq, deterministic=True)
    assert _same_bits(seq, both[0])
    # the default path (stream-K shares) is left alone and agrees to rounding
    o = torch.as_tensor(layers[2][2]).cuda()
    ops.wgrad_tn(layers[2][3], layers[2][4], out=o)
    assert float((o - runs[0][2]).abs().max()) <= 1e-4 * float(runs[0][2].abs().max())


# ---------------------------------------------------------------------------------------------------------
# the whole step
# ---------------------------------------------------------------------------------------------------------
def _feat_size(n):
    n = (n + 2 * 3 - 7) // 2 + 1
    n = -(-(n - 3) // 2) + 1
    n = (n - 1) // 2 + 1
    return (n - 1) // 2 + 1


def _setup(kind, seed):
    """tests/test_gpu_train_step.py's smallest setup: 128 x 160 image, 4 gt boxes, rpn_post_nms_top_n 40, first_n 24."""
    import relnet_amd  # noqa: F401
    from relnet_amd import backbone, train
    H, W, G = 128, 160, 4
    p = backbone.init_params(seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in ('cls_score_weight', 'bbox_pred_weight'):
        p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    p['conv_new_1_bias'] = torch.rand(256, generator=g) * 0.1 + 0.05
    if kind == 'learn_nms':          # un-saturate the duplicate classifier so that its gradients are not tiny
        g_ = torch.Generator().manual_seed(77)
        p['nms_logit_bias'] = torch.zeros(5)
        for k in ('nms_logit_weight', 'nms_rank_weight', 'roi_feat_embedding_weight', 'nms_query_1_weight', 'nms_key_1_weight',
                  'nms_linear_out_1_weight', 'nms_pair_pos_fc1_1_weight'):
            p[k] = torch.randn(p[k].shape, generator=g_) * 0.05

    def make_cfg(deterministic):
        cfg = train.TrainConfig()
        cfg.rpn_post_nms_top_n, cfg.first_n = 40, 24
        cfg.learn_nms = kind == 'learn_nms'
        if kind == 'plain':
            cfg.relation, cfg.enable_ohem = False, False
        cfg.deterministic = deterministic
        return cfg
    data = torch.randn(1, 3, H, W, generator=g)
    rng = np.random.default_rng(seed + 2)
    gt = np.zeros((1, G, 5), np.float32)
    x1 = rng.uniform(0, W - 70, G); y1 = rng.uniform(0, H - 70, G)
    gt[0, :, 0], gt[0, :, 1] = x1, y1
    gt[0, :, 2], gt[0, :, 3] = x1 + rng.uniform(30, 69, G), y1 + rng.uniform(30, 69, G)
    gt[0, :, 4] = rng.integers(1, 81, G)
    L, Tg, Wg = train.assign_anchor((_feat_size(H), _feat_size(W)), gt[0], (H, W), make_cfg(False), seed=seed)
    d = lambda a: torch.as_tensor(a).cuda()
    batch = (data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
    return p, make_cfg, batch, train, (H, W)


def _three_steps(tr, batch):
    rec = []
    with torch.no_grad():
        for _ in range(3):
            out = tr.forward_backward(*batch)
            scalars = {k: v.clone() for k, v in out.items() if torch.is_tensor(v) and v.numel() == 1 and v.is_floating_point()}
            rec.append((tr.W.grad.clone(), tr.Bv.grad.clone(), scalars))
            tr.all_reduce(); tr.update()
    torch.cuda.synchronize()
    return rec


@pytest.mark.parametrize('kind', ['learn_nms', 'relation', 'plain'])
def test_two_deterministic_trainers_give_the_same_bits_step_after_step(kind):
    """Two trainers with cfg.deterministic = True built from the same parameters run three forward_backward + update steps on the same
    batch: W.grad, Bv.grad and every loss scalar of the output are bit-equal after every step, W.master, W.mom and Bv.master after the third.
    The first step's gradients stay close to the default trainer's on the same inputs -- the forward and every discrete decision are the
    same, only float32 summation orders differ: the bound tests/test_gpu_train_step.py holds a regrouped sum of the same terms to
    (flat buffer cosine > 0.9995, norm within 5e-3)."""
    p, make_cfg, batch, train, hw = _setup(kind, 31)
    a = train.Trainer(p, make_cfg(True), im_hw=hw)
    assert a.deterministic and a._wq.deterministic and a._cq.deterministic
    ra = _three_steps(a, batch)
    b = train.Trainer(p, make_cfg(True), im_hw=hw)
    rb = _three_steps(b, batch)
    for step, ((wa, ba, sa), (wb, bb, sb)) in enumerate(zip(ra, rb)):
        assert float(wa.abs().max()) > 0 and torch.isfinite(wa).all()
        assert _same_bits(wa, wb), 'W.grad differs in step %d: %d words' % (step, int((_bits(wa) != _bits(wb)).sum()))
        assert _same_bits(ba, bb), 'Bv.grad differs in step %d: %d words' % (step, int((_bits(ba) != _bits(bb)).sum()))
        assert set(sa) == set(sb) and 'bbox_loss' in sa and 'rpn_bbox_loss' in sa
        assert ('nms_pos_loss' in sa) == (kind == 'learn_nms')
        for k in sa:
            assert _same_bits(sa[k], sb[k]), (step, k)
    assert not _same_bits(ra[0][0], ra[2][0])                                     # the steps did move the weights
    assert _same_bits(a.W.master, b.W.master) and _same_bits(a.W.mom, b.W.mom) and _same_bits(a.Bv.master, b.Bv.master)
    dflt = train.Trainer(p, make_cfg(False), im_hw=hw)
    assert not dflt.deterministic
    with torch.no_grad():
        out = dflt.forward_backward(*batch)
    for got, want, name in ((ra[0][0], dflt.W.grad, 'weights'), (ra[0][1], dflt.Bv.grad, 'biases')):
        g, w = got.double(), want.double()
        cos = float((g * w).sum() / (g.norm() * w.norm()))
        print('%s %s: cosine %.7f norm ratio %.6f' % (kind, name, cos, float(g.norm() / w.norm())))
        assert cos > 0.9995 and abs(float(g.norm() / w.norm()) - 1) < 5e-3, (name, cos)
    for k, v in ra[0][2].items():
        assert abs(float(v) - float(out[k])) <= 1e-4 * max(abs(float(out[k])), 1e-6), k


def test_captured_deterministic_step_replays_bit_for_bit():
    """CapturedStep of a deterministic trainer captures (the ordered kernels' workspaces come from the capture's own pool: no host
    synchronisation inside the step) and two replays from the same state give bit-equal gradient buffers."""
    p, make_cfg, batch, train, hw = _setup('learn_nms', 41)
    tr = train.Trainer(p, make_cfg(True), im_hw=hw)
    batch = batch[:3]                                       # anchor targets on the device, inside the step
    with torch.no_grad():
        tr.forward_backward(*batch)                        # eager warm-up
        g_eager = tr.W.grad.clone()
        tr._anchor_step.zero_()
        step = train.CapturedStep(tr, batch)
        grads = []
        for _ in range(2):
            tr._anchor_step.zero_()                        # the same random anchor subsets in both replays
            out = step.replay()
            torch.cuda.synchronize()
            grads.append((tr.W.grad.clone(), tr.Bv.grad.clone(), {k: out[k].clone() for k in ('bbox_loss', 'rpn_bbox_loss', 'nms_pos_loss', 'nms_neg_loss')}))
    assert float(grads[0][0].abs().max()) > 0
    assert _same_bits(grads[0][0], grads[1][0]) and _same_bits(grads[0][1], grads[1][1])
    for k in grads[0][2]:
        assert _same_bits(grads[0][2][k], grads[1][2][k]), k
    assert _same_bits(grads[0][0], g_eager)                 # and captured equals eager, bit for bit
