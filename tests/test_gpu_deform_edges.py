"""csrc/deform.hip on the exact border lattices of tests/deform_edge_cases.py: every sum of these cases is exact in float32 whatever its order, so
the atomic scatter, the gather + offset + far kernels at every window radius, the four-channels-per-thread and the one-channel PSROI kernels and
both im2col kernels must give the float64 restatement BIT FOR BIT (np.array_equal; no tolerance).  The restatement itself is held to the
reference's own kernels by tests/test_deform_edge_cases_host.py (tests/golden/ref_cuda_deform_edges.npz); where oracle/_ref is built the product is
also compared with those kernels directly.

Operands are views inside larger parents: NaN around the data and the column gradient (a read outside the map or past column K poisons the
result), an integer pattern under and around the gradients (the kernels accumulate: out - before is compared, and nothing outside the view may
change).  The one inexact quantity is the PSROI trans gradient at addresses that collect more than 2^24 lattice units of |terms| (the 128 / 256
channel shapes): n = channels per class * spp^2 exact terms are added there in an unknown order, n - 1 roundings each relative to a partial sum
of at most sum|terms|, so |error| <= n u sum|terms| (u = 2^-24); every other address is held to equality.  The degenerate roi (extent floored
to 0.1: off every lattice) is the second bounded set, with the constants counted in deform_edge_cases.ps_bound_k."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import deform_edge_cases as DE  # noqa: E402
from oracle import deform, refcuda as RC  # noqa: E402

pytestmark = pytest.mark.gpu
IDS = [c[0] for c in DE.COL2IM_CASES]
MODES = (1, 0, 2, 10, 11, 12, 13)          # relnet_deformable_col2im_debug: scatter, auto (radius 3), every pair far, radius 0 .. 3
KK = (DE.K, DE.K)
needs_ref = pytest.mark.skipif(not RC.available(), reason='oracle/_ref/libref_cuda.so not built (no /root/reference)')


def _mods():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib
    return ops, lib.load()


def _tdt(name):
    return torch.float32 if name == 'f32' else torch.bfloat16


def _pattern(shape):
    """Small integers: exact under every accumulation of this file."""
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.float32) % 7) - 3).reshape(shape).cuda()


def _nchw_view(logical, layout, dtype, fill):
    """logical numpy [B,C,H,W] -> (parent, view): the view is logical [B,C,H,W] inside a parent one row, one column and 8 channels (channels-last) /
    one channel (NCHW) larger, filled with `fill` (NaN, or None for the integer pattern)."""
    B, C, H, W = logical.shape
    shape = (B, H + 1, W + 1, C + 8) if layout == 'cl' else (B, C + 1, H + 1, W + 1)
    parent = (_pattern(shape) if fill is None else torch.full(shape, fill, device='cuda')).to(dtype)
    view = parent[:, :H, :W, :C].permute(0, 3, 1, 2) if layout == 'cl' else parent[:, :C, :H, :W]
    return parent, view


def _put(view, logical):
    view.copy_(torch.as_tensor(logical).to(view.dtype))


def _outside_unchanged(parent, before, view_of):
    mask = torch.ones_like(parent, dtype=torch.bool)
    view_of(mask).fill_(False)
    return bool(torch.equal(parent[mask], before[mask]))


def _col2im_operands(c, dcol_dtype):
    _, data, off, dcol, gd, go = DE.col2im_reference(c.id)
    Kc = DE.T * c.C
    rows = c.B * c.Ho * c.Wo
    dparent = torch.full((rows, Kc + 8), float('nan'), device='cuda', dtype=_tdt(dcol_dtype))
    dview = dparent[:, :Kc]
    dview.copy_(torch.as_tensor(dcol.reshape(rows, Kc)).to(dview.dtype))
    _, x = _nchw_view(data, c.layout, _tdt(c.dtype), float('nan'))
    _put(x, data)
    o = torch.as_tensor(off).cuda()
    if c.layout == 'cl':
        o = o.contiguous(memory_format=torch.channels_last)
    return dview, x, o, gd, go


def _run_col2im(ops, c, dview, x, o):
    gparent, g = _nchw_view(np.zeros((c.B, c.C, c.H, c.W), np.float32), c.layout, torch.float32, None)
    oparent, go_ = _nchw_view(np.zeros((c.B, 2 * DE.T * c.dg, c.Ho, c.Wo), np.float32), c.layout, torch.float32, None)
    gbefore, obefore = gparent.clone(), oparent.clone()
    g0, o0 = g.clone(), go_.clone()
    ops.deformable_col2im(dview, x, o, KK, c.stride, c.dil, c.pad, c.dg, grad_data=g, grad_offset=go_)
    torch.cuda.synchronize()
    assert not torch.isnan(gparent).any() and not torch.isnan(oparent).any()
    sl = (lambda m: m[:, :c.H, :c.W, :c.C]) if c.layout == 'cl' else (lambda m: m[:, :c.C, :c.H, :c.W])
    so = (lambda m: m[:, :c.Ho, :c.Wo, :2 * DE.T * c.dg]) if c.layout == 'cl' else (lambda m: m[:, :2 * DE.T * c.dg, :c.Ho, :c.Wo])
    assert _outside_unchanged(gparent, gbefore, sl) and _outside_unchanged(oparent, obefore, so)
    return (g - g0).cpu().numpy(), (go_ - o0).cpu().numpy()


@pytest.mark.parametrize('dcol_dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('id_', IDS)
def test_col2im_equals_restatement_bit_for_bit(id_, dcol_dtype):
    ops, L = _mods()
    c = DE.case(id_)
    dview, x, o, gd, go = _col2im_operands(c, dcol_dtype)
    if c.gather:       # the conditions of the gather form hold for these views (deform.hip: gather_ok)
        assert x.stride(1) == 1 and all(s % 8 == 0 for s in (x.stride(0), x.stride(2), x.stride(3), dview.stride(0)))
        assert x.data_ptr() % 16 == 0 and dview.data_ptr() % 16 == 0 and (c.cpg % 64 == 0) and c.cpg // 8 <= 64
    try:
        for mode in (MODES if c.gather else (0,)):
            L.relnet_deformable_col2im_debug(mode)
            got_d, got_o = _run_col2im(ops, c, dview, x, o)
            bad_d, bad_o = np.argwhere(got_d != gd), np.argwhere(got_o != go)
            assert len(bad_d) == 0, (id_, mode, 'grad_data', len(bad_d), bad_d[:4].tolist())
            assert len(bad_o) == 0, (id_, mode, 'grad_offset', len(bad_o), bad_o[:4].tolist())
    finally:
        L.relnet_deformable_col2im_debug(0)


@pytest.mark.parametrize('id_', IDS)
def test_im2col_equals_oracle_bit_for_bit(id_):
    """The generic kernel with float32 columns on every case; with bf16 columns the 8-channels-per-thread kernel on the channels-last cases and the
    generic kernel on the NCHW one: sampled values are exact multiples of 1/64 in float32, and their bf16 store is one round-to-nearest-even."""
    ops, _ = _mods()
    c = DE.case(id_)
    _, data, off, _, _, _ = DE.col2im_reference(id_)
    _, x, o, _, _ = _col2im_operands(c, 'f32')
    want = np.stack([deform.deformable_im2col(data[b], off[b], KK, (c.pad, c.pad), (c.stride, c.stride), (c.dil, c.dil), c.dg) for b in range(c.B)])
    assert (want == 0).any() and (want != 0).any()
    lay = lambda col: col.float().cpu().numpy().reshape(c.B, c.Ho, c.Wo, DE.T, c.C).transpose(0, 4, 3, 1, 2).reshape(c.B, c.C * DE.T, c.Ho, c.Wo)
    col, (ho, wo) = ops.deformable_im2col(x, o, KK, c.stride, c.dil, c.pad, c.dg, col_dtype=torch.float32)
    assert (ho, wo) == (c.Ho, c.Wo) and np.array_equal(lay(col), want)
    if c.dtype == 'bf16':
        colb, _ = ops.deformable_im2col(x, o, KK, c.stride, c.dil, c.pad, c.dg, col_dtype=torch.bfloat16)
        assert np.array_equal(lay(colb), torch.as_tensor(want).bfloat16().float().numpy())


@needs_ref
@pytest.mark.parametrize('id_', DE.GOLDEN_CASES)
def test_col2im_equals_reference_kernels_directly(id_):
    ops, _ = _mods()
    c = DE.case(id_)
    _, data, off, dcol, _, _ = DE.col2im_reference(id_)
    dview, x, o, _, _ = _col2im_operands(c, 'f32')
    got_d, got_o = _run_col2im(ops, c, dview, x, o)
    pad, st, dil = (c.pad, c.pad), (c.stride, c.stride), (c.dil, c.dil)
    for b in range(c.B):
        col = DE.dcol_to_reference(c, dcol, b)
        assert np.array_equal(got_d[b], RC.deformable_col2im(col, off[b], (c.C, c.H, c.W), KK, pad, st, dil, c.dg))
        assert np.array_equal(got_o[b], RC.deformable_col2im_coord(col, data[b], off[b], KK, pad, st, dil, c.dg))


# ---------------------------------------------------------------------------------------------------------------------------------------------
PS_ALL = DE.ps_configs()
WORST = {}            # kernel -> worst ratio of the bounded set (printed; profiles/r13_notes/deform_edges.txt keeps the figures of the run it records)


def _ps_device(cfg, layout, base=0):
    data, rois, trans, mult, r = DE.ps_reference(cfg)
    dt = _tdt('bf16' if layout == 'cl' else 'f32')
    _, x = _nchw_view(data, layout, dt, float('nan'))
    _put(x, data)
    rr = rois.copy(); rr[:, 0] += base
    gout = DE.ps_grad_out(r['count'], mult)
    if layout == 'cl':
        g = torch.as_tensor(gout).cuda().to(dt).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    else:
        g = torch.as_tensor(gout).cuda()
    return x, torch.as_tensor(rr).cuda(), None if trans is None else torch.as_tensor(trans).cuda(), g, r


def _ps_args(cfg, trans):
    return (trans, DE.PS_SCALE, cfg.od, cfg.group, cfg.P, cfg.part, cfg.spp, DE.PS_TRANS_STD if trans is not None else 0.0, trans is None)


def _check_trans(cfg, r, got, kernel):
    _, ut = DE.ps_exact_units(cfg, r)
    exact = ut < 2.0 ** 24
    got = got.cpu().numpy().astype(np.float64)
    bad = np.argwhere((got != r['grad_trans']) & exact)
    assert len(bad) == 0, (cfg.id, kernel, 'grad_trans', len(bad), bad[:4].tolist())
    if not exact.all():
        n = (cfg.od // cfg.ncls) * cfg.spp ** 2
        ratio = float((np.abs(got - r['grad_trans'])[~exact] / (n * DE.U * r['abs_trans'][~exact])).max())
        WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
        print('bounded set %s %s: %d addresses, worst ratio %.3e' % (cfg.id, kernel, int((~exact).sum()), ratio))
        assert ratio <= 1.0, (cfg.id, kernel, ratio)


@pytest.mark.parametrize('layout', ['nchw', 'cl'])
@pytest.mark.parametrize('cfg', PS_ALL, ids=repr)
def test_psroi_forward_equals_restatement_bit_for_bit(cfg, layout):
    ops, _ = _mods()
    x, rois, trans, _, r = _ps_device(cfg, layout)
    want = r['top'] if layout == 'nchw' else torch.as_tensor(r['top']).bfloat16().float().numpy()
    out, cnt = ops.deformable_psroi_pool(x, rois, *_ps_args(cfg, trans), want_top_count=True)
    assert np.array_equal(cnt.cpu().numpy(), r['count'])
    assert np.array_equal(out.float().cpu().numpy(), want)
    if layout == 'cl':          # without top_count, channels-last out: the 8-channels-per-thread kernel where group == 1 and the offsets have one class
        out2 = ops.deformable_psroi_pool(x, rois, *_ps_args(cfg, trans), channels_last_out=True)
        assert out2.stride(1) == 1 and np.array_equal(out2.float().cpu().numpy(), want)


@pytest.mark.parametrize('layout', ['nchw', 'cl'])
@pytest.mark.parametrize('cfg', PS_ALL, ids=repr)
def test_psroi_backward_equals_restatement_bit_for_bit(cfg, layout):
    """Mode 0 takes the four-channels-per-thread kernel for the class-agnostic 256-channel shape at spp <= 4 and the one-channel kernel elsewhere
    (its per-sample form at spp 5); mode 1 forces the one-channel kernel."""
    ops, L = _mods()
    x, rois, trans, g, r = _ps_device(cfg, layout)
    c4 = cfg.od % 256 == 0 and cfg.group == 1 and cfg.ncls == 1 and cfg.spp <= 4
    try:
        for mode in ((0, 1) if c4 else (0,)):
            L.relnet_deformable_psroi_pool_bwd_debug(mode)
            gd, gt = ops.deformable_psroi_pool_bwd(g, x, rois, *_ps_args(cfg, trans))
            torch.cuda.synchronize()
            kernel = 'bwd_c4' if (c4 and mode == 0) else ('bwd_one' if cfg.spp <= 4 else 'bwd_one_per_sample')
            got = gd.cpu().numpy()
            bad = np.argwhere(got != r['grad_data'])
            assert len(bad) == 0, (cfg.id, kernel, 'grad_data', len(bad), bad[:4].tolist())
            if trans is not None:
                _check_trans(cfg, r, gt, kernel)
            else:
                assert gt is None
    finally:
        L.relnet_deformable_psroi_pool_bwd_debug(0)


def test_psroi_batch_index_base():
    """rois numbered from 1 with batch_index_base = 1 give the results of rois numbered from 0."""
    ops, _ = _mods()
    cfg = DE.PsCfg(DE.PS_SHAPES[0], 2, True)
    x, rois, trans, g, r = _ps_device(cfg, 'nchw', base=1)
    out, cnt = ops.deformable_psroi_pool(x, rois, *_ps_args(cfg, trans), want_top_count=True, batch_index_base=1)
    assert np.array_equal(out.cpu().numpy(), r['top']) and np.array_equal(cnt.cpu().numpy(), r['count'])
    gd, gt = ops.deformable_psroi_pool_bwd(g, x, rois, *_ps_args(cfg, trans), batch_index_base=1)
    assert np.array_equal(gd.cpu().numpy(), r['grad_data'])
    _check_trans(cfg, r, gt, 'bwd_one')


@needs_ref
@pytest.mark.parametrize('cfg', DE.ps_configs(max_channels=128), ids=repr)
def test_psroi_equals_reference_kernels_directly(cfg):
    ops, _ = _mods()
    data, rois_np, trans_np, mult, r = DE.ps_reference(cfg)
    x, rois, trans, g, _ = _ps_device(cfg, 'nchw')
    args = (DE.PS_SCALE, cfg.od, cfg.group, cfg.P, cfg.part, cfg.spp, DE.PS_TRANS_STD)
    wtop, wcnt = RC.psroi_forward(data, rois_np, trans_np, *args)
    out, cnt = ops.deformable_psroi_pool(x, rois, *_ps_args(cfg, trans), want_top_count=True)
    assert np.array_equal(cnt.cpu().numpy(), wcnt) and np.array_equal(out.cpu().numpy(), wtop)
    wi, wt = RC.psroi_backward(DE.ps_grad_out(wcnt, mult), wcnt, data, rois_np, trans_np, *args)
    gd, gt = ops.deformable_psroi_pool_bwd(g, x, rois, *_ps_args(cfg, trans))
    assert np.array_equal(gd.cpu().numpy(), wi)
    if trans_np is not None:
        _, ut = DE.ps_exact_units(cfg, r)
        exact = ut < 2.0 ** 24
        assert np.array_equal(gt.cpu().numpy()[exact], wt[exact])          # (beyond: both sides round, each held to the restatement's bound)


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['nchw', 'cl'])
@pytest.mark.parametrize('k', range(len(DE.PS_DEGENERATE_CFGS)))
def test_psroi_bounded_set(k, layout):
    """The degenerate roi (extent floored to 0.1) against the float64 restatement under k u magnitude, k counted in deform_edge_cases.ps_bound_k.
    bf16 operands are exact inputs; the bf16 store of the pooled value adds half a bf16 step (8 significant bits: at most 2^-8 of the value)."""
    ops, L = _mods()
    cfg, data, rois_np, trans_np, mult, r = DE.ps_degenerate(k)
    dt = _tdt('bf16' if layout == 'cl' else 'f32')
    _, x = _nchw_view(data, layout, dt, float('nan'))
    _put(x, data)
    rois = torch.as_tensor(rois_np).cuda()
    trans = None if trans_np is None else torch.as_tensor(trans_np).cuda()
    K = DE.ps_bound_k(cfg)
    out, cnt = ops.deformable_psroi_pool(x, rois, *_ps_args(cfg, trans), want_top_count=True)
    assert np.array_equal(cnt.cpu().numpy(), r['count'])
    top64 = r['top'].astype(np.float64)
    store = 2.0 ** -8 * np.abs(top64) if layout == 'cl' else 0.0
    ratios = {'fwd': DE.worst(out.float().cpu().numpy(), top64, (K['top'] + 1) * DE.U * r['mag_top'] + store)}      # (+1: the restatement's own float32 store)
    gout = DE.ps_grad_out(r['count'], mult)
    g = torch.as_tensor(gout).cuda().to(dt)
    if layout == 'cl':
        g = g.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    c4 = cfg.od % 256 == 0 and cfg.group == 1 and cfg.ncls == 1 and cfg.spp <= 4
    try:
        for mode in ((0, 1) if c4 else (0,)):
            L.relnet_deformable_psroi_pool_bwd_debug(mode)
            gd, gt = ops.deformable_psroi_pool_bwd(g, x, rois, *_ps_args(cfg, trans))
            torch.cuda.synchronize()
            kernel = 'bwd_c4' if (c4 and mode == 0) else ('bwd_one' if cfg.spp <= 4 else 'bwd_one_per_sample')
            ratios[kernel + ' grad_data'] = DE.worst(gd.cpu().numpy(), r['grad_data'], K['grad_data'] * DE.U * r['mag_data'])
            if trans is not None:
                ratios[kernel + ' grad_trans'] = DE.worst(gt.cpu().numpy(), r['grad_trans'], K['grad_trans'] * DE.U * r['mag_trans'])
    finally:
        L.relnet_deformable_psroi_pool_bwd_debug(0)
    print('bounded set %s %s: %s' % (cfg.id, layout, ', '.join('%s %.3f' % kv for kv in sorted(ratios.items()))))
    assert np.abs(r['grad_data']).max() > 0
    assert all(v <= 1.0 for v in ratios.values()), (cfg.id, layout, ratios)
