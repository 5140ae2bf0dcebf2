"""pooling.RoiPooling on the GPU against the direct `ops` calls it stands for: every operator (ROIPooling, ROIAlign, the two-pass
deformable PSROI pooling), one map and two maps, forward bit for bit and the adjoint.

Shape: 2 images, 64 channels, bf16 channels-last maps of 6 x 9 cells at scale 1/16 and 12 x 18 at 1/8 (a 96 x 144 image); five rois per
image: the whole map, a single cell, one with x2 < x1, one half outside the image, one ordinary.

Adjoint bounds.  ROIPooling's adjoint only adds output gradients: with integer-valued d_pool in -2..2 every sum is exact in any order, so
it is compared with np.array_equal, scatter, ordered and pyramid form alike.  ROIAlign's and the deformable pooling's adjoints add
weighted terms with float atomics in an order the hardware picks: `backward_f32` is held to the direct call at the relative bound the
project holds these kernels to (_relerr <= 2e-5, tests/test_gpu_deform.py).  `backward` returns that gradient converted to bf16 (a run
of its own, so other atomics orders): one round-to-nearest to 8 significant bits (unit roundoff 2^-8), |bf16(y) - y| <= 2^-8 |y|, on
top of the 2e-5 bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

B, C, R = 2, 64, 10
SCALES = (1 / 16.0, 1 / 8.0)
ATOMIC_RELERR = 2e-5


def _mods():
    import relnet_amd  # noqa: F401
    from relnet_amd import detector, ops, pooling
    return detector, ops, pooling


_CASE = {}


def _case():
    """maps, rois, levels and d_pool: made once, never written afterwards"""
    if not _CASE:
        rng = np.random.default_rng(1807)
        maps = [torch.as_tensor(rng.standard_normal((B, h, w, C)).astype(np.float32)).cuda().to(torch.bfloat16).permute(0, 3, 1, 2)
                for h, w in ((6, 9), (12, 18))]
        per_image = np.array([[0, 0, 143, 95],          # the whole map
                              [35, 19, 37, 21],         # one cell at 1/16 (cell (1, 2)); 2 x 2 cells at 1/8
                              [100, 40, 60, 70],        # x2 < x1
                              [100, 50, 220, 130],      # half outside the image
                              [20, 10, 90, 70]], np.float32)
        rois = np.concatenate([np.concatenate([np.full((5, 1), b, np.float32), per_image + 3 * b], 1) for b in range(B)], 0)
        _CASE.update(maps=maps, rois=torch.as_tensor(rois).cuda(),
                     level=torch.as_tensor(np.array([0, 1, 0, 1, 1, 1, 0, 1, 0, 0], np.int32)).cuda(),
                     d_int=torch.as_tensor(rng.integers(-2, 3, (R, 49 * C)).astype(np.float32)).cuda().to(torch.bfloat16),
                     d_real=torch.as_tensor(rng.standard_normal((R, 49 * C)).astype(np.float32)).cuda().to(torch.bfloat16))
    return _CASE


def _cfg(**kw):
    cfg = _mods()[0].Config()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _bits(t):
    t = t.contiguous()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()


def _flat(t):
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1)


def _unflat(t):
    return t.view(t.shape[0], 7, 7, -1).permute(0, 3, 1, 2)


def _relerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-30))


# the offset FC of the deformable case: a fixed linear map without a reduction (bit-reproducible), and its adjoint
def _offset_fc(t0f):
    return (t0f.view(R, 49, C)[:, :, :2].float() * 0.5).permute(0, 2, 1).contiguous()


def _offset_fc_bwd(t0f, g_trans):
    d = torch.zeros((R, 49, C), device=g_trans.device, dtype=torch.bfloat16)
    d[:, :, :2] = (g_trans.view(R, 2, 49).permute(0, 2, 1) * 0.5).to(torch.bfloat16)
    return d.view(R, -1)


def _setup(kind, n_maps, deterministic=False):
    _, ops, pooling = _mods()
    k = _case()
    cfg = _cfg(roi_align=(kind == 'align'), dcn=(kind == 'dcn'))
    pool = pooling.RoiPooling(cfg, SCALES[:n_maps], deterministic=deterministic)
    return ops, pool, cfg, k['maps'][:n_maps], k['rois'], (k['level'] if n_maps > 1 else None)


@pytest.mark.parametrize('kind,n_maps', [('pool', 1), ('pool', 2), ('align', 1), ('align', 2), ('dcn', 1)])
def test_forward_equals_the_direct_call(kind, n_maps):
    ops, pool, cfg, maps, rois, level = _setup(kind, n_maps)
    got = pool.forward(maps, rois, level, offset_fc=_offset_fc if kind == 'dcn' else None)
    assert tuple(got.shape) == (R, 49 * C) and got.is_contiguous()
    if kind == 'pool' and n_maps == 1:
        want = [ops.roi_pool(maps[0], rois, (7, 7), SCALES[0], channels_last_out=True)]
    elif kind == 'pool':
        want = [ops.roi_pool_fpn(maps, SCALES, rois, level, (7, 7), channels_last_out=True)]
    elif kind == 'align':
        want = [ops.roi_align_fpn(maps, SCALES[:n_maps], rois, level, (7, 7), cfg.roi_align_sampling, channels_last_out=True)]
        if n_maps == 1:     # (the single-map entry: the same kernel)
            want.append(ops.roi_align(maps[0], rois, (7, 7), SCALES[0], cfg.roi_align_sampling, channels_last_out=True))
    else:
        f, spp = maps[0], cfg.dcn_sample_per_part
        t0 = ops.deformable_psroi_pool(f, rois, None, SCALES[0], C, 1, 7, 7, spp, 0.0, True, channels_last_out=True)
        trans = _offset_fc(_flat(t0)).view(R, 2, 7, 7)
        assert float(trans.abs().max()) > 0.1                   # offsets that move the samples
        want = [ops.deformable_psroi_pool(f, rois, trans, SCALES[0], C, 1, 7, 7, spp, cfg.dcn_trans_std, False, channels_last_out=True)]
    assert float(got.float().abs().max()) > 0
    for w in want:
        assert np.array_equal(_bits(got), _bits(_flat(w)))
    # want_backward only adds the context (ROIPooling: the argmax instantiation of the same kernel)
    got2, ctx = pool.forward(maps, rois, level, offset_fc=_offset_fc if kind == 'dcn' else None, want_backward=True)
    assert np.array_equal(_bits(got), _bits(got2))


@pytest.mark.parametrize('form', ['scatter', 'ordered', 'pyramid'])
def test_roi_pooling_backward_equals_the_direct_call(form):
    n_maps = 2 if form == 'pyramid' else 1
    ops, pool, cfg, maps, rois, level = _setup('pool', n_maps, deterministic=(form == 'ordered'))
    d_pool = _case()['d_int']
    _, ctx = pool.forward(maps, rois, level, want_backward=True)
    if n_maps == 1:
        _, arg = ops.roi_pool(maps[0], rois, (7, 7), SCALES[0], channels_last_out=True, want_argmax=True)
        want = [ops.roi_pool_bwd(_unflat(d_pool), arg, rois, tuple(maps[0].shape), channels_last=True, deterministic=(form == 'ordered'),
                                 spatial_scale=SCALES[0])]
    else:
        _, arg = ops.roi_pool_fpn(maps, SCALES, rois, level, (7, 7), channels_last_out=True, want_argmax=True)
        want = ops.roi_pool_fpn_bwd(_unflat(d_pool), arg, rois, level, [tuple(m.shape) for m in maps], channels_last=True)
    assert np.array_equal(_bits(ctx['argmax']), _bits(arg))
    got32, got = pool.backward_f32(d_pool, ctx), pool.backward(d_pool, ctx)
    assert len(got) == len(got32) == n_maps
    for g, g32, w, m in zip(got, got32, want, maps):
        assert float(w.abs().max()) >= 2 and bool((w == w.round()).all())           # integer sums: exact in any order
        assert np.array_equal(_bits(g32), _bits(w))
        assert g.dtype == torch.bfloat16 and g.is_contiguous() and tuple(g.shape) == tuple(m.permute(0, 2, 3, 1).shape)
        assert np.array_equal(_bits(g), _bits(w.permute(0, 2, 3, 1).to(torch.bfloat16)))


@pytest.mark.parametrize('kind,n_maps', [('align', 1), ('align', 2), ('dcn', 1)])
def test_atomic_backward_matches_the_direct_call(kind, n_maps):
    ops, pool, cfg, maps, rois, level = _setup(kind, n_maps)
    d_pool = _case()['d_real']
    shapes = [tuple(m.shape) for m in maps]
    _, ctx = pool.forward(maps, rois, level, offset_fc=_offset_fc if kind == 'dcn' else None, want_backward=True)
    if kind == 'align':
        want = ops.roi_align_fpn_bwd(_unflat(d_pool), rois, level, shapes, SCALES[:n_maps], cfg.roi_align_sampling, channels_last=True)
    else:
        f, spp = maps[0], cfg.dcn_sample_per_part
        gd1, g_trans = ops.deformable_psroi_pool_bwd(_unflat(d_pool), f, rois, ctx['trans'], SCALES[0], C, 1, 7, 7, spp, cfg.dcn_trans_std, False)
        d_t0 = _offset_fc_bwd(ctx['t0f'], g_trans.view(R, -1))
        assert float(d_t0.float().abs().max()) > 0
        gd2, _ = ops.deformable_psroi_pool_bwd(_unflat(d_t0), f, rois, None, SCALES[0], C, 1, 7, 7, spp, 0.0, True)
        want = [gd1 + gd2]
    fc_bwd = _offset_fc_bwd if kind == 'dcn' else None
    got32, got = pool.backward_f32(d_pool, ctx, fc_bwd), pool.backward(d_pool, ctx, fc_bwd)
    assert len(got) == len(got32) == n_maps
    for g, g32, w, m in zip(got, got32, want, maps):
        w64 = w.permute(0, 2, 3, 1).double().cpu().numpy()
        top = np.abs(w64).max()
        assert top > 0
        err = _relerr(g32.permute(0, 2, 3, 1).cpu().numpy(), w64)
        print('%s x%d: backward_f32 relerr %.3g' % (kind, n_maps, err))
        assert err <= ATOMIC_RELERR
        assert g.dtype == torch.bfloat16 and g.is_contiguous() and tuple(g.shape) == tuple(m.permute(0, 2, 3, 1).shape)
        slack = ATOMIC_RELERR * top
        bound = slack + 2.0 ** -8 * (np.abs(w64) + slack)
        over = np.abs(g.double().cpu().numpy() - w64) - bound
        print('%s x%d: backward (bf16) worst |err| - bound %.3g' % (kind, n_maps, over.max()))
        assert (over <= 0).all()
