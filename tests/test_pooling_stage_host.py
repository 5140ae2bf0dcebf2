"""The ROI pooling stage (pooling.RoiPooling) against a recording stand-in for its `ops` module, no GPU: for every (graph, operator)
combination the four graph classes build, the pooler calls the `ops` front end those graphs called before the stage existed, with the same
arguments, keeps for the backward what that operator's adjoint needs, and refuses at construction what has no kernel."""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, C, R = 2, 8, 5
FPN_SCALES = (1 / 4.0, 1 / 8.0, 1 / 16.0, 1 / 32.0)


def _mods():
    import relnet_amd  # noqa: F401
    from relnet_amd import detector, ops, pooling
    return detector, ops, pooling


class RecordingOps(object):
    """Stands in for pooling.ops: binds every call to the REAL front end's signature (so a default the caller left out reads as the
    default), records (name, arguments) and returns CPU tensors of the real shapes, layouts and dtypes."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def _bind(self, name, a, k):
        b = inspect.signature(getattr(self.real, name)).bind(*a, **k)
        b.apply_defaults()
        self.calls.append((name, dict(b.arguments)))
        return b.arguments

    @staticmethod
    def _pooled(n, c, dtype, want_argmax=False):
        out = torch.zeros((n, 7, 7, c), dtype=dtype).permute(0, 3, 1, 2)
        return (out, torch.zeros((n, 7, 7, c), dtype=torch.int32).permute(0, 3, 1, 2)) if want_argmax else out

    @staticmethod
    def _grad(shape):
        b, c, h, w = shape
        return torch.zeros((b, h, w, c), dtype=torch.float32).permute(0, 3, 1, 2)

    def roi_pool(self, *a, **k):
        g = self._bind('roi_pool', a, k)
        return self._pooled(g['rois'].shape[0], g['data'].shape[1], g['data'].dtype, g['want_argmax'])

    def roi_pool_fpn(self, *a, **k):
        g = self._bind('roi_pool_fpn', a, k)
        return self._pooled(g['rois'].shape[0], g['levels'][0].shape[1], g['levels'][0].dtype, g['want_argmax'])

    def roi_align_fpn(self, *a, **k):
        g = self._bind('roi_align_fpn', a, k)
        return self._pooled(g['rois'].shape[0], g['levels'][0].shape[1], g['levels'][0].dtype)

    def deformable_psroi_pool(self, *a, **k):
        g = self._bind('deformable_psroi_pool', a, k)
        return self._pooled(g['rois'].shape[0], g['output_dim'], g['data'].dtype)

    def roi_pool_bwd(self, *a, **k):
        return self._grad(self._bind('roi_pool_bwd', a, k)['in_shape'])

    def roi_pool_fpn_bwd(self, *a, **k):
        return [self._grad(s) for s in self._bind('roi_pool_fpn_bwd', a, k)['level_shapes']]

    def roi_align_fpn_bwd(self, *a, **k):
        return [self._grad(s) for s in self._bind('roi_align_fpn_bwd', a, k)['level_shapes']]

    def deformable_psroi_pool_bwd(self, *a, **k):
        g = self._bind('deformable_psroi_pool_bwd', a, k)
        return self._grad(g['data'].shape), (None if g['no_trans'] else torch.zeros_like(g['trans']))


def _maps(n):
    """n logical-NCHW views of NHWC bf16 memory, as the graphs hand them over"""
    return [torch.zeros((B, 6 * 2 ** (n - 1 - i), 9 * 2 ** (n - 1 - i), C), dtype=torch.bfloat16).permute(0, 3, 1, 2) for i in range(n)]


def _cfg(detector, **kw):
    cfg = detector.Config()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _run(monkeypatch, cfg_kw, n_maps, deterministic=False, want_backward=True):
    detector, ops, pooling = _mods()
    rec = RecordingOps(ops)
    monkeypatch.setattr(pooling, 'ops', rec)
    cfg = _cfg(detector, **cfg_kw)
    scales = FPN_SCALES if n_maps == 4 else (1.0 / cfg.feat_stride,)
    pool = pooling.RoiPooling(cfg, scales, deterministic=deterministic)
    maps, rois = _maps(n_maps), torch.zeros((R, 5))
    level = torch.zeros((R,), dtype=torch.int32) if n_maps > 1 else None

    def offset_fc(t0f):
        rec.calls.append(('offset_fc', dict(t0f=t0f)))
        return torch.zeros((R, 2 * 49), dtype=torch.float32)

    def offset_fc_bwd(t0f, g_trans):
        rec.calls.append(('offset_fc_bwd', dict(t0f=t0f, g_trans=g_trans)))
        return torch.zeros((R, 49 * C), dtype=torch.bfloat16)

    res = pool.forward(maps, rois, level, offset_fc=offset_fc if cfg.dcn else None, want_backward=want_backward)
    pooled2 = res[0] if want_backward else res
    assert tuple(pooled2.shape) == (R, 49 * C) and pooled2.is_contiguous() and pooled2.dtype == torch.bfloat16
    grads = None
    if want_backward:
        grads = pool.backward(torch.zeros((R, 49 * C), dtype=torch.bfloat16), res[1], offset_fc_bwd if cfg.dcn else None)
        assert len(grads) == n_maps
        for g, m in zip(grads, maps):       # NHWC bf16, the layout the trunk / neck backward takes
            assert g.dtype == torch.bfloat16 and g.is_contiguous() and tuple(g.shape) == tuple(m.permute(0, 2, 3, 1).shape)
    return rec.calls, maps, rois, level, cfg, scales


def _logical_grad(a, rois):
    """the output gradient as the adjoints take it: logical [R,C,7,7] over (R,7,7,C) memory"""
    return tuple(a.shape) == (rois.shape[0], C, 7, 7) and a.permute(0, 2, 3, 1).is_contiguous()


@pytest.mark.parametrize('want_backward', [False, True])
def test_roi_pooling_one_map(monkeypatch, want_backward):
    calls, maps, rois, level, cfg, scales = _run(monkeypatch, {}, 1, want_backward=want_backward)
    assert [n for n, _ in calls] == (['roi_pool', 'roi_pool_bwd'] if want_backward else ['roi_pool'])
    f = calls[0][1]
    assert f['data'] is maps[0] and f['rois'] is rois and tuple(f['pooled']) == (7, 7) and f['spatial_scale'] == 1.0 / 16
    assert f['channels_last_out'] is True and f['want_argmax'] is want_backward and f['batch_index_base'] == 0
    if want_backward:
        b = calls[1][1]
        assert _logical_grad(b['grad_out'], rois) and b['argmax'].dtype == torch.int32 and b['rois'] is rois
        assert tuple(b['in_shape']) == tuple(maps[0].shape) and b['channels_last'] is True
        assert b['deterministic'] is False and b['spatial_scale'] == 1.0 / 16


def test_deterministic_roi_pooling_one_map(monkeypatch):
    calls, maps, rois, level, cfg, scales = _run(monkeypatch, {}, 1, deterministic=True)
    assert [n for n, _ in calls] == ['roi_pool', 'roi_pool_bwd']
    assert calls[0][1]['want_argmax'] is True
    b = calls[1][1]
    assert b['deterministic'] is True and b['spatial_scale'] == 1.0 / 16 and b['channels_last'] is True


@pytest.mark.parametrize('want_backward', [False, True])
def test_roi_pooling_four_maps(monkeypatch, want_backward):
    calls, maps, rois, level, cfg, scales = _run(monkeypatch, {}, 4, want_backward=want_backward)
    assert [n for n, _ in calls] == (['roi_pool_fpn', 'roi_pool_fpn_bwd'] if want_backward else ['roi_pool_fpn'])
    f = calls[0][1]
    assert all(a is m for a, m in zip(f['levels'], maps)) and tuple(f['scales']) == FPN_SCALES and f['rois'] is rois
    assert f['roi_level'] is level and tuple(f['pooled']) == (7, 7) and f['channels_last_out'] is True and f['want_argmax'] is want_backward
    if want_backward:
        b = calls[1][1]
        assert _logical_grad(b['grad_out'], rois) and b['argmax'].dtype == torch.int32 and b['rois'] is rois and b['roi_level'] is level
        assert [tuple(s) for s in b['level_shapes']] == [tuple(m.shape) for m in maps] and b['channels_last'] is True


@pytest.mark.parametrize('n_maps', [1, 4])
@pytest.mark.parametrize('want_backward', [False, True])
def test_roi_align(monkeypatch, n_maps, want_backward):
    calls, maps, rois, level, cfg, scales = _run(monkeypatch, dict(roi_align=True, roi_align_sampling=3), n_maps, want_backward=want_backward)
    assert [n for n, _ in calls] == (['roi_align_fpn', 'roi_align_fpn_bwd'] if want_backward else ['roi_align_fpn'])
    f = calls[0][1]
    assert all(a is m for a, m in zip(f['levels'], maps)) and len(f['levels']) == n_maps and tuple(f['scales']) == tuple(scales)
    assert f['rois'] is rois and f['roi_level'] is level and tuple(f['pooled']) == (7, 7) and f['sampling_ratio'] == 3
    assert f['aligned'] is False and f['channels_last_out'] is True
    if want_backward:
        b = calls[1][1]
        assert _logical_grad(b['grad_out'], rois) and b['rois'] is rois and b['roi_level'] is level
        assert [tuple(s) for s in b['level_shapes']] == [tuple(m.shape) for m in maps] and tuple(b['scales']) == tuple(scales)
        assert b['sampling_ratio'] == 3 and b['aligned'] is False and b['channels_last'] is True


def test_deformable_psroi_two_pass(monkeypatch):
    calls, maps, rois, level, cfg, scales = _run(monkeypatch, dict(dcn=True, dcn_sample_per_part=3, dcn_trans_std=0.2), 1)
    assert [n for n, _ in calls] == ['deformable_psroi_pool', 'offset_fc', 'deformable_psroi_pool',
                                     'deformable_psroi_pool_bwd', 'offset_fc_bwd', 'deformable_psroi_pool_bwd']
    p0, fc, p1, b1, fcb, b0 = [a for _, a in calls]
    for g in (p0, p1, b1, b0):
        assert g['data'] is maps[0] and g['rois'] is rois and g['spatial_scale'] == 1.0 / 16 and g['output_dim'] == C
        assert (g['group_size'], g['pooled_size'], g['part_size'], g['sample_per_part']) == (1, 7, 7, 3)
    for g in (p0, b0):          # the pass without offsets
        assert g['trans'] is None and g['no_trans'] is True and g['trans_std'] == 0.0
    for g in (p1, b1):          # the pass with them
        assert tuple(g['trans'].shape) == (R, 2, 7, 7) and g['no_trans'] is False and g['trans_std'] == 0.2
    assert p0['channels_last_out'] is True and p1['channels_last_out'] is True
    assert tuple(fc['t0f'].shape) == (R, 49 * C) and fc['t0f'].is_contiguous()
    assert fcb['t0f'] is fc['t0f'] and tuple(fcb['g_trans'].shape) == (R, 2 * 49) and fcb['g_trans'].dtype == torch.float32
    assert _logical_grad(b1['grad_out'], rois) and _logical_grad(b0['grad_out'], rois)


def test_combinations_without_a_kernel_are_refused():
    detector, ops, pooling = _mods()
    c4 = (1.0 / 16,)
    with pytest.raises(ValueError, match='roi_align'):
        pooling.RoiPooling(_cfg(detector, dcn=True, roi_align=True), c4)
    with pytest.raises(AssertionError):
        pooling.RoiPooling(_cfg(detector, dcn=True), FPN_SCALES)
    with pytest.raises(AssertionError):
        pooling.RoiPooling(_cfg(detector), FPN_SCALES, deterministic=True)
    with pytest.raises(AssertionError):
        pooling.RoiPooling(_cfg(detector, roi_align=True), c4, deterministic=True)
    with pytest.raises(AssertionError):
        pooling.RoiPooling(_cfg(detector, dcn=True), c4, deterministic=True)
    assert detector.check_pooling is pooling.check_pooling
