"""tests/deform_edge_cases.py checked on the host: the lattices hold every class they claim (coverage), every exact case is exact (float32 in two
summation orders equals float64 bit for bit; for the PSROI sums also the stronger statement that the sum of |terms| stays below 2^24 lattice units
wherever the GPU test asks for equality), every mutant of the restatements is seen, the restatements equal float64 autograd of
oracle/deform_torch.py where the operator is smooth, and they equal the reference's own kernels (tests/golden/ref_cuda_deform_edges.npz, written
on the MI355X by tests/golden/gen_golden_deform_edges.py) bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import deform_edge_cases as DE  # noqa: E402

IDS = [c[0] for c in DE.COL2IM_CASES]
GOLDEN = os.path.join(HERE, 'golden', 'ref_cuda_deform_edges.npz')
PS_ALL = DE.ps_configs()
PS_SMALL = DE.ps_configs(max_channels=72)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64))


@pytest.mark.parametrize('id_', IDS)
def test_col2im_lattice_covers_every_class(id_):
    c, _, off, _, _, _ = DE.col2im_reference(id_)
    rep = DE.classify(c, off)
    assert DE.coverage_gaps(c, rep) == []
    assert np.array_equal(off * 8, np.round(off * 8))
    if c.gather:        # every window radius the GPU test runs splits the pairs into a non-empty near and far set
        assert all(rep['near'][D] > 0 and rep['far'][D] > 0 for D in DE.WINDOWS)


@pytest.mark.parametrize('id_', IDS)
def test_col2im_case_is_exact(id_):
    c, data, off, dcol, gd, go = DE.col2im_reference(id_)
    assert np.abs(data).min() >= 1 and np.abs(data).max() <= 8 and np.abs(dcol).min() >= 1 and np.abs(dcol).max() <= 4
    assert _same(torch.as_tensor(data).bfloat16().float().numpy(), data) and _same(torch.as_tensor(dcol).bfloat16().float().numpy(), dcol)
    for reverse in (False, True):
        gd32, go32 = DE.col2im_restate(c, data, off, dcol, dtype=np.float32, reverse=reverse)
        assert gd32.dtype == np.float32 and go32.dtype == np.float32
        assert _same(gd32, gd) and _same(go32, go)
    assert np.abs(gd).max() > 0 and np.abs(go).max() > 0
    for D in DE.WINDOWS:                                   # every pair is in exactly one of the two passes, whatever the radius
        assert _same(DE.col2im_restate(c, data, off, dcol, win=D)[0], gd)


@pytest.mark.parametrize('mutant', DE.MUTANTS)
def test_col2im_mutant_is_seen(mutant):
    seen = []
    for id_ in IDS:
        c, data, off, dcol, gd, go = DE.col2im_reference(id_)
        if (mutant == 'wrong_group' and c.dg == 1) or (mutant.startswith('near') and not c.gather):
            continue                                       # (one group / a case the gather form refuses: nothing to get wrong)
        wins = DE.WINDOWS if mutant.startswith('near') else (None,)
        for D in wins:
            a, b = DE.col2im_restate(c, data, off, dcol, mutant=mutant, win=D)
            seen.append((id_, D, not (_same(a, gd) and _same(b, go))))
    assert seen and any(s for _, _, s in seen)
    if mutant != 'trunc':          # (truncation needs an inside sample left of / above its pixel's window origin: the 3 x 4 map may hold none)
        assert all(s for _, _, s in seen), [x for x in seen if not x[2]]              # on every case (and radius) that can show it


@pytest.mark.parametrize('id_', IDS)
def test_col2im_restatement_equals_autograd_on_the_smooth_subset(id_):
    from oracle import deform_torch as DT
    c = DE.case(id_)
    data, off, dcol = DE.build_operands(c, smooth=True)
    g = DE.geometry(c, off)
    for p in (g['py'], g['px']):                           # no sample on an integer
        assert not (p == np.floor(p)).any()
    gd, go = DE.col2im_restate(c, data, off, dcol)
    kk = (DE.K, DE.K)
    for b in range(c.B):
        td = torch.tensor(data[b], dtype=torch.float64, requires_grad=True)
        to = torch.tensor(off[b], dtype=torch.float64, requires_grad=True)
        col = DT.deformable_im2col(td, to, kk, (c.pad, c.pad), (c.stride, c.stride), (c.dil, c.dil), c.dg)
        (col * torch.as_tensor(DE.dcol_to_reference(c, dcol, b)).double()).sum().backward()
        assert np.abs(gd[b] - td.grad.numpy()).max() <= 1e-12
        assert np.abs(go[b] - to.grad.numpy()).max() <= 1e-12
    assert np.abs(go).max() > 0


def _golden():
    assert os.path.exists(GOLDEN), 'tests/golden/ref_cuda_deform_edges.npz is missing'
    return np.load(GOLDEN)


@pytest.mark.parametrize('id_', DE.GOLDEN_CASES)
def test_col2im_restatement_equals_reference_kernels(id_):
    Z = _golden()
    c, data, off, dcol, gd, go = DE.col2im_reference(id_)
    assert int(Z['col2im_%s_inputs' % id_]) == int(DE.checksum(data, off, dcol))
    assert _same(Z['col2im_%s_grad_data' % id_], gd)
    assert _same(Z['col2im_%s_grad_offset' % id_], go)


# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spp', DE.PS_SPP)
def test_psroi_samples_cover_every_class(spp):
    for with_trans in (False, True):
        w, h = set(), set()
        for cfg in PS_SMALL:
            if cfg.spp == spp and cfg.with_trans == with_trans:
                r = DE.ps_reference(cfg)[-1]
                w |= r['classes']['w']; h |= r['classes']['h']
                cnt = r['count']
                assert (cnt == 0).any() and (cnt == spp * spp).any() and (spp == 1 or ((cnt > 0) & (cnt < spp * spp)).any())
                assert (cnt[len(DE.PS_ROI_CLASSES) - 1] == 0).all()                # the roi entirely outside
        assert w == set(DE.PS_SAMPLE_CLASSES) and h == set(DE.PS_SAMPLE_CLASSES), (spp, with_trans, w, h)


@pytest.mark.parametrize('cfg', PS_ALL, ids=repr)
def test_psroi_case_is_exact(cfg):
    data, rois, trans, mult, r = DE.ps_reference(cfg)
    assert r['lattice'] >= 2.0 ** -6
    gout = DE.ps_grad_out(r['count'], mult)
    assert _same(torch.as_tensor(gout).bfloat16().float().numpy(), gout)
    ud, ut = DE.ps_exact_units(cfg, r)
    for reverse in (False, True):
        q = DE.psroi_restate(cfg, data, rois, trans, mult, dtype=np.float32, reverse=reverse)
        assert _same(q['grad_data'], r['grad_data']) and _same(q['top'], r['top'])
        if trans is not None:
            exact = ut < 2.0 ** 24
            assert np.array_equal(q['grad_trans'].astype(np.float64)[exact], r['grad_trans'][exact])
            n = (cfg.od // cfg.ncls) * cfg.spp ** 2            # the bounded set: n exact terms, n - 1 rounded additions
            assert (np.abs(q['grad_trans'] - r['grad_trans']) <= n * DE.U * r['abs_trans'])[~exact].all()
    assert ud.max() < 2.0 ** 24                           # the data gradient is exact in EVERY order
    if ut is not None:
        # the trans gradient adds od / classes * spp^2 terms per address: exact in every order for the 8-channel shapes up to 4 x 4 samples; the
        # addresses beyond 2^24 units are the BOUNDED set of the GPU test (everything below stays held to equality, address by address)
        assert (ut < 2.0 ** 24).any() and ((ut < 2.0 ** 24).all() or cfg.od > 8 or cfg.spp > 4)
    assert np.abs(r['grad_data']).max() > 0 and (trans is None or np.abs(r['grad_trans']).max() > 0)


@pytest.mark.parametrize('mutant', DE.PS_MUTANTS)
def test_psroi_mutant_is_seen(mutant):
    seen = []
    for cfg in PS_SMALL:
        if (mutant == 'spp_cap4' and cfg.spp <= 4) or (mutant in ('floor_plus1', 'trans_onesided') and not cfg.with_trans):
            continue
        data, rois, trans, mult, r = DE.ps_reference(cfg)
        q = DE.psroi_restate(cfg, data, rois, trans, mult, mutant=mutant)
        same = all(_same(q[k], r[k]) for k in ('top', 'count', 'grad_data')) and (trans is None or _same(q['grad_trans'], r['grad_trans']))
        seen.append((cfg.id, not same))
    assert seen and all(s for _, s in seen), [x for x in seen if not x[1]]


@pytest.mark.parametrize('cfg', PS_SMALL, ids=repr)
def test_psroi_restatement_equals_autograd_in_the_data(cfg):
    """The pooled value is linear in the data, so its data gradient is smooth everywhere: autograd of the restated forward must give it on
    every class.  (The trans gradient is one-sided at integer samples: those are pinned by the reference's kernels below, not by autograd.)"""
    from oracle import deform_torch as DT
    data, rois, trans, mult, r = DE.ps_reference(cfg)
    td = torch.tensor(data, dtype=torch.float64, requires_grad=True)
    tt = None if trans is None else torch.tensor(trans, dtype=torch.float64)
    y = DT.deformable_psroi_pooling(td, rois, tt, DE.PS_SCALE, cfg.od, cfg.group, cfg.P, cfg.part, cfg.spp, DE.PS_TRANS_STD, trans is None)
    assert np.abs(y.detach().numpy() - r['top']).max() <= 2.0 ** -24 * max(1.0, np.abs(r['top']).max())       # (top is rounded to float32 once)
    (y * torch.as_tensor(DE.ps_grad_out(r['count'], mult)).double()).sum().backward()
    assert np.abs(td.grad.numpy() - r['grad_data']).max() <= 1e-12


@pytest.mark.parametrize('cfg', DE.ps_configs(max_channels=128), ids=repr)
def test_psroi_restatement_equals_reference_kernels(cfg):
    Z = _golden()
    data, rois, trans, mult, r = DE.ps_reference(cfg)
    k = 'psroi_%s_' % cfg.id
    assert int(Z[k + 'inputs']) == int(DE.checksum(data, rois, mult, *([] if trans is None else [trans])))
    ch = DE.GOLDEN_TOP_CHANNELS[cfg.od]
    assert _same(Z[k + 'top'], r['top'][:, ch]) and _same(Z[k + 'count'], r['count'][:, ch])
    assert _same(Z[k + 'grad_data'], r['grad_data'][:, DE.golden_data_channels(cfg)])
    if trans is not None:
        ud, ut = DE.ps_exact_units(cfg, r)
        exact = ut < 2.0 ** 24
        got, want = Z[k + 'grad_trans'].astype(np.float64), r['grad_trans']
        assert np.array_equal(got[exact], want[exact])
        assert (got[~exact] == 0).all()           # (not exact under atomics, so not stored: the file regenerates bit for bit)


@pytest.mark.parametrize('k', range(len(DE.PS_DEGENERATE_CFGS)))
def test_psroi_bounded_set_is_what_its_bounds_assume(k):
    """The degenerate rois: extent floored to 0.1, every sample valid, inside (1, 3) and at least 0.2 away from an integer (the premises of
    ps_bound_k); the restatement accumulated in float32, in either order, uses a small part of each bound."""
    cfg, data, rois, trans, mult, r = DE.ps_degenerate(k)
    assert (rois[:, 3] < rois[:, 1]).all() and (rois[:, 4] < rois[:, 2]).all()
    assert (r['count'] == cfg.spp ** 2).all()
    assert trans is None or np.abs(trans).max() <= 8
    for n in range(len(rois)):
        for start in (np.floor(rois[n, 1] + 0.5) / 16 - 0.5, np.floor(rois[n, 2] + 0.5) / 16 - 0.5):
            lo, hi = start - 0.1, start + 0.2                       # shift in [-0.1, 0.1], bins and sub-bins in [0, 0.1)
            assert 1 < lo and hi < 3 and np.floor(lo - 0.2) == np.floor(hi + 0.2)
    K = DE.ps_bound_k(cfg)
    for reverse in (False, True):
        q = DE.psroi_restate(cfg, data, rois, trans, mult, dtype=np.float32, reverse=reverse, bounds=True)
        assert DE.worst(q['grad_data'], r['grad_data'], K['grad_data'] * DE.U * r['mag_data']) <= 0.5
        if trans is not None:
            assert DE.worst(q['grad_trans'], r['grad_trans'], K['grad_trans'] * DE.U * r['mag_trans']) <= 0.5
    assert (r['mag_top'] > 0).all() and (r['mag_data'] > 0).any()
