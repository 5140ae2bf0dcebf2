"""CPU checks of the deterministic training mode (no GPU): the float32 restatements of tests/deterministic_cases.py against float64, the
assertion that ORDER MATTERS on exactly the inputs the GPU tests use (otherwise their bit-for-bit checks would pass for any order), the
configuration surface (TrainConfig.deterministic, the refusals) and the declaration / binding of the new entry points."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deterministic_cases as DC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synthetic_argmax(rng, R, C, H, W):
    """An argmax map with the structure the forward produces for DC.roi_case_rois (host stand-in: the GPU test takes the real one): whole-map
    rois spread over all cells, sub-cell rois on one cell, corner rois mostly -1."""
    P = DC.ROI_P
    arg = rng.integers(0, H * W, (R, C, P, P)).astype(np.int32)
    for r, cell in ((2, 1 * W + 1), (3, 2 * W + 3), (4, 4 * W + 6), (5, 1 * W + 1)):
        arg[r] = cell
    for r, cell, (ph, pw) in ((6, 0, (6, 6)), (7, 5 * W + 7, (0, 0))):
        arg[r] = -1
        arg[r, :, ph, pw] = cell
    arg[9] = arg[8]; arg[10] = arg[8]
    return arg


@pytest.mark.parametrize('case', DC.ROI_CASES, ids=[c[0] for c in DC.ROI_CASES])
def test_roi_pool_restatement_matches_float64_and_depends_on_the_order(case):
    id_, C, bf16, base, image1 = case
    rng = np.random.default_rng(DC.seed('roi-' + id_))
    rois = DC.roi_case_rois(base, image1)
    assert rois.shape == (DC.ROI_R, 5) and ((rois[:, 0] - base == 1).all() if image1 else set(rois[:, 0] - base) == {0, 1})
    assert (rois[8] == rois[9]).all() and (rois[9] == rois[10]).all()
    g = DC.order_sensitive(rng, (DC.ROI_R, C, DC.ROI_P, DC.ROI_P), bf16)
    arg = _synthetic_argmax(rng, DC.ROI_R, C, DC.ROI_H, DC.ROI_W)
    img = (rois[:, 0] - base).astype(np.int64)
    fwd, cnt, s64, a64 = DC.roi_pool_bwd_ordered_ref(g, arg, img, DC.ROI_B, DC.ROI_H, DC.ROI_W, stats=True)
    assert (np.abs(fwd.astype(np.float64) - s64) <= DC.sum_bound(a64, cnt)).all()
    assert int(cnt.max()) >= 49 and int((arg < 0).sum()) > 0
    if image1:
        assert not fwd[0].any() and not cnt[0].any()
    rev = DC.roi_pool_bwd_ordered_ref(g, arg, img, DC.ROI_B, DC.ROI_H, DC.ROI_W, reverse=True)
    assert (np.abs(rev.astype(np.float64) - s64) <= DC.sum_bound(a64, cnt)).all()
    assert (rev.view(np.uint32) != fwd.view(np.uint32)).any(), "the reversed order gives the same bits: these inputs cannot tell orders apart"


@pytest.mark.parametrize('case', DC.COLSUM_CASES, ids=[c[0] for c in DC.COLSUM_CASES])
def test_colsum_restatement_matches_float64_and_depends_on_the_order(case):
    id_, rows, cols, bf16 = case
    x, out0 = DC.colsum_case(id_, rows, cols, bf16)
    if bf16:
        assert not (x.view(np.uint32) & 0xffff).any()
    got = DC.colsum_ordered_ref(x, out0)
    want = out0.astype(np.float64) + x.astype(np.float64).sum(0)
    bound = DC.sum_bound(np.abs(out0).astype(np.float64) + np.abs(x).astype(np.float64).sum(0), rows + 1)
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    if rows > 64:       # (one row, or a handful: every order is the same sum)
        rev = DC.colsum_ordered_ref(x, out0, reverse=True)
        assert (rev.view(np.uint32) != got.view(np.uint32)).any()


def test_colsum_partition_depends_on_rows_only():
    assert DC.colsum_chunks(1) == (1, 1) and DC.colsum_chunks(512) == (1, 512) and DC.colsum_chunks(513) == (2, 257)
    assert DC.colsum_chunks(4100) == (9, 456) and DC.colsum_chunks(10 ** 6)[0] == 128
    assert len(DC.COLSUM_GROUP_ROWS) == len(DC.COLSUM_GROUP_COLS) == 17 and all(c % 8 == 0 for c in DC.COLSUM_GROUP_COLS)


@pytest.mark.parametrize('n', DC.SCALAR_NS)
def test_scalar_restatement_matches_float64(n):
    x = DC.scalar_case(n)
    got = float(DC.reduce_scalar_ordered_ref(x, DC.SCALAR_SCALE, 0))
    want = DC.SCALAR_SCALE * float(x.astype(np.float64).sum())
    assert abs(got - want) <= DC.sum_bound(DC.SCALAR_SCALE * np.abs(x).astype(np.float64).sum(), n)
    assert float(DC.reduce_scalar_ordered_ref(x, 1.0, 1)) == float((x >= 0).sum())


def test_take_restatement_matches_float64_and_depends_on_the_order():
    # (float32 values: five bf16 terms within 2^-8 .. 2^9 add exactly in float32 in any order, so only the float32 case can tell orders apart)
    d_x, rank = DC.take_case(bf16=False)
    hits = np.bincount(rank.reshape(-1), minlength=DC.TAKE_N)
    assert hits.max() >= 2 and (hits == 0).any() and rank.shape == (DC.TAKE_B, DC.TAKE_C, DC.TAKE_F)
    for c in range(DC.TAKE_C):
        assert len(set(rank[0, c])) == DC.TAKE_F                    # distinct within one (image, class)
    got = DC.take_bwd_ordered_ref(d_x, rank, DC.TAKE_N)
    want = np.zeros((DC.TAKE_N, 128)); mag = np.zeros((DC.TAKE_N, 128))
    for c in range(DC.TAKE_C):
        for f in range(DC.TAKE_F):
            want[rank[0, c, f]] += d_x[0, c, f]; mag[rank[0, c, f]] += np.abs(d_x[0, c, f])
    assert (np.abs(got - want) <= DC.sum_bound(mag, hits[:, None])).all() and not got[hits == 0].any()
    rev = DC.take_bwd_ordered_ref(d_x, rank, DC.TAKE_N, reverse=True)
    assert (rev.view(np.uint32) != got.view(np.uint32)).any()


def test_train_config_deterministic_defaults_to_false():
    import relnet_amd  # noqa: F401
    from relnet_amd import train
    assert train.TrainConfig.deterministic is False and train.TrainConfig().deterministic is False


@pytest.mark.parametrize('kind,names', [('dcn', ('deformable_psroi_pool_bwd', 'deformable_col2im')), ('roi_align', ('roi_align_bwd',)),
                                        ('fpn', ('roi_pool_fpn_bwd',))])
def test_deterministic_refuses_what_it_does_not_cover(kind, names):
    import relnet_amd  # noqa: F401
    from relnet_amd import train
    cfg = train.TrainConfig()
    cfg.deterministic = True
    if kind != 'fpn':
        setattr(cfg, kind, True)
    with pytest.raises(ValueError) as e:
        (train.FPNTrainer({}, cfg, device='cpu') if kind == 'fpn' else train.Trainer({}, cfg, device='cpu'))
    for n in names:
        assert n in str(e.value)


def test_new_symbols_are_declared_and_bound():
    import relnet_amd  # noqa: F401
    from relnet_amd import lib
    hdr = open(os.path.join(ROOT, 'include', 'relnet_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(relnet_\w+)\s*\(', hdr))
    for s in DC.NEW_SYMBOLS:
        assert s in declared and s in lib.exported_symbols(), s
