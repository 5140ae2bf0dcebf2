"""CPU tests of tests/psroi_cases.py (the restatement every GPU comparison of PSROIPooling leans on) and of the layers around the kernels
that need no GPU: the operator_cxx mirror's protocol, the mx.contrib.sym node, the header and the ctypes table."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psroi_cases as PC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def _fwd(data, rois, scale, od, P, g=0, dtype=F32, **kw):
    return PC.psroi_restate(np.asarray(data, F32), np.asarray(rois, F32), scale, od, P, g, dtype=dtype, **kw)


# ---- known answers, worked by hand ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F32, F64])
def test_constant_map_pools_to_the_constant(dtype):
    # 3 output channels x 2 x 2 groups on a 6 x 8 map of 3.25s: every non-empty bin averages to 3.25 exactly, whatever its size
    data = np.full((1, 12, 6, 8), 3.25, F32)
    rois = [[0, 0, 0, 15, 11], [0, 3, 2, 9, 7], [0, -6, -4, 5, 5]]
    r = _fwd(data, rois, 0.5, 3, 2, dtype=dtype)
    assert r['out'].dtype == dtype and np.all(r['n'][:2] > 0) and np.all(r['out'][:2] == 3.25)
    # the third roi: x from -3 in bins of 3 cells, [-3, 0) is clipped to nothing and gives 0; y from -2 in bins of 2.5: [-2, 1) -> row 0, [0, 3)
    assert np.array_equal(r['n'][2, 0], [[0, 3], [0, 9]]) and np.array_equal(r['out'][2, 0], np.array([[0, 3.25], [0, 3.25]], dtype))


def test_one_hot_pixel_gives_one_over_area_in_exactly_the_bins_that_hold_it():
    data = np.zeros((1, 1, 4, 4), F32)
    data[0, 0, 1, 2] = 1.0
    # roi (0,0)-(3,3), scale 1: start 0, end 4, P = 2 -> bin 2: bins [0,2) and [2,4) per axis, 4 cells each.  (y 1, x 2) is in bin (0, 1)
    r = _fwd(data, [[0, 0, 0, 3, 3]], 1.0, 1, 2, g=1)
    assert np.array_equal(r['out'][0, 0], np.array([[0, 0.25], [0, 0]], F32))
    # roi (0,0)-(2,2): end 3, bin 1.5: bins [0, ceil 1.5 = 2) and [floor 1.5 = 1, 3) SHARE cell 1; a one at (1, 1) is in all four, area 4
    data2 = np.zeros((1, 1, 4, 4), F32)
    data2[0, 0, 1, 1] = 1.0
    r = _fwd(data2, [[0, 0, 0, 2, 2]], 1.0, 1, 2, g=1)
    assert np.array_equal(r['out'][0, 0], np.full((2, 2), 0.25, F32))
    # ... and its backward sends all four bins' gradients to that cell: (1 + 2 + 3 + 4) / 4 at (1, 1); (0, 0) is in bin (0, 0) only
    go = np.array([[[[1, 2], [3, 4]]]], F32)
    b = PC.psroi_restate(data2, np.array([[0, 0, 0, 2, 2]], F32), 1.0, 1, 2, 1, grad_out=go)
    assert b['grad_in'][0, 0, 1, 1] == 2.5 and b['n_add'][0, 0, 1, 1] == 4
    assert b['grad_in'][0, 0, 0, 0] == 0.25 and b['grad_in'][0, 0, 2, 2] == 1.0 and b['grad_in'][0, 0, 0, 2] == 0.5
    assert np.all(b['grad_in'][0, 0, 3, :] == 0) and np.all(b['grad_in'][0, 0, :, 3] == 0)


def test_position_sensitivity_and_mapping_channel():
    # output_dim 2, P = g = 2: bin (ph, pw) of output channel ctop reads input channel (ctop * 2 + ph) * 2 + pw; channel k holds k
    data = np.arange(8, dtype=F32).reshape(1, 8, 1, 1) * np.ones((1, 8, 4, 4), F32)
    r = _fwd(data, [[0, 0, 0, 3, 3]], 1.0, 2, 2)
    want = np.arange(8, dtype=F32).reshape(1, 2, 2, 2)
    assert np.array_equal(r['out'], want) and np.array_equal(r['mapping'], want)
    # P = 4 > g = 2: bins 0, 1 -> group 0, bins 2, 3 -> group 1; P = 2 < g = 4: bins 0, 1 -> groups 0, 2 (1 and 3 go unused)
    assert list(PC.groups(4, 2)) == [0, 0, 1, 1] and list(PC.groups(2, 4)) == [0, 2] and list(PC.groups(7, 3)) == [0, 0, 0, 1, 1, 2, 2]


def test_roi_off_the_map_and_bad_batch_index_give_zeros():
    data = np.ones((2, 1, 4, 4), F32)
    rois = [[0, 40, 40, 50, 50], [0, -50, -50, -40, -40], [-1, 0, 0, 3, 3], [2, 0, 0, 3, 3], [1, 0, 0, 3, 3]]
    go = np.ones((5, 1, 2, 2), F32)
    r = PC.psroi_restate(data, np.array(rois, F32), 1.0, 1, 2, 1, grad_out=go)
    assert np.all(r['out'][:4] == 0) and np.all(r['n'][:4] == 0) and np.all(r['out'][4] == 1)
    assert np.all(r['grad_in'][0] == 0) and np.all(r['grad_in'][1] == 0.25)
    # batch_index_base shifts the test: index 2 is image 1 with base 1, index 0 falls out
    r = PC.psroi_restate(data, np.array(rois, F32), 1.0, 1, 2, 1, batch_index_base=1)
    assert np.all(r['out'][3] == 1) and np.all(r['out'][0] == 0)


def test_the_tenth_of_a_cell_clamp():
    # x2 < x1: start 3, end (1 + 1) = 2, width max(-1, 0.1) = 0.1; P = 1: [floor 3, ceil 3.1) = cell 3 alone, on both axes
    data = np.arange(16, dtype=F32).reshape(1, 1, 4, 4)
    r = _fwd(data, [[0, 3, 3, 1, 1]], 1.0, 1, 1)
    assert r['out'][0, 0, 0, 0] == 15.0 and r['n'][0, 0, 0, 0] == 1
    hs, he, ws, we = PC.edges(np.array([0, 3, 3, 1, 1], F32), 1.0, 1, 4, 4)
    assert (hs[0], he[0], ws[0], we[0]) == (3, 4, 3, 4)


def test_round_goes_half_away_from_zero():
    assert PC.c_round(F32(2.5)) == 3 and PC.c_round(F32(-0.5)) == -1 and PC.c_round(F32(0.5)) == 1 and PC.c_round(F32(-2.5)) == -3
    assert PC.c_round(F32(0.49999997)) == 0 and PC.c_round(F32(1.5)) == 2          # (rint gives 2, 0, 0, -2, 0, 2)
    data = np.arange(8, dtype=F32).reshape(1, 1, 1, 8)
    # x1 = 2.5 -> 3 (rint: 2), x2 = 4.5 -> 5 (rint: 4): cells 3, 4, 5 -> mean 4
    assert _fwd(data, [[0, 2.5, 0, 4.5, 0]], 1.0, 1, 1)['out'][0, 0, 0, 0] == 4.0
    # x1 = x2 = -0.5 -> -1: start -1, end 0 -> clipped to nothing -> 0 (rint: -0 -> cell 0 -> data 0 too, so look at the count)
    assert _fwd(data + 1, [[0, -0.5, 0, -0.5, 0]], 1.0, 1, 1)['n'][0, 0, 0, 0] == 0


# ---- the restatement against itself ------------------------------------------------------------------------------------------------
def _torch_forward(x, c):
    """The forward as differentiable float64 torch expressions over the restatement's own float32 edges."""
    P, g, od = c['P'], c['P'] if c['g'] == 0 else c['g'], c['output_dim']
    grp = PC.groups(P, g)
    rows = []
    for r in range(c['R']):
        b = int(c['rois'][r, 0])
        out = torch.zeros(od, P, P, dtype=torch.float64)
        if 0 <= b < c['B']:
            hs, he, ws, we = PC.edges(c['rois'][r], c['scale'], P, c['H'], c['W'])
            for ct in range(od):
                for ph in range(P):
                    for pw in range(P):
                        if he[ph] > hs[ph] and we[pw] > ws[pw]:
                            ch = (ct * g + grp[ph]) * g + grp[pw]
                            out[ct, ph, pw] = x[b, ch, hs[ph]:he[ph], ws[pw]:we[pw]].mean()
        rows.append(out)
    return torch.stack(rows) if rows else torch.zeros(0, od, P, P, dtype=torch.float64)


HOST_CASES = ['p3g3_5x7_r65', 'p7g1_9x6_r65', 'p3g7_5x7_r5', 'p7g3_9x6_r65', 'p7g0_5x7_r65', 'exact_p3g3_9x6_r5']


@pytest.mark.parametrize('name', HOST_CASES)
def test_backward_restatement_is_the_autograd_of_the_forward(name):
    c = PC.case(name)
    x = torch.tensor(c['data'], dtype=torch.float64, requires_grad=True)
    y = _torch_forward(x, c)
    assert float((y.detach() - torch.as_tensor(c['ref64']['out'])).abs().max()) <= 1e-12
    (y * torch.as_tensor(c['grad_out']).double()).sum().backward()
    assert float((x.grad - torch.as_tensor(c['ref64']['grad_in'])).abs().max()) <= 1e-12
    # kAddTo: the prior value plus that
    assert np.abs(c['ref64_acc']['grad_in'] - (c['grad_in0'].astype(F64) + c['ref64']['grad_in'])).max() <= 1e-12


@pytest.mark.parametrize('name', HOST_CASES)
def test_adjoint_identity(name):
    c = PC.case(name)
    lhs = float((c['ref64']['out'] * c['grad_out'].astype(F64)).sum())
    rhs = float((c['data'].astype(F64) * c['ref64']['grad_in']).sum())
    scale = float((np.abs(c['ref64']['out']) * np.abs(c['grad_out'])).sum()) + 1.0
    assert abs(lhs - rhs) <= 1e-12 * scale


@pytest.mark.parametrize('name', PC.CASE_NAMES)
def test_float32_form_stays_inside_the_derived_bounds_of_the_float64_form(name):
    """The documented order is one of the orders the bounds cover, so the float32 form must satisfy them."""
    c = PC.case(name)
    assert np.all(np.abs(c['ref32']['out'].astype(F64) - c['ref64']['out']) <= PC.fwd_bound(c['ref64']))
    assert np.all(np.abs(c['ref32']['grad_in'].astype(F64) - c['ref64']['grad_in']) <= PC.bwd_bound(c['ref64']))
    assert np.all(np.abs(c['ref32_acc']['grad_in'].astype(F64) - c['ref64_acc']['grad_in']) <= PC.bwd_bound(c['ref64_acc']))
    assert np.array_equal(c['ref32']['mapping'], c['ref64']['mapping']) and np.array_equal(c['ref32']['n'], c['ref64']['n'])


def test_case_table_covers_the_grid():
    t = PC.CASE_TABLE
    assert {c[1] for c in t} >= {1, 3} and max(c[1] * (c[3] or c[2]) ** 2 for c in t) > 256          # and one case past 256 channels
    assert {(c[2], c[2] if c[3] == 0 else c[3]) for c in t} == {(1, 1), (3, 3), (7, 7), (7, 1), (3, 7), (7, 3)}
    assert {(c[4], c[5]) for c in t} == {(1, 1), (5, 7), (9, 6)} and {c[6] for c in t} == {0, 1, 5, 65}
    c = PC.case('p3g3_5x7_r65')
    b = c['rois'][:, 0]
    assert -1 in b and c['B'] in b and 0 in b and c['B'] - 1 in b                      # both images, both bad indices
    assert np.any(c['rois'][:, 3] < c['rois'][:, 1])                                   # degenerate
    assert np.any(c['rois'][:, 1:] % 1 == 0.5)                                         # halves
    assert np.any(c['ref64']['n_add'] > 3)                                             # rois share pixels
    assert np.any(np.all(c['ref64']['n'] == 0, axis=(1, 2, 3)))                        # a roi wholly off the map (or a bad index)
    # P < g: unused channels exist and get exact zeros backward
    c = PC.case('p3g7_5x7_r5')
    used = np.unique(c['ref32']['mapping']).astype(int)
    unused = np.setdiff1d(np.arange(c['C']), used)
    assert len(unused) == 49 - 9 and np.all(c['ref32']['grad_in'][:, unused] == 0) and np.any(c['ref32']['grad_in'][:, used] != 0)
    # P > g: several bins of one roi feed one channel
    c = PC.case('p7g1_9x6_r65')
    assert np.all(c['ref32']['mapping'][:, 0] == 0) and c['ref64']['n_add'].max() > 49


def test_exact_cases_are_contraction_independent():
    """A case that claims exact geometry: the float32, the fused multiply-add and the float64 evaluation of every bin edge agree.  (And
    the claim is not vacuous: some other case does have an edge that moves.)"""
    moved = 0
    for name in PC.CASE_NAMES:
        c = PC.case(name)
        for roi in c['rois']:
            e = [PC.edges(roi, c['scale'], c['P'], c['H'] + 1000, c['W'] + 1000, mode=m) for m in ('f32', 'fma', 'f64')]
            same = all(np.array_equal(a, b) for k in (1, 2) for a, b in zip(e[0], e[k]))
            if c['exact']:
                assert same, (name, roi)
            moved += not same
    assert moved > 0


# ---- operator protocol of the Python mirror ----------------------------------------------------------------------------------------
def test_operator_cxx_mirror_protocol():
    import relnet_amd  # noqa: F401
    from relnet_amd import operator_cxx as OC
    prop = OC.PSROIPoolingProp(spatial_scale=0.0625, output_dim=3, pooled_size=7)
    assert prop.param_.group_size == 7                                                 # group_size 0 = pooled_size
    assert OC.PSROIPoolingProp(spatial_scale=0.0625, output_dim=3, pooled_size=7, group_size=3).param_.group_size == 3
    assert prop.ListArguments() == ['data', 'rois'] and prop.ListOutputs() == ['output', 'mapping_channel']
    assert prop.NumOutputs() == 2 and prop.NumVisibleOutputs() == 1 and prop.TypeString() == '_contrib_PSROIPooling'
    ins, outs = prop.InferShape([(2, 147, 9, 6), (65, 5)])
    assert ins == [(2, 147, 9, 6), (65, 5)] and outs == [(65, 3, 7, 7)] * 2
    assert prop.InferShape([(2, 147, 9, 6), (0, 5)])[1] == [(0, 3, 7, 7)] * 2
    assert prop.DeclareBackwardDependency(['g_out', 'g_map'], ['data', 'rois'], ['out', 'map']) == ['g_out', 'rois', 'map']
    assert prop.InferType(['float32', 'float32']) == (['float32', 'float32'], ['float32', 'float32'])
    assert isinstance(prop.CreateOperatorEx(), OC.PSROIPoolingOp)
    for bad, msg in (([(2, 147, 9), (65, 5)], '4D'), ([(2, 147, 9, 6), (65, 4)], r'\[batch, 5\]'), ([(2, 147, 9, 6), (65, 5, 1)], r'\[batch, 5\]'),
                     ([(2, 146, 9, 6), (65, 5)], 'channels'), ([(2, 147, 9, 6)], 'Input')):
        with pytest.raises(ValueError, match=msg):
            prop.InferShape(bad)
    with pytest.raises(ValueError):
        OC.PSROIPoolingProp(spatial_scale=1.5, output_dim=3, pooled_size=7)
    with pytest.raises(ValueError):
        prop.InferType(['float32', None])
    assert callable(OC.contrib.PSROIPooling)


def test_mx_contrib_sym_node_and_shape_inference():
    import relnet_amd  # noqa: F401
    from relnet_amd import mx
    data, rois = mx.sym.Variable('data'), mx.sym.Variable('rois')
    s = mx.contrib.sym.PSROIPooling(name='psroipooled', data=data, rois=rois, group_size=7, pooled_size=7, output_dim=3, spatial_scale=0.0625)
    node = s.heads[0][0]
    assert node.op == '_contrib_PSROIPooling' and node.name == 'psroipooled'
    assert set(node.attrs) >= {'group_size', 'pooled_size', 'output_dim', 'spatial_scale'}
    assert s.list_arguments() == ['data', 'rois']
    assert s.infer_shape(data=(2, 147, 38, 63), rois=(300, 5))[1] == [(300, 3, 7, 7)]
    auto = mx.contrib.sym.PSROIPooling(data=data, rois=rois, pooled_size=3, output_dim=2, spatial_scale=0.5)
    assert auto.heads[0][0].name.startswith('psroipooling') and auto.infer_shape(data=(1, 18, 4, 4), rois=(5, 5))[1] == [(5, 2, 3, 3)]


def test_entry_points_refuse_bad_arguments_before_touching_the_device():
    """RELNET_REQUIRE comes before any launch, so the refusals can be seen without a GPU (the pointers are never dereferenced)."""
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    import relnet_amd  # noqa: F401
    from relnet_amd import lib
    L = lib.load()
    s4 = (ctypes.c_long * 4)(1, 1, 1, 1)
    fwd = dict(data=64, ds=s4, rois=64, out=64, os=s4, mapping=0, R=5, B=2, C=27, H=5, W=7, od=3, P=3, g=3, scale=0.3, base=0, dtype=0, stream=0)
    bwd = dict(go=64, os=s4, rois=64, gin=64, gs=s4, R=5, B=2, C=27, H=5, W=7, od=3, P=3, g=3, scale=0.3, base=0, acc=0, dtype=0, stream=0)
    shared = [(dict(C=28), b'28 channels != output_dim 3 * group_size 3^2'), (dict(od=2), b'channels'), (dict(g=2), b'channels'),
              (dict(P=0), b'must be positive'), (dict(g=0), b'must be positive'), (dict(od=0), b'must be positive'), (dict(dtype=2), b'dtype'),
              (dict(rois=0), b'null operand'), (dict(os=None), b'null operand'), (dict(B=0), b'bad shape'), (dict(W=0), b'bad shape'),
              (dict(R=-1), b'bad shape')]
    for name, ok, own in (('relnet_psroi_pool_fwd', fwd, [dict(data=0), dict(out=0), dict(ds=None)]),
                          ('relnet_psroi_pool_bwd', bwd, [dict(go=0), dict(gin=0), dict(gs=None)])):
        for patch, msg in shared + [(p, b'null operand') for p in own]:
            assert getattr(L, name)(*dict(ok, **patch).values()) == -1, (name, patch)
            err = L.relnet_last_error()
            assert name.encode() in err and msg in err, (name, patch, err)
    # no rois: nothing to launch, nothing to dereference (the forward's operands may then be null)
    assert L.relnet_psroi_pool_fwd(*dict(fwd, R=0, data=0, rois=0, out=0).values()) == 0
    assert L.relnet_psroi_pool_bwd(*dict(bwd, R=0, go=0, rois=0, acc=1).values()) == 0


def test_new_symbols_are_declared_and_bound():
    import relnet_amd  # noqa: F401
    from relnet_amd import lib
    hdr = open(os.path.join(ROOT, 'include', 'relnet_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(relnet_\w+)\s*\(', hdr))
    for s in PC.NEW_SYMBOLS:
        assert s in declared and s in lib.exported_symbols(), s
    import __graft_entry__ as ge
    ge.build()
    lib.load()                                               # getattr on every bound name: a missing export fails here
    cxx = open(os.path.join(ROOT, 'include', 'relnet_operator_cxx.hpp')).read()
    for cls in ('struct PSROIPoolingParam', 'class PSROIPoolingProp', 'class PSROIPoolingOp'):
        assert cls in cxx, cls
