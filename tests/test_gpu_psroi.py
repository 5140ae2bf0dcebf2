"""PSROIPooling on the GPU (csrc/psroi_pool.hip through the C-ABI, ops.py, the operator_cxx mirror and the mx facade) against the
restatement of tests/psroi_cases.py: bit for bit against its float32 form in the documented summation order, and inside the derived
bounds of its float64 form; every element compared.  Shapes are the smallest at which the kernels can go wrong (psroi_cases.CASE_TABLE);
the references are computed once per case and shared."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psroi_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = np.float64
GUARD = 96          # NaN words on either side of every output


@pytest.fixture(scope='module')
def K():
    import __graft_entry__ as ge
    ge.build()
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib
    lib.load()
    return ops, lib


def _strides(t):
    return (ctypes.c_long * 4)(*[int(s) for s in t.stride()])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(shape, dtype, channels_last):
    """A NaN-filled buffer with GUARD NaN words on both sides of a logical [n, c, h, w] tensor (memory (n, h, w, c) when channels_last)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float('nan'), device='cuda', dtype=dtype)
    body = buf[GUARD:GUARD + n]
    if channels_last:
        t = body.view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)
    else:
        t = body.view(*shape)
    return buf, t


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _crop(a, dtype, channels_last):
    """`a` [n, c, h, w] as a non-dense view in the middle of a NaN tensor: a read outside the view poisons the result."""
    n, c, h, w = a.shape
    if channels_last:
        big = torch.full((n + 1, h + 3, w + 2, c + 3), float('nan'), device='cuda', dtype=dtype)
        v = big[:n, 2:2 + h, 1:1 + w, 1:1 + c].permute(0, 3, 1, 2)
    else:
        big = torch.full((n + 1, c + 2, h + 3, w + 2), float('nan'), device='cuda', dtype=dtype)
        v = big[:n, 1:1 + c, 2:2 + h, 1:1 + w]
    v.copy_(torch.as_tensor(a).to(dtype))
    assert n == 0 or (not v.is_contiguous() and not v.permute(0, 2, 3, 1).is_contiguous())
    return v


def _data(c, layout):
    x = torch.as_tensor(c['data']).cuda()
    if layout == 'nchw_f32':
        return x
    if layout == 'cl_f32':
        return x.contiguous(memory_format=torch.channels_last)
    if layout == 'cl_bf16':
        return x.bfloat16().contiguous(memory_format=torch.channels_last)       # the table's values are exact in bf16
    if layout == 'crop_nchw_f32':
        return _crop(c['data'], torch.float32, False)
    if layout == 'crop_cl_bf16':
        return _crop(c['data'], torch.bfloat16, True)
    raise KeyError(layout)


def _fwd_raw(lib, c, x, cl_out, want_mapping=True):
    """relnet_psroi_pool_fwd on guarded NaN outputs -> out, mapping (host float64 / float32 arrays), after the guard check."""
    shape = (c['R'], c['output_dim'], c['P'], c['P'])
    rois = torch.as_tensor(c['rois']).cuda()
    obuf, out = _guarded(shape, x.dtype, cl_out)
    mbuf, mapping = _guarded(shape, torch.float32, cl_out)
    g = c['P'] if c['g'] == 0 else c['g']
    lib.call('relnet_psroi_pool_fwd', x.data_ptr(), _strides(x), rois.data_ptr(), out.data_ptr(), _strides(out),
             mapping.data_ptr() if want_mapping else 0, c['R'], c['B'], c['C'], c['H'], c['W'], c['output_dim'], c['P'], g,
             float(c['scale']), 0, lib.BF16 if x.dtype == torch.bfloat16 else lib.F32, _stream())
    torch.cuda.synchronize()
    assert _guards_intact(obuf) and _guards_intact(mbuf)
    if not want_mapping:
        assert bool(torch.isnan(mbuf).all())
    return out, mapping


def _bits_equal(got, want32):
    """got: device tensor (fp32 or bf16); want32: the float32 restatement (rounded once to bf16 for a bf16 tensor)."""
    want = torch.as_tensor(want32)
    if got.dtype == torch.bfloat16:
        return torch.equal(got.cpu().view(torch.int16), want.bfloat16().view(torch.int16).reshape(got.shape))
    return torch.equal(got.cpu().view(torch.int32), want.view(torch.int32).reshape(got.shape))


LAYOUTS = ['nchw_f32', 'cl_f32', 'cl_bf16', 'crop_nchw_f32', 'crop_cl_bf16']


@pytest.mark.parametrize('cl_out', [False, True])
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('name', PC.CASE_NAMES)
def test_forward_is_the_restatement_bit_for_bit_and_inside_the_bound(K, name, layout, cl_out):
    ops, lib = K
    c = PC.case(name)
    x = _data(c, layout)
    out, mapping = _fwd_raw(lib, c, x, cl_out)
    assert out.shape == c['ref32']['out'].shape
    assert not bool(torch.isnan(out.float()).any()) and not bool(torch.isnan(mapping).any())          # every element written
    assert _bits_equal(out, c['ref32']['out'])
    assert torch.equal(mapping.cpu(), torch.as_tensor(c['ref32']['mapping']))
    err = np.abs(out.double().cpu().numpy() - c['ref64']['out'])
    assert np.all(err <= PC.fwd_bound(c['ref64'], bf16_out=x.dtype == torch.bfloat16))
    # the public entry: same bits, memory order as asked, mapping on request only
    rois = torch.as_tensor(c['rois']).cuda()
    got = ops.psroi_pool(x, rois, c['scale'], c['output_dim'], c['P'], c['g'], channels_last_out=cl_out)
    assert got.dtype == x.dtype and torch.equal(got, out)
    assert (got.permute(0, 2, 3, 1) if cl_out else got).is_contiguous()
    got2, map2 = ops.psroi_pool(x, rois, c['scale'], c['output_dim'], c['P'], c['g'], channels_last_out=cl_out, want_mapping=True)
    assert torch.equal(got2, out) and torch.equal(map2, mapping) and map2.stride() == got2.stride()


def test_forward_without_mapping_leaves_it_alone(K):
    ops, lib = K
    c = PC.case('p7g3_9x6_r65')
    out, _ = _fwd_raw(lib, c, _data(c, 'nchw_f32'), False, want_mapping=False)
    assert _bits_equal(out, c['ref32']['out'])


def _grad_out(c, dtype, form):
    """grad_out [R, OD, P, P]: 'nchw', 'cl' (memory (R, P, P, OD)) or 'crop' (non-dense view inside NaNs)."""
    if form == 'crop':
        return _crop(c['grad_out'], dtype, False)
    g = torch.as_tensor(c['grad_out']).cuda().to(dtype)
    return g.contiguous(memory_format=torch.channels_last) if form == 'cl' and c['R'] > 0 else g


def _bwd_raw(lib, c, go, gin_cl, accumulate):
    shape = (c['B'], c['C'], c['H'], c['W'])
    rois = torch.as_tensor(c['rois']).cuda()
    buf, gin = _guarded(shape, torch.float32, gin_cl)
    if accumulate:
        gin.copy_(torch.as_tensor(c['grad_in0']))
    g = c['P'] if c['g'] == 0 else c['g']
    lib.call('relnet_psroi_pool_bwd', go.data_ptr(), _strides(go), rois.data_ptr(), gin.data_ptr(), _strides(gin), c['R'], c['B'], c['C'],
             c['H'], c['W'], c['output_dim'], c['P'], g, float(c['scale']), 0, int(accumulate),
             lib.BF16 if go.dtype == torch.bfloat16 else lib.F32, _stream())
    torch.cuda.synchronize()
    assert _guards_intact(buf)
    return gin


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('go_form,go_dtype,gin_cl', [('nchw', torch.float32, False), ('cl', torch.float32, True), ('cl', torch.bfloat16, True),
                                                     ('nchw', torch.bfloat16, False), ('crop', torch.float32, True),
                                                     ('crop', torch.bfloat16, False)])
@pytest.mark.parametrize('name', PC.CASE_NAMES)
def test_backward_is_the_restatement_bit_for_bit_and_inside_the_bound(K, name, go_form, go_dtype, gin_cl, accumulate):
    ops, lib = K
    c = PC.case(name)
    go = _grad_out(c, go_dtype, go_form)                    # the table's gradients are exact in bf16
    gin = _bwd_raw(lib, c, go, gin_cl, accumulate)
    sfx = '_acc' if accumulate else ''
    assert not bool(torch.isnan(gin).any())                 # every word written: no zero fill was needed
    assert _bits_equal(gin, c['ref32' + sfx]['grad_in'])
    r64 = c['ref64' + sfx]
    assert np.all(np.abs(gin.double().cpu().numpy() - r64['grad_in']) <= PC.bwd_bound(r64))
    # the public entry
    rois = torch.as_tensor(c['rois']).cuda()
    shape = (c['B'], c['C'], c['H'], c['W'])
    if accumulate:
        prior = torch.as_tensor(c['grad_in0']).cuda()
        prior = prior.contiguous(memory_format=torch.channels_last) if gin_cl else prior
        got = ops.psroi_pool_bwd(go, rois, shape, c['scale'], c['output_dim'], c['P'], c['g'], accumulate_into=prior)
        assert got is prior
    else:
        got = ops.psroi_pool_bwd(go, rois, shape, c['scale'], c['output_dim'], c['P'], c['g'], channels_last=gin_cl)
        assert (got.permute(0, 2, 3, 1) if gin_cl else got).is_contiguous()
    assert got.dtype == torch.float32 and torch.equal(got, gin)


def test_backward_twice_and_under_graph_replay_gives_the_same_bits(K):
    ops, lib = K
    c = PC.case('p7g1_9x6_r65')                             # up to 49 bins of one roi feed one channel: the longest sums of the table
    rois = torch.as_tensor(c['rois']).cuda()
    go = torch.as_tensor(c['grad_out']).cuda()
    shape = (c['B'], c['C'], c['H'], c['W'])
    run = lambda: ops.psroi_pool_bwd(go, rois, shape, c['scale'], c['output_dim'], c['P'], c['g'], channels_last=True)
    a, b = run(), run()
    assert torch.equal(a, b) and _bits_equal(a, c['ref32']['grad_in'])
    x = torch.as_tensor(c['data']).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
        ops.psroi_pool(x, rois, c['scale'], c['output_dim'], c['P'], c['g'])
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.psroi_pool(x, rois, c['scale'], c['output_dim'], c['P'], c['g'])
        gcap = run()
    for _ in range(2):
        gcap.fill_(float('nan')); y.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gcap, a) and _bits_equal(y, c['ref32']['out'])


def test_grid_fold_70000_rois(K):
    """More rois than a grid.y / grid.z could hold: forward and backward against the restatement, every element."""
    ops, lib = K
    c = PC.grid_fold_case()
    ref = PC.psroi_restate(c['data'], c['rois'], c['scale'], 1, 1, 1, c['grad_out'])
    x, rois, go = (torch.as_tensor(c[k]).cuda() for k in ('data', 'rois', 'grad_out'))
    out, mapping = _fwd_raw(lib, c, x, False)
    assert _bits_equal(out, ref['out']) and float(mapping.abs().max()) == 0.0
    gin = _bwd_raw(lib, c, go, False, False)
    assert _bits_equal(gin, ref['grad_in']) and int(ref['n_add'].max()) > 20000


def test_refusals_launch_nothing(K):
    ops, lib = K
    L = lib.load()
    c = PC.case('p3g3_5x7_r65')
    x, rois, go = _data(c, 'nchw_f32'), torch.as_tensor(c['rois']).cuda(), torch.as_tensor(c['grad_out']).cuda()
    obuf, out = _guarded((c['R'], 3, 3, 3), torch.float32, False)
    gbuf, gin = _guarded((c['B'], c['C'], c['H'], c['W']), torch.float32, False)
    ok_f = dict(data=x.data_ptr(), ds=_strides(x), rois=rois.data_ptr(), out=out.data_ptr(), os=_strides(out), mapping=0, R=c['R'], B=c['B'],
                C=c['C'], H=c['H'], W=c['W'], od=3, P=3, g=3, scale=0.3, base=0, dtype=0, stream=_stream())
    ok_b = dict(go=go.data_ptr(), os=_strides(go), rois=rois.data_ptr(), gin=gin.data_ptr(), gs=_strides(gin), R=c['R'], B=c['B'], C=c['C'],
                H=c['H'], W=c['W'], od=3, P=3, g=3, scale=0.3, base=0, acc=0, dtype=0, stream=_stream())
    bad = [dict(C=c['C'] + 1), dict(od=2), dict(g=2), dict(P=0), dict(g=0), dict(dtype=2), dict(rois=0), dict(H=0), dict(R=-1)]
    for patch in bad + [dict(data=0), dict(out=0), dict(ds=None), dict(os=None)]:
        rc = L.relnet_psroi_pool_fwd(*dict(ok_f, **patch).values())
        assert rc != 0 and b'relnet_psroi_pool_fwd' in L.relnet_last_error(), patch
    for patch in bad + [dict(go=0), dict(gin=0), dict(gs=None), dict(os=None)]:
        rc = L.relnet_psroi_pool_bwd(*dict(ok_b, **patch).values())
        assert rc != 0 and b'relnet_psroi_pool_bwd' in L.relnet_last_error(), patch
    torch.cuda.synchronize()
    assert bool(torch.isnan(obuf).all()) and bool(torch.isnan(gbuf).all())
    # the Python front end raises on the same grounds
    with pytest.raises(lib.RelnetError, match='output_dim'):
        ops.psroi_pool(x, rois, 0.3, 2, 3, 3)
    with pytest.raises(lib.RelnetError, match='GPU tensors'):
        ops.psroi_pool(x.cpu(), rois, 0.3, 3, 3, 3)
    # and the accepted call on the same buffers does write
    assert L.relnet_psroi_pool_fwd(*ok_f.values()) == 0 and L.relnet_psroi_pool_bwd(*ok_b.values()) == 0
    torch.cuda.synchronize()
    assert _bits_equal(out, c['ref32']['out']) and _bits_equal(gin, c['ref32']['grad_in'])


def test_operator_cxx_python_op_forward_and_backward_reqs(K):
    from relnet_amd import operator_cxx as OC
    c = PC.case('p7g3_9x6_r65')
    prop = OC.PSROIPoolingProp(spatial_scale=c['scale'], output_dim=c['output_dim'], pooled_size=c['P'], group_size=c['g'])
    x, rois, go = (torch.as_tensor(c[k]).cuda() for k in ('data', 'rois', 'grad_out'))
    _, oshapes = prop.InferShape([tuple(x.shape), tuple(rois.shape)])
    out_data = [torch.full(s, float('nan'), device='cuda') for s in oshapes]
    op = prop.CreateOperatorEx()
    op.Forward(None, [x, rois], ['write', 'write'], out_data)
    assert _bits_equal(out_data[0], c['ref32']['out']) and _bits_equal(out_data[1], c['ref32']['mapping'])
    assert torch.equal(OC.contrib.PSROIPooling(x, rois, spatial_scale=c['scale'], output_dim=c['output_dim'], pooled_size=c['P'],
                                               group_size=c['g']), out_data[0])
    prior = torch.as_tensor(c['grad_in0']).cuda()
    for req, want in (('write', c['ref32']['grad_in']), ('add', c['ref32_acc']['grad_in']), ('null', c['grad_in0'])):
        gx, gr = prior.clone(), torch.full_like(rois, 5.0)
        op.Backward(None, [go], [x, rois], out_data, [req, 'write' if req != 'null' else 'null'], [gx, gr])
        assert _bits_equal(gx, want), req
        assert float(gr.abs().max()) == (5.0 if req == 'null' else 0.0)                # rois gradient zeroed on write, kept on null
    with pytest.raises(ValueError, match='kWriteInplace'):
        op.Backward(None, [go], [x, rois], out_data, ['inplace', 'null'], [prior.clone(), torch.zeros_like(rois)])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_facade_three_node_graph_equals_ops(K, dtype):
    ops, lib = K
    from relnet_amd import mx
    c = PC.case('p7g3_9x6_r65')
    s = mx.contrib.sym.PSROIPooling(name='psroi', data=mx.sym.Variable('data'), rois=mx.sym.Variable('rois'), spatial_scale=c['scale'],
                                    output_dim=c['output_dim'], pooled_size=c['P'], group_size=c['g'])
    x, rois = torch.as_tensor(c['data']), torch.as_tensor(c['rois'])
    exe = s.bind(mx.gpu(0), args={'data': x, 'rois': rois}, aux_states={}, dtype=dtype)
    got, = exe.forward(is_train=False)
    want = ops.psroi_pool(x.cuda(), rois.cuda(), c['scale'], c['output_dim'], c['P'], c['g'])
    assert got.shape == tuple(want.shape) and np.array_equal(got.asnumpy(), want.cpu().numpy())
    assert np.array_equal(got.asnumpy(), c['ref32']['out'])
