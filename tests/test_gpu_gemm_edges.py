"""csrc/gemm.hip at small, ragged, strided shapes (tests/gemm_cases.py): every tile configuration forced on launches of one to a few tiles, k-loops
of 1 / 2 / 3 / 5 / 17 slabs, broadcast / sliced / channel-padded operand views, maps of 1 to 208 pixels with several images per tile, R != S, free
padding, stride 2 and dilation 2 -- against float64 from the definition, per element, within the derived bound
(K_total + 2) 2^-23 (|A| |W|^T + |bias| + |resid|) (+ half a bf16 step for bf16 outputs).  tests/test_gemm_cases_host.py shows on the CPU that
correct fp32 accumulations use about 1 % of that bound and that the errors of a subtly wrong kernel exceed it.

Every operand lives in the middle of a buffer filled with a NaN pattern (>= 1 MiB on both sides, and every element of the parent tensor the view
does not cover): a read from outside an input turns outputs into NaN, and after every launch everything outside `out` and the whole of `resid`
are compared bit for bit.

A forced tile whose documented precondition a shape does not meet runs the fallback launch_bf16 names for it; the check is the same.  Which kernel
ran is asked of the library after every launch (relnet_gemm_last_launch): the cases written for the window, hand-scheduled, row-panel and split-K
kernels assert that those ran (RAN below), and every figure of the report is filed under the kernel that produced it, never under the tile forced.
RELNET_TEST_TILES=0,17 (development aid, as in test_gpu_gemm_tiles.py) restricts the tile list; RELNET_TEST_REPORT=<file> appends the worst
err / tolerance per kernel family and output dtype (fp32 outputs: the tolerance is the bound; bf16: bound + half a bf16 step)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as GC  # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
_ids = lambda cases: [c['id'] for c in cases]

KIND = {1: 'LDS-tiled', 2: 'ring', 3: 'window', 4: 'asm ring', 5: 'panel', 6: 'split-K'}      # low byte of relnet_gemm_last_launch()


def _ran(L):
    """-> (kernel family, split-K ways) of the launch just made."""
    code = L.relnet_gemm_last_launch()
    return KIND[code & 255], code >> 8


def _must_run(case, odt, t):
    """The family a forced tile MUST run on the cases the issue writes for it (their shapes meet the preconditions at its `case` in launch_bf16), so
    that a later change of a precondition, a fallback or the split-K work area cannot turn these checks into checks of the fallback unnoticed."""
    base = case['id'].split('-')[0]
    if t == 17 and base in ('C1', 'C2', 'C3', 'C4'):
        return 'window'                    # 3x3, stride 1, pad == dil, no shortcut, 256 + 2 (W + 1) dil <= 384
    if t in (18, 19) and base in ('C3', 'C4', 'G7'):
        return 'asm ring'                  # no shortcut, N % 256 == 0
    if t in (13, 14, 15) and base in ('G6', 'C9') and odt == BF16:
        return 'panel'                     # K in {64 .. 512}, N % 256 == 0, bf16 out, plain GEMM / 1x1 stride 1, per-column bias at most
    if t == 23 and base in ('G7', 'C11'):
        return 'split-K'                   # batch 1, N % 8 == 0, K >= 128, 16-byte aligned out / resid, the work area holds the partial tiles
    return None


WORST = {}                 # (family, 'f32' | 'bf16') -> (largest |got - ref64| / tolerance, where)
CHECKED = {}               # (family, 'f32' | 'bf16') -> launches checked


def _note(family, odt, ratio, where):
    key = (family, 'bf16' if odt == BF16 else 'f32')
    CHECKED[key] = CHECKED.get(key, 0) + 1
    if key not in WORST or ratio > WORST[key][0]:
        WORST[key] = (ratio, where)


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib
    L = lib.load()
    try:
        yield ops, lib, L
    finally:
        L.relnet_gemm_force_tile(0); L.relnet_gemm_force_nloop(0); L.relnet_gemm_set_swizzle(1); L.relnet_gemm_debug_splitk(0)
        path = os.environ.get('RELNET_TEST_REPORT')
        if path and WORST:
            with open(path, 'a') as f:
                for (fam, dt), (ratio, where) in sorted(WORST.items()):
                    f.write('%-10s %-4s %5d launches, worst err / tolerance %.4f  at %s\n' % (fam, dt, CHECKED[(fam, dt)], ratio, where))


def _tiles(L, only=None):
    tiles = [0] + list(range(1, L.relnet_gemm_tile_count() + 1))
    if os.environ.get('RELNET_TEST_TILES'):
        tiles = [int(t) for t in os.environ['RELNET_TEST_TILES'].split(',')]
    return [t for t in tiles if only is None or t in only]


def _set(L, t, s=1, nl=0, ways=0):
    L.relnet_gemm_force_tile(t); L.relnet_gemm_set_swizzle(s); L.relnet_gemm_force_nloop(nl); L.relnet_gemm_debug_splitk(ways)


def _place(t_cpu, dtype, parent=None, index=None):
    """CPU tensor -> guarded device operand holding the same values."""
    g = GC.guarded(tuple(t_cpu.shape), dtype, parent=parent, index=index)
    g.view.copy_(t_cpu.to(dtype))
    return g


def _out_buffers(case, o, odt, ldc=None):
    """-> (guarded out, guarded resid | None, pristine resid copy | None).  The view of `out` is [.., :N] of a [.., ldc] parent; for the
    zero-initialised outputs (the relation module's form) it is the whole [.., ldc] parent, zeroed, and the kernel is told n_cols."""
    shape = tuple(o['oshape'])
    N = shape[-1]
    ldc = ldc or case.get('ldc') or N
    parent = shape[:-1] + (ldc,)
    if case.get('zero_out'):
        out = GC.guarded(parent, odt)
        out.view.zero_()
    else:
        out = GC.guarded(shape, odt, parent=parent, index=(Ellipsis, slice(0, N)))
    res = keep = None
    if case['resid']:
        res = _place(GC.resid_for(o, odt), odt, parent=parent, index=(Ellipsis, slice(0, N)))
        keep = res.buf.clone()
    return out, res, keep


class _Ref(object):
    """float64 reference of one (case, output dtype) on the device, computed once."""
    def __init__(self, case, o, odt):
        pre, mag = GC.ref64(case, o, odt)
        self.pre, self.mag = pre.cuda(), mag.cuda()
        self.want = GC.activate(case, o, odt, pre).cuda()
        self.K, self.bf, self.relu = case['K'], odt == BF16, case['relu']

    def check(self, got, what):
        assert not torch.isnan(got).any(), (what, 'NaN in the output: an operand was read outside its view')
        ok, worst = GC.accept(got, self.want, self.pre, self.mag, self.K, self.bf, self.relu)
        assert ok, (what, 'worst |got - ref64| / tolerance', worst)
        return worst


def _after_launch(case, out, res, keep, got_view, N, what):
    assert GC.guards_intact(out.buf, got_view if not case.get('zero_out') else out.view), (what, 'stored outside out[.., :N]')
    if case.get('zero_out'):
        assert bool((out.view[..., N:] == 0).all()), (what, 'pad columns written')
    if res is not None:
        assert torch.equal(res.buf.view(torch.int16 if res.buf.element_size() == 2 else torch.int32),
                           keep.view(torch.int16 if keep.element_size() == 2 else torch.int32)), (what, 'resid changed')


# ---------------------------------------------------------------------------------------------------------------------------------------------
# ops.gemm_nt, bf16 operands
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', GC.GEMM_CASES, ids=_ids(GC.GEMM_CASES))
def test_gemm_nt_case(rn, case):
    ops, lib, L = rn
    o = GC.operands(case)
    N = case['N']
    a = _place(o['a'], BF16, parent=case['a_parent'], index=case['a_index'])
    w = _place(o['w'], BF16, parent=case['w_parent'], index=case['w_index'])
    bias = o['bias'].cuda() if o['bias'] is not None else None
    for odt in case['odts']:
        ref = _Ref(case, o, odt)
        out, res, keep = _out_buffers(case, o, odt)
        got_view = out.view[..., :N]

        def launch():
            if not case.get('zero_out'):
                GC._fill_pattern(out.buf)
            else:
                out.view[..., :N] = float('nan')
            return ops.gemm_nt(a.view, w.view, bias, bias_mode=case['bias'] or 1, resid=None if res is None else res.view, relu=case['relu'],
                               out=out.view, n_cols=N if case.get('zero_out') else None)

        variants = [(t, 1, 0, 0) for t in _tiles(L)]
        if case['knobs']:
            variants += [(t, s, nl, 0) for t in _tiles(L) if t for s in (0, 1) for nl in (1, 2, 4)]
        for (t, s, nl, ways) in variants:
            what = (case['id'], str(odt), 'tile', t, 'swizzle', s, 'n_loop', nl)
            _set(L, t, s, nl, ways)
            launch()
            fam = _ran(L)[0]
            assert _must_run(case, odt, t) in (None, fam), (what, 'ran', fam)
            _note(fam, odt, ref.check(got_view, what), what)
            _after_launch(case, out, res, keep, got_view, N, what)
            if t == 0:
                first = got_view.clone()
                launch()
                assert torch.equal(first, got_view), (what, 'second launch differs')
        for ways in (case['splitk'] if 23 in _tiles(L) else ()):
            what = (case['id'], str(odt), 'tile 23, ways', ways)
            _set(L, 23, 1, 0, ways)
            runs = []
            for _ in range(3):
                launch()
                assert _ran(L) == ('split-K', ways), (what, 'ran', _ran(L))
                runs.append(got_view.clone())
                _after_launch(case, out, res, keep, got_view, N, what)
            assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), (what, 'not deterministic')
            _note('split-K', odt, ref.check(runs[0], what), what)
        _set(L, 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# relnet_gemm_nt with fp32 operands (one kernel, no tiles)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', GC.GEMM_F32_CASES, ids=_ids(GC.GEMM_F32_CASES))
def test_gemm_nt_f32_operands_case(rn, case):
    ops, lib, L = rn
    _set(L, 0)
    o = GC.operands(case)
    a, w = _place(o['a'], F32), _place(o['w'], F32)
    bias = o['bias'].cuda()
    for odt in case['odts']:
        ref = _Ref(case, o, odt)
        out, res, keep = _out_buffers(case, o, odt)
        what = (case['id'], str(odt))
        for rep in range(2):
            GC._fill_pattern(out.buf)
            ops.gemm_nt(a.view, w.view, bias, resid=res.view, relu=True, out=out.view)
            _note('fp32', odt, ref.check(out.view, what), what)
            _after_launch(case, out, res, keep, out.view, case['N'], what)
            if rep == 0:
                first = out.view.clone()
        assert torch.equal(first, out.view)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# ops.gemm_nt_mask
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', GC.GEMM_MASK_CASES, ids=_ids(GC.GEMM_MASK_CASES))
def test_gemm_nt_mask_case(rn, case):
    ops, lib, L = rn
    o = GC.operands(case)
    a, w = _place(o['a'], BF16), _place(o['w'], BF16)
    mask = _place(o['mask'], BF16)
    ref = _Ref(case, o, BF16)
    out, res, keep = _out_buffers(case, o, BF16)
    mkeep = mask.buf.clone()
    off = (o['mask'] <= 0).cuda()
    for t in _tiles(L, only=GC.MASK_TILES):
        what = (case['id'], 'tile', t)
        _set(L, t)
        for rep in range(2 if t == 0 else 1):
            GC._fill_pattern(out.buf)
            ops.gemm_nt_mask(a.view, w.view, mask.view, resid=None if res is None else res.view, out=out.view)
            _note('mask', BF16, ref.check(out.view, what), what)
            assert bool((out.view[off] == 0).all()), (what, 'a masked entry is not an exact zero')
            _after_launch(case, out, res, keep, out.view, case['N'], what)
            assert torch.equal(mask.buf.view(torch.int16), mkeep.view(torch.int16))
            if rep == 0:
                first = out.view.clone()
        assert torch.equal(first, out.view), (what, 'second launch differs')
    _set(L, 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# convolutions
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _conv_input(case, o, dtype):
    """-> (guarded input, the tensor handed to the kernel).  views: channels 64 .. 64 + Cin of a [B, H + 2, W, Cin + 128] buffer, rows 1 .. H;
    holes: only the pixels a stride-2 1x1 convolution reads are written, the others keep the NaN pattern."""
    B, H, W, Cin = case['B'], case['H'], case['W'], case['Cin']
    if case['views']:
        g = _place(o['a'], dtype, parent=(B, H + 2, W, Cin + 128), index=(slice(None), slice(1, H + 1), slice(None), slice(64, 64 + Cin)))
        return g, g.view
    if case['holes']:
        g = _place(o['a'][:, ::2, ::2], dtype, parent=(B, H, W, Cin), index=(slice(None), slice(None, None, 2), slice(None, None, 2)))
        return g, g.parent
    g = _place(o['a'], dtype)
    return g, g.view


def _conv_abi(lib, entry, x, w, wf, bias, res, relu, out, case, odt):
    stream = torch.cuda.current_stream().cuda_stream
    geo = (case['B'], case['H'], case['W'], case['Cin'], case['Cout'], case['R'], case['S'], case['stride'], case['dil'], case['pad'])
    if entry == 'relnet_conv2d_nhwc_f32':
        lib.call(entry, x.data_ptr(), x.stride(2), x.stride(0), w.data_ptr(), bias.data_ptr(), 0 if res is None else res.data_ptr(), int(relu),
                 out.data_ptr(), out.stride(2), *geo, stream)
    else:
        lib.call(entry, x.data_ptr(), x.stride(2), x.stride(0), w.data_ptr(), 0 if wf is None else wf.data_ptr(), bias.data_ptr(),
                 0 if res is None else res.data_ptr(), int(relu), out.data_ptr(), out.stride(2), *geo, lib.BF16 if odt == BF16 else lib.F32, stream)


@pytest.mark.parametrize('case', GC.CONV_CASES, ids=_ids(GC.CONV_CASES))
def test_conv2d_case(rn, case):
    ops, lib, L = rn
    o = GC.operands(case)
    N = case['Cout']
    xg, x = _conv_input(case, o, BF16)
    xkeep = xg.buf.clone()
    w = _place(o['w'], BF16)
    bias = o['bias'].cuda()
    _set(L, 0)
    wfs = [None]
    if case['wfrag']:
        wf = ops.pack_w_frag(w.view)
        assert wf is not None
        wfs = [None, wf]
    for odt in case['odts']:
        ref = _Ref(case, o, odt)
        out, res, keep = _out_buffers(case, o, odt, ldc=N + 64 if case['views'] else None)

        def launch(wf):
            GC._fill_pattern(out.buf)
            if case['abi']:
                ops.gemm_workspace()
                _conv_abi(lib, 'relnet_conv2d_nhwc_wf', x, w.view, wf, bias, None if res is None else res.view, case['relu'], out.view, case, odt)
            else:
                assert case['R'] == case['S']
                ops.conv2d_nhwc(x, w.view, bias, ksize=case['R'], stride=case['stride'], pad=case['pad'], dil=case['dil'], relu=case['relu'],
                                resid=None if res is None else res.view, out=out.view, w_frag=wf)

        for wf in wfs:
            for t in _tiles(L):
                what = (case['id'], str(odt), 'tile', t, 'w_frag' if wf is not None else '')
                _set(L, t)
                launch(wf)
                fam = _ran(L)[0]
                assert _must_run(case, odt, t) in (None, fam), (what, 'ran', fam)
                _note(fam, odt, ref.check(out.view, what), what)
                _after_launch(case, out, res, keep, out.view, N, what)
                if t == 0:
                    first = out.view.clone()
                    launch(wf)
                    assert torch.equal(first, out.view), (what, 'second launch differs')
        for ways in (case['splitk'] if 23 in _tiles(L) else ()):
            what = (case['id'], str(odt), 'tile 23, ways', ways)
            _set(L, 23, 1, 0, ways)
            runs = []
            for _ in range(3):
                launch(None)
                assert _ran(L) == ('split-K', ways), (what, 'ran', _ran(L))
                runs.append(out.view.clone())
                _after_launch(case, out, res, keep, out.view, N, what)
            assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), (what, 'not deterministic')
            _note('split-K', odt, ref.check(runs[0], what), what)
        _set(L, 0)
    assert torch.equal(xg.buf.view(torch.int16), xkeep.view(torch.int16))


@pytest.mark.parametrize('case', GC.CONV_F32_CASES, ids=_ids(GC.CONV_F32_CASES))
def test_conv2d_f32_case(rn, case):
    ops, lib, L = rn
    _set(L, 0)
    o = GC.operands(case)
    xg, x = _conv_input(case, o, F32)
    w = _place(o['w'], F32)
    bias = o['bias'].cuda()
    ref = _Ref(case, o, F32)
    out, res, keep = _out_buffers(case, o, F32)
    what = (case['id'],)
    for rep in range(2):
        GC._fill_pattern(out.buf)
        if case['R'] == case['S']:
            ops.conv2d_nhwc_f32(x, w.view, bias, ksize=case['R'], stride=case['stride'], pad=case['pad'], dil=case['dil'], relu=case['relu'],
                                resid=None if res is None else res.view, out=out.view)
        else:
            _conv_abi(lib, 'relnet_conv2d_nhwc_f32', x, w.view, None, bias, None if res is None else res.view, case['relu'], out.view, case, F32)
        _note('fp32', F32, ref.check(out.view, what), what)
        if case['relu'] == 2:
            assert bool((out.view[res.view <= 0] == 0).all()), (what, 'a masked entry is not an exact zero')
        _after_launch(case, out, res, keep, out.view, case['Cout'], what)
        if rep == 0:
            first = out.view.clone()
    assert torch.equal(first, out.view)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_unsupported_operands_are_refused(rn):
    """bf16 K = 96, lda = K + 4, conv Cin = 32 and in_pix = Cin + 4: RelnetError, and nothing is written."""
    ops, lib, L = rn
    _set(L, 0)
    out = GC.guarded((8, 64), BF16)
    empty = out.buf[:0]

    def untouched():
        return GC.guards_intact(out.buf, empty)
    a = torch.zeros(8, 96, device='cuda', dtype=BF16)
    w = torch.zeros(64, 96, device='cuda', dtype=BF16)
    with pytest.raises(lib.RelnetError):
        ops.gemm_nt(a, w, out=out.view)
    assert untouched()
    a = torch.zeros(8, 68, device='cuda', dtype=BF16)[:, :64]          # lda = K + 4
    w = torch.zeros(64, 64, device='cuda', dtype=BF16)
    with pytest.raises(lib.RelnetError):
        ops.gemm_nt(a, w, out=out.view)
    assert untouched()
    bias = torch.zeros(64, device='cuda')
    cout = GC.guarded((1, 2, 4, 64), BF16)
    x = torch.zeros(1, 2, 4, 32, device='cuda', dtype=BF16)            # Cin = 32
    w = torch.zeros(64, 32, device='cuda', dtype=BF16)
    with pytest.raises(lib.RelnetError):
        ops.conv2d_nhwc(x, w, bias, out=cout.view)
    assert GC.guards_intact(cout.buf, cout.buf[:0])
    x = torch.zeros(1, 2, 4, 68, device='cuda', dtype=BF16)[..., :64]  # in_pix = Cin + 4
    w = torch.zeros(64, 64, device='cuda', dtype=BF16)
    with pytest.raises(lib.RelnetError):
        ops.conv2d_nhwc(x, w, bias, out=cout.view)
    assert GC.guards_intact(cout.buf, cout.buf[:0])
