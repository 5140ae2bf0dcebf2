"""The DEFAULT gradient-accumulation kernels of a training step at their edges (tests/grad_accum_cases.py): wgrad_streamk_kernel through
ops.wgrad_tn / ops.WgradQueue (Wout at the slab width, maps smaller than a slab, 1x1 stride 2 over NaN holes, 7x7, every pixel count around one
and two slabs, both wave-tile heights, every stream-K share cut, operands that are slices of NaN-filled parents), the colsum kernels through
train_ops.colsum_add / ColsumQueue (rows at the chunk boundaries and the 128-chunk cap, every width on every load path, queues of 1 / 16 / 17
problems), the ROI pooling backward in its owner and scatter forms (list segments, the pair loop's tails, the channel-group permutation, the
largest map) and relnet_strided_scatter -- each against the float64 definition, EVERY element, within the bound derived in grad_accum_cases
(strided_scatter: bit for bit).

Outputs are views inside larger buffers with non-zero contents; whatever lies outside the view is compared bit for bit with a copy taken before
the launch, and so are the inputs.  Debug setters are restored in `finally`.

Every test prints its worst err / bound under the kernel's name; RELNET_TEST_REPORT=<file> appends the worst per kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as GC  # noqa: E402
import grad_accum_cases as AC  # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
_ids = lambda cs: [c['id'] for c in cs]
WORST = {}                 # kernel / output -> [largest err / bound, where, launches]
_REF = {}


def _note(kernel, ratio, where):
    print('%-34s %-40s worst err / bound %.4f' % (kernel, where, ratio))
    w = WORST.setdefault(kernel, [0.0, where, 0])
    w[2] += 1
    if ratio >= w[0]:
        w[0], w[1] = ratio, where


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import lib, ops, train_ops
    try:
        yield lib, ops, train_ops
    finally:
        path = os.environ.get('RELNET_TEST_REPORT')
        if path and WORST:
            with open(path, 'a') as f:
                for k, (ratio, where, n) in sorted(WORST.items()):
                    f.write('%-34s %4d launches, worst err / bound %.4f  at %s\n' % (k, n, ratio, where))


def _memo(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


class Watched(object):
    """A buffer whose bits outside `view` (and, for an input, inside it too) must survive a launch."""

    def __init__(self, buf, view, is_input):
        self.buf, self.view, self.is_input = buf, view, is_input
        self.snap()

    def snap(self):
        self.before = AC.bits(self.buf).clone()

    def _inside(self, flat):
        return flat.as_strided(self.view.shape, self.view.stride(), self.view.storage_offset() - self.buf.storage_offset())

    def intact(self):
        now = AC.bits(self.buf).clone()
        if not self.is_input:
            self._inside(now).copy_(self._inside(self.before))
        return torch.equal(now, self.before)


def _inp(values, dtype, parent=None, index=None):
    g = GC.guarded(tuple(values.shape), dtype, parent, index)
    g.view.copy_(values)
    return g


def _cpu64(t):
    return t.detach().double().cpu()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# csrc/wgrad.hip
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _wg_ref(case):
    def make():
        o = AC.wgrad_operands(case)
        ref, mag = AC.wgrad_ref64(case, o)
        return o, ref, AC.wgrad_bound(case, mag)
    return _memo(('wg', case['id']), make)


class WgradDevice(object):
    """The operands of one layer on the device: x a channel slice of a NaN-pattern parent (xpad) inside NaN guards, dy2d a column slice (dypad)
    with zero columns behind the real ones (dyzero), out a view inside a wider non-zero fp32 buffer."""

    def __init__(self, case, o):
        self.case, self.o = case, o
        Cin, Cout, K, P = case['Cin'], case['Cout'], case['K'], case['P']
        xs = tuple(o['x'].shape)
        cut = lambda n, lo, w: (slice(None),) * n + (slice(lo, lo + w),)
        gx = _inp(torch.nan_to_num(o['x']), BF16, xs[:-1] + (Cin + case['xpad'],) if case['xpad'] else None,
                  cut(len(xs) - 1, 8, Cin) if case['xpad'] else None)
        if case['holes']:                                  # the pixels stride 2 never reads hold the guard pattern
            pi = gx.parent.view(torch.int16)
            vi = pi[cut(len(xs) - 1, 8, Cin)] if case['xpad'] else pi
            vi[torch.isnan(o['x']).cuda()] = GC._PATTERN[2]
            assert bool(torch.isnan(gx.view).any())
        self.x = gx.view
        cols = Cout + case['dyzero']
        dy = torch.zeros(P, cols)
        dy[:, :Cout] = o['dy']
        gdy = _inp(dy, BF16, (P, cols + case['dypad']) if case['dypad'] else None, cut(1, 8, cols) if case['dypad'] else None)
        self.dy = gdy.view
        self.scale = None if o['scale'] is None else o['scale'].cuda()
        gen = torch.Generator().manual_seed(AC.seed(case['id']) + 1)
        gout = _inp(torch.randn(Cout + 4, K + 24, generator=gen), F32)
        self.out = gout.view[2:2 + Cout, 8:8 + K]
        self.old = o['old'].cuda()
        self.inputs = [Watched(gx.buf, gx.view, True), Watched(gdy.buf, gdy.view, True)]
        self.outw = Watched(gout.buf, self.out, False)
        self.conv = (case['ks'], case['stride'], case['dil'], case['pad']) if case['conv'] else None
        assert (self.x.stride(-2) > Cin) == bool(case['xpad']) and (self.dy.stride(0) > cols) == bool(case['dypad'])

    def reset(self):
        self.out.copy_(self.old)
        self.outw.snap()

    def queue(self, q):
        q.add(self.dy, self.x, self.out, self.scale, self.case['Cout'], self.conv)

    def check(self, ref, bound, kernel, where):
        torch.cuda.synchronize()
        assert self.outw.intact(), 'a store outside the [Cout, K] view'
        assert all(w.intact() for w in self.inputs), 'an input changed'
        got = _cpu64(self.out)
        r = AC.worst(got, ref, bound)
        _note(kernel, r, where)
        assert r <= 1.0, (where, r)
        return AC.bits(self.out).clone()


@pytest.mark.parametrize('case', AC.WGRAD_CASES, ids=_ids(AC.WGRAD_CASES))
def test_wgrad_every_share_cut_within_the_bound(rn, case):
    """ops.wgrad_tn at the default grid, then the same layer through a queue flushed with 1, 2, 3, 7, units - 1, units and units + 5 workgroups
    (the grid size is an argument of the launch): every cut position between (tile, slab) units occurs."""
    lib, ops, _ = rn
    o, ref, bound = _wg_ref(case)
    d = WgradDevice(case, o)
    d.reset()
    ret = ops.wgrad_tn(d.dy, d.x, out=d.out, row_scale=d.scale, cout=case['Cout'], conv=d.conv)
    assert ret.data_ptr() == d.out.data_ptr()
    d.check(ref, bound, 'wgrad_streamk wgrad_tn', case['id'])
    units = AC.wgrad_units(case)
    assert units <= AC.WGRAD_FEW_UNITS
    for k in AC.wgrad_grids(units):
        d.reset()
        q = ops.WgradQueue()
        d.queue(q)
        q.flush(workgroups=k)
        assert len(q) == 0
        d.check(ref, bound, 'wgrad_streamk shares', '%s workgroups=%d of %d units' % (case['id'], k, units))


@pytest.mark.parametrize('case', AC.WGRAD_CASES, ids=_ids(AC.WGRAD_CASES))
def test_wgrad_plain_and_transposed_reads_and_the_deterministic_grids_agree_bit_for_bit(rn, case):
    """One writer per word in a fixed order (one workgroup, or the deterministic queue's whole-tile shares): the plain-LDS-read kernel and the
    transposed-read kernel give the same bits, and the deterministic queue the same bits at 1, 3 and 1000 workgroups."""
    lib, ops, _ = rn
    o, ref, bound = _wg_ref(case)
    d = WgradDevice(case, o)
    res = {}
    for plain in (0, 1):
        lib.load().relnet_wgrad_debug_plain(plain)
        try:
            for det, k in ((False, 1), (True, 1), (True, 3), (True, 1000)):
                d.reset()
                q = ops.WgradQueue(deterministic=det)
                d.queue(q)
                q.flush(workgroups=k)
                res[plain, det, k] = d.check(ref, bound, 'wgrad_streamk %s%s' % ('plain' if plain else 'tr', ' det' if det else ''),
                                             '%s workgroups=%d' % (case['id'], k))
        finally:
            lib.load().relnet_wgrad_debug_plain(0)
    assert torch.equal(res[0, False, 1], res[1, False, 1])
    for key in ((0, True, 3), (0, True, 1000), (1, True, 1), (1, True, 3), (1, True, 1000)):
        assert torch.equal(res[0, True, 1], res[key]), key


@pytest.mark.parametrize('gid', sorted(AC.WGRAD_GROUPS))
def test_wgrad_grouped_layers_of_8_and_264_rows_on_the_tall_tile(rn, gid):
    """Several layers in ONE launch: the 8-row layers run on the 256-row tile the 264-row layer selects, the shares cut across layers."""
    lib, ops, _ = rn
    cases = [AC.WGRAD_BY_ID[i] for i in AC.WGRAD_GROUPS[gid]]
    rows = AC.wgrad_tile_rows(cases)
    total = sum(AC.wgrad_units(c, rows) for c in cases)
    devs = [(WgradDevice(c, _wg_ref(c)[0]),) + _wg_ref(c)[1:] for c in cases]
    for k in AC.wgrad_grids(total) + [0]:
        q = ops.WgradQueue()
        for d, _, _ in devs:
            d.reset()
            d.queue(q)
        assert len(q) == len(cases)
        q.flush(workgroups=k)
        for d, ref, bound in devs:
            d.check(ref, bound, 'wgrad_streamk grouped', '%s/%s workgroups=%d of %d units' % (gid, d.case['id'], k, total))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# csrc/train_ops.hip: column sums
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _colsum_device(x, old, dtype, ld, offset=0):
    """x as rows of pitch ld inside a NaN-pattern buffer (its first element `offset` elements behind a 256-byte boundary), out on its start value
    inside a pattern-guarded buffer."""
    rows, cols = x.shape
    g = GC.guarded((rows * ld + 8,), dtype)
    xv = g.view[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    xv.copy_(x)
    go = _inp(old, F32)
    assert xv.data_ptr() % 16 == (offset * g.view.element_size()) % 16
    return xv, go.view, Watched(g.buf, xv, True), Watched(go.buf, go.view, False)


def _colsum_check(xw, ow, out, ref, bound, kernel, where):
    torch.cuda.synchronize()
    assert ow.intact(), 'a store outside out[0:cols]'
    assert xw.intact(), 'the operand changed'
    r = AC.worst(_cpu64(out), ref, bound)
    _note(kernel, r, where)
    assert r <= 1.0, (where, r)


@pytest.mark.parametrize('case', AC.COLSUM_CASES, ids=_ids(AC.COLSUM_CASES))
def test_colsum_add_rows_widths_and_load_paths(rn, case):
    _, _, T = rn
    x, old = AC.colsum_operands(case['id'], case['rows'], case['cols'], case['dtype'])
    ref, mag = AC.colsum_ref64(x, old)
    xv, out, xw, ow = _colsum_device(x, old, case['dtype'], case['ld'], case['offset'])
    assert xv.stride(0) == case['ld'] or case['rows'] == 1
    T.colsum_add(xv, out)
    _colsum_check(xw, ow, out, ref, AC.colsum_bound(case['rows'], case['lanes'], mag), 'colsum_add ' + case['path'], case['id'])


@pytest.mark.parametrize('qid', sorted(AC.COLSUM_QUEUES))
def test_colsum_queue_of_1_16_and_17_problems(rn, qid):
    _, _, T = rn
    operands = AC.colsum_queue_operands(qid)
    refs = AC.colsum_queue_ref64(qid, operands)
    q = T.ColsumQueue()
    devs = []
    for (x, old), (_, c, pad) in zip(operands, AC.COLSUM_QUEUES[qid]):
        devs.append(_colsum_device(x, old, BF16, c + pad))
        T.colsum_add(devs[-1][0], devs[-1][1], q)
    assert len(q) == len(operands)                            # every operand takes the grouped kernel
    torch.cuda.synchronize()
    assert all(torch.equal(out.cpu(), old) for (_, out, _, _), (_, old) in zip(devs, operands))          # nothing launched yet
    q.flush()
    assert len(q) == 0
    for i, ((xv, out, xw, ow), (ref, mag)) in enumerate(zip(devs, refs)):
        _colsum_check(xw, ow, out, ref, AC.colsum_bound(xv.shape[0], 8, mag), 'colsum_add_grouped', '%s[%d] %dx%d' % ((qid, i) + tuple(xv.shape)))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# csrc/roi_pool.hip: backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _roi_ref(case):
    def make():
        o = AC.roi_operands(case)
        return o, AC.roi_ref64(case, o)
    return _memo(('roi', case['id']), make)


def _roi_device(case, o, channels_last):
    gout = AC.roi_to_layout(o['gout'].to(case['dtype']).cuda(), channels_last)
    argmax = AC.roi_to_layout(o['argmax'].cuda(), channels_last)
    assert gout.stride() == argmax.stride() and (gout.stride(1) == 1) == (channels_last or case['C'] == 1)
    return gout, argmax, o['rois'].cuda(), (None if o['level'] is None else o['level'].cuda())


def _roi_check(case, got_levels, refs, owner, kernel, where=''):
    """got_levels: logical [B, C, H, W] per level -> worst err / bound over every element; also the bounds (for the owner / scatter comparison)."""
    worst, outs = 0.0, []
    for got, (ref, mag, cnt), (h, w) in zip(got_levels, refs, case['levels']):
        assert tuple(got.shape) == (case['B'], case['C'], h, w)
        g = _cpu64(got).reshape(case['B'], case['C'], h * w)
        bound = AC.roi_bound(mag, cnt, owner)
        worst = max(worst, AC.worst(g, ref, bound))
        outs.append((g, bound))
    _note(kernel, worst, case['id'] + where)
    assert worst <= 1.0, (case['id'], kernel, worst)
    return outs


@pytest.mark.parametrize('case', [c for c in AC.ROI_CASES if c['form'] == 'cl'], ids=lambda c: c['id'])
def test_roi_pool_backward_channels_last_owner_and_scatter(rn, case):
    """relnet_roi_pool_bwd_cl as it decides for itself (the owner form wherever the table says so) and under relnet_roi_pool_bwd_debug(1) (the
    scatter form) on the same operands: both within their bound of the definition, and within the sum of the bounds of each other."""
    lib, ops, _ = rn
    o, refs = _roi_ref(case)
    gout, argmax, rois, _ = _roi_device(case, o, True)
    snaps = [t.clone() for t in (gout, argmax, rois)]
    (h, w), res = case['levels'][0], {}
    for mode in (0, 1):
        lib.load().relnet_roi_pool_bwd_debug(mode)
        try:
            got = ops.roi_pool_bwd(gout, argmax, rois, (case['B'], case['C'], h, w), batch_index_base=case['base'], channels_last=True)
            torch.cuda.synchronize()
        finally:
            lib.load().relnet_roi_pool_bwd_debug(0)
        assert got.permute(0, 2, 3, 1).is_contiguous()
        owner = case['owner'] and mode == 0
        res[mode] = _roi_check(case, [got], refs, owner, 'roi_pool_bwd_owner' if owner else 'roi_pool_bwd scatter (cl)', ' mode %d' % mode)
        del got
    assert all(AC.bits(t).equal(AC.bits(s)) for t, s in zip((gout, argmax, rois), snaps)), 'an input changed'
    (g0, b0), (g1, b1) = res[0][0], res[1][0]
    assert AC.worst(g0, g1, b0 + b1) <= 1.0


@pytest.mark.parametrize('case', [c for c in AC.ROI_CASES if c['form'] != 'cl'], ids=lambda c: c['id'])
def test_roi_pool_backward_scatter_entry_points(rn, case):
    """relnet_roi_pool_bwd_ex with NCHW and with NHWC gradient strides, relnet_roi_pool_fpn_bwd_ex over 2 and 4 levels; channels-last and dense
    grad_out / argmax."""
    lib, ops, _ = rn
    o, refs = _roi_ref(case)
    B, C, R = case['B'], case['C'], case['R']
    cl = case['id'] in ('X-nhwc', 'X-fpn2')
    gout, argmax, rois, level = _roi_device(case, o, cl)
    snaps = [t.clone() for t in (gout, argmax, rois)]
    (h, w) = case['levels'][0]
    if case['form'] == 'nchw':
        got = [ops.roi_pool_bwd(gout, argmax, rois, (B, C, h, w), batch_index_base=case['base'])]
        assert got[0].is_contiguous()
    elif case['form'] == 'nhwc':
        g = _inp(torch.zeros(B, h * w, C), F32)
        watch = Watched(g.buf, g.view, False)
        lib.call('relnet_roi_pool_bwd_ex', gout.data_ptr(), argmax.data_ptr(), ops._strides4(gout), rois.data_ptr(), g.view.data_ptr(),
                 h * w * C, 1, C, R, C, w, case['PH'], case['PW'], case['base'], ops._dt(gout), ops._stream())
        torch.cuda.synchronize()
        assert watch.intact(), 'a store outside grad_in'
        got = [g.view.view(B, h, w, C).permute(0, 3, 1, 2)]
    else:
        shapes = [(B, C, lh, lw) for lh, lw in case['levels']]
        got = ops.roi_pool_fpn_bwd(gout, argmax, rois, level, shapes, batch_index_base=case['base'], channels_last=cl)
    torch.cuda.synchronize()
    _roi_check(case, got, refs, False, 'roi_pool_bwd scatter (%s)' % case['form'])
    assert all(AC.bits(t).equal(AC.bits(s)) for t, s in zip((gout, argmax, rois), snaps)), 'an input changed'


# ---------------------------------------------------------------------------------------------------------------------------------------------
# csrc/train_ops.hip: strided scatter
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', AC.SCATTER_CASES, ids=_ids(AC.SCATTER_CASES))
def test_strided_scatter_moves_bits(rn, case):
    _, _, T = rn
    low, mask = AC.scatter_operands(case)
    gl = _inp(low, case['dtype'])
    gm = None if mask is None else _inp(mask, case['dtype'])
    watch = [Watched(g.buf, g.view, True) for g in (gl, gm) if g is not None]
    shape = (case['B'], case['H'], case['W'], case['C'])
    out = T.strided_scatter(gl.view, shape, case['stride'], mask=None if gm is None else gm.view)
    torch.cuda.synchronize()
    assert tuple(out.shape) == shape and out.dtype == case['dtype']
    want = AC.scatter_ref(case, low, mask)
    assert torch.equal(AC.bits(out).cpu(), AC.bits(want)), case['id']
    assert all(w.intact() for w in watch), 'an input changed'
    _note('strided_scatter', 0.0, case['id'])
