"""The hand-scheduled trunk kernels at the edges of their persistent loops (tests/trunk_cases.py): every instantiation of bottleneck_chain_kernel,
chain256_roles_kernel, conv3x3_c64_halo_kernel<false / true> (csrc/bottleneck.hip) and the fused stem with its uint8 twin (csrc/stem.hip), at
less than a tile, a tile and a lock-step set +- one pixel, the grid cap hit exactly, a second iteration in one and in several workgroups and a
third one -- against float64 on the same bf16 operands, per element, within the derived bound of tests/gemm_cases.py (no measured constant;
tests/test_trunk_cases_host.py shows that a correct fp32 evaluation uses a small part of it and that a moved value exceeds it).

Every activation operand and every output lives in the middle of a buffer filled with a NaN pattern: a read outside an operand turns outputs into
NaN, a store outside an output (a row mask one tile off, an idle wavefront of a last set) is found bit for bit, and an output element left
unwritten still holds the pattern.  The full shortcut map of the gather form holds the pattern at every pixel stride 2 does not read.  (The 3x3
stride-2 kernel has no such pixel: with pad 1, output row Ho - 1 of an even H reads input rows H - 3 .. H - 1, so its even-sized inputs are
dense like the odd-sized ones.)  The ops wrappers allocate their outputs themselves, so the guarded launches go through the C ABI with the
wrapper's own arguments, and every case is also run through the wrapper and compared bit for bit.

The largest operands (270 MB) are made on the device; the float64 reference runs there in chunks of 16 384 pixels.  RELNET_TEST_REPORT=<file>
appends the worst err / tolerance per form."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trunk_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32

WORST = {}                 # form -> (largest |got - ref64| / tolerance, where)


def _note(form, ratio, where):
    if form not in WORST or ratio > WORST[form][0]:
        WORST[form] = (ratio, where)


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, lib
    lib.load()
    try:
        yield ops, lib
    finally:
        path = os.environ.get('RELNET_TEST_REPORT')
        if path and WORST:
            with open(path, 'a') as f:
                for form, (ratio, where) in sorted(WORST.items()):
                    f.write('%-12s worst err / tolerance %.4f  at %s\n' % (form, ratio, where))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _place(t, parent=None, index=None):
    g = TC.guarded(tuple(t.shape), t.dtype, parent=parent, index=index)
    g.view.copy_(t)
    return g


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


_WEIGHTS = {}


def _weights(ops, mid):
    """Weights of a width, with their fragment images, made once."""
    if mid not in _WEIGHTS:
        w = TC.chain_weights(mid, 'cuda')
        w['w3f'] = ops.pack_w_frag(w['w3'])
        w['w1f'] = ops.pack_chain_w1(w['w1'])
        if mid == 64:
            w['wpf'] = ops.pack_w_frag(w['wp'])
        assert w['w3f'] is not None
        _WEIGHTS[mid] = w
    return _WEIGHTS[mid]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# chain kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------
class _Chain(object):
    """One (form, case): operands and outputs in guarded buffers, launched through the C ABI."""

    def __init__(self, rn, form, case):
        self.ops, self.lib = rn
        self.form, self.case, self.f = form, case, TC.FORMS[form]
        f = self.f
        self.mid, self.cout = f['mid'], 4 * f['mid']
        self.P = TC.case_pixels(form, case)
        self.w = _weights(self.ops, self.mid)
        o = TC.chain_operands(form, case, 'cuda')
        self.m2 = _place(o['m2'])
        if f['gather']:                            # the full map: every pixel stride 2 never reads keeps the NaN pattern
            B, H, W = case
            ev = (slice(None), slice(None, None, 2), slice(None, None, 2))
            self.sc = _place(o['x'][ev], parent=(B, H, W, self.cout), index=ev)
            self.sc_arg = self.sc.parent
        else:
            self.sc = _place(o['xin'] if f['proj'] else o['x'])
            self.sc_arg = self.sc.view
        del o
        self.keep = [(g, g.buf.clone()) for g in (self.m2, self.sc)]
        self.xn = TC.guarded(tuple(self.m2.view.shape[:-1]) + (self.cout,), BF16)
        self.m1 = TC.guarded(tuple(self.m2.view.shape), BF16) if f['reduce'] else None

    # flat [P, C] views
    def rows(self, g):
        return g.view.reshape(self.P, -1)

    def sc_rows(self):
        """The shortcut operand the P pixels read, [P, C] (a copy for the gather form)."""
        return self.sc.view.reshape(self.P, -1)

    def launch(self, xn=None, m1=None, m2=None, sc=None):
        """Into the guarded outputs (or the tensors given).  -> (x_next, mid1' | None) views."""
        f, w, lib = self.f, self.w, self.lib
        if xn is None:
            TC.fill_pattern(self.xn.buf)
            xn = self.xn.view
        if f['reduce'] and m1 is None:
            TC.fill_pattern(self.m1.buf)
            m1 = self.m1.view
        m2 = self.m2.view if m2 is None else m2
        sc = self.sc_arg if sc is None else sc
        red = (w['w1f'].data_ptr(), w['b1'].data_ptr(), m1.data_ptr()) if f['reduce'] else (0, 0, 0)
        if f['gather']:
            B, H, W = self.case
            lib.call('relnet_bottleneck_chain_s2', m2.data_ptr(), sc.data_ptr(), w['w3f'].data_ptr(), w['b3'].data_ptr(), xn.data_ptr(), B, H, W,
                     self.mid, _stream())
        elif f['proj']:
            lib.call('relnet_bottleneck_chain_proj', m2.data_ptr(), sc.data_ptr(), w['w3f'].data_ptr(), w['wpf'].data_ptr(), red[0],
                     w['b3p'].data_ptr(), red[1], xn.data_ptr(), red[2], self.P, self.mid, _stream())
        else:
            lib.call('relnet_bottleneck_chain', m2.data_ptr(), sc.data_ptr(), w['w3f'].data_ptr(), red[0], w['b3'].data_ptr(), red[1],
                     xn.data_ptr(), red[2], self.P, self.mid, _stream())
        return xn, m1

    def through_ops(self):
        """The same case through the ops wrapper (outputs allocated by it)."""
        f, w, ops = self.f, self.w, self.ops
        red = (w['w1f'], w['b1']) if f['reduce'] else (None, None)
        if f['gather']:
            return ops.bottleneck_chain_s2(self.m2.view, self.sc_arg, w['w3f'], w['b3']), None
        if f['proj']:
            return ops.bottleneck_chain_proj(self.m2.view, self.sc.view, w['w3f'], w['wpf'], red[0], w['b3p'], red[1])
        return ops.bottleneck_chain(self.m2.view, self.sc.view, w['w3f'], red[0], w['b3'], red[1])

    def check_guards(self, what, outputs=True):
        for g, keep in self.keep:
            assert _same_bits(g.buf, keep), (what, 'an input operand or its guard changed')
        if outputs:
            for name, g in (('x_next', self.xn), ('mid1_next', self.m1)):
                if g is not None:
                    assert TC.guards_intact(g.buf, g.view), (what, name, 'stored outside the output')
                    assert TC.is_pattern_free(g.view), (what, name, 'an output element was not written')
                    assert not torch.isnan(g.view).any(), (what, name, 'NaN in the output: an operand was read outside its view')


_CHAIN = [(form, case) for form in TC.FORMS for case in TC.chain_cases(form)]


def _cid(form, case):
    return '%s-%s' % (form, case if isinstance(case, int) else 'x'.join(str(v) for v in case))


@pytest.mark.parametrize('form,case', _CHAIN, ids=[_cid(*c) for c in _CHAIN])
def test_chain_case(rn, form, case):
    c = _Chain(rn, form, case)
    what = _cid(form, case)
    xn, m1 = c.launch()
    c.check_guards(what)
    okx, wx, okm, wm = TC.accept_chain(form, c.w, c.rows(c.m2), c.sc_rows(), c.rows(c.xn), None if m1 is None else c.rows(c.m1))
    print('%-16s P = %6d: worst err / tolerance  x_next %.4f  mid1 %.4f' % (what, c.P, wx, wm))
    assert okx, (what, 'x_next: worst |got - ref64| / tolerance', wx)
    assert okm, (what, 'mid1_next: worst |got - ref64| / tolerance', wm)
    _note(form + ' x_next', wx, what)
    if m1 is not None:
        _note(form + ' mid1', wm, what)
    first = (xn.clone(), None if m1 is None else m1.clone())
    xn, m1 = c.launch()                                                       # the same bits from a second launch
    c.check_guards(what)
    assert torch.equal(xn, first[0]) and (m1 is None or torch.equal(m1, first[1])), (what, 'second launch differs')
    oxn, om1 = c.through_ops()                                                # ... and from the wrapper
    assert oxn.shape == xn.shape and torch.equal(oxn, xn) and (m1 is None) == (om1 is None) and (m1 is None or torch.equal(om1, m1)), what


_EXPAND = [(e, P) for e in TC.TWO_PRODUCT_OF for P in TC.FORMS[e]['P'] if P in TC.FORMS[TC.TWO_PRODUCT_OF[e]]['P']]


@pytest.mark.parametrize('form,P', _EXPAND, ids=[_cid(*c) for c in _EXPAND])
def test_expand_only_form_gives_the_bits_of_the_two_product_form(rn, form, P):
    e = _Chain(rn, form, P)
    xe, _ = e.launch()
    r = _Chain(rn, TC.TWO_PRODUCT_OF[form], P)
    assert _same_bits(r.m2.view, e.m2.view) and _same_bits(r.sc.view, e.sc.view)          # (the forms of a width share their operands)
    xr, _ = r.launch()
    assert torch.equal(xe, xr), (form, P)


_INPLACE = [(form, P) for form in TC.DENSE_FORMS if not TC.FORMS[form]['proj'] for P in (33, TC.isolation_case(form))]


@pytest.mark.parametrize('form,P', _INPLACE, ids=[_cid(*c) for c in _INPLACE])
def test_in_place_over_the_shortcut_gives_the_same_bits(rn, form, P):
    c = _Chain(rn, form, P)
    what = _cid(form, P)
    xn, m1 = c.launch()
    m1 = None if m1 is None else m1.clone()
    xi = TC.guarded(tuple(c.sc.view.shape), BF16)                             # a second copy of the shortcut, overwritten
    xi.view.copy_(c.sc.view)
    got, m1i = c.launch(xn=xi.view, m1=None, sc=xi.view)
    assert torch.equal(got, xn) and (m1 is None or torch.equal(m1i, m1)), (what, 'in place differs')
    assert TC.guards_intact(xi.buf, xi.view), what
    c.check_guards(what, outputs=False)
    xo = c.sc.view.clone()                                                    # the wrapper's in-place form
    oxn, om1 = c.ops.bottleneck_chain(c.m2.view, xo, c.w['w3f'], c.w['w1f'] if c.f['reduce'] else None, c.w['b3'],
                                      c.w['b1'] if c.f['reduce'] else None, inplace=True)
    assert oxn.data_ptr() == xo.data_ptr() and torch.equal(oxn, xn) and (m1 is None or torch.equal(om1, m1))


_GATHER = [(form, shape) for form in TC.GATHER_FORMS for shape in TC.GATHER_SHAPES]


@pytest.mark.parametrize('form,shape', _GATHER, ids=[_cid(*c) for c in _GATHER])
def test_gather_form_equals_the_dense_form_at_the_even_pixels(rn, form, shape):
    """The dense expand-only kernel runs on the full map (whose other pixels hold the NaN pattern: its outputs there are NaN and are not looked
    at); the shortcut operand is bit-unchanged afterwards (check_guards compares the whole buffer)."""
    c = _Chain(rn, form, shape)
    what = _cid(form, shape)
    xn, _ = c.launch()
    c.check_guards(what)
    full_m2 = torch.zeros(tuple(c.sc_arg.shape[:-1]) + (c.mid,), device='cuda', dtype=BF16)
    full_m2[:, ::2, ::2] = c.m2.view
    dense = c.ops.bottleneck_chain(full_m2, c.sc_arg, c.w['w3f'], None, c.w['b3'], None)[0][:, ::2, ::2]
    assert dense.shape == xn.shape and torch.equal(xn, dense), what
    c.check_guards(what)


def _isolation_pixels(form, case):
    f = TC.FORMS[form]
    P = TC.case_pixels(form, case)
    return [0, 31, 32, P - 1, TC.second_iteration_pixel(f['plan'], P)]


@pytest.mark.parametrize('form', list(TC.FORMS))
def test_a_poisoned_pixel_changes_no_other_pixel(rn, form):
    """mid2 and the shortcut operand of ONE pixel q set to NaN, then to +inf: every other row of both outputs keeps the bits of the clean run, and
    row q is written (the ReLU maps NaN to 0, so its value is not prescribed)."""
    case = TC.isolation_case(form)
    c = _Chain(rn, form, case)
    xn, m1 = c.launch()
    clean = (xn.reshape(c.P, -1).clone(), None if m1 is None else m1.reshape(c.P, -1).clone())
    m2p = _place(c.m2.view)
    if c.f['gather']:
        B, H, W = case
        ev = (slice(None), slice(None, None, 2), slice(None, None, 2))
        scp = _place(c.sc.view, parent=(B, H, W, c.cout), index=ev)
        sc_arg = scp.parent
    else:
        scp = _place(c.sc.view)
        sc_arg = scp.view
    m2r = m2p.view.view(c.P, -1)
    scr = None if c.f['gather'] else scp.view.view(c.P, -1)
    for q in _isolation_pixels(form, case):
        for poison in (float('nan'), float('inf')):
            what = (form, case, 'pixel', q, poison)
            m2r[q] = poison
            if c.f['gather']:
                Ho, Wo = TC.out_hw(H, W)
                b, r = divmod(q, Ho * Wo)
                scp.view[b, r // Wo, r % Wo] = poison
            else:
                scr[q] = poison
            xn, m1 = c.launch(m2=m2p.view, sc=sc_arg)
            for name, g, ref in (('x_next', c.xn, clean[0]), ('mid1_next', c.m1, clean[1])):
                if g is None:
                    continue
                got = g.view.reshape(c.P, -1)
                assert torch.equal(got[:q], ref[:q]) and torch.equal(got[q + 1:], ref[q + 1:]), (what, name, 'another pixel changed')
                assert TC.is_pattern_free(got[q:q + 1]), (what, name, 'the row of the poisoned pixel was not written')
                assert TC.guards_intact(g.buf, g.view), (what, name)
            m2r[q] = c.m2.view.view(c.P, -1)[q]                                # restore
            if c.f['gather']:
                scp.view[b, r // Wo, r % Wo] = c.sc.view[b, r // Wo, r % Wo]
            else:
                scr[q] = c.sc.view[q]
    assert _same_bits(m2p.view, c.m2.view) and _same_bits(scp.view, c.sc.view)


def test_chain_entry_points_refuse_what_they_do_not_support(rn):
    """Each call returns an error before any launch: the outputs keep the guard pattern everywhere."""
    ops, lib = rn
    w = _weights(ops, 64)
    w512 = _weights(ops, 512)
    P = 40
    m2 = torch.zeros(P, 512, device='cuda', dtype=BF16)
    x = torch.zeros(P, 2048, device='cuda', dtype=BF16)
    xn, m1 = TC.guarded((P, 2048), BF16), TC.guarded((P, 512), BF16)
    p = lambda t: t.data_ptr()

    def chain(P_, mid, w1f, b1, m1_, w3f=w['w3f'], b3=w['b3']):
        lib.call('relnet_bottleneck_chain', p(m2), p(x), p(w3f), w1f, p(b3), b1, p(xn.view), m1_, P_, mid, _stream())

    def untouched():
        torch.cuda.synchronize()
        return TC.guards_intact(xn.buf, xn.buf[:0]) and TC.guards_intact(m1.buf, m1.buf[:0])
    for args in ((0, 64, p(w['w1f']), p(w['b1']), p(m1.view)),                  # P = 0
                 (P, 96, p(w['w1f']), p(w['b1']), p(m1.view)),                  # mid = 96
                 (P, 96, 0, 0, 0),
                 (P, 64, p(w['w1f']), 0, p(m1.view)),                           # w1f without b1
                 (P, 64, p(w['w1f']), 0, 0),
                 (1 << 23, 64, 0, 0, 0),                                        # P * 8 * mid = 2^32 (the count only: refused before anything is read)
                 (1 << 21, 256, p(w['w1f']), p(w['b1']), p(m1.view))):
        with pytest.raises(lib.RelnetError):
            chain(*args)
        assert untouched(), args
    with pytest.raises(lib.RelnetError):                                       # mid = 512 with a reduce weight
        chain(P, 512, p(w['w1f']), p(w['b1']), p(m1.view), w3f=w512['w3f'], b3=w512['b3'])
    assert untouched()
    with pytest.raises(lib.RelnetError):                                       # the gather form is never in place
        lib.call('relnet_bottleneck_chain_s2', p(m2), p(xn.view), p(w['w3f']), p(w['b3']), p(xn.view), 1, 8, 12, 64, _stream())
    assert untouched()
    with pytest.raises(lib.RelnetError):
        lib.call('relnet_bottleneck_chain_s2', p(m2), p(x), p(w['w3f']), p(w['b3']), p(xn.view), 1, 8, 12, 96, _stream())
    assert untouched()
    with pytest.raises(lib.RelnetError):                                       # the full map at 4 GiB
        lib.call('relnet_bottleneck_chain_s2', p(m2), p(x), p(w['w3f']), p(w['b3']), p(xn.view), 2, 2048, 2048, 64, _stream())
    assert untouched()
    for args in ((0, 64), (P, 128), (1 << 23, 64)):                             # the projection form: P = 0, mid = 128, 4 GiB
        with pytest.raises(lib.RelnetError):
            lib.call('relnet_bottleneck_chain_proj', p(m2), p(m2), p(w['w3f']), p(w['wpf']), 0, p(w['b3p']), 0, p(xn.view), 0, args[0], args[1],
                     _stream())
        assert untouched(), args


# ---------------------------------------------------------------------------------------------------------------------------------------------
# halo 3x3 kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _halo_launch(lib, entry, x, wf, b, relu, out, shape):
    TC.fill_pattern(out.buf)
    lib.call(entry, x.data_ptr(), wf.data_ptr(), b.data_ptr(), int(relu), out.view.data_ptr(), shape[0], shape[1], shape[2], _stream())
    return out.view


def _halo_case(rn, shape, stride):
    ops, lib = rn
    B, H, W = shape
    x, w, b = TC.halo_operands(shape, 'cuda')
    xg = _place(x)
    keep = xg.buf.clone()
    wf = ops.pack_w_frag(ops.pack_conv_weight(w, BF16, 'cuda'), panel_only=False)
    Ho, Wo = (H, W) if stride == 1 else TC.out_hw(H, W)
    out = TC.guarded((B, Ho, Wo, 64), BF16)
    entry, wrapper = ('relnet_conv3x3_c64', ops.conv3x3_halo) if stride == 1 else ('relnet_conv3x3_c64_s2', ops.conv3x3_halo_s2)
    pre, mag = TC.halo_ref(xg.view, w, b, stride)
    got = {}
    for relu in (True, False):
        what = ('halo' if stride == 1 else 'halo_s2', shape, 'relu', relu)
        y = _halo_launch(lib, entry, xg.view, wf, b, relu, out, shape)
        assert TC.guards_intact(out.buf, out.view), (what, 'stored outside the output')
        assert TC.is_pattern_free(y), (what, 'an output element was not written')
        assert not torch.isnan(y).any(), (what, 'NaN in the output: the input was read outside its view')
        assert _same_bits(xg.buf, keep), (what, 'the input or its guard changed')
        ok, worst = TC.accept(y, pre.clamp_min(0) if relu else pre, pre, mag, 576, bf16_out=True, relu=relu)
        print('%s: worst err / tolerance %.4f' % (what, worst))
        assert ok, (what, 'worst |got - ref64| / tolerance', worst)
        _note(what[0], worst, what)
        got[relu] = y.clone()
        assert torch.equal(_halo_launch(lib, entry, xg.view, wf, b, relu, out, shape), got[relu]), (what, 'second launch differs')
        assert torch.equal(wrapper(xg.view, wf, b, relu=relu), got[relu]), (what, 'the wrapper differs')
    return xg, wf, b, got


@pytest.mark.parametrize('shape', TC.HALO_SHAPES, ids=['%dx%dx%d' % s for s in TC.HALO_SHAPES])
def test_halo_dense_case(rn, shape):
    _halo_case(rn, shape, 1)


@pytest.mark.parametrize('shape', TC.HALO_S2_SHAPES, ids=['%dx%dx%d' % s for s in TC.HALO_S2_SHAPES])
def test_halo_stride2_case(rn, shape):
    ops, lib = rn
    xg, wf, b, got = _halo_case(rn, shape, 2)
    for relu in (True, False):                                                # the dense kernel at the even pixels, bit for bit
        assert torch.equal(ops.conv3x3_halo(xg.view, wf, b, relu=relu)[:, ::2, ::2], got[relu]), (shape, relu)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fused stem
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', TC.STEM_SIZES, ids=['%dx%d' % s for s in TC.STEM_SIZES])
def test_stem_fused_case(rn, size):
    ops, lib = rn
    H, W = size
    img, u8, w, b = TC.stem_operands(size, 'cuda')
    w256 = ops.pack_stem_weight(w)
    wb = w.to(BF16).double()
    Hc, Wc, Hp, Wp = TC.stem_hw(H, W)
    out = TC.guarded((2, Hp, Wp, 64), BF16)
    im_info = torch.tensor(TC.stem_extents(H, W), device='cuda', dtype=F32)
    assert float(im_info[1, 0]) < H and float(im_info[1, 1]) < W
    u8f = ops.image_transform_u8(u8, TC.STEM_MEANS, im_info)                  # the fp32 tensor the uint8 kernel is documented to equal
    assert float(u8f[1, :, int(im_info[1, 0]):].abs().max()) == 0 and float(u8f[1, :, :, int(im_info[1, 1]):].abs().max()) == 0

    def fused(data, info=None):
        TC.fill_pattern(out.buf)
        if data.dtype == torch.uint8:
            lib.call('relnet_stem_fused_u8', data.data_ptr(), info.data_ptr(), *[float(v) for v in TC.STEM_MEANS], w256.data_ptr(), b.data_ptr(),
                     out.view.data_ptr(), 2, H, W, _stream())
        else:
            lib.call('relnet_stem_fused', data.data_ptr(), lib.BF16 if data.dtype == BF16 else lib.F32, w256.data_ptr(), b.data_ptr(),
                     out.view.data_ptr(), 2, H, W, _stream())
        what = (size, str(data.dtype))
        assert TC.guards_intact(out.buf, out.view), (what, 'stored outside the output')
        assert TC.is_pattern_free(out.view), (what, 'an output element was not written')
        return out.view.clone()

    def three_launches(x):
        return ops.stem_bias_relu_pool(ops.stem_conv7(x, w256, b, relu=True), torch.zeros(64, device='cuda'))

    for name, x, runs in (('fp32', img, [lambda: fused(img), lambda: fused(img.to(BF16))]),
                          ('uint8', u8f, [lambda: fused(u8, im_info), lambda: fused(u8f)])):
        want, tol = TC.stem_ref(x.to(BF16).double(), wb, b)
        assert tuple(want.shape) == (2, Hp, Wp, 64)
        three = three_launches(x)
        for i, run in enumerate(runs):
            got = run()
            what = (size, name, i)
            assert got.shape == three.shape and torch.equal(got, three), (what, 'differs from the three-launch stem')
            ok, worst = TC.stem_accept(got, want, tol)
            print('%s: worst err / tolerance %.4f' % (what, worst))
            assert ok, (what, 'worst |got - ref64| / tolerance', worst)
            _note('stem ' + name, worst, what)
    assert torch.equal(ops.stem_fused(img, w256, b), fused(img))              # the wrappers
    assert torch.equal(ops.stem_fused(u8, w256, b, im_info, TC.STEM_MEANS), fused(u8, im_info))
