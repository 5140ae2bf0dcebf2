"""The reference, bound and guards of tests/gemm_cases.py checked on the CPU, so that what tests/test_gpu_gemm_edges.py relies on is shown here:
  * the loop-definition convolution equals torch.nn.functional.conv2d in float64 (geometry, R != S, free pad, stride, dilation);
  * two correct fp32 evaluations (a library matmul and a strictly sequential fmaf chain) stay inside the bound, with the headroom printed;
  * the acceptance function REJECTS the errors a subtly wrong kernel makes (a dropped / repeated k-slab, a tap read from the next row, an ignored
    image boundary, swapped filter rows, a store into the pad columns), and a single missing product on most elements."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as GC  # noqa: E402

CONVS = GC.CONV_CASES + GC.CONV_F32_CASES
_ids = lambda cases: [c['id'] for c in cases]


def _slab(case):
    return 16 if case.get('f32_in') else 64            # k-slab of the kernel that runs the case


def _round_out(t, odt):
    return t.to(torch.float32).to(odt)


@pytest.mark.parametrize('case', CONVS, ids=_ids(CONVS))
def test_loop_reference_equals_conv2d(case):
    o = GC.operands(case)
    odt = case['odts'][0]
    pre, mag = GC.ref64(case, o, odt)
    w = o['w'].double().reshape(case['Cout'], case['R'], case['S'], case['Cin']).permute(0, 3, 1, 2)
    res = GC.resid_for(o, odt) if case['relu'] != 2 else None
    for (x, ww, b, r, mine) in ((o['a'].double(), w, o['bias'].double(), res, pre),
                                (o['a'].double().abs(), w.abs(), o['bias'].double().abs(), None if res is None else res.abs(), mag)):
        want = F.conv2d(x.permute(0, 3, 1, 2), ww, b, stride=case['stride'], padding=case['pad'], dilation=case['dil']).permute(0, 2, 3, 1)
        assert want.shape == mine.shape == o['oshape']
        if r is not None:
            want = want + r.double()
        assert (mine - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    # ... and the implicit-GEMM matrix used below for the fp32 evaluations is the same convolution
    col = GC.im2col(case, o['a'].double()) @ o['w'].double().t() + o['bias'].double()
    if res is not None:
        col = col + res.double().reshape(col.shape)
    assert (col.reshape(pre.shape) - pre).abs().max().item() <= 1e-12 * pre.abs().max().item()


def _gemm_views(case, o):
    """-> (A [batch, M, K], W [batch, N, K]) float32, convolutions as their implicit GEMM."""
    a = GC.im2col(case, o['a'])
    w = o['w']
    nb = case['batch'] if case['kind'] == 'gemm' else 1
    a = a if a.dim() == 3 else a.expand(nb, -1, -1)
    w = w if w.dim() == 3 else w.expand(nb, -1, -1)
    return a, w


def _tail32(case, o, odt, acc):
    """bias and shortcut added in fp32, the way a kernel's epilogue does."""
    acc = acc.reshape(o['oshape'])
    if o['bias'] is not None:
        acc = acc + (o['bias'][:, None] if (case['kind'] == 'gemm' and case['bias'] == 2) else o['bias'])
    if case['resid'] and case['relu'] != 2:
        acc = acc + GC.resid_for(o, odt)
    return acc


@pytest.mark.parametrize('case', GC.ALL_CASES, ids=_ids(GC.ALL_CASES))
def test_fp32_evaluations_stay_inside_the_bound(case):
    o = GC.operands(case)
    odt = torch.float32
    pre, mag = GC.ref64(case, o, odt)
    a, w = _gemm_views(case, o)
    bnd = GC.bound(mag, case['K'])
    assert (bnd > 0).any()
    worst = {}
    lib = torch.matmul(a, w.transpose(1, 2))
    chain = torch.zeros_like(lib)
    for k in range(case['K']):                         # strictly sequential fmaf chain: round(acc + a w) per k (the product of two fp32 is exact in float64)
        chain = (chain.double() + a[:, :, k, None].double() * w[:, None, :, k].double()).float()
    for name, acc in (('matmul', lib), ('chain', chain)):
        got = _tail32(case, o, odt, acc).double()
        ratio = ((got - pre).abs() / bnd.clamp_min(1e-300))[bnd > 0]
        assert ((got - pre).abs() <= bnd).all(), (case['id'], name, ratio.max().item())
        worst[name] = ratio.max().item()
    print('%-16s M x N x K = %d x %d x %d: worst err / bound  matmul %.4f  chain %.4f' % (case['id'], case['M'], case['N'], case['K'], worst['matmul'], worst['chain']))
    assert max(worst.values()) <= 1.0


def _mutations(case, o, odt, pre):
    """name -> mutated pre-activation (float64), for every mutation that applies to the case."""
    K, sl = case['K'], _slab(case)
    a, w = _gemm_views(case, o)
    a, w = a.double(), w.double()
    out = {}

    def part(k0, k1):
        return (a[:, :, k0:k1] @ w[:, :, k0:k1].transpose(1, 2)).reshape(pre.shape)
    live = [k0 for k0 in range(0, K, sl) if bool(a[:, :, k0:k0 + sl].any())]      # (a slab whose taps all lie in the padding multiplies zeros: nothing to get wrong)
    mid = min(live, key=lambda k0: abs(k0 - (K // sl) // 2 * sl))
    out['k-slab dropped'] = pre - part(mid, mid + sl)
    out['last k-slab twice'] = pre + part(live[-1], live[-1] + sl)
    # a fixed pair in the middle; a ReLU or a mask that zeroes BOTH columns in every row (possible where the output is one row) makes a swap there
    # no error at all, so the pair moves on to the next one of which some entry survives the activation
    act = GC.activate(case, o, odt, pre)
    N = case['N']
    n = next(c % (N - 1) for c in range(N // 2, N // 2 + N - 1) if bool(((act[..., c % (N - 1)] != 0) | (act[..., c % (N - 1) + 1] != 0)).any()))
    sw = pre.clone()
    sw[..., n], sw[..., n + 1] = pre[..., n + 1], pre[..., n]
    out['W rows n, n + 1 swapped'] = sw
    if case['kind'] == 'conv':
        tap = (case['R'] // 2, case['S'] // 2)
        out['tap from the next row'] = GC.ref64(case, o, odt, tap_row_shift=tap)[0]
        if case['B'] > 1 and case['pad'] > 0:          # (without padding, or with one image, there is no boundary to ignore)
            out['image boundary ignored'] = GC.ref64(case, o, odt, ignore_image_boundary=True)[0]
    return out


@pytest.mark.parametrize('case', GC.ALL_CASES, ids=_ids(GC.ALL_CASES))
def test_acceptance_rejects_the_errors_of_a_wrong_kernel(case):
    o = GC.operands(case)
    for odt in case['odts']:
        bf = odt == torch.bfloat16
        pre, mag = GC.ref64(case, o, odt)
        want = GC.activate(case, o, odt, pre)
        ok, worst = GC.accept(_round_out(want, odt), want, pre, mag, case['K'], bf, case['relu'])
        assert ok and worst <= 1.0, (case['id'], odt, 'the correctly rounded reference itself must pass', worst)
        for name, mpre in _mutations(case, o, odt, pre).items():
            assert not torch.equal(mpre, pre), (case['id'], name, 'mutation changed nothing')
            got = _round_out(GC.activate(case, o, odt, mpre), odt)
            ok, worst = GC.accept(got, want, pre, mag, case['K'], bf, case['relu'])
            assert not ok, (case['id'], str(odt), name, 'accepted', worst)
        # NaN (an operand read from outside its view) is rejected too
        got = _round_out(want, odt).clone()
        got.view(-1)[got.numel() // 2] = float('nan')
        assert not GC.accept(got, want, pre, mag, case['K'], bf, case['relu'])[0]


@pytest.mark.parametrize('case', GC.ALL_CASES, ids=_ids(GC.ALL_CASES))
def test_guards_find_a_store_outside_the_view(case):
    """`pad columns written`: the output of every case lives in a guarded buffer; one element stored behind a row's N columns (a pad column where
    ldc > N, else the next row's guard), in front of the view or behind it is found, and for the zero-initialised outputs the pad columns are
    compared with zero exactly."""
    o = GC.operands(case)
    odt = case['odts'][0]
    shape = tuple(o['oshape'])
    N = shape[-1]
    ldc = case.get('ldc') or (N + 64 if case.get('views') else N)
    parent = shape[:-1] + (ldc,)
    g = GC.guarded(parent if case.get('zero_out') else shape, odt, parent=parent, index=None if case.get('zero_out') else (Ellipsis, slice(0, N)),
                   device='cpu')
    assert torch.isnan(g.view.float()).all() and GC.guards_intact(g.buf, g.view)
    g.view.zero_()
    assert GC.guards_intact(g.buf, g.view) and GC.is_pattern_free(g.view)
    first = g.view.storage_offset()
    last = first + sum((s - 1) * st for s, st in zip(g.view.shape, g.view.stride()))
    spots = [first - 1, last + 1, first - 256 * ldc, last + 256 * ldc]
    if ldc > N and not case.get('zero_out'):
        spots.append(first + N)                        # a pad column of the first row
    for p in spots:
        keep = g.buf[p].clone()
        g.buf[p] = 1.0
        assert not GC.guards_intact(g.buf, g.view), (case['id'], p - first)
        g.buf[p] = keep
        assert GC.guards_intact(g.buf, g.view)
    if case.get('zero_out'):
        g.view[..., N:] = 0
        g.view[..., :N] = 1
        assert bool((g.view[..., N:] == 0).all())
        g.view[..., N] = 1e-30                         # the smallest store into a pad column
        assert not bool((g.view[..., N:] == 0).all())


FOUR_SHAPES = ((33, 72, 64), (65, 89, 192), (257, 300, 320), (31, 264, 576))


def _single_product_rejection(a, w, pre, mag, K, k):
    """Fraction of fp32-output elements on which dropping the single product a[m, k] w[n, k] is rejected."""
    delta = a[..., :, k, None].double() * w[..., None, :, k].double()
    got = (pre - delta.reshape(pre.shape)).float()
    good, _ = GC.accept_map(got, pre, pre, mag, K, False)
    return 1.0 - good.double().mean().item()


@pytest.mark.parametrize('M,N,K', FOUR_SHAPES)
def test_one_dropped_product_is_rejected_on_most_elements(M, N, K):
    case = GC._g('S%dx%dx%d' % (M, N, K), M, N, K)
    o = GC.operands(case)
    pre, mag = GC.ref64(case, o, torch.float32)
    # (the four shapes only: the bound grows as K^1.5 and one product shrinks as K^-0.5, so the fraction falls with K_total -- about half at the
    # K_total = 2304 of the largest convolution case -- and an output pixel whose tap lies in the padding has no product to lose)
    frac = min(_single_product_rejection(o['a'], o['w'], pre, mag, K, k) for k in (0, K // 2, K - 1))
    print('%d x %d x %d: one dropped product rejected on %.1f %% of the fp32-output elements' % (M, N, K, 100 * frac))
    assert frac >= 0.85
