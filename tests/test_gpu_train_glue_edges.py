"""The training step's small kernels one by one at their edges (tests/train_glue_cases.py): csrc/losses.hip (softmax_output_ex with per-image
normalisation groups, smooth_l1_loss, nms_loss), csrc/lnms_train.hip (pad_params, residual_relu, cond_multi, cond_bwd, take_bwd, softmax_bwd,
gather_bias), relnet_lnms_embed, and csrc/train_ops.hip (reduce_scalar, wgrad_accumulate, sgd_update, relation_bwd_pack, relu_bwd) -- each against a
float64 reference written from its definition, per element, within the bound derived in train_glue_cases (bit for bit where the kernel only moves
or rounds data).  No element is left out of a comparison.

Guarded buffers (gemm_cases.guarded): every operand and output is a view in the middle of a NaN-pattern-filled parent, outputs start as pattern.
After every launch: nothing outside the views changed, no input changed, the documented output region holds no pattern, the documented untouched
region (pad rows / columns, rows of other images, the neighbours of a scalar slot) is still pattern or still its old value, bit for bit.
Integer rank lists, which kernels use as indices, sit between zeros instead (a stray read must not become a wild address).
Arguments an entry point documents as rejected return an error before anything is launched: the outputs are still all pattern.

Every test prints its worst err / bound under the kernel's name; RELNET_TEST_REPORT=<file> appends the worst per kernel."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as GC  # noqa: E402
import train_glue_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
_ids = lambda cs: [c['id'] for c in cs]
WORST = {}                 # kernel / output -> [largest err / bound, where, launches]


def _note(kernel, ratio, where):
    print('%-28s %-32s worst err / bound %.4f' % (kernel, where, ratio))
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
                    f.write('%-28s %4d launches, worst err / bound %.4f  at %s\n' % (k, n, ratio, where))


class Box(object):
    """The guarded operands of one launch."""

    def __init__(self):
        self.ins, self.outs, self.ranks = [], [], []

    def inp(self, t, parent=None, index=None):
        g = GC.guarded(tuple(t.shape), t.dtype, parent, index)
        g.view.copy_(t)
        self.ins.append((g, TC.bits(g.view).clone()))
        return g.view

    def out(self, shape, dtype, parent=None, index=None):
        g = GC.guarded(tuple(shape), dtype, parent, index)
        self.outs.append(g)
        return g.view

    def inout(self, t, parent=None, index=None):
        g = GC.guarded(tuple(t.shape), t.dtype, parent, index)
        g.view.copy_(t)
        self.outs.append(g)
        return g.view

    def rank(self, t):
        buf = torch.zeros(t.numel() + 2 * 4096, dtype=I32, device='cuda')
        v = buf[4096:4096 + t.numel()].view(t.shape)
        v.copy_(t)
        self.ranks.append((buf, buf.clone()))
        return v

    def check(self):
        torch.cuda.synchronize()
        for g, snap in self.ins:
            assert GC.guards_intact(g.buf, g.view), 'a store next to an input'
            assert bool((TC.bits(g.view) == snap).all()), 'an input changed'
        for g in self.outs:
            assert GC.guards_intact(g.buf, g.view), 'a store outside the output'
        for buf, snap in self.ranks:
            assert torch.equal(buf, snap), 'the rank list changed'

    def untouched(self):
        """A rejected call: every output is still all pattern."""
        torch.cuda.synchronize()
        for g in self.outs:
            assert bool((TC.bits(g.buf) == GC._PATTERN[g.buf.element_size()]).all()), 'a rejected call wrote its output'


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _rejected(rn, box, name, *args):
    lib, ops, _ = rn
    with pytest.raises(lib.RelnetError):
        lib.call(name, *(args + (ops._stream(),)))
    box.untouched()


def _cpu(t):
    return t.detach().cpu()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# csrc/losses.hip
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', TC.SOFTMAX_CASES, ids=_ids(TC.SOFTMAX_CASES))
def test_softmax_output_groups(rn, case):
    lib, ops, _ = rn
    data, label = TC.softmax_operands(case)
    prob_ref, grad_ref = TC.softmax_ref64(case, data, label)
    G, ng = TC.softmax_groups(case)
    bx = Box()
    d = bx.inp(data)
    l = bx.inp(label) if label is not None else None
    prob = bx.out(case['shape'], F32)
    grad = bx.out(case['shape'], F32) if label is not None else None
    cnt = bx.out((ng,), I32) if label is not None else None
    lib.call('relnet_softmax_output_ex', d.data_ptr(), _ptr(l), prob.data_ptr(), _ptr(grad), _ptr(cnt), case['outer'], case['C'], case['inner'],
             case['use_ignore'], case['ignore_label'], case['grad_scale'], case['group'], ops._stream())
    bx.check()
    assert GC.is_pattern_free(prob)
    rp = TC.close_ratio(_cpu(prob), prob_ref)
    rs = TC.prob_rows_sum_to_one(case, _cpu(prob))
    _note('softmax_output prob', rp, case['id'])
    _note('softmax_output rowsum', rs, case['id'])
    assert rp <= 1.0 and rs <= 1.0
    if label is None:
        return
    assert GC.is_pattern_free(grad) and GC.is_pattern_free(cnt)
    valid = TC.softmax_valid(case, label)
    assert torch.equal(_cpu(cnt).long(), valid.reshape(ng, G).sum(1))
    rg = TC.close_ratio(_cpu(grad), grad_ref)
    _note('softmax_output grad', rg, case['id'])
    assert rg <= 1.0
    g2 = TC.softmax_to2d(case, _cpu(grad))
    assert bool((TC.bits(g2[~valid]) == 0).all())                        # ignored rows: exact (+0) zeros
    if case['special'] == 'all_ignored':
        assert float(g2.reshape(ng, G, -1)[ng // 2].abs().max()) == 0.0


def test_softmax_output_wrapper_passes_the_group_and_rejects_a_ragged_one(rn):
    """losses.softmax_output(group=...) is the call train.py makes; total % group != 0 is refused before anything is launched."""
    lib, ops, _ = rn
    from relnet_amd import losses
    case = [c for c in TC.SOFTMAX_CASES if c['id'] == 'S616x81-g308'][0]
    data, label = TC.softmax_operands(case)
    prob, grad = losses.softmax_output(data.cuda(), label.cuda(), use_ignore=True, ignore_label=case['ignore_label'], grad_scale=case['grad_scale'],
                                       group=308)
    prob_ref, grad_ref = TC.softmax_ref64(case, data, label)
    assert TC.close_ratio(_cpu(prob), prob_ref) <= 1.0 and TC.close_ratio(_cpu(grad), grad_ref) <= 1.0
    bx = Box()
    d, l = bx.inp(data), bx.inp(label)
    prob, grad, cnt = bx.out(case['shape'], F32), bx.out(case['shape'], F32), bx.out((616,), I32)
    _rejected(rn, bx, 'relnet_softmax_output_ex', d.data_ptr(), l.data_ptr(), prob.data_ptr(), grad.data_ptr(), cnt.data_ptr(), 616, 81, 1, 1, 255.0, 1.0, 300)


@pytest.mark.parametrize('case', TC.SMOOTH_L1_CASES, ids=_ids(TC.SMOOTH_L1_CASES))
def test_smooth_l1_loss_edges(rn, case):
    lib, ops, _ = rn
    pred, target, weight = TC.smooth_l1_operands(case)
    loss_ref, grad_ref = TC.smooth_l1_ref64(case, pred, target, weight)
    n = case['n']
    res = {}
    for what in ('both', 'loss', 'grad'):
        bx = Box()
        p, t = bx.inp(pred), bx.inp(target)
        w = bx.inp(weight) if weight is not None else None
        loss = bx.out((n,), F32) if what != 'grad' else None
        grad = bx.out((n,), F32) if what != 'loss' else None
        lib.call('relnet_smooth_l1_loss', p.data_ptr(), t.data_ptr(), _ptr(w), _ptr(loss), _ptr(grad), n, case['sigma'], case['grad_scale'], ops._stream())
        bx.check()
        for o in (loss, grad):
            assert o is None or GC.is_pattern_free(o)
        res[what] = (loss, grad)
    rl, rg = TC.close_ratio(_cpu(res['both'][0]), loss_ref), TC.close_ratio(_cpu(res['both'][1]), grad_ref)
    _note('smooth_l1_loss loss', rl, case['id'])
    _note('smooth_l1_loss grad', rg, case['id'])
    assert rl <= 1.0 and rg <= 1.0
    assert TC.same_bits(res['loss'][0], res['both'][0]) and TC.same_bits(res['grad'][1], res['both'][1])


@pytest.mark.parametrize('case', TC.NMS_LOSS_CASES, ids=_ids(TC.NMS_LOSS_CASES))
def test_nms_loss_edges(rn, case):
    lib, ops, _ = rn
    score, target = TC.nms_loss_operands(case)
    refs = TC.nms_loss_ref64(case, score, target)
    assert all(bool(torch.isfinite(r).all()) for r in refs)
    n = case['n']
    k = case['loss_scale'] / float(case['first_n'] * case['num_thresh'])
    res = {}
    for what in ('all', 'pos', 'neg', 'grad'):
        bx = Box()
        s, t = bx.inp(score), bx.inp(target)
        outs = [bx.out((n,), F32) if what in ('all', name) else None for name in ('pos', 'neg', 'grad')]
        lib.call('relnet_nms_loss', s.data_ptr(), t.data_ptr(), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), n, case['eps'], k, case['pos_scale'], ops._stream())
        bx.check()
        assert all(o is None or GC.is_pattern_free(o) for o in outs)
        res[what] = outs
    for i, name in enumerate(('pos', 'neg', 'grad')):
        r = TC.rel_ratio(_cpu(res['all'][i]), refs[i])
        _note('nms_loss ' + name, r, case['id'])
        assert r <= 1.0
        assert TC.same_bits(res[name][i], res['all'][i])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# csrc/lnms_train.hip
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _pad_params_box(T):
    o = TC.pad_params_operands(T)
    bx = Box()
    ins = [bx.inp(o[k]) for k in ('wo', 'bo', 'wl', 'bl')]
    sl = slice(None)
    outs = [bx.out((16, 8, 128), BF16, parent=(16, 64, 128), index=(sl, slice(0, 8))), bx.out((16, 8), F32, parent=(16, 64), index=(sl, slice(0, 8))),
            bx.out((min(T, 64), 128), BF16, parent=(64, 128), index=(slice(0, min(T, 64)),)), bx.out((min(T, 64),), F32, parent=(64,), index=(slice(0, min(T, 64)),))]
    return o, bx, ins, outs


@pytest.mark.parametrize('T', TC.PAD_PARAMS_T)
def test_lnms_pad_params_writes_the_real_rows_only(rn, T):
    """Bit-exact against slicing; the 56 pad rows per head of wout_pad / bout_pad and rows T .. 63 of wl_pad / bl_pad keep the pattern (they are part
    of the guard of the strided output views)."""
    lib, ops, _ = rn
    o, bx, ins, outs = _pad_params_box(T)
    lib.call('relnet_lnms_pad_params', *([t.data_ptr() for t in ins] + [t.data_ptr() for t in outs] + [T, ops._stream()]))
    bx.check()
    ref = TC.pad_params_ref(o, T)
    for got, key in zip(outs, ('wout', 'bout', 'wl', 'bl')):
        assert TC.same_bits(_cpu(got), ref[key].contiguous()), key
    _note('lnms_pad_params', 0.0, 'T=%d bit-exact' % T)


def test_lnms_pad_params_rejects_more_than_64_thresholds(rn):
    o, bx, ins, outs = _pad_params_box(65)
    _rejected(rn, bx, 'relnet_lnms_pad_params', *([t.data_ptr() for t in ins] + [t.data_ptr() for t in outs] + [65]))


@pytest.mark.parametrize('rows', TC.RESIDUAL_ROWS)
def test_lnms_residual_relu_bit_exact(rn, rows):
    """relu((x + att8) rounded to bf16), bit for bit, with NaN pattern in the 56 columns per head the kernel must not read; -0.0, bf16 ties and
    subnormal sums in the last row."""
    lib, ops, _ = rn
    x, att8 = TC.residual_operands(rows)
    bx = Box()
    sl = slice(None)
    xv = bx.inp(x)
    av = bx.inp(att8, parent=(rows, 16, 64), index=(sl, sl, slice(0, 8)))
    out = bx.out((rows, 128), BF16)
    lib.call('relnet_lnms_residual_relu', av.data_ptr(), xv.data_ptr(), out.data_ptr(), rows, ops._stream())
    bx.check()
    assert GC.is_pattern_free(out)
    want = torch.relu((xv.float() + av.reshape(rows, 128).float()).bfloat16())            # the expression itself, on the device
    k = len(TC.RESIDUAL_SPECIALS)
    print('residual_relu specials: kernel %s\n                        torch  %s' % (TC.bits(out[rows - 1, :k]).tolist(), TC.bits(want[rows - 1, :k]).tolist()))
    assert torch.equal(_cpu(out), TC.residual_ref(x, att8))                               # values (the CPU evaluation of the same expression)
    assert TC.same_bits(out, want)
    _note('lnms_residual_relu', 0.0, 'rows=%d bit-exact' % rows)


def test_lnms_residual_relu_rejects_a_misaligned_operand(rn):
    bx = Box()
    x, att8 = TC.residual_operands(16)
    sl = slice(None)
    av = bx.inp(att8, parent=(16, 16, 64), index=(sl, sl, slice(0, 8)))
    xv = bx.inp(x.reshape(-1), parent=(16 * 128 + 1,), index=(slice(1, None),))            # 2 bytes off a 16-byte boundary
    out = bx.out((16, 128), BF16)
    _rejected(rn, bx, 'relnet_lnms_residual_relu', av.data_ptr(), xv.data_ptr(), out.data_ptr(), 16)


@pytest.mark.parametrize('case', TC.COND_CASES, ids=_ids(TC.COND_CASES))
def test_lnms_cond_multi_and_cond_bwd(rn, case):
    lib, ops, _ = rn
    B, C, F, T, ld = (case[k] for k in ('B', 'C', 'F', 'T', 'ld'))
    rows = B * C * F
    o = TC.cond_operands(case)
    cond_ref, multi_ref, xt = TC.cond_ref64(case, o['logit_buf'], o['score'])
    bx = Box()
    sl = slice(None)
    logit = bx.inp(o['logit_buf'][:, :T], parent=(rows, ld), index=(sl, slice(0, T)))      # the pad columns of the rows hold the NaN pattern
    score = bx.inp(o['score'])
    cond, multi = bx.out((B, F, C, T), F32), bx.out((B, F, C, T), F32)
    lib.call('relnet_lnms_cond_multi', logit.data_ptr(), ld, score.data_ptr(), cond.data_ptr(), multi.data_ptr(), B, C, F, T, ops._stream())
    bx.check()
    assert GC.is_pattern_free(cond) and GC.is_pattern_free(multi)
    rc = TC.worst(_cpu(cond), cond_ref, TC.cond_bound(xt))
    rm = TC.worst(_cpu(multi), multi_ref, TC.multi_bound(xt, o['score']))
    _note('lnms_cond_multi cond', rc, case['id'])
    _note('lnms_cond_multi multi', rm, case['id'])
    assert rc <= 1.0 and rm <= 1.0
    # backward, on the cond the forward kernel wrote
    p32 = _cpu(cond).clone()
    ds_ref, dl_ref, mag = TC.cond_bwd_ref64(case, o['d_multi'], p32, o['score'])
    bs, bl = TC.cond_bwd_bounds(case, ds_ref, dl_ref, mag)
    bx = Box()
    dm, cd, sc = bx.inp(o['d_multi']), bx.inp(p32), bx.inp(o['score'])
    d_sorted, d_logit = bx.out((B, F, C), F32), bx.out((rows, 64), BF16)
    lib.call('relnet_lnms_cond_bwd', dm.data_ptr(), cd.data_ptr(), sc.data_ptr(), d_sorted.data_ptr(), d_logit.data_ptr(), B, C, F, T, ops._stream())
    bx.check()
    assert GC.is_pattern_free(d_sorted) and GC.is_pattern_free(d_logit)                  # the whole 64-column row is written
    r1 = TC.worst(_cpu(d_sorted), ds_ref, bs)
    r2 = TC.worst(_cpu(d_logit), dl_ref, bl)
    _note('lnms_cond_bwd d_sorted', r1, case['id'])
    _note('lnms_cond_bwd d_logit', r2, case['id'])
    assert r1 <= 1.0 and r2 <= 1.0
    assert bool((TC.bits(d_logit[:, T:]) == 0).all())                                      # columns T .. 63: exact zeros


def test_lnms_cond_bwd_rejects_nine_thresholds(rn):
    g = torch.Generator().manual_seed(9)
    bx = Box()
    dm, cd, sc = bx.inp(torch.randn(1, 3, 2, 9, generator=g)), bx.inp(torch.rand(1, 3, 2, 9, generator=g)), bx.inp(torch.rand(1, 3, 2, generator=g))
    d_sorted, d_logit = bx.out((1, 3, 2), F32), bx.out((6, 64), BF16)
    _rejected(rn, bx, 'relnet_lnms_cond_bwd', dm.data_ptr(), cd.data_ptr(), sc.data_ptr(), d_sorted.data_ptr(), d_logit.data_ptr(), 1, 2, 3, 9)


@pytest.mark.parametrize('case', TC.TAKE_CASES, ids=_ids(TC.TAKE_CASES))
def test_lnms_embed_and_take_bwd_are_adjoint(rn, case):
    lib, ops, _ = rn
    B, N, C, F = (case[k] for k in ('B', 'N', 'C', 'F'))
    o = TC.take_operands(case)
    ref, mag = TC.take_bwd_ref64(o['d_x'], o['rank'], N)
    bound = TC.take_bwd_bound(case, ref, mag)
    bx = Box()
    d_x, rank = bx.inp(o['d_x']), bx.rank(o['rank'])
    d_emb = bx.out((B * N, TC.D), BF16)
    lib.call('relnet_lnms_take_bwd', d_x.data_ptr(), rank.data_ptr(), d_emb.data_ptr(), B, N, C, F, ops._stream())
    bx.check()
    assert GC.is_pattern_free(d_emb)                                                       # every row < B N is written
    got = _cpu(d_emb).view(B, N, TC.D)
    r = TC.worst(got, ref, bound)
    _note('lnms_take_bwd', r, case['id'])
    assert r <= 1.0
    ranked = TC.ranked_mask(o['rank'], N)
    assert bool((TC.bits(got[~ranked]) == 0).all())                                        # unranked rois: exact zeros
    if case['kind'] == 'neg':
        return                                                                            # (negative ranks never go to embed)
    x_ref = TC.embed_ref64(o['emb'], o['rank_feat'], o['rank'])
    bx = Box()
    emb, rf, rank = bx.inp(o['emb']), bx.inp(o['rank_feat']), bx.rank(o['rank'])
    x = bx.out((B, C, F, TC.D), BF16)
    lib.call('relnet_lnms_embed', emb.data_ptr(), rf.data_ptr(), rank.data_ptr(), x.data_ptr(), B, N, C, F, TC.D, 1, ops._stream())
    bx.check()
    assert GC.is_pattern_free(x)
    xg = _cpu(x)
    r = TC.worst(xg, x_ref, TC.embed_bound(x_ref))
    _note('lnms_embed', r, case['id'])
    assert r <= 1.0
    # <embed(e) - rank_feat, y> = <e, take_bwd(y)> on the GPU pair, within the sum of both bounds
    y, e = o['d_x'].double(), o['emb'].double()
    lhs = float(((xg.double() - o['rank_feat'].double()[None, None]) * y).sum())
    rhs = float((e * got.double()).sum())
    tol = float((TC.embed_bound(x_ref) * y.abs()).sum() + (bound * e.abs()).sum())
    _note('embed / take_bwd adjoint', abs(lhs - rhs) / tol, case['id'])
    assert abs(lhs - rhs) <= tol


def test_lnms_take_bwd_rejects_129_classes(rn):
    bx = Box()
    g = torch.Generator().manual_seed(3)
    d_x = bx.inp(torch.randn(1, 129, 2, TC.D, generator=g).to(BF16))
    rank = bx.rank(torch.zeros(1, 129, 2, dtype=I32))
    d_emb = bx.out((4, TC.D), BF16)
    _rejected(rn, bx, 'relnet_lnms_take_bwd', d_x.data_ptr(), rank.data_ptr(), d_emb.data_ptr(), 1, 4, 129, 2)


@pytest.mark.parametrize('case', TC.SOFTMAX_BWD_CASES, ids=_ids(TC.SOFTMAX_BWD_CASES))
def test_lnms_softmax_bwd_accumulates_into_a_strided_buffer(rn, case):
    lib, ops, _ = rn
    B, N, C, pad, R = (case[k] for k in ('B', 'N', 'C', 'pad', 'R'))
    o = TC.softmax_bwd_operands(case)
    ref, mag = TC.softmax_bwd_ref64(case, o['prob'], o['d_prob'], o['d_cls'])
    ld = C + 1 + pad
    bx = Box()
    prob, d_prob = bx.inp(o['prob']), bx.inp(o['d_prob'])
    d_cls = bx.inout(o['d_cls'])
    lib.call('relnet_lnms_softmax_bwd', prob.data_ptr(), d_prob.data_ptr(), d_cls.data_ptr(), ld, R * ld, B, N, C, ops._stream())
    bx.check()
    got = _cpu(d_cls)
    r = TC.worst(got, ref, TC.softmax_bwd_bound(case, mag))
    _note('lnms_softmax_bwd', r, case['id'])
    assert r <= 1.0
    assert TC.same_bits(got[:, N:], o['d_cls'][:, N:]) and TC.same_bits(got[:, :, C + 1:], o['d_cls'][:, :, C + 1:])     # rows >= N, pad columns


@pytest.mark.parametrize('case', TC.GATHER_CASES, ids=_ids(TC.GATHER_CASES))
def test_lnms_gather_bias_every_path(rn, case):
    """<= 64 columns (4 rows per trip), 65 .. 256, > 256; distinct integers in the table, so any wrong index shows; the pad columns F .. Fpad keep
    the pattern (they are part of the guard of the output view)."""
    lib, ops, _ = rn
    B, C, N, Npad, F, Fpad = (case[k] for k in ('B', 'C', 'N', 'Npad', 'F', 'Fpad'))
    img, rank = TC.gather_operands(case)
    bx = Box()
    iv, rv = bx.inp(img), bx.rank(rank)
    sl = slice(None)
    out = bx.out((B * C, 16, F, F), F32, parent=(B * C, 16, F, Fpad), index=(sl, sl, sl, slice(0, F)))
    lib.call('relnet_lnms_gather_bias', iv.data_ptr(), rv.data_ptr(), out.data_ptr(), B, C, N, Npad, F, Fpad, ops._stream())
    bx.check()
    assert GC.is_pattern_free(out)
    assert TC.same_bits(out, TC.gather_ref(case, iv, rv))
    _note('lnms_gather_bias', 0.0, case['id'] + ' bit-exact')


def test_lnms_gather_bias_rejects_513_ranks(rn):
    bx = Box()
    iv = bx.inp(torch.zeros(1, 16, 513, 513))
    rv = bx.rank(torch.arange(513, dtype=I32).view(1, 513))
    sl = slice(None)
    out = bx.out((1, 16, 513, 513), F32, parent=(1, 16, 513, 544), index=(sl, sl, sl, slice(0, 513)))
    _rejected(rn, bx, 'relnet_lnms_gather_bias', iv.data_ptr(), rv.data_ptr(), out.data_ptr(), 1, 1, 513, 513, 513, 544)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# csrc/train_ops.hip
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', TC.REDUCE_N)
def test_reduce_scalar_sums_and_counts(rn, n):
    """Mode 0 against the float64 sum (scale 1 and 1/8), mode 1 the exact count of entries >= 0 (-0.0 counts, NaN does not).  The slot is one float
    inside a pattern-filled row: the entry point zeroes it itself, its neighbours keep the pattern, a second call overwrites."""
    lib, ops, _ = rn
    x0, x1 = TC.reduce_operands(n, 0), TC.reduce_operands(n, 1)
    bx = Box()
    v0, v1 = bx.inp(x0), bx.inp(x1)
    slot = bx.out((1,), F32, parent=(8,), index=(slice(3, 4),))
    for scale in TC.REDUCE_SCALES:                                      # (the second call finds the first call's result in the slot)
        lib.call('relnet_reduce_scalar', v0.data_ptr(), n, scale, 0, slot.data_ptr(), ops._stream())
        bx.check()
        want, bound = TC.reduce_ref64(x0, scale, 0), TC.reduce_bound(x0, n, scale)
        r = abs(float(slot.item()) - want) / bound
        _note('reduce_scalar sum', r, 'n=%d scale=%g' % (n, scale))
        assert np.isfinite(slot.item()) and r <= 1.0
    lib.call('relnet_reduce_scalar', v1.data_ptr(), n, 1.0, 1, slot.data_ptr(), ops._stream())
    bx.check()
    assert float(slot.item()) == TC.reduce_ref64(x1, 1.0, 1)
    _note('reduce_scalar count', 0.0, 'n=%d exact' % n)


@pytest.mark.parametrize('case', TC.WGRAD_CASES, ids=_ids(TC.WGRAD_CASES))
def test_wgrad_accumulate_edges(rn, case):
    lib, ops, _ = rn
    o = TC.wgrad_operands(case)
    ref, mag = TC.wgrad_ref64(case, o['parts'], o['grad'], o['scale'])
    bx = Box()
    parts = bx.inp(o['parts'])
    scale = bx.inp(o['scale']) if o['scale'] is not None else None
    grad = bx.inout(o['grad'])
    lib.call('relnet_wgrad_accumulate', parts.data_ptr(), case['splits'], case['rows'], case['cols'], _ptr(scale), grad.data_ptr(), ops._stream())
    bx.check()
    r = TC.worst(_cpu(grad), ref, TC.wgrad_bound(case, mag))
    _note('wgrad_accumulate', r, case['id'])
    assert r <= 1.0


def test_wgrad_accumulate_rejects_six_columns(rn):
    bx = Box()
    parts = bx.inp(torch.ones(2, 4, 6))
    grad = bx.out((4, 6), F32)
    _rejected(rn, bx, 'relnet_wgrad_accumulate', parts.data_ptr(), 2, 4, 6, 0, grad.data_ptr())


@pytest.mark.parametrize('case', TC.SGD_CASES, ids=_ids(TC.SGD_CASES))
def test_sgd_update_edges(rn, case):
    lib, ops, _ = rn
    o = TC.sgd_operands(case)
    n = case['n']
    m_ref, w_ref, mag = TC.sgd_ref64(case, o['w'], o['mom'], o['grad'])
    bm, bw = TC.sgd_bounds(w_ref, mag)
    bx = Box()
    w, mom = bx.inout(o['w']), bx.inout(o['mom'])
    grad = bx.inp(o['grad'])
    wb = bx.out((n,), BF16) if case['bf16'] else None
    lib.call('relnet_sgd_update', w.data_ptr(), mom.data_ptr(), grad.data_ptr(), _ptr(wb), n, TC.SGD_LR, TC.SGD_MOMENTUM, case['wd'], case['rescale'],
             ops._stream())
    bx.check()                                                          # guards of all four buffers
    rm, rw = TC.worst(_cpu(mom), m_ref, bm), TC.worst(_cpu(w), w_ref, bw)
    _note('sgd_update mom', rm, case['id'])
    _note('sgd_update w', rw, case['id'])
    assert rm <= 1.0 and rw <= 1.0
    if wb is not None:
        assert GC.is_pattern_free(wb) and TC.same_bits(wb, w.to(BF16))


@pytest.mark.parametrize('shape', TC.PACK_SHAPES)
def test_relation_bwd_pack_small_shapes(rn, shape):
    lib, ops, _ = rn
    B, N, M, d = shape
    dq, dk, dvw = TC.pack_operands(shape)
    bx = Box()
    q, k, v = bx.inp(dq), bx.inp(dk), bx.inp(dvw)
    out = bx.out((B, N, 3 * d), BF16)
    lib.call('relnet_relation_bwd_pack', q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, N, M, d, ops._stream())
    bx.check()
    assert GC.is_pattern_free(out)
    assert TC.same_bits(_cpu(out), TC.pack_ref(dq, dk, dvw))
    assert bool((TC.bits(out[:, M:, d:]) == 0).all())                   # rows >= M of the key blocks: exact zeros
    _note('relation_bwd_pack', 0.0, '%dx%dx%dx%d bit-exact' % shape)


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_relu_bwd_masks_negative_zero_and_nan(rn, dtype):
    lib, ops, T = rn
    dy, y, add = TC.relu_bwd_operands(dtype)
    n = dy.numel()
    for with_add in (False, True):
        bx = Box()
        dyv, yv = bx.inp(dy), bx.inp(y)
        av = bx.inp(add) if with_add else None
        out = bx.out((n,), dtype)
        T.relu_bwd(dyv, yv, av, out=out)
        bx.check()
        assert GC.is_pattern_free(out)
        assert TC.same_bits(_cpu(out), TC.relu_bwd_ref(dy, y, add if with_add else None))
    # a misaligned `add`
    bx = Box()
    dyv, yv = bx.inp(dy), bx.inp(y)
    av = bx.inp(add, parent=(n + 1,), index=(slice(1, None),))
    out = bx.out((n,), dtype)
    _rejected(rn, bx, 'relnet_relu_bwd', dyv.data_ptr(), yv.data_ptr(), av.data_ptr(), out.data_ptr(), n, ops._dt(dyv))
    _note('relu_bwd', 0.0, '%s bit-exact' % str(dtype).split('.')[-1])
