"""The optimizer-step guard on the GPU (csrc/guard.hip; train.GradGuard), kernel by kernel through the C-ABI against the float64 reference
and the bounds of tests/grad_guard_cases.py, then through Trainer.update() on the 128 x 160 one-image step of test_gpu_train_step.py.

Every operand sits inside a larger buffer filled with a bit pattern (a NaN, so a stray READ also shows: it would be counted as non-finite); after
each launch the surroundings are compared bit for bit.  Every test prints the figure it is about to assert."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_guard_cases as GG  # noqa: E402

pytestmark = pytest.mark.gpu
_ids = lambda cs: [c['id'] for c in cs]
PAD = 64                                   # floats of pattern on each side of an operand (a multiple of 4: keeps the alignment class)
PATTERN = 0x7fc5a5a5                       # a quiet NaN with a recognisable payload
I64_PATTERN = 0x7ff8a5a5a5a5a5a5           # int64 word = a NaN as double, a large positive count as int64
F32, BF16, I32, I64, F64 = torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.float64


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import lib, ops, train_ops
    return lib, ops, train_ops


def _bits(t):
    return t.view({2: torch.int16, 4: I32, 8: I64}[t.element_size()])


class Guarded(object):
    """A tensor of `n` elements `mis` elements past a 16-byte boundary, with PAD elements of pattern on both sides."""

    def __init__(self, values, dtype=F32, mis=0):
        values = torch.as_tensor(values)
        n = values.numel()
        self.buf = torch.empty(n + 2 * PAD + 4, dtype=dtype, device='cuda')
        _bits(self.buf).fill_(PATTERN if self.buf.element_size() == 4 else 0x7fc5)
        assert self.buf.data_ptr() % 16 == 0
        lo = PAD + mis
        self.view = self.buf[lo:lo + n]
        self.view.copy_(values.to(dtype))
        self.lo, self.n = lo, n
        self.snap = _bits(self.buf).clone()

    def surroundings_intact(self):
        b = _bits(self.buf)
        return bool((b[:self.lo] == self.snap[:self.lo]).all()) and bool((b[self.lo + self.n:] == self.snap[self.lo + self.n:]).all())

    def unchanged(self):
        return bool((_bits(self.buf) == self.snap).all())


def _workspace(T, slots, extra=8):
    ws = torch.full((2 * (slots + extra),), I64_PATTERN, dtype=I64, device='cuda')
    return ws


def _run_stats(T, case, slot_base=0):
    ops_ = GG.stats_operands(case)
    gs = [Guarded(x, F32, mis) for mis, x in ops_]
    for g, (mis, _) in zip(gs, ops_):
        assert g.view.data_ptr() % 16 == 4 * mis
    slots = GG.stats_slots([x.size for _, x in ops_])
    ws = _workspace(T, slot_base + slots)
    used = T.grad_stats([g.view for g in gs], ws, slot_base)
    torch.cuda.synchronize()
    assert used == slots
    assert all(g.unchanged() for g in gs), 'relnet_grad_stats wrote to its input'
    w = ws.cpu()
    assert bool((w[:2 * slot_base] == I64_PATTERN).all()) and bool((w[2 * (slot_base + slots):] == I64_PATTERN).all()), 'a slot outside the launch'
    part = w[2 * slot_base:2 * (slot_base + slots)].view(-1, 2)
    return ws, slots, part, [x for _, x in ops_]


@pytest.mark.parametrize('case', GG.STATS_CASES, ids=_ids(GG.STATS_CASES))
def test_grad_stats_cases(rn, case):
    lib, ops, T = rn
    ws, slots, part, arrays = _run_stats(T, case, slot_base=3)
    ref, bad, n = GG.stats_ref(arrays)
    # the slots, added on the host in extended precision: no further rounding of the sum beyond the final one
    sums = part[:, 0].contiguous().view(F64).numpy()
    got = float(np.sum(sums.astype(np.longdouble)))
    cnt = int(part[:, 1].sum())
    bound = GG.sumsq_bound(n, ref)
    print('grad_stats %-26s n %9d slots %5d  count %d (want %d)  |sum - ref| / bound %.4f' % (case['id'], n, slots, cnt, bad,
                                                                                             abs(got - ref) / bound if bound else 0.0))
    assert cnt == bad
    assert np.isfinite(sums).all() and (sums >= 0).all() and np.isfinite(got)
    assert abs(got - ref) <= bound
    # the same through the decide kernel (its own fold of the slots)
    ws2, _, _, _ = _run_stats(T, case, slot_base=0)
    st = T.grad_guard_state('cuda')
    T.grad_guard_decide(ws2, slots, st, 0.0)
    s = st.cpu()
    norm, want = float(s.view(F64)[1]), float(np.sqrt(ref))
    print('   decide: last_norm %.17g (ref %.17g, |err| / bound %.4f), last_nonfinite %d' % (norm, want, abs(norm - want) / GG.norm_bound(n, want)
                                                                                            if want else 0.0, int(s[2])))
    assert int(s[2]) == bad and int(s.view(I32)[0]) == (1 if bad else 0) and np.isfinite(norm)
    assert abs(norm - want) <= GG.norm_bound(n, want)
    # two runs on the same input: the same bits, slot by slot and in the decided norm
    ws3, _, part3, _ = _run_stats(T, case, slot_base=3)
    assert torch.equal(part3, part)
    st3 = T.grad_guard_state('cuda')
    T.grad_guard_decide(ws3[6:], slots, st3, 0.0)
    assert torch.equal(st3.cpu(), s)


def test_grad_stats_rejects_bad_tables(rn):
    lib, ops, T = rn
    import ctypes as C
    x = Guarded(np.ones(8, np.float32))
    ws = _workspace(T, 4)
    s = ops._stream()
    one = lambda p, n: ((C.c_void_p * 1)(p), (C.c_long * 1)(n))
    for ptrs, ns, n, wsp, base, cap in (one(x.view.data_ptr(), 0) + (1, ws.data_ptr(), 0, 4),              # empty range
                                        one(0, 8) + (1, ws.data_ptr(), 0, 4),                               # null range
                                        one(x.view.data_ptr() + 2, 4) + (1, ws.data_ptr(), 0, 4),           # 2-byte aligned
                                        one(x.view.data_ptr(), 8) + (0, ws.data_ptr(), 0, 4),               # no range
                                        one(x.view.data_ptr(), 8) + (17, ws.data_ptr(), 0, 4),              # more than 16
                                        one(x.view.data_ptr(), 8) + (1, 0, 0, 4),                           # null workspace
                                        one(x.view.data_ptr(), 8) + (1, ws.data_ptr(), 4, 4),               # slot past the capacity
                                        one(x.view.data_ptr(), 8) + (1, ws.data_ptr(), -1, 4)):
        with pytest.raises(lib.RelnetError):
            lib.call('relnet_grad_stats', ptrs, ns, n, wsp, base, cap, s)
    st = T.grad_guard_state('cuda')
    for args in ((0, 1, 0.0, st.data_ptr()), (ws.data_ptr(), 0, 0.0, st.data_ptr()), (ws.data_ptr(), 1, 0.0, 0), (ws.data_ptr(), 1, float('nan'), st.data_ptr())):
        with pytest.raises(lib.RelnetError):
            lib.call('relnet_grad_guard_decide', *(args + (s,)))
    w = Guarded(np.ones(8, np.float32))
    for args in ((0, w.view.data_ptr(), w.view.data_ptr(), 0, 8, .1, .9, 0., 1., st.data_ptr(), -1.0),
                 (w.view.data_ptr(), w.view.data_ptr(), w.view.data_ptr(), 0, 8, .1, .9, 0., 1., 0, -1.0),
                 (w.view.data_ptr(), w.view.data_ptr(), w.view.data_ptr(), 0, 0, .1, .9, 0., 1., st.data_ptr(), -1.0),
                 (w.view.data_ptr(), w.view.data_ptr(), w.view.data_ptr(), 0, 8, .1, .9, 0., 1., st.data_ptr(), float('nan'))):
        with pytest.raises(lib.RelnetError):
            lib.call('relnet_sgd_update_guarded', *(args + (s,)))
    torch.cuda.synchronize()
    assert x.unchanged() and w.unchanged() and bool((ws == I64_PATTERN).all())
    assert lib.load().relnet_grad_stats_slots((C.c_long * 3)(5000, 1, 300), 3) == 4
    assert lib.load().relnet_grad_stats_slots((C.c_long * 1)(0), 1) == -1
    assert lib.load().relnet_grad_guard_workspace_bytes(5) == 5 * T.GUARD_SLOT_BYTES


# ---------------------------------------------------------------------------------------------------------------------------------------------
# decide
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _state_dict(st):
    s = st.cpu()
    f = s.view(F64)
    return dict(skip=int(s.view(I32)[0]), scale=np.float32(s.view(F32)[1].item()), last_norm=float(f[1]), last_nonfinite=int(s[2]), steps=int(s[3]),
                skipped=int(s[4]), clipped=int(s[5]), norm_sum=float(f[6]), norm_max=float(f[7]))


def _slots(pairs):
    """A workspace holding the given (sum of squares, count) slots, pattern behind them."""
    ws = torch.full((2 * len(pairs) + 16,), I64_PATTERN, dtype=I64)
    for i, (s, c) in enumerate(pairs):
        ws[2 * i] = int(np.float64(s).view(np.int64))
        ws[2 * i + 1] = c
    return ws.cuda()


def _same_state(got, want, exact=True):
    for k in GG.STATE_FIELDS:
        g, w = got[k], want[k]
        if exact or k not in ('last_norm', 'norm_sum', 'norm_max'):
            assert g == w and type(g) == type(w), (k, g, w)
        else:
            assert abs(g - w) <= 2 * 2.0 ** -53 * abs(w), (k, g, w)


@pytest.mark.parametrize('n_slots', (1, 255, 256, 257, 1000))
def test_decide_folds_every_slot_and_nothing_else(rn, n_slots):
    """Integer partial sums (exact in any order): slot i holds i + 1, every 7th slot a count of 2.  Then one slot more is NOT read."""
    lib, ops, T = rn
    pairs = [(float(i + 1), 0) for i in range(n_slots)]
    ws = _slots(pairs + [(1e300, 1 << 40)])
    st = T.grad_guard_state('cuda')
    T.grad_guard_decide(ws, n_slots, st, 0.0)
    got = _state_dict(st)
    want = GG.decide_ref(GG.fresh_state(), n_slots * (n_slots + 1) / 2.0, 0, None)
    print('decide %d slots: norm %.17g want %.17g' % (n_slots, got['last_norm'], want['last_norm']))
    _same_state(got, want, exact=False)
    assert got['last_nonfinite'] == 0 and got['skip'] == 0
    ws = _slots([(s, 2 if i % 7 == 0 else 0) for i, (s, _) in enumerate(pairs)])
    T.grad_guard_decide(ws, n_slots, st, 0.0)
    got2 = _state_dict(st)
    assert got2['last_nonfinite'] == 2 * ((n_slots + 6) // 7) and got2['skip'] == 1 and got2['skipped'] == 1 and got2['steps'] == 2
    assert got2['norm_sum'] == got['norm_sum'] and got2['norm_max'] == got['norm_max']        # a skipped step leaves the norm totals alone


def test_decide_scale_cases(rn):
    lib, ops, T = rn
    # below max_norm: exactly 1.0f, clipped unchanged
    st = T.grad_guard_state('cuda')
    T.grad_guard_decide(_slots([(9.0, 0), (16.0, 0)]), 2, st, 7.0)
    g = _state_dict(st)
    _same_state(g, GG.decide_ref(GG.fresh_state(), 25.0, 0, 7.0))
    assert g['scale'] == np.float32(1.0) and g['clipped'] == 0 and g['last_norm'] == 5.0
    # above: float32 of the float64 coefficient
    T.grad_guard_decide(_slots([(36.0, 0), (64.0, 0)]), 2, st, 7.0)
    g2 = _state_dict(st)
    want = GG.decide_ref(GG.decide_ref(GG.fresh_state(), 25.0, 0, 7.0), 100.0, 0, 7.0)
    print('decide scale %.9g want %.9g' % (g2['scale'], want['scale']))
    _same_state(g2, want)
    assert g2['scale'] == np.float32(7.0 / (10.0 + 1e-6)) and g2['scale'] < 1 and g2['clipped'] == 1
    # a general (not perfect-square) total: the coefficient of the reference norm, rounded to float32
    st = T.grad_guard_state('cuda')
    T.grad_guard_decide(_slots([(1234.5678, 0), (0.1, 0), (77.0, 0)]), 3, st, 3.3)
    ref = GG.decide_ref(GG.fresh_state(), 1234.5678 + 0.1 + 77.0, 0, 3.3)       # (the fold order may differ from this one by an ulp of the sum)
    g3 = _state_dict(st)
    _same_state(g3, ref, exact=False)
    assert g3['scale'] == ref['scale'] and g3['clipped'] == 1
    # a norm a hair under max_norm: max_norm / (norm + 1e-6) is still below 1 in float64, and so is its float32 value
    st = T.grad_guard_state('cuda')
    T.grad_guard_decide(_slots([(25.0, 0)]), 1, st, 5.0000001)
    _same_state(_state_dict(st), GG.decide_ref(GG.fresh_state(), 25.0, 0, 5.0000001))
    # zero gradient with max_norm set: scale 1; max_norm <= 0: never clips
    st = T.grad_guard_state('cuda')
    T.grad_guard_decide(_slots([(0.0, 0)] * 3), 3, st, 1e-3)
    g4 = _state_dict(st)
    _same_state(g4, GG.decide_ref(GG.fresh_state(), 0.0, 0, 1e-3))
    assert g4['scale'] == np.float32(1.0) and g4['skip'] == 0 and g4['clipped'] == 0 and g4['last_norm'] == 0.0
    T.grad_guard_decide(_slots([(1e20, 0)]), 1, st, -1.0)
    assert _state_dict(st)['scale'] == np.float32(1.0)
    # non-finite: skip, scale 1, totals of the norm untouched
    st = T.grad_guard_state('cuda')
    T.grad_guard_decide(_slots([(4.0, 0)]), 1, st, 1.0)
    T.grad_guard_decide(_slots([(1e12, 0), (4.0, 1)]), 2, st, 1.0)
    g5 = _state_dict(st)
    _same_state(g5, GG.decide_ref(GG.decide_ref(GG.fresh_state(), 4.0, 0, 1.0), 1e12 + 4.0, 1, 1.0), exact=False)
    assert (g5['skip'], g5['skipped'], g5['norm_sum'], g5['norm_max'], g5['clipped']) == (1, 1, 2.0, 2.0, 1) and g5['scale'] == np.float32(1.0)


def test_scripted_sequence_of_five_steps(rn):
    """clean, clipped, NaN, clean, inf through the real statistics kernel and one state: every field after every step equals the reference's."""
    lib, ops, T = rn
    st = T.grad_guard_state('cuda')
    ref = GG.fresh_state()
    for kind, g in GG.SCRIPT:
        x = Guarded(g, F32, mis=1)
        slots = GG.stats_slots([g.size])
        ws = _workspace(T, slots)
        assert T.grad_stats([x.view], ws, 0) == slots
        T.grad_guard_decide(ws, slots, st, GG.SCRIPT_MAX_NORM)
        s, bad, _ = GG.stats_ref([g])
        ref = GG.decide_ref(ref, s, bad, GG.SCRIPT_MAX_NORM)
        got = _state_dict(st)
        print('script %-8s %s' % (kind, got))
        _same_state(got, ref)
    assert (ref['steps'], ref['skipped'], ref['clipped']) == (5, 2, 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# guarded SGD
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _state(T, skip=0, scale=1.0):
    st = T.grad_guard_state('cuda')
    st.view(I32)[0] = skip
    st.view(F32)[1] = float(scale)
    return st


def _sgd_buffers(case, o, mis=1):
    w, mom, grad = Guarded(o['w'], F32, mis), Guarded(o['mom'], F32, mis), Guarded(o['grad'], F32, mis)
    wb = Guarded(np.zeros(case['n'], np.float32), BF16, mis) if case['bf16'] else None
    return w, mom, grad, wb


def _guarded_call(T, bufs, st, rescale=1.0, clip=-1.0, wd=GG.SGD_WD):
    w, mom, grad, wb = bufs
    T.sgd_update_guarded(w.view, mom.view, grad.view, GG.SGD_LR, st, GG.SGD_MOMENTUM, wd, rescale, clip, w_bf16=None if wb is None else wb.view)
    torch.cuda.synchronize()
    assert grad.unchanged() and all(b.surroundings_intact() for b in (w, mom) + ((wb,) if wb is not None else ()))


def _plain_call(T, bufs, rescale=1.0, wd=GG.SGD_WD):
    w, mom, grad, wb = bufs
    T.sgd_update(w.view, mom.view, grad.view, GG.SGD_LR, GG.SGD_MOMENTUM, wd, rescale, w_bf16=None if wb is None else wb.view)
    torch.cuda.synchronize()


def _same_bits(a, b):
    return a is None and b is None or bool((_bits(a.view) == _bits(b.view)).all())


@pytest.mark.parametrize('case', GG.SGD_CASES, ids=_ids(GG.SGD_CASES))
def test_guarded_sgd_neutral_state_equals_sgd_update_bit_for_bit(rn, case):
    lib, ops, T = rn
    o = GG.sgd_operands(case)
    for wd in (GG.SGD_WD, 0.0):
        a, b = _sgd_buffers(case, o), _sgd_buffers(case, o)
        _plain_call(T, a, wd=wd)
        st = _state(T)
        _guarded_call(T, b, st, wd=wd)
        assert all(_same_bits(x, y) for x, y in zip(a, b))
        assert not _same_bits(b[0], Guarded(o['w'], F32, 1))              # (something was updated)
        assert torch.equal(st.cpu(), _state(T).cpu())                    # the kernel only reads the state


@pytest.mark.parametrize('case', GG.SGD_CASES, ids=_ids(GG.SGD_CASES))
def test_guarded_sgd_skip_writes_nothing(rn, case):
    lib, ops, T = rn
    o = GG.sgd_operands(case)
    o['grad'][case['n'] // 2] = np.nan
    bufs = _sgd_buffers(case, o)
    _guarded_call(T, bufs, _state(T, skip=1, scale=0.5), clip=0.5)
    assert all(b.unchanged() for b in bufs if b is not None)


@pytest.mark.parametrize('case', GG.SGD_CASES, ids=_ids(GG.SGD_CASES))
def test_guarded_sgd_scale_equals_rescale_grad_bit_for_bit(rn, case):
    lib, ops, T = rn
    o = GG.sgd_operands(case)
    a, b = _sgd_buffers(case, o), _sgd_buffers(case, o)
    _plain_call(T, a, rescale=GG.SGD_SCALE)
    _guarded_call(T, b, _state(T, scale=GG.SGD_SCALE))
    assert all(_same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('clip', GG.SGD_CLIPS, ids=lambda c: 'c%g-rs%g-sc%g' % (c['clip'], c['rescale'], c['scale']))
@pytest.mark.parametrize('case', GG.SGD_CASES, ids=_ids(GG.SGD_CASES))
def test_guarded_sgd_clip_gradient_against_float64(rn, case, clip):
    lib, ops, T = rn
    o = GG.sgd_operands(case)
    m_ref, w_ref, bm, bw = GG.sgd_guarded_ref64(o['w'], o['mom'], o['grad'], clip['clip'], clip['rescale'], clip['scale'])
    bufs = _sgd_buffers(case, o)
    _guarded_call(T, bufs, _state(T, scale=clip['scale']), rescale=clip['rescale'], clip=clip['clip'])
    w, mom, _, wb = bufs
    em = np.abs(mom.view.cpu().numpy().astype(np.float64) - m_ref)
    ew = np.abs(w.view.cpu().numpy().astype(np.float64) - w_ref)
    print('sgd_update_guarded %s clip %g: worst err / bound mom %.4f, w %.4f' % (case['id'], clip['clip'], float((em / bm).max()), float((ew / bw).max())))
    assert (em <= bm).all() and (ew <= bw).all()
    if wb is not None:
        assert bool((_bits(wb.view) == _bits(w.view.to(BF16))).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Trainer.update() with a guard
# ---------------------------------------------------------------------------------------------------------------------------------------------
class _Snap(object):
    FIELDS = ('master', 'mom', 'work', 'grad')

    def __init__(self, tr):
        self.t = {(b, f): getattr(getattr(tr, b), f).clone() for b in ('W', 'Bv') for f in self.FIELDS}

    def restore(self, tr):
        for (b, f), v in self.t.items():
            getattr(getattr(tr, b), f).copy_(v)

    def same(self, other, fields=('master', 'mom', 'work')):
        return all(bool((_bits(self.t[(b, f)]) == _bits(other.t[(b, f)])).all()) for b in ('W', 'Bv') for f in fields)


def _trainable_grads(tr):
    return [tr.W.grad[a:b].cpu().numpy() for a, b in tr._trainable_ranges(tr.W)] + [tr.Bv.grad[a:b].cpu().numpy() for a, b in tr._trainable_ranges(tr.Bv)]


@pytest.fixture(scope='module')
def stepped():
    """The 128 x 160 one-image trainer of test_gpu_train_step.py after one forward_backward, with a snapshot of its flat buffers."""
    import test_gpu_train_step as TS
    H, W, G = 128, 160, 4
    p, cfg, data, gt, L, Tg, Wg, train = TS._setup(H, W, G, 33)
    tr = train.Trainer(p, cfg, im_hw=(H, W))
    d = lambda a: torch.as_tensor(a).cuda()
    with torch.no_grad():
        tr.forward_backward(data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
        tr.all_reduce()
    torch.cuda.synchronize()
    return tr, _Snap(tr), train


def test_trainer_neutral_guard_gives_the_unguarded_bits(stepped):
    tr, snap, train = stepped
    snap.restore(tr); tr.guard = None
    tr.update(); torch.cuda.synchronize()
    r0 = _Snap(tr)
    assert not r0.same(snap)                                              # the step moved the weights
    snap.restore(tr)
    tr.guard = train.GradGuard()
    n0 = tr.step_count
    tr.update(); torch.cuda.synchronize()
    rep = tr.guard.report()
    tr.guard = None
    assert _Snap(tr).same(r0) and tr.step_count == n0 + 1
    ref, bad, n = GG.stats_ref(_trainable_grads(tr))
    want = float(np.sqrt(ref))
    print('trainer neutral guard: %s; float64 norm of %d gradients %.17g, |err| / bound %.4f' % (rep, n, want, abs(rep['last_norm'] - want) / GG.norm_bound(n, want)))
    assert bad == 0 and rep['steps'] == 1 and rep['skipped'] == 0 and rep['clipped'] == 0 and rep['last_nonfinite'] == 0
    assert np.isfinite(rep['last_norm']) and rep['last_norm'] > 0 and abs(rep['last_norm'] - want) <= GG.norm_bound(n, want)
    assert rep['mean_norm'] == rep['last_norm'] == rep['max_norm_seen']


def test_trainer_poisoned_gradient_skips_the_update(stepped):
    tr, snap, train = stepped
    snap.restore(tr)
    tr.W.grad[tr.W.size // 2] = float('nan')
    before = _Snap(tr)
    g = tr.guard = train.GradGuard(max_norm=1.0, clip_gradient=0.1)
    n0 = tr.step_count
    tr.update(); torch.cuda.synchronize()
    rep = g.report()
    tr.guard = None
    print('trainer poisoned gradient:', rep)
    assert _Snap(tr).same(before, _Snap.FIELDS)
    assert rep['steps'] == 1 and rep['skipped'] == 1 and rep['last_nonfinite'] == 1 and rep['clipped'] == 0 and rep['mean_norm'] == 0.0
    assert tr.step_count == n0 + 1                                        # the host does not know: the call count advances
    # the same guard, a clean gradient next: the update goes through; reset() zeroes the totals
    snap.restore(tr)
    tr.guard = g
    tr.update(); torch.cuda.synchronize()
    tr.guard = None
    rep = g.report()
    assert rep['steps'] == 2 and rep['skipped'] == 1 and rep['last_nonfinite'] == 0 and not _Snap(tr).same(snap)
    g.reset()
    assert g.report() == {'steps': 0, 'skipped': 0, 'clipped': 0, 'last_norm': 0.0, 'last_nonfinite': 0, 'mean_norm': 0.0, 'max_norm_seen': 0.0}


@pytest.mark.parametrize('fraction', (0.5, 1.0 / 3.0), ids=('half', 'third'))
def test_trainer_global_norm_clipping_equals_rescale_grad(stepped, monkeypatch, fraction):
    """max_norm = half of the measured norm (the scale then rounds to exactly 0.5f: 0.5 / (1 + 1e-6 / norm) is closer to 0.5 than half a
    float32 step) and a third of it (a scale that is no power of two)."""
    tr, snap, train = stepped
    snap.restore(tr)
    tr.guard = train.GradGuard()
    tr.update(); torch.cuda.synchronize()
    norm = tr.guard.report()['last_norm']
    snap.restore(tr)
    g = tr.guard = train.GradGuard(max_norm=fraction * norm)
    tr.update(); torch.cuda.synchronize()
    tr.guard = None
    clipped = _Snap(tr)
    rep = g.report()
    scale = float(g.state.cpu().view(F32)[1])
    print('trainer clipping: norm %.9g, max_norm %.9g, scale %.9g, report %s' % (norm, fraction * norm, scale, rep))
    assert rep['clipped'] == 1 and rep['skipped'] == 0 and rep['last_norm'] == norm
    assert np.float32(scale) == np.float32(GG.clip_coef(norm, fraction * norm)) and 0.98 * fraction < scale <= np.float32(fraction)
    # the unguarded update with rescale_grad = that scale
    plain = train.T.sgd_update
    monkeypatch.setattr(train.T, 'sgd_update', lambda w, mom, grad, lr, momentum=0.9, wd=0.0005, rescale_grad=1.0, w_bf16=None:
                        plain(w, mom, grad, lr, momentum, wd, scale, w_bf16=w_bf16))
    snap.restore(tr)
    tr.update(); torch.cuda.synchronize()
    assert _Snap(tr).same(clipped) and not clipped.same(snap)


def test_trainer_frozen_slice_does_not_trigger_a_skip():
    """The learn-NMS-only experiment fixes the whole detector: a NaN in a frozen slice of W.grad is outside the statistics; one in a trainable
    slice skips."""
    import test_gpu_train_step as TS
    H, W, G = 128, 160, 4
    p, _, data, gt, L, Tg, Wg, train = TS._setup(H, W, G, 57)
    g_ = torch.Generator().manual_seed(58)
    p['nms_logit_bias'] = torch.zeros(5)
    for k in ('nms_logit_weight', 'nms_rank_weight', 'roi_feat_embedding_weight', 'nms_query_1_weight', 'nms_key_1_weight',
              'nms_linear_out_1_weight', 'nms_pair_pos_fc1_1_weight'):
        p[k] = torch.randn(p[k].shape, generator=g_) * 0.05
    cfg = train.TrainConfig.from_experiment('rcnn_end2end_learn_nms_3epoch', train=True)
    cfg.rpn_post_nms_top_n, cfg.first_n = 40, 24
    tr = train.Trainer(p, cfg, im_hw=(H, W), guard=train.GradGuard())
    assert tr.frozen_names and 'fc_new_1' in tr.frozen_names and 'nms_logit' not in tr.frozen_names
    d = lambda a: torch.as_tensor(a).cuda()
    with torch.no_grad():
        tr.forward_backward(data.cuda(), torch.tensor([[H, W, 1.0]]).cuda(), d(gt), d(L[None]), d(Tg[None]), d(Wg[None]))
        tr.all_reduce()
    snap = _Snap(tr)
    off, shape = tr.W.slices['fc_new_1']
    assert not any(a <= off < b for a, b in tr._trainable_ranges(tr.W))
    tr.W.grad[off + 5] = float('nan')
    tr.Bv.grad[tr.Bv.slices['fc_new_1'][0]] = float('inf')
    tr.update(); torch.cuda.synchronize()
    rep = tr.guard.report()
    print('trainer frozen slice:', rep)
    assert rep['skipped'] == 0 and rep['last_nonfinite'] == 0 and rep['steps'] == 1
    now = _Snap(tr)
    assert not now.same(snap)                                             # the head was updated
    a, b = off, off + int(np.prod(shape))
    assert torch.equal(tr.W.master[a:b], snap.t[('W', 'master')][a:b])    # the frozen slice was not
    ref, bad, n = GG.stats_ref(_trainable_grads(tr))
    assert bad == 0 and abs(rep['last_norm'] - float(np.sqrt(ref))) <= GG.norm_bound(n, float(np.sqrt(ref)))
    # a NaN in a trainable slice does skip
    snap.restore(tr)
    tr.W.grad[tr.W.slices['nms_logit'][0]] = float('nan')
    before = _Snap(tr)
    tr.update(); torch.cuda.synchronize()
    assert tr.guard.report()['skipped'] == 1 and _Snap(tr).same(before, _Snap.FIELDS)
