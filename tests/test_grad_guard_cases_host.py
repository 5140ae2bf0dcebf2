"""tests/grad_guard_cases.py on the CPU: the float64 reference of the optimizer-step guard is consistent with itself and agrees with
torch.nn.utils.clip_grad_norm_ (float64) on every finite case; the cases hit the edges they are named after; the guarded-SGD reference
reduces to train_glue_cases' sgd reference when nothing clips."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_guard_cases as GG  # noqa: E402

_ids = lambda cs: [c['id'] for c in cs]
SMALL = [c for c in GG.STATS_CASES if c['id'] != 'grid-cap']


def test_case_ids_are_unique_and_cover_the_edges():
    ids = _ids(GG.STATS_CASES)
    assert len(set(ids)) == len(ids)
    by = {c['id']: c for c in GG.STATS_CASES}
    assert {by['n%d' % n]['ranges'][0]['n'] for n in (1, 3, 255, 256, 257)} == {1, 3, 255, 256, 257}
    r = by['unaligned-4097']['ranges'][0]
    assert (r['n'], r['mis']) == (4097, 1)                    # 4 bytes past a 16-byte boundary
    head = (4 - r['mis']) % 4
    assert head == 3 and (r['n'] - head) // 4 == 1023 and (r['n'] - head) % 4 == 2
    assert by['nan-in-tail']['ranges'][0]['poison'][0][0] == 4095 and by['nan-last-tail']['ranges'][0]['poison'][0][0] == 4096
    assert sorted(x['n'] for x in by['table3']['ranges']) == [1, 300, 5000]
    assert len(by['table16']['ranges']) == GG.MAX_RANGES
    # the grid cap: reached, and the grid-stride loop runs more than once
    assert GG.range_blocks(GG.N_CAP) == GG.MAX_BLOCKS_PER_RANGE and GG.N_CAP // 4 > GG.MAX_BLOCKS_PER_RANGE * 256
    assert GG.range_blocks(1) == 1 and GG.range_blocks(4096) == 1 and GG.range_blocks(4097) == 2
    assert GG.stats_slots([5000, 1, 300]) == 4


@pytest.mark.parametrize('case', SMALL, ids=_ids(SMALL))
def test_stats_reference_is_consistent(case):
    arrays = [x for _, x in GG.stats_operands(case)]
    again = [x for _, x in GG.stats_operands(case)]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(arrays, again))          # seeded
    s, bad, n = GG.stats_ref(arrays)
    assert n == sum(r['n'] for r in case['ranges']) and bad == sum(len(r['poison']) for r in case['ranges'])
    flat = np.concatenate(arrays)
    fin = flat[np.isfinite(flat)]
    exact = math.fsum(float(v) * float(v) for v in fin)                                     # squares exact, fsum correctly rounded
    assert abs(s - exact) <= 2.0 ** -52 * exact and math.isfinite(s)
    assert GG.sumsq_bound(n, s) >= 0
    if case['id'] == 'huge-3e38':
        with np.errstate(over='ignore'):
            assert np.isinf(np.square(flat)).all() and s > 1e80                            # float32 squares overflow, float64 ones do not
    if case['id'] == 'denormal':
        assert (np.abs(flat) < 2.0 ** -126).all() and (flat != 0).all() and bad == 0 and s > 0
    if case['id'] == 'zeros':
        assert s == 0.0 and bad == 0


@pytest.mark.parametrize('case', [c for c in SMALL if not any(r['poison'] for r in c['ranges'])], ids=lambda c: c['id'])
@pytest.mark.parametrize('max_norm', (0.5, 1e6))
def test_reference_agrees_with_clip_grad_norm(case, max_norm):
    arrays = [x for _, x in GG.stats_operands(case)]
    s, bad, n = GG.stats_ref(arrays)
    assert bad == 0
    ps = [torch.nn.Parameter(torch.zeros(x.size, dtype=torch.float64)) for x in arrays]
    for p, x in zip(ps, arrays):
        p.grad = torch.as_tensor(x.astype(np.float64)).clone()
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    norm = math.sqrt(s)
    assert abs(total - norm) <= GG.norm_bound(n, norm)
    coef = GG.clip_coef(norm, max_norm)
    for p, x in zip(ps, arrays):
        want = x.astype(np.float64) * coef
        assert np.allclose(p.grad.numpy(), want, rtol=1e-12, atol=0.0)
    st = GG.decide_ref(GG.fresh_state(), s, 0, max_norm)
    assert st['skip'] == 0 and st['scale'] == np.float32(coef) and st['clipped'] == int(np.float32(coef) < 1)
    if norm == 0:
        assert st['scale'] == 1.0


def test_decide_reference_on_the_scripted_sequence():
    st = GG.fresh_state()
    seen = []
    for kind, g in GG.SCRIPT:
        s, bad, _ = GG.stats_ref([g])
        st = GG.decide_ref(st, s, bad, GG.SCRIPT_MAX_NORM)
        seen.append((kind, st['skip'], float(st['scale'])))
        assert (st['skip'] == 1) == (kind in ('nan', 'inf'))
    assert [k for k, _, _ in seen] == ['clean', 'clipped', 'nan', 'clean', 'inf']
    assert seen[0][2] == 1.0 and seen[1][2] == float(np.float32(7.0 / (10.0 + 1e-6))) and seen[3][2] == 1.0
    rep = GG.report_ref(st)
    assert rep == {'steps': 5, 'skipped': 2, 'clipped': 1, 'last_norm': 2.0, 'last_nonfinite': 2, 'mean_norm': 17.0 / 3, 'max_norm_seen': 10.0}
    # a skipped step leaves the norm totals alone
    s0 = GG.decide_ref(GG.fresh_state(), 9.0, 0, None)
    s1 = GG.decide_ref(s0, 1e30, 3, None)
    assert (s1['norm_sum'], s1['norm_max'], s1['clipped']) == (3.0, 3.0, 0) and s1['skipped'] == 1 and s1['last_nonfinite'] == 3


def test_guarded_sgd_reference_reduces_to_the_plain_one():
    import train_glue_cases as TC
    for case in GG.SGD_CASES:
        o = GG.sgd_operands(case)
        m1, w1, bm, bw = GG.sgd_guarded_ref64(o['w'], o['mom'], o['grad'], clip=-1.0, rescale=1.0, scale=1.0, wd=0.0005)
        tm, tw, mag = TC.sgd_ref64(dict(wd=0.0005, rescale=1.0), torch.as_tensor(o['w']), torch.as_tensor(o['mom']), torch.as_tensor(o['grad']))
        assert np.array_equal(m1, tm.numpy()) and np.array_equal(w1, tw.numpy())
        assert (bm >= TC.sgd_bounds(tw, mag)[0].numpy()).all()              # the two extra roundings only widen it
        assert (TC.SGD_LR, TC.SGD_MOMENTUM) == (GG.SGD_LR, GG.SGD_MOMENTUM)
    # the clamp: a float32 evaluation in the kernel's operation order stays inside the bound, a clamp applied BEFORE the global scale does not
    case = dict(id='n4099-bf', n=4099, bf16=True)
    o = GG.sgd_operands(case)
    for cl in GG.SGD_CLIPS:
        f = np.float32
        c, rs, sc, lr, mo, wd = f(cl['clip']), f(cl['rescale']), f(cl['scale']), f(GG.SGD_LR), f(GG.SGD_MOMENTUM), f(GG.SGD_WD)
        m1, w1, bm, bw = GG.sgd_guarded_ref64(o['w'], o['mom'], o['grad'], cl['clip'], cl['rescale'], cl['scale'])
        t = np.clip((rs * o['grad']) * sc, -c, c)
        got = mo * o['mom'] - lr * (t + wd * o['w'])
        assert got.dtype == np.float32 and (np.abs(got - m1) <= bm).all()
        assert (np.abs((o['w'] + got).astype(np.float64) - w1) <= bw).all()
        if cl['scale'] != 1.0:
            wrong = mo * o['mom'] - lr * (np.clip(rs * o['grad'], -c, c) * sc + wd * o['w'])
            assert (np.abs(wrong - m1) > bm).any()
    assert (np.abs(o['grad']) > 0.5).mean() > 0.2                            # the clamp is exercised
