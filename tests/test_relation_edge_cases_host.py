"""CPU-side checks of tests/relation_edge_cases.py (no GPU, no library): the bound the GPU results of tests/test_gpu_relation_edges.py are held to
separates a correct float32 evaluation of the kernels' algorithm from subtly wrong ones, and every case of the tables meets the preconditions of
the variant it names.

The emulation (relation_edge_cases.emulate) is the algorithm of relation_attention_kernel in float32: online softmax over key tiles of 32, P rounded
to bf16 before the second product, float32 accumulation.  Correct, its unrounded result stays under HALF of the derived bound at every case of the
forward table (and its bf16-rounded result inside half the bound plus the half step the tolerance grants the output rounding).  The fused variant
evaluates the geometry itself and is held to the project's own criterion on the GPU, so it has no reference here.  Each mutant exceeds the tolerance
on at least one element at the cases written for it, with the operands (seeds) the GPU test uses."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relation_edge_cases as RC  # noqa: E402
import gemm_cases as GC  # noqa: E402

_ids = lambda cases: [c['id'] for c in cases]
_REF = {}


def _setup(case):
    """(operands, float64 reference with bout, float64 reference without) of a case, computed once per (shape, formats)."""
    key = (case['N'], case['M'], case['B'], case['in_dtype'], case['bias_dtype'])
    if key not in _REF:
        o = RC.operands(case)
        _REF[key] = (o, RC.ref64(o['q'], o['k'], o['vwt'], o['bias'], o['bout'], o['resid'], case['M']))
        if len(_REF) > 4:                       # the big cases hold a few hundred MB: keep the cache short
            _REF.pop(next(iter(_REF)))
    return _REF[key]


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        key = (c['N'], c['M'], c['B'], c['in_dtype'], c['bias_dtype'])
        if c['variant'] != 'fused' and key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize('case', RC.FORWARD_CASES + RC.GUARDED_CASES, ids=_ids(RC.FORWARD_CASES + RC.GUARDED_CASES))
def test_case_meets_the_preconditions_of_its_variant(case):
    assert RC.check_case(case)


def test_case_table_covers_the_edges_the_issue_names():
    have = {(c['variant'], c['N'], c['M'], c['B'], c['waves']) for c in RC.FORWARD_CASES}
    for v in RC.VARIANTS:
        for (n, m) in RC.SHAPES:
            assert (v, n, m, 1, None) in have
        for (n, m) in RC.SHAPES_B9:
            assert (v, n, m, 9, None) in have
        assert ((v, 641, 640, 1, None) in have) == (v in ('fused', 'lds_f16', 'lds_f32'))
    for v in ('lds_f16', 'lds_f32'):
        for (n, m) in RC.WAVES_SHAPES:
            for w in (1, 3):
                assert (v, n, m, 1, w) in have
    with pytest.raises(AssertionError):          # the table could not name the fused kernel past its limit
        RC.check_case(dict(RC._case('fused', 641, 641)))


@pytest.mark.parametrize('case', _unique(RC.FORWARD_CASES), ids=_ids(_unique(RC.FORWARD_CASES)))
def test_correct_emulation_uses_under_half_of_the_bound(case):
    o, ref = _setup(case)
    bf = case['in_dtype'] == RC.BF16
    M = case['M']
    bnd = RC.bound(ref, M, bf)
    y = RC.emulate(o, case, bf)
    r = RC.worst_ratio(y, ref['y'], bnd)
    print('%s: emulation err / bound %.4f' % (case['id'], r))
    assert r <= 0.5, (case['id'], r)
    if bf:                                       # rounded like the kernel's output: half the bound plus the half step the tolerance grants
        yr = RC.emulate(o, case, bf, round_out=True)
        assert RC.worst_ratio(yr, ref['y'], 0.5 * bnd + 0.5 * GC.step(ref['y'])) <= 1.0, case['id']
        t_y, _ = RC.tolerances(ref, M, bf)
        assert RC.worst_ratio(yr, ref['y'], t_y) <= 1.0


# mutant -> (emulate switches as a function of the case, the shapes written for it)
MUTANTS = {
    'mask off by one: key M included': (lambda c: dict(mask_limit=c['M'] + 1), [(31, 31), (33, 33), (65, 33), (322, 321)]),
    'mask off by one: key M - 1 dropped': (lambda c: dict(mask_limit=c['M'] - 1), [(31, 31), (32, 32), (33, 33), (321, 320)]),
    'bias pad column enters with value 0': (lambda c: dict(pad_bias_zero=True), [(33, 1), (31, 31), (33, 33), (322, 321)]),
    'last partial tile skipped': (lambda c: dict(skip_last_partial=True), [(33, 33), (65, 33), (322, 321), (513, 33)]),
    'bout dropped': (lambda c: dict(use_bout=False), [(1, 1), (33, 33), (321, 320)]),
    '1 / l from one 32-lane half': (lambda c: dict(half_l=True), [(31, 31), (32, 32), (129, 128), (322, 321)]),
    'chunk boundary drops key 320': (lambda c: dict(drop_key=320), [(322, 321), (513, 321), (641, 640)]),
}


@pytest.mark.parametrize('name', list(MUTANTS))
@pytest.mark.parametrize('variant', ['stream_f32', 'lds_f16', 'lds_f32'])
def test_mutant_exceeds_the_tolerance(name, variant):
    switches, shapes = MUTANTS[name]
    for (n, m) in shapes:
        if (n, m) == (641, 640) and variant == 'stream_f32':
            continue                             # not a case of that variant
        case = RC._case(variant, n, m)
        o, ref = _setup(case)
        bf = case['in_dtype'] == RC.BF16
        t_y, _ = RC.tolerances(ref, m, bf)
        good = RC.worst_ratio(RC.emulate(o, case, bf, round_out=bf), ref['y'], t_y)
        bad = RC.worst_ratio(RC.emulate(o, case, bf, round_out=bf, **switches(case)), ref['y'], t_y)
        print('%s, %s %dx%d: correct %.3f, mutant %.3g of the tolerance' % (name, variant, n, m, good, bad))
        assert good <= 1.0 and bad > 1.0, (name, variant, n, m, good, bad)


def test_reference_masks_by_key_count():
    """ref64 with key_count equals ref64 of the image cut to its count (what the GPU test compares against), clamps included."""
    case = RC._case('stream_f32', 33, 33, B=3)
    o = RC.operands(case)
    full = RC.ref64(o['q'], o['k'], o['vwt'], o['bias'], o['bout'], o['resid'], 33, key_count=[0, 17, 40])
    for b, c in enumerate([1, 17, 33]):
        one = RC.ref64(o['q'][b:b + 1], o['k'][b:b + 1, :c], o['vwt'][b:b + 1, :, :c], o['bias'][b:b + 1, :, :, :c], o['bout'], o['resid'][b:b + 1], c)
        assert torch.allclose(full['y'][b], one['y'][0], rtol=0, atol=1e-12)
