"""csrc/relation.hip and csrc/relation_bwd.hip at the pad edges (tests/relation_edge_cases.py): every forward variant -- streaming fp32, streaming
bf16 with an fp32 bias, LDS kernel with the fp16 log2 G bias, LDS kernel with the float32 ln G bias, fused geometry + attention -- on both sides of a
32-key tile, of the 320-key LDS chunk, of 16 wavefronts per workgroup and of the fused kernel's 640 keys, with M = 1, B = 9 and several workgroups
per (image, head); against float64 from the definition, per element, within the bound derived in relation_edge_cases (the fused kernel: the project's
own criterion against the fp32-geometry streaming result).  Which kernel ran is asked of the library after every launch
(relnet_relation_attention_last_launch).

Guarded buffers: every operand a strided view in the middle of a NaN-filled parent, outputs in sentinel-filled parents through the C ABI; after every
launch no output element is non-finite, nothing outside the outputs changed and no input changed, bit for bit.

key_count: NaN, +Inf and zeros in the padding rows of features / q / k (so that the VW^T columns of the padded keys are non-finite themselves) and in
the bias columns of padded keys give bit-identical, finite real rows; the clamps min(max(count, 1), M) hold bit for bit; once through
RelationHead.forward with NaN in the padding rows of `pooled` and `rois`.

Backward: fp32 and bf16 against float64 autograd of oracle/relation_torch.py at the pad edges and on both sides of the small-kernel limit
(N, Mpad <= 128), and the one-workgroup form against the two-kernel form bit for bit.

RELNET_TEST_REPORT=<file> appends the worst err / tolerance per forward variant and output."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import cases  # noqa: E402
import gemm_cases as GC  # noqa: E402
import relation_edge_cases as RC  # noqa: E402
from oracle import relation_torch as ORT  # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32, F16 = torch.bfloat16, torch.float32, torch.float16
_ids = lambda cs: [c['id'] for c in cs]

WORST = {}                 # (variant, output) -> (largest err / tolerance, where)
CHECKED = {}


def _note(variant, what, ratio, where):
    key = (variant, what)
    CHECKED[key] = CHECKED.get(key, 0) + 1
    if key not in WORST or ratio > WORST[key][0]:
        WORST[key] = (ratio, where)


@pytest.fixture(scope='module')
def rn():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops, relation, lib
    L = lib.load()
    try:
        yield ops, relation, lib, L
    finally:
        L.relnet_relation_attention_debug_lds_f32(1)
        path = os.environ.get('RELNET_TEST_REPORT')
        if path and WORST:
            with open(path, 'a') as f:
                for (v, what), (ratio, where) in sorted(WORST.items()):
                    f.write('%-12s %-7s %5d launches, worst err / tolerance %.4f  at %s\n' % (v, what, CHECKED[(v, what)], ratio, where))


def _attention(rn, variant, q, k, vwt, bias, M, cfg, bout, resid, key_count=None, boxes=None, wp=None, bp=None):
    """One launch of `variant` through the kernel-level wrapper; asserts that the variant asked for is the one that ran."""
    ops, _, _, L = rn
    bo = bout if cfg['bout'] else None
    rs = resid if cfg['resid'] else None
    if variant == 'fused':
        out, act = ops.relation_attention_fused(q, k, vwt, boxes, wp, bp, bout=bo, resid=rs, M=M, want_out=cfg['out'], want_act=cfg['act'])
        logits = None
    else:
        want_logits = cfg['logits'] and variant.startswith('stream')
        try:
            if variant == 'stream_bf16':
                L.relnet_relation_attention_debug_lds_f32(0)
            out, act, logits = ops.relation_attention(q, k, vwt, bias, bout=bo, resid=rs, M=M, want_out=cfg['out'], want_act=cfg['act'],
                                                      want_logits=want_logits, key_count=key_count)
        finally:
            L.relnet_relation_attention_debug_lds_f32(1)
    assert L.relnet_relation_attention_last_launch() == RC.LAUNCH[variant], (variant, 'ran', L.relnet_relation_attention_last_launch())
    return out, act, logits


def _device_operands(case, o):
    dt = case['in_dtype']
    d = dict(q=o['q'].cuda().to(dt), k=o['k'].cuda().to(dt), vwt=o['vwt'].cuda().to(dt), bout=o['bout'].cuda(), resid=o['resid'].cuda().to(dt))
    if case['variant'] == 'fused':
        d.update(boxes=o['boxes'].cuda(), wp=o['wp'].cuda(), bp=o['bp'].cuda(), bias=None)
    else:
        d['bias'] = o['bias_raw'].cuda()
    return d


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. every forward variant at the tile, chunk and workgroup edges
# ---------------------------------------------------------------------------------------------------------------------------------------------
_FWD = [c for c in RC.FORWARD_CASES if c['variant'] != 'fused']
_FUSED = [c for c in RC.FORWARD_CASES if c['variant'] == 'fused']


@pytest.mark.parametrize('case', _FWD, ids=_ids(_FWD))
def test_forward_variant_at_the_edges(rn, case, monkeypatch):
    RC.check_case(case)
    if case['waves']:
        monkeypatch.setenv('RELNET_ATTN_WAVES', str(case['waves']))
    else:
        monkeypatch.delenv('RELNET_ATTN_WAVES', raising=False)
    v, M = case['variant'], case['M']
    bf = case['in_dtype'] == BF16
    o = RC.operands(case)
    d = _device_operands(case, o)
    base = RC.ref64_base(d['q'], d['k'], d['vwt'], o['bias'].cuda(), M)
    assert base['max_logit'] <= 100.0
    for cfg in RC.CONFIGS:
        ref = RC.configure(base, d['bout'] if cfg['bout'] else None, d['resid'] if cfg['resid'] else None)
        t_y, t_act = RC.tolerances(ref, M, bf)
        out, act, logits = _attention(rn, v, d['q'], d['k'], d['vwt'], d['bias'], M, cfg, d['bout'], d['resid'])
        where = (case['id'], cfg['id'])
        assert (out is not None) == cfg['out'] and (act is not None) == cfg['act']
        if out is not None:
            r = RC.worst_ratio(out, ref['y'], t_y)
            print('%s %s out: worst err / tolerance %.4f' % (where + (r,)))
            _note(v, 'out', r, where)
            assert r <= 1.0, (where, 'out', r)
        if act is not None:
            r = RC.worst_ratio(act, ref['act'], t_act)
            print('%s %s act: worst err / tolerance %.4f' % (where + (r,)))
            _note(v, 'act', r, where)
            assert r <= 1.0, (where, 'act', r)
            assert bool((act >= 0).all())
        if logits is not None:
            assert tuple(logits.shape) == (case['B'], case['N'], RC.H, M)
            e = float((logits.double() - ref['logits']).abs().max())
            print('%s %s logits: max |dL| %.3e' % (where + (e,)))
            _note(v, 'logits', e / RC.LOGIT_TOL, where)
            assert e <= RC.LOGIT_TOL, (where, 'logits', e)
        else:
            assert not (cfg['logits'] and v.startswith('stream'))


@pytest.mark.parametrize('case', _FUSED, ids=_ids(_FUSED))
def test_fused_variant_at_the_edges(rn, case):
    """The project's own criterion (tests/test_gpu_relation.py::test_fused_geometry_attention_kernel) at the new shapes: against the fp32-geometry
    streaming result on the same bf16 operands, max error <= 2^-6 of the output scale and mean error <= 1.25 x the two-kernel path's + 1e-6 scale."""
    ops, relation, lib, L = rn
    RC.check_case(case)
    M = case['M']
    o = RC.operands(case)
    d = _device_operands(case, o)
    wp_t = d['wp'].t().contiguous()
    b32 = ops.geometry_bias(d['boxes'], wp_t, d['bp'], M, half=False)[0]
    b16 = ops.geometry_bias(d['boxes'], wp_t, d['bp'], M, half=True)[0]
    for cfg in RC.CONFIGS:
        ref = _attention(rn, 'stream_bf16', d['q'], d['k'], d['vwt'], b32, M, dict(cfg, logits=False), d['bout'], d['resid'])
        two = _attention(rn, 'lds_f16', d['q'], d['k'], d['vwt'], b16, M, cfg, d['bout'], d['resid'])
        fus = _attention(rn, 'fused', d['q'], d['k'], d['vwt'], None, M, cfg, d['bout'], d['resid'], boxes=d['boxes'], wp=d['wp'], bp=d['bp'])
        for i, what in ((0, 'out'), (1, 'act')):
            if ref[i] is None:
                assert fus[i] is None
                continue
            r, t, u = ref[i].float(), two[i].float(), fus[i].float()
            assert bool(torch.isfinite(u).all())
            scale = r.abs().max().item()
            e_two, e_fus = (t - r).abs().max().item(), (u - r).abs().max().item()
            m_two, m_fus = (t - r).abs().mean().item(), (u - r).abs().mean().item()
            print('%s %s %s: two-kernel - ref max %.3e mean %.3e | fused - ref max %.3e mean %.3e (scale %.3e)'
                  % (case['id'], cfg['id'], what, e_two, m_two, e_fus, m_fus, scale))
            _note('fused', what, e_fus / (2.0 ** -6 * scale), (case['id'], cfg['id']))
            assert e_fus <= 2.0 ** -6 * scale, (what, e_fus, scale)
            assert m_fus <= 1.25 * m_two + 1e-6 * scale, (what, m_fus, m_two)
        if fus[1] is not None:
            assert torch.equal(fus[1], torch.relu(fus[1]))


def test_fused_limit_of_640_keys(rn):
    """Past FUSED_MAX_KEYS the module takes the two-kernel path (bit for bit the same tensor), and the fused entry point refuses instead of launching."""
    ops, relation, lib, L = rn
    n = m = 641
    boxes, feat, p = cases.relation_case(n, m, 641, 0.02)
    pt = {k: torch.as_tensor(v) for k, v in p.items()}
    mod = relation.RelationParams(pt, 1, BF16, 'cuda')
    f, bx = torch.as_tensor(feat).cuda().to(BF16)[None], torch.as_tensor(boxes).cuda()[None]
    assert not relation.fused_ok(BF16, m) and relation.fused_ok(BF16, m - 1)
    y_fused = relation.attention_module_multi_head(f, bx, pt, nongt_dim=m, dtype=BF16, packed=mod, fused=True)
    assert L.relnet_relation_attention_last_launch() == RC.LAUNCH['lds_f16']
    y_two = relation.attention_module_multi_head(f, bx, pt, nongt_dim=m, dtype=BF16, packed=mod, fused=False)
    assert torch.equal(y_fused, y_two) and bool(torch.isfinite(y_two).all())
    # the kernel-level entry points: the wrapper and the C ABI both refuse M = 641
    d = 1024
    qk = torch.zeros(1, n, 2 * d, device='cuda', dtype=BF16)
    vwt = torch.zeros(1, d, RC.pad32(m), device='cuda', dtype=BF16)
    with pytest.raises((AssertionError, lib.RelnetError)):
        ops.relation_attention_fused(qk[:, :, :d], qk[:, :m, d:], vwt, bx, mod.wp_dev, mod.bp_dev, M=m)
    out = torch.full((1, n, d), 7.0, device='cuda', dtype=BF16)
    div = ops.embedding_divisors().contiguous()
    q, k = qk[:, :, :d], qk[:, :m, d:]
    with pytest.raises(lib.RelnetError, match='M <= 640'):
        lib.call('relnet_relation_attention_fused', q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0),
                 vwt.data_ptr(), vwt.stride(1), vwt.stride(0), bx.data_ptr(), 4, 0, mod.wp_dev.data_ptr(), mod.bp_dev.data_ptr(), div.data_ptr(),
                 0, 0, 0, 0, out.data_ptr(), d, n * d, 0, d, n * d, 1, 16, n, m, RC.pad32(m), 0.125, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert L.relnet_relation_attention_last_launch() == RC.LAUNCH['lds_f16'] and bool((out == 7.0).all())      # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. guarded buffers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _abi_launch(rn, G, case, cfg, key_count):
    """The C-ABI entry points on the guarded views (outputs included)."""
    ops, _, lib, L = rn
    B, N, M, Mpad = case['B'], case['N'], case['M'], case['Mpad']
    q, k, vwt = G.q, G.k, G.vwt.view
    out, act, lg = G.out.view, G.act.view, G.logits.view
    want_logits = cfg['logits'] and case['variant'].startswith('stream')
    p = lambda t, on=True: t.data_ptr() if on else 0
    rs = G.resid.view
    st = torch.cuda.current_stream().cuda_stream
    if case['variant'] == 'fused':
        div = ops.embedding_divisors().contiguous()
        lib.call('relnet_relation_attention_fused', q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0),
                 vwt.data_ptr(), vwt.stride(1), vwt.stride(0), G.boxes.view.data_ptr(), 4, 0, G.wp.view.data_ptr(), G.bp.view.data_ptr(),
                 div.data_ptr(), p(G.bout.view, cfg['bout']), p(rs, cfg['resid']), rs.stride(1) if cfg['resid'] else 0,
                 rs.stride(0) if cfg['resid'] else 0, p(out, cfg['out']), out.stride(1), out.stride(0), p(act, cfg['act']), act.stride(1), act.stride(0),
                 B, RC.H, N, M, Mpad, RC.SCALE, st)
    else:
        dt = lib.F32 if case['in_dtype'] == F32 else lib.BF16
        bias = G.bias.view
        try:
            if case['variant'] == 'stream_bf16':
                L.relnet_relation_attention_debug_lds_f32(0)
            lib.call('relnet_relation_attention_kc', q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0),
                     vwt.data_ptr(), vwt.stride(1), vwt.stride(0), bias.data_ptr(), int(bias.dtype == F16), bias.stride(0),
                     p(G.bout.view, cfg['bout']), p(rs, cfg['resid']), rs.stride(1) if cfg['resid'] else 0, rs.stride(0) if cfg['resid'] else 0,
                     p(out, cfg['out']), out.stride(1), out.stride(0), p(act, cfg['act']), act.stride(1), act.stride(0), p(lg, want_logits),
                     B, RC.H, N, M, Mpad, RC.SCALE, dt, dt, p(G.key_count.view, key_count is not None), st)
        finally:
            L.relnet_relation_attention_debug_lds_f32(1)
    assert L.relnet_relation_attention_last_launch() == RC.LAUNCH[case['variant']]
    return (out if cfg['out'] else None, act if cfg['act'] else None, lg if want_logits else None)


@pytest.mark.parametrize('case', RC.GUARDED_CASES, ids=_ids(RC.GUARDED_CASES))
def test_operands_in_nan_filled_parents(rn, case):
    """A kernel that reads outside an operand, or lets a pad column of the bias reach an output, shows up as NaN; a store outside an output breaks the
    sentinel.  The values must equal, bit for bit, what the same kernel gives on dense copies of the operands (checked against float64 in part 1)."""
    RC.check_case(case)
    v, M, B = case['variant'], case['M'], case['B']
    o = RC.operands(case)
    G = RC.GuardedOperands(case, o)
    d = _device_operands(case, o)
    assert G.q.stride(1) == 2 * RC.D and G.k.shape[1] > M and G.resid.view.stride(1) > RC.D and G.vwt.view.stride(1) > case['Mpad']
    counts = None
    if v in RC.KC_VARIANTS and M > 1:
        counts = [M, (2 * M) // 3][:B] if B > 1 else [M - 1]
        G.key_count.view.copy_(torch.tensor(counts, dtype=torch.int32))
    kc_dense = torch.tensor(counts, dtype=torch.int32).cuda() if counts is not None else None
    snap = G.snapshot()
    for cfg in RC.CONFIGS:
        G.reset_outputs()
        got = _abi_launch(rn, G, case, cfg, counts)
        torch.cuda.synchronize()
        want = _attention(rn, v, d['q'], d['k'], d['vwt'], d['bias'], M, cfg, d['bout'], d['resid'], key_count=kc_dense,
                          boxes=d.get('boxes'), wp=d.get('wp'), bp=d.get('bp'))
        where = (case['id'], cfg['id'])
        for g_, w_, buf, name in zip(got, want, (G.out, G.act, G.logits), ('out', 'act', 'logits')):
            if g_ is None:
                assert w_ is None and GC.guards_intact(buf.buf, buf.view[:0]), (where, name, 'an output that was not asked for was written')
                continue
            if name == 'logits' and counts is not None:      # masked keys are -inf by definition; every other element is finite
                for b, c in enumerate(counts):
                    assert bool(torch.isfinite(g_[b, :, :, :c]).all()) and bool((g_[b, :, :, c:] == float('-inf')).all()), (where, name)
            else:
                assert bool(torch.isfinite(g_).all()), (where, name, 'non-finite output: a read outside an operand, or a pad column, reached it')
            assert GC.guards_intact(buf.buf, buf.view), (where, name, 'stored outside the output')
            assert torch.equal(g_, w_), (where, name, 'differs from the launch on dense operands')
        assert G.inputs_unchanged(snap), (where, 'an input changed')


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. key_count with non-finite padding rows
# ---------------------------------------------------------------------------------------------------------------------------------------------
_KC_SETUPS = [(70, [70, 1, 31, 32, 33, 69]), (322, [322, 320, 321, 1])]
_POISON = (('nan', float('nan')), ('inf', float('inf')), ('zero', 0.0))


def _kc_operands(rn, variant, n, counts, poison):
    """q | k and VW^T from the features through ops.gemm_nt as relation._module_forward forms them, the padding rows of features / q / k and the bias
    columns of the padded keys holding `poison`."""
    ops, relation, _, _ = rn
    dt = F32 if variant == 'stream_f32' else BF16
    B, m = len(counts), n
    _, _, p = cases.relation_case(8, 8, 300 + n, 0.03)
    mod = relation.RelationParams({k: torch.as_tensor(v) for k, v in p.items()}, 1, dt, 'cuda')
    g = torch.Generator().manual_seed(1000 + n)
    f = torch.randn(B, n, 1024, generator=g).cuda().to(dt)
    lo, hi = RC.LN_G_RANGE
    u = (torch.rand(B, RC.H, n, RC.pad32(m), generator=g) * (hi - lo) + lo).cuda()
    bias = (u / RC.LN2).to(F16) if variant == 'lds_f16' else u
    for b, c in enumerate(counts):
        f[b, c:] = poison
        bias[b, :, :, c:] = poison
    qk = ops.gemm_nt(f.reshape(B * n, 1024), mod.wqk, mod.bqk).reshape(B, n, -1)
    for b, c in enumerate(counts):
        qk[b, c:] = poison
    vwt = torch.zeros((B, 1024, RC.pad32(m)), device='cuda', dtype=dt)
    ops.gemm_nt(mod.wout, f[:, :m, :], out=vwt, n_cols=m)
    return dict(f=f, q=qk[:, :, :1024], k=qk[:, :m, 1024:], vwt=vwt, bias=bias, bout=mod.bout)


_CFG_ALL = dict(id='out+act', out=True, act=True, bout=True, resid=True, logits=True)


@pytest.mark.parametrize('variant', RC.KC_VARIANTS)
@pytest.mark.parametrize('n,counts', _KC_SETUPS, ids=['70', '322'])
def test_key_count_with_non_finite_padding_rows(rn, variant, n, counts):
    """Keys >= key_count[b] contribute an exact zero whatever their rows hold: the real rows of out / act / logits are bit-identical whether the padding
    rows hold NaN, +Inf or zeros, finite, and equal to the image run alone at nongt_dim = count (2e-5 fp32 / 3e-2 bf16 of max-abs, the tolerances of
    test_gpu_relation_bwd.py::test_key_count_masks_padding_rows)."""
    tol = 2e-5 if variant == 'stream_f32' else 3e-2
    kc = torch.tensor(counts, dtype=torch.int32).cuda()
    runs = {}
    for name, poison in _POISON:
        d = _kc_operands(rn, variant, n, counts, poison)
        if name != 'zero':
            for b, c in enumerate(counts):
                if c < n:                    # the setup does what it says: the VW^T columns of the padded keys are non-finite themselves
                    assert not bool(torch.isfinite(d['vwt'][b, :, c:n]).any())
        runs[name] = (d, _attention(rn, variant, d['q'], d['k'], d['vwt'], d['bias'], n, _CFG_ALL, d['bout'], d['f'], key_count=kc))
    for b, c in enumerate(counts):
        for i, what in ((0, 'out'), (1, 'act'), (2, 'logits')):
            z = runs['zero'][1][i]
            if z is None:
                assert what == 'logits' and not variant.startswith('stream')
                continue
            real = z[b, :c, :, :c] if what == 'logits' else z[b, :c]
            assert bool(torch.isfinite(real).all()), (variant, b, c, what, 'zeros in the padding rows')
            for name in ('nan', 'inf'):
                t = runs[name][1][i]
                got = t[b, :c, :, :c] if what == 'logits' else t[b, :c]
                nonfinite = int((~torch.isfinite(got)).sum())
                assert nonfinite == 0, (variant, 'image', b, 'count', c, what, name + ' in the padding rows', '%d non-finite elements in the real rows' % nonfinite)
                assert torch.equal(got, real), (variant, b, c, what, name)
            if what == 'logits':
                assert bool((z[b, :c, :, c:] == float('-inf')).all())
        # the same image alone at nongt_dim = count
        d, (out, act, _) = runs['zero']
        cp = RC.pad32(c)
        vw1 = torch.zeros((1, 1024, cp), device='cuda', dtype=d['vwt'].dtype)
        vw1[..., :c] = d['vwt'][b, :, :c]
        b1 = torch.zeros((1, RC.H, c, cp), device='cuda', dtype=d['bias'].dtype)
        b1[..., :c] = d['bias'][b, :, :c, :c]
        o1, a1, _ = _attention(rn, variant, d['q'][b:b + 1, :c], d['k'][b:b + 1, :c], vw1, b1, c, dict(_CFG_ALL, logits=False), d['bout'], d['f'][b:b + 1, :c])
        for full, one, what in ((out, o1, 'out'), (act, a1, 'act')):
            err = (full[b, :c].float() - one[0].float()).abs().max().item() / one.float().abs().max().item()
            assert err <= tol, (variant, b, c, what, err)


@pytest.mark.parametrize('variant', RC.KC_VARIANTS)
def test_key_count_clamps(rn, variant):
    """key_count[b] = 0 behaves as 1 and a count above M as M: the min(max(count, 1), M) of every kernel, bit for bit."""
    n = 70
    d = _kc_operands(rn, variant, n, [n] * 4, 0.0)
    res = []
    for counts in ([0, n + 5, 1, n], [1, n, 1, n]):
        kc = torch.tensor(counts, dtype=torch.int32).cuda()
        res.append(_attention(rn, variant, d['q'], d['k'], d['vwt'], d['bias'], n, _CFG_ALL, d['bout'], d['f'], key_count=kc))
    none = _attention(rn, variant, d['q'], d['k'], d['vwt'], d['bias'], n, _CFG_ALL, d['bout'], d['f'])
    for i in range(3):
        if res[0][i] is None:
            continue
        assert torch.equal(res[0][i], res[1][i]), (variant, i)
        assert torch.equal(res[0][i][1], none[i][1]) and torch.equal(res[0][i][3], none[i][3])      # a count of M (or more) is no count
        assert bool(torch.isfinite(res[0][i][:, :, :64] if i < 2 else res[0][i][1]).all())


@pytest.mark.parametrize('small', ['1', '0'])
def test_key_count_clamps_backward(rn, small, monkeypatch):
    ops = rn[0]
    monkeypatch.setenv('RELNET_REL_BWD_SMALL', small)
    B, n, m, d = 4, 64, 40, 1024
    g = torch.Generator().manual_seed(64040)
    mpad = ops.pad32(m)
    qk = (torch.randn(B, n, 2 * d, generator=g) * 0.3).cuda().to(BF16)
    q, k = qk[:, :, :d], qk[:, :m, d:]
    vw = (torch.randn(B, m, d, generator=g) * 0.3).cuda().to(BF16)
    dy = torch.randn(B, n, d, generator=g).cuda().to(BF16)
    y = torch.randn(B, n, d, generator=g).cuda().to(BF16)
    bout = torch.randn(d, generator=g).cuda()
    bias = (torch.randn(B, 16, n, mpad, generator=g) - 2.0).cuda()
    kt = torch.zeros(B, d, mpad, device='cuda', dtype=BF16); ops.transpose_2d(k, out=kt)
    qt = ops.transpose_2d(q, pad_cols_to=32); dyt = ops.transpose_2d(dy, pad_cols_to=32)
    res = [ops.relation_attention_bwd(q, k, kt, vw, bias, dy, y, bout, qt, dyt, m, key_count=torch.tensor(c, dtype=torch.int32).cuda())
           for c in ([0, m + 9, 1, m], [1, m, 1, m])]
    assert (res[0][3] is None) == (small == '1')
    for i in (0, 1, 2):
        assert torch.equal(res[0][i], res[1][i]) and bool(torch.isfinite(res[0][i]).all())
    assert torch.equal(res[0][4][..., :m], res[1][4][..., :m])


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_relation_head_with_nan_padding_rows(rn, dtype):
    """RelationHead.forward(pooled, rois, key_count=...) with NaN in the padding rows of both `pooled` and `rois`: the real rows of every output are
    finite and bit-identical to the run with zeros there (two relation modules in a row: the second one's VW^T comes from the first one's NaN rows)."""
    ops, relation, _, _ = rn
    dt = F32 if dtype == 'f32' else BF16
    B, n, C = 3, 40, 5
    counts = [40, 1, 33]
    rng = np.random.default_rng(4033)
    params = {}
    for i in (1, 2):
        params.update(cases.relation_case(8, 8, 70 + i, 0.03, index=i)[2])
    nrm = lambda *s, std=0.02: torch.as_tensor(rng.normal(0, std, s).astype(np.float32))
    params.update(fc_new_1_weight=nrm(1024, 12544, std=0.01), fc_new_1_bias=nrm(1024), fc_new_2_weight=nrm(1024, 1024, std=0.03), fc_new_2_bias=nrm(1024),
                  cls_score_weight=nrm(C, 1024), cls_score_bias=nrm(C), bbox_pred_weight=nrm(8, 1024), bbox_pred_bias=nrm(8))
    params = {k: torch.as_tensor(v) for k, v in params.items()}
    head = relation.RelationHead(params, dtype=dt)
    pooled = torch.as_tensor(rng.normal(0, 1, (B, n, 12544)).astype(np.float32)).cuda().to(dt)
    rois = torch.zeros(B, n, 5, device='cuda')
    for b in range(B):
        rois[b, :, 0] = b
        rois[b, :, 1:] = torch.as_tensor(cases.random_boxes(n, 900 + b)).cuda()
    kc = torch.tensor(counts, dtype=torch.int32).cuda()
    outs = []
    for poison in (float('nan'), 0.0):
        pl, rs = pooled.clone(), rois.clone()
        for b, c in enumerate(counts):
            pl[b, c:] = poison
            rs[b, c:] = poison
        outs.append(head.forward(pl, rs, key_count=kc))
    for b, c in enumerate(counts):
        for t_nan, t_zero, what in zip(outs[0], outs[1], ('cls_score', 'bbox_pred', 'fc_all_2_relu')):
            assert bool(torch.isfinite(t_nan[b, :c]).all()), (dtype, b, c, what, 'non-finite real rows with NaN padding rows')
            assert torch.equal(t_nan[b, :c], t_zero[b, :c]), (dtype, b, c, what)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. backward at the pad edges
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _autograd(feat, boxes, p, m, d_out):
    ft = torch.tensor(feat.astype(np.float64), requires_grad=True)
    pt = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in p.items()}
    y = ORT.relation_module(ft, boxes, pt, 1, m)
    (y * torch.as_tensor(d_out.astype(np.float64))).sum().backward()
    g = {k: v.grad.numpy() for k, v in pt.items()}
    g['d_roi_feat'] = ft.grad.numpy()
    return g


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


_ZERO_AT_M1 = ('query_1_weight', 'query_1_bias', 'key_1_weight', 'key_1_bias', 'pair_pos_fc1_1_weight', 'pair_pos_fc1_1_bias')


@pytest.mark.parametrize('n,m', RC.BWD_F32)
def test_backward_fp32_at_the_edges(rn, n, m):
    """attention_module_backward in fp32 against float64 autograd: every gradient within 2e-4 of its max-abs (pair_pos_fc1: 2e-3).  With one key the
    softmax has one term: the query, key and pair_pos gradients are exactly zero in exact arithmetic and are held, like key_1_bias everywhere, to an
    absolute 1e-5 of linear_out's gradient scale.

    The float32 backward forms D = sum_j p_j ds_j from the p and ds it uses itself, so sum_j dL_j cancels exactly with one key; a D taken from the
    stored output would leave a rounding residue that the geometry backward multiplies by 1 / G (up to 1e6)."""
    relation = rn[1]
    boxes, feat, p = cases.relation_case(n, m, 7000 + 13 * n + m, 0.04)
    d_out = np.random.default_rng(n * 1000 + m).normal(0, 1, (n, 1024)).astype(np.float32)
    want = _autograd(feat, boxes, p, m, d_out)
    pt = {k: torch.as_tensor(v) for k, v in p.items()}
    got = relation.attention_module_backward(torch.as_tensor(feat).cuda(), torch.as_tensor(boxes).cuda(), pt, torch.as_tensor(d_out).cuda(),
                                             nongt_dim=m, dtype=F32)
    assert set(got) == set(want)
    lin = np.abs(want['linear_out_1_weight']).max()
    missed = []
    for k in sorted(want):
        g = got[k].cpu().numpy().reshape(want[k].shape)
        assert np.isfinite(g).all(), k
        if m == 1 and k in _ZERO_AT_M1:
            assert np.abs(want[k]).max() < 1e-12 * max(lin, 1.0), (k, np.abs(want[k]).max())
            print('%dx%d %s: max |g| %.3e, %.3e of the linear_out scale %.3e' % (n, m, k, np.abs(g).max(), np.abs(g).max() / lin, lin))
            if not np.abs(g).max() <= 1e-5 * lin:
                missed.append((k, float(np.abs(g).max()), float(lin)))
            continue
        if k == 'key_1_bias':      # exactly zero in exact arithmetic (softmax is invariant to a shift of all keys): as test_gpu_relation_bwd.py
            assert np.abs(want[k]).max() < 1e-12 and np.abs(g).max() <= 1e-5 * np.abs(want['query_1_bias']).max()
            continue
        tol = 2e-3 if k.startswith('pair_pos') else 2e-4
        print('%dx%d %s: rel err %.3e' % (n, m, k, _rel(g, want[k])))
        assert _rel(g, want[k]) <= tol, (k, _rel(g, want[k]))
    assert not missed, ('exactly zero in exact arithmetic, above 1e-5 of the linear_out scale: (name, max |g|, scale)', missed)


@pytest.mark.parametrize('n,m', RC.BWD_BF16)
def test_backward_bf16_at_the_edges(rn, n, m):
    """bf16, B = 2, against autograd on the bf16-rounded operands within 4e-2; (128,128), (129,97), (160,129) put the limit of the one-workgroup
    kernel (N <= 128, Mpad <= 128) on both sides."""
    ops, relation = rn[0], rn[1]
    assert ops.relation_bwd_small_ok(BF16, n, ops.pad32(m)) == (n <= 128 and ops.pad32(m) <= 128)
    assert ops.relation_bwd_small_ok(BF16, n, ops.pad32(m)) == ((n, m) in ((33, 32), (65, 33), (128, 128)))
    boxes0, feat0, p = cases.relation_case(n, m, 8000 + 13 * n + m, 0.04)
    boxes1 = cases.random_boxes(n, 777 + n)
    rng = np.random.default_rng(n * 1000 + m + 1)
    feat1 = rng.normal(0, 1, feat0.shape).astype(np.float32)
    d_out = rng.normal(0, 1, (2, n, 1024)).astype(np.float32)
    r = lambda a: torch.as_tensor(a).to(BF16).float().numpy()
    pr = {k: (r(v) if 'pair_pos' not in k and 'bias' not in k else v) for k, v in p.items()}
    w0 = _autograd(r(feat0), boxes0, pr, m, r(d_out[0]))
    w1 = _autograd(r(feat1), boxes1, pr, m, r(d_out[1]))
    pt = {k: torch.as_tensor(v) for k, v in p.items()}
    got = relation.attention_module_backward(torch.as_tensor(np.stack([feat0, feat1])).cuda(), torch.as_tensor(np.stack([boxes0, boxes1])).cuda(), pt,
                                             torch.as_tensor(d_out).cuda(), nongt_dim=m, dtype=BF16)
    for k in sorted(w0):
        want = np.stack([w0[k], w1[k]]) if k == 'd_roi_feat' else w0[k] + w1[k]
        g = got[k].float().cpu().numpy().reshape(want.shape)
        assert np.isfinite(g).all(), k
        if k == 'key_1_bias':
            assert np.abs(g).max() <= 1e-2 * np.abs(w0['query_1_bias'] + w1['query_1_bias']).max()
            continue
        print('%dx%d %s: rel err %.3e' % (n, m, k, _rel(g, want)))
        assert _rel(g, want) <= 4e-2, (k, _rel(g, want))


@pytest.mark.parametrize('n,m,counts', RC.BWD_SMALL, ids=['%dx%d%s' % (n, m, '-kc' if c else '') for n, m, c in RC.BWD_SMALL])
def test_small_backward_equals_the_two_kernel_form_at_the_edges(rn, n, m, counts, monkeypatch):
    """relation_attention_bwd_small_kernel against the two-kernel form on the same operands, bit for bit (as
    test_gpu_relation_bwd.py::test_small_n_fused_backward_equals_the_two_kernel_form), at one query / one key, 33 = one tile + 1 and the 128 limit."""
    ops = rn[0]
    B, H, d = 5, 16, 1024
    g = torch.Generator().manual_seed(n * 7 + m)
    mpad = ops.pad32(m)
    qk = (torch.randn(B, n, 2 * d, generator=g) * 0.3).cuda().to(BF16)
    q, k = qk[:, :, :d], qk[:, :m, d:]
    vw = (torch.randn(B, m, d, generator=g) * 0.3).cuda().to(BF16)
    dy = torch.randn(B, n, d, generator=g).cuda().to(BF16)
    y = torch.randn(B, n, d, generator=g).cuda().to(BF16)
    bout = torch.randn(d, generator=g).cuda()
    bias = (torch.randn(B, H, n, mpad, generator=g) - 2.0).cuda()
    kt = torch.zeros(B, d, mpad, device='cuda', dtype=BF16); ops.transpose_2d(k, out=kt)
    qt = ops.transpose_2d(q, pad_cols_to=32); dyt = ops.transpose_2d(dy, pad_cols_to=32)
    key_count = torch.tensor(counts, dtype=torch.int32).cuda() if counts else None
    assert ops.relation_bwd_small_ok(BF16, n, mpad)
    res = {}
    for small in ('1', '0'):
        monkeypatch.setenv('RELNET_REL_BWD_SMALL', small)
        res[small] = ops.relation_attention_bwd(q, k, kt, vw, bias, dy, y, bout, qt, dyt, m, key_count=key_count)
    assert res['1'][3] is None and res['0'][3] is not None
    for i, name in ((0, 'dq'), (1, 'dk'), (2, 'dvw')):
        assert torch.equal(res['1'][i], res['0'][i]), name
        assert bool(torch.isfinite(res['1'][i]).all()), name
    assert torch.equal(res['1'][4][..., :m], res['0'][4][..., :m])
    assert float(res['1'][2].abs().max()) > 0
    monkeypatch.setenv('RELNET_REL_BWD_SMALL', '1')
    a3 = torch.zeros(B, n, 3 * d, device='cuda', dtype=BF16)
    out = ops.relation_attention_bwd(q, k, kt, vw, bias, dy, y, bout, qt, dyt, m, key_count=key_count, packed_out=a3)
    assert out[0] is a3 and out[1] is None and out[2] is None
    assert torch.equal(a3, ops.relation_bwd_pack(res['1'][0], res['1'][1], res['1'][2]))
    assert torch.equal(out[4][..., :m], res['1'][4][..., :m])
