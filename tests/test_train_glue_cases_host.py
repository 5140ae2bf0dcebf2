"""CPU-side checks of tests/train_glue_cases.py (no GPU, no library).  Per kernel of the training step's glue:
  * the float64 reference equals float64 torch autograd / indexing of the same definition to 1e-12 (relative to the tensor's largest magnitude);
  * the float32 / bf16 emulation of the kernel's arithmetic order stays at or under HALF of the bound the GPU result is held to, on every case
    (bf16 outputs: before the store; the four formulas that grant a rounding exactly its worst case -- see train_glue_cases -- : inside the bound);
  * each mutant named in the case tables exceeds the bound at the cases named for it, with the operands (seeds) the GPU test uses;
  * the adjoint identity <embed(e), y> = <e, take_bwd(y)> holds for the references."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_glue_cases as TC  # noqa: E402

F64 = torch.float64
_ids = lambda cases: [c['id'] for c in cases]
_by_id = lambda cases: {c['id']: c for c in cases}


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# softmax_output
# ---------------------------------------------------------------------------------------------------------------------------------------------
_SM = {}


def _sm(case):
    if case['id'] not in _SM:
        data, label = TC.softmax_operands(case)
        _SM[case['id']] = (data, label) + TC.softmax_ref64(case, data, label)
    return _SM[case['id']]


def test_softmax_table_holds_the_shapes_groups_and_switches_of_the_issue():
    cs = TC.SOFTMAX_CASES
    flat = {(c['outer'], c['C']) for c in cs if not c['multi']}
    assert {(1, 1), (1, 2), (63, 81), (64, 81), (65, 81), (616, 81), (130, 300)} <= flat
    assert {(c['outer'], c['inner']) for c in cs if c['multi'] and c['group'] == c['inner']} >= {(B, i) for B in (1, 3) for i in (1, 63, 65, 420)}
    assert {c['group'] for c in cs} >= {0, 1, 7, 63, 64, 65, 308}
    assert {(c['total'], c['group']) for c in cs} >= {(616, 308), (130, 65)}
    for key, vals in (('use_ignore', {0, 1}), ('ignore_label', {-1.0, 255.0}), ('grad_scale', {1.0, 3.0}), ('special', {'all_ignored', 'one_valid'}),
                      ('label', {True, False})):
        assert {c[key] for c in cs} >= vals, key
    assert TC.SOFTMAX_BIG['total'] == 4096 * 256 + 257 and TC.SOFTMAX_BIG['C'] == 2 and TC.SOFTMAX_BIG['group'] == TC.SOFTMAX_BIG['inner']
    for c in cs:
        G, ng = TC.softmax_groups(c)
        assert G * ng == c['total']


@pytest.mark.parametrize('case', TC.SOFTMAX_CASES, ids=_ids(TC.SOFTMAX_CASES))
def test_softmax_reference_is_autograd_and_the_emulation_halves_the_tolerance(case):
    data, label, prob, grad = _sm(case)
    assert torch.isfinite(prob).all()
    x = data.double().requires_grad_(True)
    logits = TC.softmax_to2d(case, x)
    assert _rel(TC.softmax_to2d(case, prob), torch.softmax(logits, 1).detach()) <= 1e-12
    ep, eg = TC.softmax_emulate32(case, data, label)
    assert TC.close_ratio(ep, prob) <= 0.5
    assert TC.prob_rows_sum_to_one(case, ep) <= 0.5
    if label is None:
        assert grad is None and eg is None
        return
    # sum over groups of (sum of cross entropies of the non-ignored positions) / max(valid, 1), times grad_scale
    lab = label.reshape(-1)
    valid = TC.softmax_valid(case, label)
    G, ng = TC.softmax_groups(case)
    logp = torch.log_softmax(logits, 1)
    ce = -logp[torch.arange(lab.numel()), lab.clamp(0, case['C'] - 1).long()] * valid.double()
    per_group = ce.reshape(ng, G).sum(1) / valid.reshape(ng, G).sum(1).clamp_min(1).double()
    (per_group.sum() * case['grad_scale']).backward()
    assert _rel(grad, x.grad) <= 1e-12
    assert TC.close_ratio(eg, grad) <= 0.5
    ign = ~valid
    if bool(ign.any()):
        assert float(TC.softmax_to2d(case, grad)[ign].abs().max()) == 0.0 and float(TC.softmax_to2d(case, eg)[ign].abs().max()) == 0.0
    if case['special'] == 'all_ignored':                      # neighbours are normalised by their own count
        gi = ng // 2
        cnt = valid.reshape(ng, G).sum(1)
        assert int(cnt[gi]) == 0 and all(int(cnt[nb]) > 0 for nb in (gi - 1, gi + 1) if 0 <= nb < ng)
        assert float(TC.softmax_to2d(case, grad).reshape(ng, G, -1)[gi].abs().max()) == 0.0
    if case['special'] == 'one_valid':
        assert int(valid[:G].sum()) == 1


@pytest.mark.parametrize('mutant,cid', [(m, cid) for m, ids in sorted(TC.SOFTMAX_MUTANTS.items()) for cid in ids])
def test_softmax_mutant_is_rejected(mutant, cid):
    case = _by_id(TC.SOFTMAX_CASES)[cid]
    data, label, prob, grad = _sm(case)
    _, bad = TC.softmax_ref64(case, data, label, mutant=mutant)
    assert TC.close_ratio(bad.float(), grad) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# smooth_l1_loss, nms_loss
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', TC.SMOOTH_L1_CASES, ids=_ids(TC.SMOOTH_L1_CASES))
def test_smooth_l1_reference_is_autograd(case):
    pred, target, weight = TC.smooth_l1_operands(case)
    loss, grad = TC.smooth_l1_ref64(case, pred, target, weight)
    p = pred.double().requires_grad_(True)
    x = p - target.double()
    s2 = case['sigma'] ** 2
    l = torch.where(x.abs() < 1 / s2, 0.5 * s2 * x * x, x.abs() - 0.5 / s2) * (1 if weight is None else weight.double())
    (l.sum() * case['grad_scale']).backward()
    assert _rel(loss, l.detach()) <= 1e-12 and _rel(grad, p.grad) <= 1e-12
    # float32 in the kernel's order
    x32 = pred - target
    w32 = torch.ones_like(x32) if weight is None else weight
    inv = torch.tensor(1.0) / torch.tensor(s2)
    quad = x32.abs() < inv
    l32 = w32 * torch.where(quad, 0.5 * x32 * x32 * s2, x32.abs() - 0.5 * inv)
    g32 = torch.tensor(case['grad_scale']) * w32 * torch.where(quad, s2 * x32, torch.where(x32 > 0, 1.0, -1.0))
    assert TC.close_ratio(l32, loss) <= 0.5 and TC.close_ratio(g32, grad) <= 0.5


@pytest.mark.parametrize('case', TC.NMS_LOSS_CASES, ids=_ids(TC.NMS_LOSS_CASES))
def test_nms_loss_reference_is_finite_everywhere_and_is_autograd(case):
    score, target = TC.nms_loss_operands(case)
    assert float(score.min()) >= 0.0 and float(score.max()) <= 1.0
    k = min(case['n'], 8)
    assert score[:k].tolist() == [float(np.float32(v)) for v in (TC.NMS_SPECIAL_SCORES * 2)[:k]]
    pos, neg, grad = TC.nms_loss_ref64(case, score, target)
    for t in (pos, neg, grad):
        assert bool(torch.isfinite(t).all())                 # eps = 1e-8 keeps log and the quotients finite at s = 0 and s = 1: nothing to mask
    # autograd of pos_scale sum(pos) + sum(neg) with respect to the float32 operands a and b (da/ds = 1, db/ds = -1)
    eps = torch.tensor(case['eps'])
    a = (score + eps).double().requires_grad_(True)
    b = ((1.0 - score) + eps).double().requires_grad_(True)
    kk = float(np.float32(case['loss_scale'] / float(case['first_n'] * case['num_thresh'])))
    t = target.double()
    p_ = kk * (-(t * torch.log(a)))
    n_ = kk * (-((1 - t) * torch.log(b)))
    (case['pos_scale'] * p_.sum() + n_.sum()).backward()
    assert _rel(pos, p_.detach()) <= 1e-12 and _rel(neg, n_.detach()) <= 1e-12 and _rel(grad, a.grad - b.grad) <= 1e-12
    # float32 in the kernel's order
    a32, b32, t32, k32 = score + eps, (1.0 - score) + eps, target, torch.tensor(kk)
    assert TC.rel_ratio(k32 * (-(t32 * torch.log(a32))), pos) <= 0.5
    assert TC.rel_ratio(k32 * (-((1.0 - t32) * torch.log(b32))), neg) <= 0.5
    assert TC.rel_ratio(k32 * (case['pos_scale'] * (-t32 / a32) + (1.0 - t32) / b32), grad) <= 0.5


# ---------------------------------------------------------------------------------------------------------------------------------------------
# pad_params, residual_relu
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', TC.PAD_PARAMS_T)
def test_pad_params_reference_is_row_by_row_slicing(T):
    o = TC.pad_params_operands(T)
    r = TC.pad_params_ref(o, T)
    for h in range(16):
        for j in range(8):
            assert TC.same_bits(r['wout'][h, j], o['wo'][h * 8 + j]) and float(r['bout'][h, j]) == float(o['bo'][h * 8 + j])
    assert r['wl'].shape == (T, 128) and r['bl'].shape == (T,)


@pytest.mark.parametrize('rows', TC.RESIDUAL_ROWS)
def test_residual_relu_reference_and_its_special_inputs(rows):
    x, att = TC.residual_operands(rows)
    want = TC.residual_ref(x, att)
    k = len(TC.RESIDUAL_SPECIALS)
    xs, as_ = x[rows - 1, :k].double(), att.view(rows, 128)[rows - 1, :k].double()
    for i, (a, b) in enumerate(TC.RESIDUAL_SPECIALS):
        assert float(xs[i]) == a and float(as_[i]) == b, (i, 'is not a bf16 value')
    s = xs + as_                                              # exact in float64
    r = s.float().bfloat16()
    got = want[rows - 1, :k]
    relu = torch.where(r.float() > 0, r, torch.zeros_like(r))                # the definition's ReLU: s > 0 ? s : 0
    assert torch.equal(got, relu) and bool((TC.bits(got) == TC.bits(relu))[relu != 0].all())
    assert bool(((TC.bits(got) & 0x7fff) == 0)[relu == 0].all())             # (only the sign of a zero is left to the ReLU's implementation)
    assert bool((TC.bits(x[rows - 1, :2]) & 0x7fff == 0).all()) and bool((TC.bits(x[rows - 1, :1]) != 0).all())             # -0.0 is there
    halfway = [i for i in range(k) if s[i] != 0 and abs(float(r[i].double()) - float(s[i])) * 2 == 2.0 ** (np.floor(np.log2(abs(float(s[i])))) - 7)]
    assert len(halfway) >= 4, halfway                         # sums exactly between two bf16 values
    assert any(float(s[i]) < 0 and abs(float(s[i])) < 2.0 ** -126 for i in range(k))       # a negative sum in the subnormal range


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cond_multi, cond_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _exp_ratio(c):
    """Largest relative error of the emulated exponential over its half of the factor, (|x| + c) U, on every logit of every case (results in the
    normal range of float32: below it the bound's 2^-126 term stands in)."""
    worst = 0.0
    for case in TC.COND_CASES:
        x = TC.cond_operands(case)['logit_buf'][:, :case['T']].reshape(-1)
        ref = torch.exp(-x.double())
        ok = (ref >= TC.TINY) & (ref < 3e38)
        worst = max(worst, TC.worst(TC.exp_emulate32(-x)[ok], ref[ok], (x.double().abs()[ok] + c) * TC.U * ref[ok]))
    return worst


def test_cond_multi_constant_is_the_smallest_that_halves():
    """COND_C is the smallest integer c at which exp2(fl(-x log2e)) in float32 uses at most half of the factor (|x| + c) 2 U the bound gives the
    exponential; the whole emulation (1 + e and the quotient rounded too) is inside the bound on every case."""
    r = _exp_ratio(TC.COND_C)
    assert r <= 1.0 and (TC.COND_C == 0 or _exp_ratio(TC.COND_C - 1) > 1.0)
    worst = 0.0
    for case in TC.COND_CASES:
        o = TC.cond_operands(case)
        cond, multi, xt = TC.cond_ref64(case, o['logit_buf'], o['score'])
        ec, em = TC.cond_emulate32(case, o['logit_buf'], o['score'])
        worst = max(worst, TC.worst(ec, cond, TC.cond_bound(xt)), TC.worst(em, multi, TC.multi_bound(xt, o['score'])))
    print('cond_multi: c = %d, exponential err / ((|x| + c) U) = %.4f, emulation err / bound = %.4f' % (TC.COND_C, r, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('case', TC.COND_CASES, ids=_ids(TC.COND_CASES))
def test_cond_references_are_autograd_and_the_emulations_halve_the_bounds(case):
    B, C, F, T = (case[k] for k in ('B', 'C', 'F', 'T'))
    o = TC.cond_operands(case)
    assert bool(torch.isnan(o['logit_buf'][:, T:]).all())
    cond, multi, xt = TC.cond_ref64(case, o['logit_buf'], o['score'])
    # the definition by loops on a few entries, and by autograd
    flat = o['logit_buf'][:, :T].double()
    for (b, c, f) in {(0, 0, 0), (B - 1, C - 1, F - 1), (B - 1, 0, F - 1), (0, C - 1, F // 2)}:
        row = flat[(b * C + c) * F + f]
        assert torch.allclose(cond[b, f, c], torch.sigmoid(row), rtol=1e-13, atol=0)
        assert torch.allclose(multi[b, f, c], o['score'][b, f, c].double() * torch.sigmoid(row), rtol=1e-13, atol=0)
    logit = flat.clone().requires_grad_(True)
    s = o['score'].double().requires_grad_(True)
    p = torch.sigmoid(logit).reshape(B, C, F, T).permute(0, 2, 1, 3)
    m = s[..., None] * p
    assert _rel(multi, m.detach()) <= 1e-12
    (m * o['d_multi'].double()).sum().backward()
    ds, dl, mag = TC.cond_bwd_ref64(case, o['d_multi'], p.detach(), o['score'])
    assert _rel(ds, s.grad) <= 1e-12 and _rel(dl[:, :T], logit.grad) <= 1e-12 and float(dl[:, T:].abs().max() if T < 64 else 0) == 0.0
    # backward emulation on the float32 cond the forward kernel hands over
    p32, _ = TC.cond_emulate32(case, o['logit_buf'], o['score'])
    ds, dl, mag = TC.cond_bwd_ref64(case, o['d_multi'], p32, o['score'])
    eds, edl = TC.cond_bwd_emulate32(case, o['d_multi'], p32, o['score'])
    bs, bl = TC.cond_bwd_bounds(case, ds, dl, mag)
    assert TC.worst(eds, ds, bs) <= 0.5
    assert TC.worst(edl, dl, bl) <= 0.5 and TC.worst(edl.to(TC.BF16), dl, bl) <= 1.0
    assert float(edl[:, T:].abs().max() if T < 64 else 0) == 0.0


@pytest.mark.parametrize('mutant,cid', [(m, cid) for m, ids in sorted(TC.COND_MUTANTS.items()) for cid in ids])
def test_cond_mutant_is_rejected(mutant, cid):
    case = _by_id(TC.COND_CASES)[cid]
    o = TC.cond_operands(case)
    cond, multi, xt = TC.cond_ref64(case, o['logit_buf'], o['score'])
    bc, bm, _ = TC.cond_ref64(case, o['logit_buf'], o['score'], mutant=mutant)
    assert max(TC.worst(bc.float(), cond, TC.cond_bound(xt)), TC.worst(bm.float(), multi, TC.multi_bound(xt, o['score']))) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# embed + take_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_take_table_holds_the_cases_of_the_issue():
    shapes = {(c['B'], c['N'], c['C'], c['F']) for c in TC.TAKE_CASES}
    assert shapes == {(1, 1, 1, 1), (1, 15, 3, 15), (2, 16, 5, 7), (2, 17, 80, 17), (1, 33, 128, 20), (2, 300, 80, 100)}
    assert {c['kind'] for c in TC.TAKE_CASES} == {'plain', 'same', 'unranked', 'neg'}


@pytest.mark.parametrize('case', TC.TAKE_CASES, ids=_ids(TC.TAKE_CASES))
def test_take_bwd_reference_is_index_add_and_the_adjoint_of_embed(case):
    B, N, C, F = (case[k] for k in ('B', 'N', 'C', 'F'))
    o = TC.take_operands(case)
    rank = o['rank']
    for b in range(B):
        for c in range(C):
            r = rank[b, c][rank[b, c] >= 0]
            assert len(set(r.tolist())) == r.numel() and int(rank[b, c].max()) < N          # a class ranks a roi at most once
    if case['kind'] == 'same':
        assert torch.equal(rank[:, 0], rank[:, 1])
    if case['kind'] == 'neg':
        assert int((rank < 0).sum()) > 0 and all(bool((rank[b, c][int((rank[b, c] >= 0).sum()):] < 0).all()) for b in range(B) for c in range(C))
    ranked = TC.ranked_mask(rank, N)
    if case['kind'] == 'unranked':
        assert not bool(ranked.all())
    ref, mag = TC.take_bwd_ref64(o['d_x'], rank, N)
    # index_add_ over the flattened (image, roi) rows
    flat = torch.zeros(B * N + 1, TC.D, dtype=F64)
    idx = rank.long() + (torch.arange(B) * N).view(B, 1, 1)
    idx = torch.where(rank >= 0, idx, torch.full_like(idx, B * N))
    flat.index_add_(0, idx.reshape(-1), o['d_x'].double().reshape(-1, TC.D))
    assert _rel(ref, flat[:B * N].view(B, N, TC.D)) <= 1e-12
    assert float(ref[~ranked].abs().max() if bool((~ranked).any()) else 0) == 0.0
    em = TC.take_bwd_emulate(o['d_x'], rank, N)
    assert TC.worst(em, ref, TC.take_bwd_bound(case, ref, mag)) <= 0.5
    assert TC.worst(em.to(TC.BF16), ref, TC.take_bwd_bound(case, ref, mag)) <= 1.0
    assert float(em[~ranked].abs().max() if bool((~ranked).any()) else 0) == 0.0
    if case['kind'] != 'neg':
        x = TC.embed_ref64(o['emb'], o['rank_feat'], rank)
        for (b, c, f) in {(0, 0, 0), (B - 1, C - 1, F - 1)}:
            assert torch.equal(x[b, c, f], o['emb'][b, rank[b, c, f]].double() + o['rank_feat'][f].double())
        ex = (x.float()).to(TC.BF16)
        assert TC.worst(ex, x, TC.embed_bound(x)) <= 1.0 + 1e-6   # (one float32 sum, one bf16 store: the half step is the store's rounding)
        # <embed(e) - embed(0), y> = <e, take_bwd(y)>
        lin = TC.embed_ref64(o['emb'], None, rank)
        lhs = float((lin * o['d_x'].double()).sum())
        rhs = float((o['emb'].double() * ref).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((lin * o['d_x'].double()).abs().sum())


@pytest.mark.parametrize('cid', TC.TAKE_MUTANTS['last_class_only'])
def test_take_bwd_mutant_last_class_only_is_rejected(cid):
    case = _by_id(TC.TAKE_CASES)[cid]
    o = TC.take_operands(case)
    ref, mag = TC.take_bwd_ref64(o['d_x'], o['rank'], case['N'])
    bad, _ = TC.take_bwd_ref64(o['d_x'], o['rank'], case['N'], mutant='last_class_only')
    assert TC.worst(bad.to(TC.BF16), ref, TC.take_bwd_bound(case, ref, mag)) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# softmax_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', TC.SOFTMAX_BWD_CASES, ids=_ids(TC.SOFTMAX_BWD_CASES))
def test_softmax_bwd_reference_is_autograd_and_the_emulation_halves_the_bound(case):
    N, C = case['N'], case['C']
    o = TC.softmax_bwd_operands(case)
    cls = o['cls'].clone().requires_grad_(True)
    p = torch.softmax(cls, 2)[..., 1:]
    (p * o['d_prob'].double()).sum().backward()
    ref, _ = TC.softmax_bwd_ref64(case, p.detach(), o['d_prob'], o['d_cls'])
    want = o['d_cls'].double().clone()
    want[:, :N, :C + 1] += cls.grad
    assert _rel(ref, want) <= 1e-12
    assert torch.equal(ref[:, N:], o['d_cls'].double()[:, N:]) and torch.equal(ref[:, :, C + 1:], o['d_cls'].double()[:, :, C + 1:])
    ref, mag = TC.softmax_bwd_ref64(case, o['prob'], o['d_prob'], o['d_cls'])
    em = TC.softmax_bwd_emulate32(case, o['prob'], o['d_prob'], o['d_cls'])
    assert TC.worst(em, ref, TC.softmax_bwd_bound(case, mag)) <= 0.5
    bad, _ = TC.softmax_bwd_ref64(case, o['prob'], o['d_prob'], o['d_cls'], mutant='no_background')
    assert TC.worst(bad.float(), ref, TC.softmax_bwd_bound(case, mag)) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# gather_bias
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_gather_table_holds_the_sizes_of_the_issue():
    assert {c['F'] for c in TC.GATHER_CASES} == {1, 63, 64, 65, 100, 128, 150, 192, 193, 256, 257, 512}
    for F in TC.GATHER_F:
        cs = [c for c in TC.GATHER_CASES if c['F'] == F]
        assert {c['N'] for c in cs} == {F, F + 5} and {c['C'] for c in cs} == {1, 3} and {c['B'] for c in cs} == {1, 2}
        assert {c['Npad'] == c['N'] for c in cs} == {True, False} or F + 5 == TC.pad32(F + 5)
        assert all(c['Fpad'] == TC.pad32(F) for c in cs)


@pytest.mark.parametrize('case', [c for c in TC.GATHER_CASES if c['F'] <= 65], ids=_ids([c for c in TC.GATHER_CASES if c['F'] <= 65]))
def test_gather_bias_reference_is_the_indexing_of_the_definition(case):
    img, rank = TC.gather_operands(case)
    assert img.unique().numel() == img.numel()
    for bc in range(rank.shape[0]):
        assert len(set(rank[bc].tolist())) == case['F'] and 0 <= int(rank[bc].min()) and int(rank[bc].max()) < case['N']
    ref = TC.gather_ref(case, img, rank)
    assert ref.shape == (case['B'] * case['C'], 16, case['F'], case['F'])
    g = torch.Generator().manual_seed(1)
    for _ in range(50):
        bc, h, f1, f2 = (int(torch.randint(0, n, (1,), generator=g)) for n in ref.shape)
        assert float(ref[bc, h, f1, f2]) == float(img[bc // case['C'], h, rank[bc, f1], rank[bc, f2]])
    for bc in range(rank.shape[0]):
        r = rank[bc].long()
        assert torch.equal(ref[bc], img[bc // case['C'], :][:, r][:, :, r])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# reduce_scalar, wgrad_accumulate, sgd_update
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', TC.REDUCE_N)
def test_reduce_scalar_emulation_halves_the_bound_and_counts_exactly(n):
    assert [TC.reduce_blocks(k) for k in (1, 4096, 4097, 64 * 4096, 64 * 4096 + 1, 700001)] == [1, 1, 2, 64, 64, 64]
    x = TC.reduce_operands(n, 0)
    for scale in TC.REDUCE_SCALES:
        want = TC.reduce_ref64(x, scale, 0)
        assert abs(want - scale * float(x.double().sum())) <= 1e-12 * abs(want)
        assert abs(TC.reduce_emulate32(x, scale, 0) - want) <= 0.5 * TC.reduce_bound(x, n, scale)
    x1 = TC.reduce_operands(n, 1)
    want = TC.reduce_ref64(x1, 1.0, 1)
    assert want == sum(1 for v in x1.tolist() if v >= 0) and TC.reduce_emulate32(x1, 1.0, 1) == want
    if n >= 5:
        tail = x1[n - 5:]
        assert bool(torch.isnan(tail[4])) and float(tail[3]) > 0 and TC.bits(tail[:1]).item() == -2 ** 31 and TC.reduce_ref64(tail, 1.0, 1) == 3.0


@pytest.mark.parametrize('case', TC.WGRAD_CASES, ids=_ids(TC.WGRAD_CASES))
def test_wgrad_accumulate_reference_emulation_and_mutant(case):
    o = TC.wgrad_operands(case)
    ref, mag = TC.wgrad_ref64(case, o['parts'], o['grad'], o['scale'])
    want = o['grad'].double().clone()
    for r in range(min(case['rows'], 5)):
        s2 = 1.0 if o['scale'] is None else float(o['scale'][r].double()) ** 2
        assert _rel(ref[r], want[r] + s2 * o['parts'][:, r].double().sum(0)) <= 1e-12
    assert TC.worst(TC.wgrad_emulate32(case, o['parts'], o['grad'], o['scale']), ref, TC.wgrad_bound(case, mag)) <= (1.0 if case['scale'] else 0.5)
    assert TC.worst(TC.wgrad_emulate32(case, o['parts'], o['grad'], o['scale'], fused=False), ref, TC.wgrad_bound(case, mag)) <= 1.0
    if case['id'] in TC.WGRAD_MUTANTS['scale_per_column']:
        bad, _ = TC.wgrad_ref64(case, o['parts'], o['grad'], o['scale'], mutant='scale_per_column')
        assert TC.worst(bad.float(), ref, TC.wgrad_bound(case, mag)) > 1.0
    assert (case['rows'] * case['cols'] // 4 > 4096 * 256) == (case['rows'] == 2048)


@pytest.mark.parametrize('case', TC.SGD_CASES, ids=_ids(TC.SGD_CASES))
def test_sgd_emulation_halves_the_bounds(case):
    o = TC.sgd_operands(case)
    m1, w1, mag = TC.sgd_ref64(case, o['w'], o['mom'], o['grad'])
    em, ew = TC.sgd_emulate32(case, o['w'], o['mom'], o['grad'])
    bm, bw = TC.sgd_bounds(w1, mag)
    assert TC.worst(em, m1, bm) <= (1.0 if case['wd'] else 0.5)              # (see "half of the bound" in train_glue_cases)
    assert TC.worst(ew, w1, bw) <= 1.0                                       # (w: the last addition is granted exactly its U |w|)
    um, uw = TC.sgd_emulate32(case, o['w'], o['mom'], o['grad'], fused=False)
    assert TC.worst(um, m1, bm) <= 1.0 and TC.worst(uw, w1, bw) <= 1.0
    # a rescale_grad that is ignored, or a weight decay that is dropped, is outside the bound
    other = dict(case, rescale=1.5 - case['rescale'], wd=0.0005 - case['wd'])
    bad, _, _ = TC.sgd_ref64(dict(case, rescale=other['rescale']), o['w'], o['mom'], o['grad'])
    assert TC.worst(bad.float(), m1, bm) > 1.0
    bad, _, _ = TC.sgd_ref64(dict(case, wd=other['wd']), o['w'], o['mom'], o['grad'])
    assert TC.worst(bad.float(), m1, bm) > 1.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# relation_bwd_pack, relu_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', TC.PACK_SHAPES)
def test_pack_reference_is_the_concatenation(shape):
    B, N, M, d = shape
    dq, dk, dvw = TC.pack_operands(shape)
    want = TC.pack_ref(dq, dk, dvw)
    assert want.shape == (B, N, 3 * d)
    assert torch.equal(want[:, :, :d], dq.to(TC.BF16)) and torch.equal(want[:, :M, d:2 * d], dk.to(TC.BF16)) and torch.equal(want[:, :M, 2 * d:], dvw.to(TC.BF16))
    assert float(want[:, M:, d:].float().abs().max() if M < N else 0) == 0.0


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_relu_bwd_reference_masks_negative_zero_and_nan(dtype):
    dy, y, add = TC.relu_bwd_operands(dtype)
    neg0 = TC.bits(y) == (-2 ** 31 if dtype == torch.float32 else -2 ** 15)
    nan = torch.isnan(y)
    assert int(neg0.sum()) > 100 and int(nan.sum()) > 100 and bool(nan[-1]) and bool(neg0[-2])
    out = TC.relu_bwd_ref(dy, y)
    assert float(out[neg0 | nan].float().abs().max()) == 0.0 and bool(torch.isfinite(out.float()).all())
    assert torch.equal(out[y.float() > 0], dy[y.float() > 0])
    assert torch.equal(TC.relu_bwd_ref(dy, y, add)[neg0 | nan], add[neg0 | nan])
