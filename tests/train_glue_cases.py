"""Shared by tests/test_train_glue_cases_host.py and tests/test_gpu_train_glue_edges.py: the edge cases of the training step's small kernels
(csrc/losses.hip, csrc/lnms_train.hip, csrc/train_ops.hip and relnet_lnms_embed of csrc/learn_nms.hip), seeded operand builders, one float64
reference per kernel written from the definition in the kernel files' header comments, the bound every GPU result is held to, and float32 / bf16
emulations of each kernel's arithmetic order (the host file shows that a correct evaluation uses at most half of each bound and that the mutants
named here exceed it).  Imports torch / numpy and tests/gemm_cases.py only (never the library), so it loads on a machine without a GPU.

Notation: U = 2^-24 (unit roundoff of float32), step(t) = max(|t|, 2^-126) 2^-7 as in gemm_cases: half a step is the rounding of one bf16 store.

Where the bounds come from (first order; every reference is evaluated in float64 on exactly the float32 / bf16 values the kernel reads):
  softmax_output     the project's own criterion (test_gpu_losses._close): 2e-6 of the tensor's largest magnitude, per element.  Every row of prob
                     sums to 1 within 4 C U: exp(x - m) errs by 2 U, the C - 1 additions of the sum by (C - 1) U, 1 / s and the product by U each.
  nms_loss           The definition takes a = fl(s + eps) and b = fl(fl(1 - s) + eps) as float32 operands -- these sums are float32 operators of
                     the graph the loss is defined on (oracle/losses.py evaluates them in float32 as well), so the reference forms them in float32
                     and takes the logarithms / quotients in float64.  3e-6 per element (+ 1e-9), the figure test_gpu_losses has always used.
  cond_multi         p = 1 / (1 + e), e = exp(-x) through the fast exponential exp2(fl(-x log2e)): the rounding of the product and of the
                     constant move the exponent by <= |x| 1.22 U ln-units, the instruction by c' U, so e errs by (|x| 1.22 + c') U relative and
                     p by p (1 - p) times that; 1 + e and the quotient add 2 U p.  Bound: p (1 - p) (|x| + c) 2 U + 2 U p + 2^-126 (results below
                     the normal range may be flushed).  c = COND_C is the smallest integer at which the emulated exponential (exp_emulate32: the
                     part of the evaluation c stands for) uses at most half of its factor, i.e. errs by <= (|x| + c) U relative, on every case
                     (test_cond_multi_constant_is_the_smallest_that_halves).  The two roundings behind it (1 + e and the quotient, U p each) are
                     granted exactly 2 U p, so a correctly rounded evaluation may use the whole of that term: the full emulation is held to
                     the bound itself, not to half of it.  multi = s p: one more product.
  cond_bwd           d_sorted = sum_t dm p: T products and T additions of float32: (T + 1) U sum |dm p|.  d_logit = dm s p (1 - p): three
                     products and one difference (4 U) and the bf16 store.
  bf16 outputs       (d_logit, take_bwd, embed) the store alone may use the whole half step, so, as in relation_edge_cases, "half of the bound"
                     is asked of the UNROUNDED float32 emulation; the rounded emulation is held to the whole bound.
  half of the bound  is what the host file asks of every emulation where the formula leaves that room.  Four formulas grant the roundings exactly
                     their worst case, and a correctly rounded evaluation uses more than half of them: the 2 U p of cond_multi (above); the
                     U |w| of sgd_update's final addition (0.99 observed); sgd_update's mom with a weight decay, where the gradient term does
                     see three roundings (0.73 observed where mom is small; without weight decay: under half); wgrad_accumulate with a row
                     scale (sum, square and fused accumulation are 3 of the 4 U at two splits: 0.71 observed).  There the emulation is
                     asserted inside the whole bound.
  take_bwd           <= C float32 additions of exact bf16 values: C U sum |terms|, and the bf16 store.
  softmax_bwd        two C-term sums (C U each, relative to the sums of magnitudes), 1 - sum p, products and the accumulation into d_cls:
                     (C + 2) U (|old| + magnitude), magnitude = p_c (|d_c| + sum p |d|) for class c, (1 + sum p) sum p |d| for the background.
  reduce_scalar      a thread adds ceil(n / (256 blocks)) values, the wavefront 6 shuffle steps, the workgroup 3 additions, the slot <= 64
                     atomics (order free): (trips + 72) U sum |x| covers 6 + 3 + 63.
  wgrad_accumulate   splits - 1 additions, the square, the product, the accumulation: (splits + 2) U (|grad| + s^2 sum |parts|).
  sgd_update         the reference uses the float32 values of lr / momentum / wd / rescale_grad the entry point receives; mom: three roundings on
                     the largest term, 3 U (|momentum m| + lr |g| + lr wd |w|); w: one more addition, + U |w|.  The emulation contracts a b + c
                     into one fused operation where the compiler does by default (fma(wd, w, rescale g), fma(momentum, m, -lr (..))): half the
                     bound of mom; every product rounded separately uses up to 0.77 of it, still inside (both are asserted).  wgrad_accumulate
                     (fma(scale^2, sum, grad)) and cond_bwd (ds = fma(dm, p, ds)) likewise.
Bit-exact kernels (pad_params, residual_relu, gather_bias, relation_bwd_pack, relu_bwd, the bf16 copy of sgd_update) have no bound.

residual_relu and the sign of zero: two bf16 values below 2^-126 add exactly in float32 and the sum is itself a bf16 value (both are multiples of
2^-133), so no negative sum rounds to -0; the inputs that reach the -0 / +0 edge are (-0) + (-0), x + (-x), and negative / positive sums in the
subnormal range, all in RESIDUAL_SPECIALS."""
import zlib

import numpy as np
import torch

import gemm_cases as GC

U = 2.0 ** -24
TINY = 2.0 ** -126
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
step = GC.step


def seed(id_):
    return zlib.crc32(id_.encode())


def gen(id_):
    return torch.Generator().manual_seed(seed(id_))


def pad32(m):
    return (m + 31) // 32 * 32


def worst(got, want, tol):
    """Largest |got - want| / tol over all elements (0 / 0 = 0, a non-finite result = inf).  No element is left out."""
    got, want, tol = torch.broadcast_tensors(got.double(), want.double(), torch.as_tensor(tol, dtype=F64, device=got.device))
    if got.numel() == 0:
        return 0.0
    err = (got - want).abs()
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float('inf')))
    return float(r.max())


def fma32(a, b, c):
    """fl(a b + c) with one rounding (the product of two float32 values is exact in float64)."""
    return (a.double() * b.double() + c.double()).float()


def bits(t):
    """Integer view of a float tensor (bit-for-bit comparisons; NaN patterns compare equal to themselves)."""
    return t.contiguous().view(GC.INT_VIEW[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


# =============================================================================================================================================
# relnet_softmax_output_ex
# =============================================================================================================================================
def _sm(id_, shape, group=0, use_ignore=1, ignore_label=-1.0, grad_scale=1.0, multi=False, special=None, label=True):
    shape = tuple(shape)
    outer, C = shape[0], shape[1]
    inner = int(np.prod(shape[2:])) if multi else 1
    return dict(id=id_, shape=shape, outer=outer, C=C, inner=inner, total=outer * inner, group=group, use_ignore=use_ignore,
                ignore_label=float(ignore_label), grad_scale=float(grad_scale), multi=multi, special=special, label=label)


_MULTI_SHAPES = {1: (1, 1), 63: (9, 7), 65: (13, 5), 420: (12 * 5, 7)}            # inner -> (A h, w)
SOFTMAX_BIG = _sm('SB-1048833x2', (3, 2, 349611, 1), group=349611, multi=True)      # 4096 * 256 + 257 positions: both kernels' grid-stride loops
SOFTMAX_CASES = [
    _sm('S1x1', (1, 1), use_ignore=0),
    _sm('S1x2-g1', (1, 2), group=1),
    _sm('S63x81-g63', (63, 81), group=63),
    _sm('S63x81-g7', (63, 81), group=7, grad_scale=3.0),
    _sm('S63x81-g1', (63, 81), group=1, ignore_label=255.0),
    _sm('S63x81-g7-allign', (63, 81), group=7, special='all_ignored'),
    _sm('S63x81-g7-onevalid', (63, 81), group=7, special='one_valid', ignore_label=255.0),
    _sm('S64x81-g64', (64, 81), group=64, ignore_label=255.0, grad_scale=3.0),
    _sm('S64x81-g1-noign', (64, 81), group=1, use_ignore=0),
    _sm('S65x81-g65', (65, 81), group=65),
    _sm('S65x81-g0', (65, 81), group=0, use_ignore=0, grad_scale=3.0),
    _sm('S65x81-prob', (65, 81), label=False),
    _sm('S616x81-g308', (616, 81), group=308, ignore_label=255.0, grad_scale=3.0),     # wavefront 4 (positions 256 .. 319) straddles 308
    _sm('S616x81-g308-noign', (616, 81), group=308, use_ignore=0),
    _sm('S616x81-g7', (616, 81), group=7),
    _sm('S616x81-g0', (616, 81), group=0),
    _sm('S616x81-g308-allign', (616, 81), group=308, special='all_ignored'),
    _sm('S616x81-g308-onevalid', (616, 81), group=308, special='one_valid'),
    _sm('S130x300-g65', (130, 300), group=65, grad_scale=3.0),                         # wavefronts 1 and 2 straddle 65 and 130
    _sm('S130x300-g0', (130, 300), group=0, ignore_label=255.0),
] + [
    _sm('M%dx%d' % (B, inner), (B, 2) + _MULTI_SHAPES[inner], group=inner, multi=True, grad_scale=3.0 if B == 3 else 1.0,
        use_ignore=0 if (B, inner) == (3, 63) else 1)
    for B in (1, 3) for inner in (1, 63, 65, 420)
] + [
    _sm('M3x65-allign', (3, 2, 13, 5), group=65, multi=True, special='all_ignored'),
    _sm('M3x420-onevalid', (3, 2, 60, 7), group=420, multi=True, special='one_valid'),
    _sm('M3x65-prob', (3, 2, 13, 5), group=65, multi=True, label=False),
    SOFTMAX_BIG,
]
# mutant -> ids of the cases at which the host file shows that it is rejected
SOFTMAX_MUTANTS = {
    'count_whole_call': ('S63x81-g7', 'S616x81-g308', 'S130x300-g65', 'M3x65'),
    'count_first_lane': ('S616x81-g308', 'S616x81-g308-noign', 'S130x300-g65', 'M3x65'),
    'ignored_counted': ('S63x81-g63', 'S616x81-g308', 'M1x420'),
    'no_max_1': ('S63x81-g7-allign', 'S616x81-g308-allign', 'M3x65-allign'),
}


def softmax_to2d(case, t):
    """[positions, C] with position = outer index * inner + inner index (the index the kernels and the label use)."""
    if case['multi']:
        return t.reshape(case['outer'], case['C'], case['inner']).permute(0, 2, 1).reshape(-1, case['C'])
    return t.reshape(case['outer'], case['C'])


def softmax_from2d(case, t2):
    if case['multi']:
        return t2.reshape(case['outer'], case['inner'], case['C']).permute(0, 2, 1).reshape(case['shape']).contiguous()
    return t2.reshape(case['shape']).contiguous()


def softmax_groups(case):
    G = case['group'] or case['total']
    return G, case['total'] // G


def softmax_operands(case):
    """-> (data float32 in the call's layout, label float32 [outer] / [outer, inner] | None).  Logits N(0, 2); position 1 holds +-80, position 2
    equal values."""
    g = gen(case['id'])
    total, C = case['total'], case['C']
    x2 = torch.randn(total, C, generator=g) * 2
    if total >= 3:
        x2[1] = 80.0 * (1 - 2 * (torch.arange(C) % 2)).float()
        x2[2] = 0.75
    data = softmax_from2d(case, x2)
    if not case['label']:
        return data, None
    ign = case['ignore_label']
    lab = torch.randint(0, C, (total,), generator=g).float()
    if case['use_ignore']:
        drop = torch.rand(total, generator=g) < (0.6 if case['multi'] else 0.4)
        lab[drop] = ign
    G, ng = softmax_groups(case)
    if case['special'] == 'all_ignored':
        gi = ng // 2
        for nb in (gi - 1, gi + 1):                                    # the neighbours keep at least one valid label
            if 0 <= nb < ng:
                lab[nb * G] = float(C - 1)
        lab[gi * G:(gi + 1) * G] = ign
    elif case['special'] == 'one_valid':
        lab[:G] = ign
        # the one valid label names the class with the SMALLEST logit: its gradient p - 1 is the tensor's largest entry (the other groups divide by
        # their ~G / 2 labels), so the criterion "relative to the largest magnitude" is not asked to resolve the cancellation of a p close to 1
        lab[G // 2] = float(x2[G // 2].argmin())
    return data, lab.reshape((case['outer'], case['inner']) if case['multi'] else (case['outer'],))


def softmax_valid(case, lab):
    lab = lab.reshape(-1)
    return (lab != case['ignore_label']) if case['use_ignore'] else torch.ones_like(lab, dtype=torch.bool)


def softmax_counts(case, valid, mutant=None):
    """Valid labels per normalisation group -> the count of each POSITION's group (float64 [total])."""
    G, ng = softmax_groups(case)
    pos = torch.arange(case['total'])
    grp = pos // G
    if mutant == 'count_first_lane':           # a wavefront (64 consecutive positions) credits all it counts to the group of its first lane
        credit = grp[(pos // 64) * 64]
    else:
        credit = grp
    cnt = torch.zeros(ng, dtype=F64).index_add_(0, credit, valid.double())
    if mutant == 'count_whole_call':
        cnt = torch.full_like(cnt, float(valid.sum()))
    if mutant == 'ignored_counted':
        cnt = torch.full_like(cnt, float(G))
    return cnt[grp]


def _onehot(lab, C, dtype):
    lab = lab.reshape(-1)
    oh = torch.zeros(lab.numel(), C, dtype=dtype)
    ok = (lab >= 0) & (lab < C)
    oh[torch.nonzero(ok)[:, 0], lab[ok].long()] = 1
    return oh


def softmax_ref64(case, data, label, mutant=None):
    """prob = softmax over the class axis; grad = (prob - onehot(label)) grad_scale / max(valid labels of the position's group, 1), zero where
    the label is ignored.  Both in the call's layout, float64."""
    p = torch.softmax(softmax_to2d(case, data.double()), dim=1)
    if label is None:
        return softmax_from2d(case, p), None
    valid = softmax_valid(case, label)
    cnt = softmax_counts(case, valid, mutant)
    if mutant == 'no_max_1':                   # (the mask as a factor, the division unprotected: 0 / 0 where a group holds no valid label)
        grad = (p - _onehot(label, case['C'], F64)) * (case['grad_scale'] / cnt)[:, None] * valid.double()[:, None]
    else:
        grad = (p - _onehot(label, case['C'], F64)) * (case['grad_scale'] / cnt.clamp_min(1))[:, None]
        grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    return softmax_from2d(case, p), softmax_from2d(case, grad)


def softmax_emulate32(case, data, label):
    """softmax_output_kernel in float32: running maximum, sequential sum of exp(x - m), one reciprocal, (p - onehot) * (grad_scale / count)."""
    x = softmax_to2d(case, data.float())
    m = x.max(1, keepdim=True)[0]
    e = torch.exp(x - m)
    s = torch.zeros(x.shape[0])
    for c in range(case['C']):
        s = s + e[:, c]
    p = e * (1.0 / s)[:, None]
    if label is None:
        return softmax_from2d(case, p), None
    valid = softmax_valid(case, label)
    cnt = softmax_counts(case, valid).float()
    gs = torch.tensor(case['grad_scale'], dtype=F32) / cnt.clamp_min(1)
    grad = (p - _onehot(label, case['C'], F32)) * gs[:, None]
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    return softmax_from2d(case, p), softmax_from2d(case, grad)


def close_ratio(got, want, rtol=2e-6, atol=1e-9):
    """test_gpu_losses._close as a ratio: largest |got - want| over atol + rtol max |want| (every element; non-finite = inf)."""
    want = want.double()
    return worst(got, want, atol + rtol * float(want.abs().max()))


def prob_rows_sum_to_one(case, prob):
    """Largest |sum_c prob - 1| / (4 C U) over the positions."""
    s = softmax_to2d(case, prob.double()).sum(1)
    return worst(s, torch.ones_like(s), 4 * case['C'] * U)


# =============================================================================================================================================
# relnet_smooth_l1_loss, relnet_nms_loss
# =============================================================================================================================================
LOSS_BIG_N = 4096 * 256 + 3
SMOOTH_L1_CASES = [dict(id='L1-n%d-%s-s%g' % (n, 'w' if w else 'now', sigma), n=n, weight=w, sigma=sigma, grad_scale=gs)
                   for (n, w, sigma, gs) in ((1, True, 3.0, 1.0 / 256), (1, False, 1.0, 1.0 / 128), (2464, False, 3.0, 1.0 / 256),
                                             (2464, True, 1.0, 1.0 / 128), (LOSS_BIG_N, True, 3.0, 1.0 / 256), (LOSS_BIG_N, False, 3.0, 1.0))]
NMS_LOSS_CASES = [dict(id='NL-n%d' % n, n=n, first_n=100, num_thresh=5, eps=1e-8, loss_scale=1.0, pos_scale=4.0) for n in (1, 40000, LOSS_BIG_N)]
NMS_SPECIAL_SCORES = (0.0, 1e-9, 1.0 - 2.0 ** -24, 1.0)


def smooth_l1_operands(case):
    g = gen(case['id'])
    n, s2 = case['n'], case['sigma'] ** 2
    pred, target = torch.randn(n, generator=g) * 0.6, torch.randn(n, generator=g) * 0.6
    if n >= 4:
        pred[:4] = target[:4] + torch.tensor([1 / s2, -1 / s2, 0.0, 1e-8])            # on the branch boundary
    weight = (torch.rand(n, generator=g) < 0.3).float() * (1 + torch.rand(n, generator=g)) if case['weight'] else None
    return pred, target, weight


def smooth_l1_ref64(case, pred, target, weight):
    """loss = w smooth_l1(pred - target), grad = grad_scale w smooth_l1'(pred - target); quadratic inside |x| < 1 / sigma^2."""
    x = pred.double() - target.double()
    w = torch.ones_like(x) if weight is None else weight.double()
    s2 = case['sigma'] ** 2
    quad = x.abs() < 1.0 / s2
    loss = w * torch.where(quad, 0.5 * s2 * x * x, x.abs() - 0.5 / s2)
    grad = case['grad_scale'] * w * torch.where(quad, s2 * x, torch.sign(x))
    return loss, grad


def nms_loss_operands(case):
    """Scores in [0, 1] (a product of two uniform draws, like the head's class score times the conditional probability), the first entries the
    special scores with targets 1 and 0; targets ~2 % positives."""
    g = gen(case['id'])
    n = case['n']
    score = torch.rand(n, generator=g) * torch.rand(n, generator=g)
    target = (torch.rand(n, generator=g) < 0.02).float()
    sp = torch.tensor(NMS_SPECIAL_SCORES + NMS_SPECIAL_SCORES, dtype=F64).float()
    tg = torch.tensor([1.0] * 4 + [0.0] * 4)
    k = min(n, 8)
    score[:k], target[:k] = sp[:k], tg[:k]
    return score, target


def nms_loss_ref64(case, score, target):
    """pos = -k t log a, neg = -k (1 - t) log b, grad = k (pos_scale (-t / a) + (1 - t) / b), k = loss_scale / (first_n num_thresh), with the
    float32 operands a = fl(s + eps), b = fl(fl(1 - s) + eps) (see the module docstring) and everything else in float64."""
    eps = torch.tensor(case['eps'], dtype=F32)
    a = (score.float() + eps).double()
    b = ((1.0 - score.float()) + eps).double()
    t = target.double()
    k = float(np.float32(case['loss_scale'] / float(case['first_n'] * case['num_thresh'])))
    pos = k * (-(t * torch.log(a)))
    neg = k * (-((1 - t) * torch.log(b)))
    grad = k * (case['pos_scale'] * (-t / a) + (1 - t) / b)
    return pos, neg, grad


def rel_ratio(got, want, rtol=3e-6, atol=1e-9):
    """numpy.testing.assert_allclose(got, want, rtol, atol) as a ratio over ALL elements."""
    want = want.double()
    return worst(got, want, atol + rtol * want.abs())


# =============================================================================================================================================
# relnet_lnms_pad_params, relnet_lnms_residual_relu
# =============================================================================================================================================
PAD_PARAMS_T = (1, 5, 8, 64)
RESIDUAL_ROWS = (1, 15, 16, 17, 4099)
# (x, att) pairs: -0 + -0; +0 + -0; x + (-x); ties of the bf16 rounding (1 + 2^-8 -> 1, 1 + 2^-7 + 2^-8 -> 1 + 2^-6, the same negated); sums in
# the subnormal range of either sign; a negative sum that the ReLU zeroes
RESIDUAL_SPECIALS = ((-0.0, -0.0), (0.0, -0.0), (1.5, -1.5), (1.0, 2.0 ** -8), (1.0 + 2.0 ** -7, 2.0 ** -8), (-1.0, -(2.0 ** -8)),
                     (256.0, 1.0), (258.0, 1.0), (-(2.0 ** -133), 0.0), (2.0 ** -133, 0.0), (-(2.0 ** -127), 2.0 ** -128), (2.0 ** -127, -(2.0 ** -133)),
                     (-3.0, 1.0), (2.0 ** -126, -(2.0 ** -127)))


def pad_params_operands(T):
    g = gen('pad-T%d' % T)
    return dict(wo=torch.randn(128, 128, generator=g).to(BF16), bo=torch.randn(128, generator=g), wl=torch.randn(T, 128, generator=g).to(BF16),
                bl=torch.randn(T, generator=g))


def pad_params_ref(o, T):
    """What the four written regions hold (slicing): wout_pad.view(16, 64, 128)[:, :8], bout_pad.view(16, 64)[:, :8], wl_pad[:T], bl_pad[:T]."""
    return dict(wout=o['wo'].view(16, 8, 128), bout=o['bo'].view(16, 8), wl=o['wl'], bl=o['bl'])


def residual_operands(rows):
    """x [rows, 128] bf16, att8 [rows, 16, 8] bf16 (the 8 real columns per head of the padded [rows, 16, 64] operand)."""
    g = gen('resid-%d' % rows)
    x = torch.randn(rows, 128, generator=g).to(BF16)
    att = torch.randn(rows, 16, 8, generator=g).to(BF16)
    xs = torch.tensor([p[0] for p in RESIDUAL_SPECIALS], dtype=F64).to(BF16)
    as_ = torch.tensor([p[1] for p in RESIDUAL_SPECIALS], dtype=F64).to(BF16)
    k = len(RESIDUAL_SPECIALS)
    r = rows - 1                                                      # the last row (the tail of the last workgroup) holds the specials
    x[r, :k] = xs
    att.view(rows, 128)[r, :k] = as_
    return x, att


def residual_ref(x, att8):
    """relu((x + att8) rounded to bf16).  The GPU test evaluates the same expression on the device and compares bit for bit; on the CPU torch's
    relu hands (-0) + (-0) back as -0 where the device (like the graph's s > 0 ? s : 0) gives +0, so this CPU result is compared by value."""
    return torch.relu((x.float() + att8.reshape(x.shape).float()).bfloat16())


# =============================================================================================================================================
# relnet_lnms_cond_multi, relnet_lnms_cond_bwd
# =============================================================================================================================================
COND_C = 2                                   # see the module docstring; pinned by test_cond_multi_constant_is_the_smallest_that_halves
COND_SHAPES = ((1, 1, 1, 1), (1, 3, 5, 5), (2, 80, 7, 5), (1, 2, 129, 8), (3, 5, 100, 3))
COND_CASES = [dict(id='CM-%dx%dx%dx%d-ld%d' % (B, C, F, T, ld), B=B, C=C, F=F, T=T, ld=ld)
              for (B, C, F, T) in COND_SHAPES for ld in sorted({64, T})]
COND_MUTANTS = {
    'no_transpose': [c['id'] for c in COND_CASES if c['C'] > 1 and c['F'] > 1],
    'ld_ignored': [c['id'] for c in COND_CASES if c['ld'] != c['T'] and c['B'] * c['C'] * c['F'] > 1],
    'score_logit_order': [c['id'] for c in COND_CASES if c['C'] > 1 and c['F'] > 1],
}
LOG2E32 = float(np.float32(1.4426950408889634))


def cond_operands(case):
    """logit_buf [B C F, ld] float32: row (b C + c) F + f, T logits N(0, 4) (the first ones +-30, +-100), NaN in the pad columns; score [B, F, C];
    d_multi [B, F, C, T]."""
    g = gen(case['id'])
    B, C, F, T, ld = (case[k] for k in ('B', 'C', 'F', 'T', 'ld'))
    rows = B * C * F
    logit = torch.randn(rows, T, generator=g) * 4
    if rows * T >= 4:
        logit.view(-1)[:4] = torch.tensor([30.0, -30.0, 100.0, -100.0])
    buf = torch.full((rows, ld), float('nan'))
    buf[:, :T] = logit
    score = torch.rand(B, F, C, generator=g) * 1.5 - 0.25
    d_multi = torch.randn(B, F, C, T, generator=g)
    return dict(logit_buf=buf, score=score, d_multi=d_multi)


def cond_ref64(case, logit_buf, score, mutant=None):
    """cond[b, f, c, t] = sigmoid(logit[(b C + c) F + f, t]); multi = score[b, f, c] cond.  -> (cond, multi, x transposed to [B, F, C, T])."""
    B, C, F, T, ld = (case[k] for k in ('B', 'C', 'F', 'T', 'ld'))
    rows = B * C * F
    x = (logit_buf.reshape(-1)[:rows * T].reshape(rows, T) if mutant == 'ld_ignored' else logit_buf[:, :T]).double().reshape(B, C, F, T)
    xt = x.reshape(B, F, C, T) if mutant == 'no_transpose' else x.permute(0, 2, 1, 3)
    s = score.double()
    if mutant == 'score_logit_order':
        s = s.reshape(B, C, F).permute(0, 2, 1)
    cond = torch.sigmoid(xt)
    return cond, s[..., None] * cond, xt


def cond_bound(x, c=COND_C):
    p, q = torch.sigmoid(x), torch.sigmoid(-x)                       # (1 - p as sigmoid(-x): no cancellation at large x)
    return p * q * (x.abs() + c) * 2 * U + 2 * U * p + TINY


def multi_bound(x, score, c=COND_C):
    s = score.double().abs()[..., None]
    return cond_bound(x, c) * s + U * s * torch.sigmoid(x)


def exp_emulate32(x32):
    """exp(x) as exp2(fl(x log2e)) in float32 (the fast-exponential path): the product and the result rounded to float32, exp2 itself correctly
    rounded."""
    t = x32.float() * torch.tensor(LOG2E32, dtype=F32)
    return torch.exp2(t.double()).float()


def sigmoid_emulate32(x32):
    """1 / (1 + exp(-x)), each operation rounded to float32."""
    return 1.0 / (1.0 + exp_emulate32(-x32.float()))


def cond_emulate32(case, logit_buf, score):
    B, C, F, T = (case[k] for k in ('B', 'C', 'F', 'T'))
    p = sigmoid_emulate32(logit_buf[:, :T]).reshape(B, C, F, T).permute(0, 2, 1, 3).contiguous()
    return p, score.float()[..., None] * p


def cond_bwd_ref64(case, d_multi, cond, score):
    """Adjoint of cond = sigmoid(logit), multi = score cond: d_sorted[b, f, c] = sum_t dm cond; d_logit[(b C + c) F + f, t] = dm s cond (1 - cond),
    columns T .. 63 zero.  -> (d_sorted [B, F, C], d_logit [B C F, 64], mag = sum_t |dm cond|)."""
    B, C, F, T = (case[k] for k in ('B', 'C', 'F', 'T'))
    dm, p, s = d_multi.double(), cond.double(), score.double()
    ds = (dm * p).sum(3)
    mag = (dm * p).abs().sum(3)
    dl = torch.zeros(B * C * F, 64, dtype=F64)
    dl[:, :T] = (dm * s[..., None] * p * (1 - p)).permute(0, 2, 1, 3).reshape(B * C * F, T)
    return ds, dl, mag


def cond_bwd_emulate32(case, d_multi, cond, score):
    B, C, F, T = (case[k] for k in ('B', 'C', 'F', 'T'))
    dm, p, s = d_multi.float(), cond.float(), score.float()
    ds = torch.zeros(B, F, C)
    for t in range(T):
        ds = fma32(dm[..., t], p[..., t], ds)
    dl = torch.zeros(B * C * F, 64)
    dl[:, :T] = (dm * s[..., None] * p * (1.0 - p)).permute(0, 2, 1, 3).reshape(B * C * F, T)
    return ds, dl                                  # (d_logit before its bf16 store)


def cond_bwd_bounds(case, ds_ref, dl_ref, mag):
    """-> (bound of d_sorted, bound of d_logit: the bf16 store + 4 U; a zero stays an exact zero)."""
    return (case['T'] + 1) * U * mag, 4 * U * dl_ref.abs() + 0.5 * step(dl_ref) * (dl_ref != 0)


# =============================================================================================================================================
# relnet_lnms_embed + relnet_lnms_take_bwd   (D = 128 features)
# =============================================================================================================================================
D = 128


def _tk(B, N, C, F, kind='plain'):
    return dict(id='TK-%dx%dx%dx%d%s' % (B, N, C, F, '' if kind == 'plain' else '-' + kind), B=B, N=N, C=C, F=F, kind=kind)


TAKE_CASES = [_tk(1, 1, 1, 1), _tk(1, 15, 3, 15), _tk(2, 16, 5, 7), _tk(2, 16, 5, 7, 'same'), _tk(2, 16, 5, 7, 'unranked'), _tk(2, 17, 80, 17),
              _tk(2, 17, 80, 17, 'neg'), _tk(1, 33, 128, 20), _tk(1, 33, 128, 20, 'unranked'), _tk(2, 300, 80, 100)]
TAKE_MUTANTS = {'last_class_only': [c['id'] for c in TAKE_CASES if c['C'] > 1]}


def take_operands(case):
    """rank [B, C, F] int32: per class a random prefix of a permutation of the rois ('same': classes 0 and 1 identical; 'unranked': only the
    first 3/4 of the rois are ever ranked; 'neg': -1 in the tail of some lists -- take_bwd ONLY); roi_emb [B, N, 128] bf16, rank_feat [F, 128]
    float32, d_x [B, C, F, 128] bf16.  Image b's operands are 4^b times larger, so that a row taken from the wrong image shows."""
    g = gen(case['id'])
    B, N, C, F = (case[k] for k in ('B', 'N', 'C', 'F'))
    pool = max(F, (3 * N) // 4) if case['kind'] == 'unranked' else N
    rank = torch.stack([torch.stack([torch.randperm(pool, generator=g)[:F] for _ in range(C)]) for _ in range(B)]).to(torch.int32)
    if case['kind'] == 'same':
        rank[:, 1] = rank[:, 0]
    if case['kind'] == 'neg':
        for b in range(B):
            for c in range(0, C, 3):
                rank[b, c, F - 1 - (c % 4):] = -1
    mag = (4.0 ** torch.arange(B).float()).view(B, 1, 1)
    emb = (torch.randn(B, N, D, generator=g) * mag).to(BF16)
    rank_feat = torch.randn(F, D, generator=g)
    d_x = (torch.randn(B, C, F, D, generator=g) * mag[..., None]).to(BF16)
    return dict(rank=rank, emb=emb, rank_feat=rank_feat, d_x=d_x)


def embed_ref64(emb, rank_feat, rank):
    """x[b, c, f, :] = roi_emb[b, rank[b, c, f], :] + rank_feat[f, :] (ranks >= 0 only)."""
    B, C, F = rank.shape
    assert int(rank.min()) >= 0
    idx = rank.long().reshape(B, C * F, 1).expand(B, C * F, emb.shape[2])
    taken = torch.gather(emb.double(), 1, idx).reshape(B, C, F, -1)
    return taken + (0 if rank_feat is None else rank_feat.double()[None, None])


def take_bwd_ref64(d_x, rank, N, mutant=None):
    """d_emb[b, n, :] = sum over the (c, f) with rank[b, c, f] == n of d_x[b, c, f, :]; negative ranks are skipped.  -> (d_emb, sum |terms|)."""
    B, C, F = rank.shape
    out = torch.zeros(B, N, d_x.shape[3], dtype=F64)
    mag = torch.zeros_like(out)
    for b in range(B):
        for c in range(C):
            r = rank[b, c].long()
            ok = r >= 0
            v = d_x[b, c].double()[ok]
            if mutant == 'last_class_only':
                out[b][r[ok]] = v
                mag[b][r[ok]] = v.abs()
            else:
                out[b].index_add_(0, r[ok], v)
                mag[b].index_add_(0, r[ok], v.abs())
    return out, mag


def take_bwd_emulate(d_x, rank, N):
    """float32 accumulation in class order, one bf16 rounding at the store."""
    B, C, F = rank.shape
    acc = torch.zeros(B, N, d_x.shape[3])
    for b in range(B):
        for c in range(C):
            r = rank[b, c].long()
            ok = r >= 0
            acc[b].index_add_(0, r[ok], d_x[b, c].float()[ok])         # (a class ranks a roi at most once: one addition per roi and class)
    return acc                                     # (before the bf16 store)


def take_bwd_bound(case, ref, mag):
    """C U sum |terms| + the bf16 store; a roi nobody ranks stays an exact zero."""
    return case['C'] * U * mag + 0.5 * step(ref) * (mag > 0)


def embed_bound(ref):
    return 0.5 * step(ref)


def ranked_mask(rank, N):
    """[B, N] bool: roi n of image b is ranked by at least one class."""
    B = rank.shape[0]
    m = torch.zeros(B, N + 1, dtype=torch.bool)
    r = rank.long().reshape(B, -1)
    m.scatter_(1, torch.where(r >= 0, r, torch.full_like(r, N)), True)
    return m[:, :N]


# =============================================================================================================================================
# relnet_lnms_softmax_bwd
# =============================================================================================================================================
SOFTMAX_BWD_CASES = [dict(id='SBW-%dx%dx%d-p%d' % (B, N, C, pad), B=B, N=N, C=C, pad=pad, R=N + 2)
                     for (B, N, C) in ((1, 1, 1), (1, 3, 63), (2, 5, 64), (1, 7, 65), (2, 300, 80), (1, 9, 130)) for pad in (0, 3)]
SOFTMAX_BWD_MUTANTS = {'no_background': [c['id'] for c in SOFTMAX_BWD_CASES]}


def softmax_bwd_operands(case):
    """cls [B, N, C + 1] (float64 logits), prob = softmax(cls)[..., 1:] float32, d_prob [B, N, C], d_cls [B, R, C + 1 + pad] pre-filled."""
    g = gen(case['id'])
    B, N, C, pad, R = (case[k] for k in ('B', 'N', 'C', 'pad', 'R'))
    cls = torch.randn(B, N, C + 1, generator=g, dtype=F64) * 2
    prob = torch.softmax(cls, 2)[..., 1:].float().contiguous()
    d_prob = torch.randn(B, N, C, generator=g)
    d_cls = torch.randn(B, R, C + 1 + pad, generator=g)
    return dict(cls=cls, prob=prob, d_prob=d_prob, d_cls=d_cls)


def softmax_bwd_ref64(case, prob, d_prob, d_cls, mutant=None):
    """d_cls[b, n, 0] += -(1 - sum_c p_c) inner, d_cls[b, n, 1 + c] += p_c (d_c - inner), inner = sum_c p_c d_c; rows >= N and the pad columns keep
    their values.  -> (result [B, R, ld], magnitude of the same shape: |old| + the sums of magnitudes the bound is relative to)."""
    N, C = case['N'], case['C']
    p, d, old = prob.double(), d_prob.double(), d_cls.double()
    inner = (p * d).sum(2, keepdim=True)
    ainner = (p * d.abs()).sum(2, keepdim=True)
    sp = p.sum(2, keepdim=True)
    out, mag = old.clone(), old.abs()
    if mutant != 'no_background':
        out[:, :N, 0:1] += -(1 - sp) * inner
    out[:, :N, 1:C + 1] += p * (d - inner)
    mag[:, :N, 0:1] += (1 + sp) * ainner
    mag[:, :N, 1:C + 1] += p * (d.abs() + ainner)
    return out, mag


def softmax_bwd_emulate32(case, prob, d_prob, d_cls):
    """One wavefront per row: lane l adds the classes l, l + 64, ..., a 6-step butterfly, then the updates."""
    N, C = case['N'], case['C']
    p, d = prob.float(), d_prob.float()
    B = p.shape[0]
    sp, si = torch.zeros(B, N, 64), torch.zeros(B, N, 64)
    for c in range(C):
        sp[..., c % 64] = sp[..., c % 64] + p[..., c]
        si[..., c % 64] = si[..., c % 64] + p[..., c] * d[..., c]
    sp, si = _butterfly(sp), _butterfly(si)
    out = d_cls.float().clone()
    out[:, :N, 0] += -(1.0 - sp) * si
    out[:, :N, 1:C + 1] += p * (d - si[..., None])
    return out


def _butterfly(v):
    """The xor-shuffle reduction over the last axis (64 lanes) in float32; every lane ends with the same sum: lane 0 is returned."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., torch.arange(v.shape[-1]) ^ o]
    return v[..., 0]


def softmax_bwd_bound(case, mag):
    return (case['C'] + 2) * U * mag


# =============================================================================================================================================
# relnet_lnms_gather_bias
# =============================================================================================================================================
GATHER_F = (1, 63, 64, 65, 100, 128, 150, 192, 193, 256, 257, 512)
GATHER_CASES = [dict(id='GB-F%d-%s' % (F, v), F=F, Fpad=pad32(F), **kw)
                for F in GATHER_F
                for v, kw in (('a', dict(N=F, Npad=F, C=1, B=1)), ('b', dict(N=F + 5, Npad=pad32(F + 5), C=3, B=2)))]


def gather_operands(case):
    """img [B, 16, N, Npad]: distinct integers (exact in float32), rank [B C, F]: per (image, class) a random permutation prefix."""
    g = gen(case['id'])
    B, C, N, Npad, F = (case[k] for k in ('B', 'C', 'N', 'Npad', 'F'))
    n = B * 16 * N * Npad
    assert n < 2 ** 24
    img = torch.arange(n, dtype=F32).reshape(B, 16, N, Npad)
    rank = torch.stack([torch.randperm(N, generator=g)[:F] for _ in range(B * C)]).to(torch.int32)
    return img, rank


def gather_ref(case, img, rank):
    """out[bc, h, f1, f2] = img[bc // C, h, rank[bc, f1], rank[bc, f2]] for f2 < F (any device; indexing only, so bit-exact)."""
    C = case['C']
    return torch.stack([img[bc // C][:, rank[bc].long()[:, None], rank[bc].long()[None, :]] for bc in range(rank.shape[0])])


# =============================================================================================================================================
# relnet_reduce_scalar
# =============================================================================================================================================
REDUCE_N = (1, 63, 64, 255, 256, 4095, 4096, 4097, 64 * 4096 + 1, 700001)
REDUCE_SCALES = (1.0, 0.125)


def reduce_blocks(n):
    """Workgroups the entry point launches: ceil(n / 4096) clamped to 1 .. 64."""
    return min(max((n + 4095) // 4096, 1), 64)


def reduce_operands(n, mode):
    g = gen('reduce-%d-%d' % (n, mode))
    x = torch.randn(n, generator=g) * (1 + 9 * (torch.rand(n, generator=g) < 0.1).float())
    if mode == 1:
        sp = torch.tensor([-0.0, -1.0, 0.0, 1e-42, float('nan')])
        k = min(n, 5)
        x[n - k:] = sp[:k]                                            # (the tail: the last, partial wavefront counts them)
    return x


def reduce_ref64(x, scale, mode):
    if mode:
        return float((x >= 0).sum())                                  # (-0.0 >= 0 holds, NaN >= 0 does not)
    return float(np.float32(scale)) * float(x.double().sum())


def reduce_bound(x, n, scale):
    trips = -(-n // (256 * reduce_blocks(n)))
    return (trips + 72) * U * abs(float(np.float32(scale))) * float(x.double().abs().sum())


def reduce_emulate32(x, scale, mode):
    """reduce_scalar_kernel in float32: strided per-thread sums, butterfly per wavefront, four partial sums, the scaled workgroup sums added to the
    slot in workgroup order."""
    n = x.numel()
    blocks = reduce_blocks(n)
    stride = blocks * 256
    trips = -(-n // stride)
    v = torch.zeros(trips * stride)
    v[:n] = (x >= 0).float() if mode else x.float()
    v = v.reshape(trips, stride)
    acc = torch.zeros(stride)
    for t in range(trips):
        acc = acc + v[t]
    wave = _butterfly(acc.reshape(blocks, 4, 64))
    part = ((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]
    part = part * torch.tensor(1.0 if mode else scale, dtype=F32)
    out = torch.zeros(())
    for b in range(blocks):
        out = out + part[b]
    return float(out)


# =============================================================================================================================================
# relnet_wgrad_accumulate
# =============================================================================================================================================
WGRAD_CASES = [dict(id='WG-%dx%dx%d-%s' % (s, r, c, 'scale' if sc else 'noscale'), splits=s, rows=r, cols=c, scale=sc)
               for (s, r, c) in ((1, 1, 4), (2, 3, 12), (7, 89, 136), (3, 64, 1152), (2, 2048, 2052)) for sc in (False, True)]
WGRAD_MUTANTS = {'scale_per_column': [c['id'] for c in WGRAD_CASES if c['scale'] and c['rows'] > 1]}


def wgrad_operands(case):
    g = gen(case['id'])
    s, r, c = case['splits'], case['rows'], case['cols']
    return dict(parts=torch.randn(s, r, c, generator=g), grad=torch.randn(r, c, generator=g),
                scale=(torch.rand(r, generator=g) + 0.5) if case['scale'] else None)


def wgrad_ref64(case, parts, grad, scale, mutant=None):
    """grad[r, c] += scale[r]^2 sum_s parts[s, r, c].  -> (result, |grad| + scale^2 sum |parts|)."""
    m = torch.ones(case['rows'], 1, dtype=F64) if scale is None else (scale.double() ** 2)[:, None]
    if mutant == 'scale_per_column':
        m = (scale.double() ** 2)[torch.arange(case['cols']) % case['rows']][None, :]
    return grad.double() + m * parts.double().sum(0), grad.double().abs() + m * parts.double().abs().sum(0)


def wgrad_emulate32(case, parts, grad, scale, fused=True):
    acc = parts[0].float().clone()
    for s in range(1, case['splits']):
        acc = acc + parts[s].float()
    m = torch.ones(case['rows'], 1) if scale is None else (scale.float() * scale.float())[:, None]
    return fma32(m, acc, grad) if fused else grad.float() + m * acc


def wgrad_bound(case, mag):
    return (case['splits'] + 2) * U * mag


# =============================================================================================================================================
# relnet_sgd_update
# =============================================================================================================================================
SGD_LR, SGD_MOMENTUM = 0.0005, 0.9
SGD_CASES = [dict(id='SGD-n%d-r%g-%s-wd%g' % (n, r, 'bf' if bf else 'nobf', wd), n=n, rescale=r, bf16=bf, wd=wd)
             for n in (1, 255, 3005, 8192 * 256 + 5) for (r, bf, wd) in ((1.0, True, 0.0005), (0.5, False, 0.0), (0.5, True, 0.0), (1.0, False, 0.0005))]


def sgd_operands(case):
    g = gen(case['id'])
    n = case['n']
    return dict(w=torch.randn(n, generator=g), mom=torch.randn(n, generator=g) * 0.1, grad=torch.randn(n, generator=g))


def _f32(v):
    return float(np.float32(v))


def sgd_ref64(case, w, mom, grad):
    """mom' = momentum mom - lr (rescale grad + wd w), w' = w + mom', with the float32 values of the four constants.
    -> (mom', w', magnitude of mom' = |momentum mom| + lr |grad| + lr wd |w|)."""
    lr, mo, wd, rs = _f32(SGD_LR), _f32(SGD_MOMENTUM), _f32(case['wd']), _f32(case['rescale'])
    w, m, g = w.double(), mom.double(), grad.double()
    m1 = mo * m - lr * (rs * g + wd * w)
    return m1, w + m1, (mo * m).abs() + lr * g.abs() + lr * wd * w.abs()


def sgd_emulate32(case, w, mom, grad, fused=True):
    c = lambda v: torch.tensor(v, dtype=F32)
    w, m, g = w.float(), mom.float(), grad.float()
    if fused:
        m1 = fma32(c(SGD_MOMENTUM), m, -(c(SGD_LR) * fma32(c(case['wd']), w, c(case['rescale']) * g)))
    else:
        m1 = c(SGD_MOMENTUM) * m - c(SGD_LR) * (c(case['rescale']) * g + c(case['wd']) * w)
    return m1, w + m1


def sgd_bounds(w1_ref, mag):
    bm = 3 * U * mag
    return bm, bm + U * w1_ref.abs()


# =============================================================================================================================================
# relnet_relation_bwd_pack, relnet_relu_bwd
# =============================================================================================================================================
PACK_SHAPES = ((1, 1, 1, 8), (2, 5, 5, 64), (3, 44, 1, 128), (3, 44, 40, 128))       # (B, N, M, d); the last is the shape of the existing test


def pack_operands(shape):
    B, N, M, d = shape
    g = gen('pack-%dx%dx%dx%d' % shape)
    return torch.randn(B, N, d, generator=g), torch.randn(B, M, d, generator=g), torch.randn(B, M, d, generator=g)


def pack_ref(dq, dk, dvw):
    """[B, N, 3 d] bf16 = (dQ | dK | dVW), rows >= M of the key blocks zero."""
    B, N, d = dq.shape
    M = dk.shape[1]
    want = torch.zeros(B, N, 3 * d)
    want[:, :, :d] = dq
    want[:, :M, d:2 * d] = dk
    want[:, :M, 2 * d:] = dvw
    return want.to(BF16)


def relu_bwd_operands(dtype, n=3005):
    """y holds -0.0 and NaN (the mask y > 0 is false for both), zeros and positive values; dy and add are finite."""
    g = gen('relubwd-%s' % dtype)
    y = torch.relu(torch.randn(n, generator=g)).to(dtype)
    y[::7] = -0.0
    y[3::11] = float('nan')
    y[n - 1], y[n - 2] = float('nan'), -0.0                          # the scalar tail too
    return torch.randn(n, generator=g).to(dtype), y, torch.randn(n, generator=g).to(dtype)


def relu_bwd_ref(dy, y, add=None):
    out = torch.where(y.float() > 0, dy.float(), torch.zeros_like(dy.float()))
    return (out if add is None else out + add.float()).to(dy.dtype)
