"""Shared by tests/test_grad_guard_cases_host.py and tests/test_gpu_grad_guard.py: the cases of the optimizer-step guard (csrc/guard.hip:
relnet_grad_stats, relnet_grad_guard_decide, relnet_sgd_update_guarded), seeded operand builders, a float64 numpy reference of each kernel and
the bound every GPU result is held to.  Imports numpy only (never the library), so it loads on a machine without a GPU.

Where the bounds come from (U = 2^-24, the unit roundoff of float32; u = 2^-53, of float64):

  sum of squares   A float32 value has a 24-bit significand, so its square has at most 48 bits and is EXACT in float64 (53 bits); it can neither
                   overflow (|x| < 2^128 -> x^2 < 2^256) nor leave the normal range (|x| >= 2^-149 -> x^2 >= 2^-298).  What is left is the
                   summation of n non-negative terms: n - 1 additions in whatever order (per thread, shuffle tree, waves, slots), each with a
                   relative error <= u of a partial sum that never exceeds the total S.  Hence |computed - S| <= gamma_(n-1) S with
                   gamma_k = k u / (1 - k u), and gamma_(n-1) <= n u as long as n (n - 1) u <= 1, i.e. for every n below 9.4e7.
                   Bound: n 2^-53 S (0 where S is 0: a sum of exact zeros is exact).  The reference S is summed in extended precision.
  norm             sqrt halves a relative error and adds one rounding of its own: (n / 2 + 1) u <= n u relative for n >= 2; max(n, 2) u is used.
  counts           exact.
  decide           compared bit for bit where the inputs make every operation exact (integer-valued partial sums whose total is a perfect
                   square); a general total allows 2 u relative on the norm (the square root) and on the running norm sum.
  sgd, guarded     bit for bit against relnet_sgd_update wherever the guard is neutral or only scales.  With clip_gradient = c the float64
                   reference is  T = clip(rs sc g, +-c),  mom' = mo mom - lr (T + wd w),  w' = w + mom'  on the float32 values of every operand
                   and constant.  train_glue_cases derives sgd_update's bound as three roundings on the whole magnitude,
                   3 U (|mo mom| + lr |g| + lr wd |w|), + U |w'| for the last addition.  Here the gradient term enters as T, and two products
                   (rs g, then by sc) are rounded AHEAD of the clamp: 2 U |rs sc g| before it, and no more after it, because clamping rounds
                   nothing and is non-expansive (|clip(a) - clip(b)| <= |a - b|).  Bound of mom':
                       3 U (|mo mom| + lr |T| + lr wd |w|) + 2 U lr |rs sc g|,   of w': that + U |w'|.
                   The bf16 copy is the rounded w', bit for bit."""
import zlib

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53

# the grid rule of relnet_grad_stats (include/relnet_hip.h): range i runs on min(ceil(n / 4096), 2048) workgroups
ELEMS_PER_BLOCK, MAX_BLOCKS_PER_RANGE, MAX_RANGES = 4096, 2048, 16


def seed(id_):
    return zlib.crc32(id_.encode())


def range_blocks(n):
    return max(1, min(-(-n // ELEMS_PER_BLOCK), MAX_BLOCKS_PER_RANGE))


def stats_slots(ns):
    return sum(range_blocks(n) for n in ns)


# =============================================================================================================================================
# relnet_grad_stats
# =============================================================================================================================================
NAN, INF = float('nan'), float('inf')
N_CAP = MAX_BLOCKS_PER_RANGE * ELEMS_PER_BLOCK + 4099        # the cap of 2048 workgroups is reached and every thread loops more than four times


def _r(n, mis=0, kind='randn', poison=()):
    """One range: n elements starting `mis` floats (4 mis bytes) past a 16-byte boundary; poison = ((index, value), ...)."""
    return dict(n=n, mis=mis, kind=kind, poison=tuple(poison))


STATS_CASES = (
    [dict(id='n%d' % n, ranges=[_r(n)]) for n in (1, 3, 255, 256, 257)] +
    [dict(id='n%d-mis%d' % (n, m), ranges=[_r(n, m)]) for n, m in ((1, 1), (2, 3), (3, 1), (257, 2))] +
    [dict(id='unaligned-4097', ranges=[_r(4097, 1)]),                                  # head 3, body 1023 vectors, tail 2
     dict(id='table3', ranges=[_r(5000, 0), _r(1, 3), _r(300, 2)]),
     dict(id='table16', ranges=[_r(17 * (i + 1) + (4096 if i == 7 else 0), i % 4) for i in range(16)]),
     dict(id='grid-cap', ranges=[_r(N_CAP, 1)]),
     dict(id='huge-3e38', ranges=[_r(4099, 1, 'huge')]),
     dict(id='denormal', ranges=[_r(1029, 3, 'denormal')]),
     dict(id='zeros', ranges=[_r(513, 0, 'zeros')]),
     dict(id='nan-first', ranges=[_r(4097, 0, poison=[(0, NAN)])]),
     dict(id='nan-first-head', ranges=[_r(4097, 1, poison=[(0, NAN)])]),
     dict(id='nan-last', ranges=[_r(4096, 0, poison=[(4095, NAN)])]),
     dict(id='nan-last-tail', ranges=[_r(4097, 1, poison=[(4096, NAN)])]),
     dict(id='nan-in-tail', ranges=[_r(4097, 1, poison=[(4095, NAN)])]),          # the tail is elements 4095, 4096
     dict(id='nan-body-second-block', ranges=[_r(3 * 4096, 0, poison=[(4096 + 1024 + 5, NAN)])]),
     dict(id='nan-last-range', ranges=[_r(5000, 0), _r(1, 3), _r(300, 2, poison=[(299, NAN)])]),
     dict(id='nan-single-element-range', ranges=[_r(5000, 0), _r(1, 3, poison=[(0, NAN)]), _r(300, 2)]),
     dict(id='pos-inf', ranges=[_r(1000, 0, poison=[(500, INF)])]),
     dict(id='neg-inf', ranges=[_r(1000, 0, poison=[(501, -INF)])]),
     dict(id='both-inf-and-nan', ranges=[_r(1000, 1, poison=[(0, INF), (2, -INF), (999, NAN), (500, NAN)])])])


def stats_operands(case):
    """-> [(mis, float32 array)] per range."""
    out = []
    for k, r in enumerate(case['ranges']):
        g = np.random.default_rng(seed('%s/%d' % (case['id'], k)))
        n = r['n']
        if r['kind'] == 'randn':
            x = g.standard_normal(n).astype(np.float32)
        elif r['kind'] == 'huge':            # squares overflow float32 (9e76 > 3.4e38), not float64
            x = (g.choice([-1.0, 1.0], n) * g.uniform(2.9e38, 3.1e38, n)).astype(np.float32)
        elif r['kind'] == 'denormal':        # below 2^-126 = 1.18e-38: k 2^-149, the smallest and the largest denormal included
            bits = g.integers(1, 1 << 23, n).astype(np.uint32)
            bits[0], bits[-1] = 1, (1 << 23) - 1
            bits[1::2] |= np.uint32(0x80000000)
            x = bits.view(np.float32)
        else:
            x = np.zeros(n, np.float32)
        for i, v in r['poison']:
            x[i] = v
        out.append((r['mis'], x))
    return out


def stats_ref(arrays):
    """-> (sum of squares of the finite elements: float64 rounded from an extended-precision sum, number of inf / NaN elements, elements)."""
    s, bad, n = np.longdouble(0), 0, 0
    for x in arrays:
        fin = np.isfinite(x)
        s += np.sum(np.square(x[fin].astype(np.float64)).astype(np.longdouble))
        bad += int(x.size - fin.sum())
        n += x.size
    return float(s), bad, n


def sumsq_bound(n, ref):
    return n * U64 * ref


def norm_bound(n, ref_norm):
    return max(n, 2) * U64 * ref_norm


# =============================================================================================================================================
# relnet_grad_guard_decide
# =============================================================================================================================================
STATE_FIELDS = ('skip', 'scale', 'last_norm', 'last_nonfinite', 'steps', 'skipped', 'clipped', 'norm_sum', 'norm_max')


def fresh_state():
    return dict(skip=0, scale=np.float32(1.0), last_norm=0.0, last_nonfinite=0, steps=0, skipped=0, clipped=0, norm_sum=0.0, norm_max=0.0)


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6)) in float64; 1 without a max_norm or for a zero gradient."""
    if max_norm is None or max_norm <= 0 or norm == 0:
        return 1.0
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def decide_ref(state, sumsq, nonfinite, max_norm):
    """One decide step on a state dict (returns a new one)."""
    s = dict(state)
    norm = float(np.sqrt(np.float64(sumsq)))
    s['steps'] += 1
    s['last_norm'], s['last_nonfinite'] = norm, int(nonfinite)
    if nonfinite > 0:
        s['skip'], s['scale'] = 1, np.float32(1.0)
        s['skipped'] += 1
    else:
        s['skip'], s['scale'] = 0, np.float32(clip_coef(norm, max_norm))
        s['clipped'] += int(s['scale'] < np.float32(1.0))
        s['norm_sum'] += norm
        s['norm_max'] = max(s['norm_max'], norm)
    return s


def report_ref(s):
    return {'steps': s['steps'], 'skipped': s['skipped'], 'clipped': s['clipped'], 'last_norm': s['last_norm'],
            'last_nonfinite': s['last_nonfinite'], 'mean_norm': s['norm_sum'] / max(s['steps'] - s['skipped'], 1), 'max_norm_seen': s['norm_max']}


def _grad(n, entries):
    x = np.zeros(n, np.float32)
    for i, v in entries:
        x[i] = v
    return x


# Five steps on one state, max_norm 7: integer-valued gradients whose sums of squares are perfect squares, so every figure is exact.
SCRIPT_MAX_NORM = 7.0
SCRIPT = [('clean', _grad(300, [(0, 3.0), (299, 4.0)])),                       # norm 5
          ('clipped', _grad(4099, [(1, 6.0), (4098, 8.0)])),                   # norm 10 -> scale float32(7 / (10 + 1e-6))
          ('nan', _grad(300, [(7, NAN), (8, 1.0)])),
          ('clean', _grad(257, [(256, 2.0)])),                                 # norm 2
          ('inf', _grad(300, [(0, INF), (1, -INF), (2, 2.0)]))]


# =============================================================================================================================================
# relnet_sgd_update_guarded
# =============================================================================================================================================
SGD_LR, SGD_MOMENTUM, SGD_WD = 0.0005, 0.9, 0.0005
SGD_SIZES = (1, 257, 4099)
SGD_CASES = [dict(id='n%d-%s' % (n, 'bf' if bf else 'nobf'), n=n, bf16=bf) for n in SGD_SIZES for bf in (True, False)]
SGD_SCALE = 0.37            # a scale below 1 whose float32 value is not a power of two
SGD_CLIPS = (dict(clip=0.5, rescale=1.0, scale=1.0),          # about a third of N(0, 1) gradients are clamped
             dict(clip=0.25, rescale=0.5, scale=0.37),        # global scale first, then the clamp
             dict(clip=0.0, rescale=1.0, scale=1.0))          # c = 0 is ON (only c < 0 is off): the gradient term vanishes, weight decay stays


def sgd_operands(case):
    g = np.random.default_rng(seed('sgd-' + case['id']))
    n = case['n']
    return dict(w=g.standard_normal(n).astype(np.float32), mom=(0.1 * g.standard_normal(n)).astype(np.float32),
                grad=g.standard_normal(n).astype(np.float32))


def _f32(v):
    return float(np.float32(v))


def sgd_guarded_ref64(w, mom, grad, clip, rescale=1.0, scale=1.0, wd=SGD_WD):
    """-> (mom', w', bound of mom', bound of w') in float64 on the float32 values of the operands and constants; clip < 0: no clamp."""
    lr, mo, wd, rs, sc, c = _f32(SGD_LR), _f32(SGD_MOMENTUM), _f32(wd), _f32(rescale), _f32(scale), _f32(clip)
    w, m, g = w.astype(np.float64), mom.astype(np.float64), grad.astype(np.float64)
    raw = rs * g * sc
    t = np.clip(raw, -c, c) if c >= 0 else raw
    m1 = mo * m - lr * (t + wd * w)
    w1 = w + m1
    bm = 3 * U * (np.abs(mo * m) + lr * np.abs(t) + lr * wd * np.abs(w)) + 2 * U * lr * np.abs(raw)
    return m1, w1, bm, bm + U * np.abs(w1)
