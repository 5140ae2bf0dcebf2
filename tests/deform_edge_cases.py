"""Shared by tests/test_deform_edge_cases_host.py, tests/test_gpu_deform_edges.py and tests/golden/gen_golden_deform_edges.py: the deformable
kernels of csrc/deform.hip on inputs where EVERY SUMMATION ORDER GIVES THE SAME BITS.  numpy only (never the library), so it loads without a GPU.

Exact lattice.  Offsets are multiples of 1/8, data are non-zero integers in +-{1..8}, column gradients non-zero integers in +-{1..4} (all exact
in bf16).  Bilinear weights are then multiples of 1/64 <= 1, a data-gradient term w * g is a multiple of 1/64 of magnitude <= 4, an
offset-gradient term g (hw (v3 - v1) + lw (v4 - v2)) a multiple of 1/8 of magnitude <= 64; a feature cell collects fewer than 2^12 terms and a
(pixel, tap, group) fewer than 2^11, so every partial sum is a multiple of 2^-6 below 2^18: exactly representable in float32.  Atomic scatter,
gather + far, the reference's own kernels and the float64 restatement below agree bit for bit or one of them is wrong; no tolerance exists here.
test_deform_edge_cases_host.py certifies it per case (float32 in two summation orders == float64).

Offsets are ASSIGNED, not drawn: the (image, pixel, tap, group) pairs are walked in a seeded permutation and each gets a target sample position
p = base + off per axis from POS_CLASSES (L the map size on that axis); gather-capable cases also get the corner reaches at which
pair_near() (deform.hip) splits the pairs between the gather and the far kernel.  classify() recomputes every class from the offsets alone and
coverage_gaps() == [] is asserted by the host test, so a lattice that merely looks right cannot pass.

The restatement (col2im_restate) is written from the FORWARD definition (nn/deformable_im2col.cuh:76-113, 241-256: relative coordinates
map_h = i dil + off, cur_height = H - h_in, floor, the clamp band h_low >= cur_height - 1) as its exact adjoint; `mutant=` switches one rule to a
plausible wrong one (MUTANTS) and the host test shows each is seen on at least one case."""
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24             # unit roundoff of float32
K = 3                      # every case is a 3 x 3 kernel
T = K * K

# id, operand dtype, layout, B, C, H, W, pad, stride, dil, dg  -- the smallest shapes that reach every dispatch branch of relnet_deformable_col2im
COL2IM_CASES = [
    ('f32_ragged', 'f32', 'nchw', 2, 24, 7, 9, 1, 1, 1, 3),       # scatter, per-lane offset atomics, total % 256 != 0
    ('f32_wave', 'f32', 'nchw', 1, 128, 5, 6, 2, 1, 2, 2),        # scatter, in-wave offset reduction
    ('g64', 'bf16', 'cl', 2, 64, 9, 11, 2, 1, 2, 1),              # gather CPL = 1, lpg 8
    ('g128_tiny', 'bf16', 'cl', 1, 128, 5, 5, 1, 1, 1, 1),        # gather CPL = 2, lpg 16; map smaller than the 7 x 7 window
    ('g128_dg2', 'bf16', 'cl', 2, 128, 6, 7, 2, 1, 2, 2),         # gather CPL = 1, two groups with different offsets
    ('g512', 'bf16', 'cl', 1, 512, 4, 5, 1, 1, 1, 1),             # lpg 64: whole-wave shuffle in the offset kernel
    ('cl_s2', 'bf16', 'cl', 1, 64, 7, 9, 1, 2, 1, 1),             # stride 2 (7x9 -> 4x5): gather refused -> bf16 scatter
    ('cl_1024', 'bf16', 'cl', 1, 1024, 3, 4, 1, 1, 1, 1),         # lpg 128 > 64 -> scatter
    ('nchw_bf16', 'bf16', 'nchw', 1, 64, 5, 6, 1, 1, 1, 1),       # ds_c != 1 -> scatter
]
GATHER_CASES = ('g64', 'g128_tiny', 'g128_dg2', 'g512')
GOLDEN_CASES = tuple(c[0] for c in COL2IM_CASES if c[4] <= 128)
WINDOWS = (0, 1, 2, 3)

POS_CLASSES = ('le_m1', 'm1_0', 'zero', 'frac', 'int', 'last', 'band', 'L', 'gt_L')
INSIDE_CLASSES = ('zero', 'frac', 'int', 'last', 'band')
SMOOTH_CLASSES = ('lt_m1', 'm1_0', 'frac', 'band', 'gt_L')        # the subset float64 autograd can be asked about
MUTANTS = ('inside_le', 'trunc', 'no_clamp', 'left_deriv', 'near_lt', 'near_le_both', 'wrong_group')


class Case(object):
    def __init__(self, spec):
        (self.id, self.dtype, self.layout, self.B, self.C, self.H, self.W, self.pad, self.stride, self.dil, self.dg) = spec
        self.Ho = (self.H + 2 * self.pad - (self.dil * (K - 1) + 1)) // self.stride + 1
        self.Wo = (self.W + 2 * self.pad - (self.dil * (K - 1) + 1)) // self.stride + 1
        self.cpg = self.C // self.dg
        self.gather = self.id in GATHER_CASES

    def __repr__(self):
        return self.id


def case(id_):
    return Case([c for c in COL2IM_CASES if c[0] == id_][0])


def seed(id_):
    return zlib.crc32(id_.encode())


def _bases(c):
    """Undeformed tap positions cy [Ho, T], cx [Wo, T]."""
    i, j = np.arange(T) // K, np.arange(T) % K
    cy = (np.arange(c.Ho) * c.stride - c.pad)[:, None] + (i * c.dil)[None, :]
    cx = (np.arange(c.Wo) * c.stride - c.pad)[:, None] + (j * c.dil)[None, :]
    return cy, cx


def _position(cls, L, rng):
    """A sample position of class `cls` on the 1/8 lattice."""
    f = rng.integers(1, 8) / 8.0
    if cls == 'le_m1':
        return float(rng.choice([-1.0, -1.5, -2.25, -3.0]))
    if cls == 'lt_m1':
        return -1.0 - f
    if cls == 'm1_0':
        return -f
    if cls == 'zero':
        return 0.0
    if cls == 'frac':
        return float(rng.integers(0, L - 1)) + f
    if cls == 'int':
        return float(rng.integers(1, L - 1))
    if cls == 'last':
        return float(L - 1)
    if cls == 'band':
        return L - 1 + f
    if cls == 'L':
        return float(L)
    if cls == 'gt_L':
        return L + float(rng.choice([0.125, 1.375, 2.625]))
    raise KeyError(cls)


def _reach_targets(smooth):
    """(axis, kind, D): the offsets at which pair_near() decides, per axis, sign and window radius D.  'pos_near' off = D-1+f and 'neg_near'
    off = -D keep every corner within D cells; 'pos_far' off = D and 'neg_far' off = -D-f put one corner at D+1; 'clamp_near' is off = D at the
    row / column L-1-D, where the clamp band pulls the corner at D+1 back onto L-1."""
    kinds = ('pos_near', 'neg_far') if smooth else ('pos_near', 'neg_near', 'pos_far', 'neg_far', 'clamp_near')
    return [(ax, kind, D) for D in WINDOWS for ax in (0, 1) for kind in kinds]


def _reach_offset(kind, D, rng):
    f = rng.integers(1, 8) / 8.0
    return {'pos_near': D - 1 + f, 'neg_near': -float(D), 'pos_far': float(D), 'neg_far': -D - f, 'clamp_near': float(D)}[kind]


def build_offsets(c, smooth=False):
    """offset [B, 2 T dg, Ho, Wo] float32 (channel dg_i 2T + 2 tap + {0: h, 1: w}), every value a multiple of 1/8."""
    rng = np.random.default_rng(seed(c.id + ('/smooth' if smooth else '')))
    cy, cx = _bases(c)
    off = np.zeros((c.B, 2 * T * c.dg, c.Ho, c.Wo), F64)
    classes = SMOOTH_CLASSES if smooth else POS_CLASSES
    combos = [(a, b) for a in classes for b in classes]
    todo = [('pos',) + cb for cb in combos]
    if c.gather:
        todo += [('reach',) + t for t in _reach_targets(smooth)]
    pending = list(todo)
    L = (c.H, c.W)
    pairs = [(b, ho, wo, t, g) for b in range(c.B) for ho in range(c.Ho) for wo in range(c.Wo) for t in range(T) for g in range(c.dg)]
    for n in rng.permutation(len(pairs)):
        b, ho, wo, t, g = pairs[n]
        base = (int(cy[ho, t]), int(cx[wo, t]))
        if not pending:
            pending = list(todo)
        o = None
        for k, tgt in enumerate(pending):
            if tgt[0] == 'pos':
                o = (_position(tgt[1], c.H, rng) - base[0], _position(tgt[2], c.W, rng) - base[1])
            else:
                _, ax, kind, D = tgt
                d = _reach_offset(kind, D, rng)
                p = base[ax] + d
                if not (0 <= p < L[ax]) or (kind == 'clamp_near' and base[ax] != L[ax] - 1 - D):
                    continue
                # the other axis must not decide: its corners stay within D (clamped onto the last row / column when D == 0)
                q = base[1 - ax]
                if D == 0:
                    if q != L[1 - ax] - 1:
                        continue
                    e = 0.0 if not smooth else rng.integers(1, 8) / 8.0
                else:
                    e = rng.integers(1, 8) / 8.0
                    if not (0 <= q + e < L[1 - ax]):
                        continue
                o = (d, e) if ax == 0 else (e, d)
            del pending[k]
            break
        if o is None:                     # no pending target fits this pair: any class pair does
            a, b_ = combos[rng.integers(len(combos))]
            o = (_position(a, c.H, rng) - base[0], _position(b_, c.W, rng) - base[1])
        off[b, g * 2 * T + 2 * t, ho, wo] = o[0]
        off[b, g * 2 * T + 2 * t + 1, ho, wo] = o[1]
    assert np.array_equal(off * 8, np.round(off * 8)) and np.abs(off).max() < 64
    return off.astype(F32)


def build_operands(c, smooth=False):
    """-> data [B,C,H,W], offset, dcol [B,Ho,Wo,T,C] as float32 arrays of exact small values."""
    rng = np.random.default_rng(seed(c.id + '/operands'))
    data = (rng.integers(1, 9, (c.B, c.C, c.H, c.W)) * rng.choice([-1, 1], (c.B, c.C, c.H, c.W))).astype(F32)
    dcol = (rng.integers(1, 5, (c.B, c.Ho, c.Wo, T, c.C)) * rng.choice([-1, 1], (c.B, c.Ho, c.Wo, T, c.C))).astype(F32)
    return data, build_offsets(c, smooth), dcol


def checksum(*arrays):
    h = 0
    for a in arrays:
        h = zlib.crc32(np.ascontiguousarray(a).tobytes(), h)
    return np.uint32(h)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# geometry of every (image, pixel, tap, group) pair, from the forward definition
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _axis(base, in0, tapoff, off, L, mutant):
    """One axis.  base = in0 + tapoff the undeformed position, off the learned offset -> p, inside, absolute corner rows (lo, hi), the weight l
    of the high corner, whether the clamp band applies, whether the high corner is dropped (no_clamp mutant only)."""
    p = base + off
    inside = (p >= 0) & ((p <= L - 1) if mutant == 'inside_le' else (p < L))
    m = tapoff + off                                   # map_h: relative to in0 (:248)
    cur = L - in0                                      # cur_height (:250)
    low = np.trunc(m) if mutant == 'trunc' else np.floor(m)
    band = low >= cur - 1
    drop_hi = np.zeros_like(band)
    if mutant == 'no_clamp':
        drop_hi, band = band, np.zeros_like(band)      # plain bilinear with zeros beyond the map instead of the clamp band
    low = np.where(band, cur - 1, low)
    high = np.where(band, low, low + 1)
    m = np.where(band, low, m)
    l = m - low
    lo = np.clip(in0 + low, 0, L - 1).astype(np.int64)
    hi = np.clip(in0 + high, 0, L - 1).astype(np.int64)
    return p, inside, lo, hi, l, band, drop_hi


def geometry(c, offset, mutant=None):
    """Arrays [B, Ho, Wo, T, dg] (float64 / int64 / bool)."""
    off = np.asarray(offset, F64).reshape(c.B, c.dg, T, 2, c.Ho, c.Wo).transpose(0, 4, 5, 2, 1, 3)        # [B,Ho,Wo,T,dg,2]
    i, j = np.arange(T) // K, np.arange(T) % K
    sh = (1, c.Ho, 1, 1, 1); sw = (1, 1, c.Wo, 1, 1); st = (1, 1, 1, T, 1)
    h_in = (np.arange(c.Ho) * c.stride - c.pad).reshape(sh).astype(F64)
    w_in = (np.arange(c.Wo) * c.stride - c.pad).reshape(sw).astype(F64)
    th, tw = (i * c.dil).reshape(st).astype(F64), (j * c.dil).reshape(st).astype(F64)
    g = {}
    g['cy'], g['cx'] = np.broadcast_to(h_in + th, off.shape[:5]), np.broadcast_to(w_in + tw, off.shape[:5])
    g['py'], iy, g['ya'], g['yb'], g['lh'], g['band_h'], g['drop_h'] = _axis(g['cy'], h_in, th, off[..., 0], c.H, mutant)
    g['px'], ix, g['xa'], g['xb'], g['lw'], g['band_w'], g['drop_w'] = _axis(g['cx'], w_in, tw, off[..., 1], c.W, mutant)
    g['inside'] = iy & ix
    # signed corner reaches from the undeformed tap position (pair_near, deform.hip)
    g['ry'] = (g['ya'] - g['cy'], g['yb'] - g['cy'])
    g['rx'] = (g['xa'] - g['cx'], g['xb'] - g['cx'])
    g['reach'] = np.maximum(np.maximum(np.abs(g['ry'][0]), np.abs(g['ry'][1])), np.maximum(np.abs(g['rx'][0]), np.abs(g['rx'][1])))
    return g


def _pos_class(p, L):
    out = np.empty(p.shape, dtype='U6')
    integer = p == np.floor(p)
    out[p <= -1] = 'le_m1'
    out[(p > -1) & (p < 0)] = 'm1_0'
    out[p == 0] = 'zero'
    out[(p > 0) & (p < L - 1) & ~integer] = 'frac'
    out[(p > 0) & (p < L - 1) & integer] = 'int'
    out[p == L - 1] = 'last'
    out[(p > L - 1) & (p < L)] = 'band'
    out[p == L] = 'L'
    out[p > L] = 'gt_L'
    return out


def classify(c, offset):
    """What the lattice of one case holds, recomputed from the offsets alone."""
    g = geometry(c, offset)
    ch, cw = _pos_class(g['py'], c.H), _pos_class(g['px'], c.W)
    rep = {'h': set(np.unique(ch)), 'w': set(np.unique(cw)), 'combos': set(zip(ch.ravel(), cw.ravel())), 'reach': set()}
    ins = g['inside']
    for ax, (r, other) in enumerate(((g['ry'], g['rx']), (g['rx'], g['ry']))):
        omax = np.maximum(np.abs(other[0]), np.abs(other[1]))
        unclamped_hi = np.floor(g['py' if ax == 0 else 'px']) + 1 - (g['cy'] if ax == 0 else g['cx'])
        for D in WINDOWS:
            rest = ins & (omax <= D)
            if (rest & (r[1] == D) & (r[0] >= -D)).any():
                rep['reach'].add((ax, 'pos_near', D))
            if (rest & (r[0] == -D) & (r[1] <= D)).any():
                rep['reach'].add((ax, 'neg_near', D))
            if (rest & (r[1] == D + 1) & (r[0] >= -D)).any():
                rep['reach'].add((ax, 'pos_far', D))
            if (rest & (r[0] == -D - 1) & (r[1] <= D)).any():
                rep['reach'].add((ax, 'neg_far', D))
            if (rest & (r[1] == D) & (r[0] >= -D) & (unclamped_hi == D + 1)).any():
                rep['reach'].add((ax, 'clamp_near', D))
    rep['near'] = {D: int((ins & (g['reach'] <= D)).sum()) for D in WINDOWS}
    rep['far'] = {D: int((ins & (g['reach'] > D)).sum()) for D in WINDOWS}
    rep['inside'] = int(ins.sum()); rep['pairs'] = int(ins.size)
    return rep


def coverage_gaps(c, rep):
    """The classes a case must hold and does not (empty = covered)."""
    gaps = [('h', k) for k in POS_CLASSES if k not in rep['h']] + [('w', k) for k in POS_CLASSES if k not in rep['w']]
    gaps += [('combo', a, b) for a in INSIDE_CLASSES for b in INSIDE_CLASSES if (a, b) not in rep['combos']]
    if c.gather:
        gaps += [('reach',) + t for t in _reach_targets(False) if t not in rep['reach']]
        gaps += [('split', D) for D in WINDOWS if not (rep['near'][D] and rep['far'][D])]
    return gaps


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the restatement: exact adjoint of the forward definition
# ---------------------------------------------------------------------------------------------------------------------------------------------
def col2im_restate(c, data, offset, dcol, dtype=F64, mutant=None, win=None, reverse=False):
    """-> (grad_data [B,C,H,W], grad_offset [B, 2 T dg, Ho, Wo]) accumulated in `dtype` onto zeros.  win = D evaluates the data gradient as the
    product's gather + far pair of passes does (every pair once: the result does not depend on D unless a near_* mutant is on); reverse walks
    the pairs and the channels backwards (another summation order)."""
    assert mutant in (None,) + MUTANTS
    g = geometry(c, offset, mutant)
    data = np.asarray(data, dtype); dcol = np.asarray(dcol, dtype)
    rep = lambda a: np.repeat(a, c.cpg, axis=-1)                                   # [B,Ho,Wo,T,dg] -> [B,Ho,Wo,T,C] (channel c uses group c // cpg)
    lh, lw = rep(g['lh']).astype(dtype), rep(g['lw']).astype(dtype)
    one = dtype(1)
    hh, hw = one - lh, one - lw
    ya, yb, xa, xb = rep(g['ya']), rep(g['yb']), rep(g['xa']), rep(g['xb'])
    keep_h, keep_w = (~rep(g['drop_h'])).astype(dtype), (~rep(g['drop_w'])).astype(dtype)
    w1, w2, w3, w4 = hh * hw, hh * lw * keep_w, lh * hw * keep_h, lh * lw * keep_h * keep_w
    inside = rep(g['inside'])
    mult = np.ones(inside.shape, np.int64)
    if win is not None:
        near = g['reach'] <= win
        gathered, scattered = near, ~near
        if mutant == 'near_lt':            # the gather tests `< D` on the positive side: the pair at reach exactly D is in neither pass
            gathered = near & (g['ry'][1] < win) & (g['rx'][1] < win)
        if mutant == 'near_le_both':       # the far pass tests `>= D`: the pair at reach exactly D is in both
            scattered = g['reach'] >= win
        mult = rep(gathered.astype(np.int64) + scattered.astype(np.int64))
    bi = np.arange(c.B).reshape(-1, 1, 1, 1, 1); ci = np.arange(c.C).reshape(1, 1, 1, 1, -1)
    flat = lambda y, x: (((bi * c.C + ci) * c.H + y) * c.W + x)
    gd = np.zeros(c.B * c.C * c.H * c.W, dtype)
    sel = inside & (mult > 0)
    idx = np.concatenate([flat(ya, xa)[sel], flat(ya, xb)[sel], flat(yb, xa)[sel], flat(yb, xb)[sel]])
    val = np.concatenate([((w * dcol) * mult.astype(dtype))[sel] for w in (w1, w2, w3, w4)]).astype(dtype)
    if reverse:
        idx, val = idx[::-1], val[::-1]
    np.add.at(gd, idx, val)
    # offset gradient: d/d off_h = hw (v3 - v1) + lw (v4 - v2), d/d off_w = hh (v2 - v1) + lh (v4 - v3); a clamped axis has ya == yb
    def corners(ya_, yb_, xa_, xb_):
        return (data[bi, ci, ya_, xa_], data[bi, ci, ya_, xb_] * keep_w, data[bi, ci, yb_, xa_] * keep_h, data[bi, ci, yb_, xb_] * keep_h * keep_w)
    v1, v2, v3, v4 = corners(ya, yb, xa, xb)
    dh = hw * (v3 - v1) + lw * (v4 - v2)
    dw = hh * (v2 - v1) + lh * (v4 - v3)
    if mutant == 'left_deriv':             # at an integer position take the cell below / left of it instead of the one above / right
        at_h = (lh == 0) & ~rep(g['band_h']); at_w = (lw == 0) & ~rep(g['band_w'])
        u1, u2, u3, u4 = corners(np.maximum(ya - 1, 0), ya, xa, xb)
        dh = np.where(at_h, hw * (u3 - u1) + lw * (u4 - u2), dh)
        u1, u2, u3, u4 = corners(ya, yb, np.maximum(xa - 1, 0), xa)
        dw = np.where(at_w, hh * (u2 - u1) + lh * (u4 - u3), dw)
    dh = np.where(inside, dcol * dh, dtype(0)).astype(dtype); dw = np.where(inside, dcol * dw, dtype(0)).astype(dtype)
    gidx = np.arange(c.C) % c.dg if mutant == 'wrong_group' else np.arange(c.C) // c.cpg
    go = np.zeros((c.B, c.dg, T, 2, c.Ho, c.Wo), dtype)
    order = np.arange(c.C)[::-1] if reverse else np.arange(c.C)
    for ch in order:                       # sequential, in `dtype`
        go[:, gidx[ch], :, 0] += dh[..., ch].transpose(0, 3, 1, 2)
        go[:, gidx[ch], :, 1] += dw[..., ch].transpose(0, 3, 1, 2)
    return gd.reshape(c.B, c.C, c.H, c.W), go.reshape(c.B, 2 * T * c.dg, c.Ho, c.Wo)


def dcol_to_reference(c, dcol, b):
    """dcol [B,Ho,Wo,T,C] -> the reference's column layout of image b: [C T, Ho, Wo], row c T + tap."""
    return np.ascontiguousarray(dcol[b].transpose(3, 2, 0, 1).reshape(c.C * T, c.Ho, c.Wo))


# =============================================================================================================================================
# Deformable PSROI pooling (deformable_psroi_pooling.cu:51-138 forward, :178-300 backward) on a dyadic geometry
# =============================================================================================================================================
# Map 6 x 8, two images, spatial_scale 1/16, trans_std 1/8.  A roi's extent in pixels is P * spp * s with s (the sub-bin in pixels) in {1, 2, 4}:
# the extent is a multiple of 7 px (of 3 px for P = 3), bins and sub-bins are dyadic, trans is a multiple of 1/2, so every sample coordinate is a
# multiple of 2^-6, every bilinear weight of 2^-12 and every term of the four sums below an exact float32 with room for its whole sum (psroi_restate
# returns the largest sum of |terms| per address in units of the lattice; the host test asserts it stays below 2^24, which makes EVERY order exact).
# The forward's one inexact operation, sum / count, is a single correctly rounded float32 division of an exact sum: the same bits everywhere.
PS_H, PS_W, PS_B = 6, 8, 2
PS_SCALE, PS_TRANS_STD = 0.0625, 0.125
PS_SHAPES = [(1, 7, 7, 1, 8), (1, 7, 7, 2, 128), (3, 3, 3, 2, 8), (1, 7, 7, 1, 256)]      # (group, P, part, classes, output_dim)
PS_SPP = (1, 2, 3, 4, 5)
PS_ROI_CLASSES = [('in_int', 'in_int'), ('in_frac', 'in_frac'), ('low', 'in_int'), ('high', 'in_frac'), ('in_frac', 'low'), ('in_int', 'high'),
                  ('low', 'low'), ('high', 'high'), ('low', 'high'), ('high', 'low'), ('out', 'in_int'), ('in_frac', 'out'), ('out', 'out')]
PS_SAMPLE_CLASSES = ('invalid_low', 'edge_low', 'clamp_low', 'int', 'frac', 'clamp_high', 'edge_high', 'invalid_high')
PS_MUTANTS = ('valid_open', 'floor_plus1', 'trans_onesided', 'spp_cap4')


class PsCfg(object):
    def __init__(self, shape, spp, with_trans):
        self.group, self.P, self.part, self.ncls, self.od = shape
        self.spp, self.with_trans = spp, with_trans
        self.C = self.od * self.group * self.group
        self.id = 'g%d_P%d_k%d_od%d_spp%d_%s' % (self.group, self.P, self.ncls, self.od, spp, 'trans' if with_trans else 'notrans')
        self.sub_px = (2, 4) if spp <= 2 else (1, 2)          # sub-bin sizes in pixels: extents P * spp * {these}

    def __repr__(self):
        return self.id


def ps_configs(max_channels=None):
    return [PsCfg(s, spp, t) for s in PS_SHAPES for spp in PS_SPP for t in (False, True) if max_channels is None or s[4] * s[0] ** 2 <= max_channels]


def _ps_axis(cls, ext, s, L, spp):
    """First pixel of a roi of class `cls` on an axis of L cells: its samples sit at x1/16 - 0.5 + n s/16, n = 0 .. ext/s - 1."""
    n = ext // s
    k = 3 if spp == 2 else 2                       # samples beyond the border: never a whole number of bins (spp > 1), so a bin is cut
    if cls == 'in_int':
        return 24                                  # first sample exactly on cell 1
    if cls == 'in_frac':
        return 21
    if cls == 'low':
        return -k * s                              # sample k exactly on -0.5 (valid), the k before it one, two.. sub-bins beyond (invalid)
    if cls == 'high':
        return 16 * L - (n - 1 - k) * s            # sample n-1-k exactly on L - 0.5 (valid), the last k beyond
    return -400                                    # every sample invalid


def ps_operands(cfg):
    """-> data [B,C,H,W], rois [R,5], trans [R, 2 ncls, part, part] | None, mult [R,od,P,P] (grad_out = top_count * mult), float32."""
    rng = np.random.default_rng(seed(cfg.id))
    data = (rng.integers(1, 9, (PS_B, cfg.C, PS_H, PS_W)) * rng.choice([-1, 1], (PS_B, cfg.C, PS_H, PS_W))).astype(F32)
    rois = []
    for k, (cx, cy) in enumerate(PS_ROI_CLASSES):
        sx, sy = cfg.sub_px[k % 2], cfg.sub_px[(k // 2) % 2]
        ex, ey = cfg.P * cfg.spp * sx, cfg.P * cfg.spp * sy
        x1, y1 = _ps_axis(cx, ex, sx, PS_W, cfg.spp), _ps_axis(cy, ey, sy, PS_H, cfg.spp)
        rois.append([k % PS_B, x1, y1, x1 + ex - 1, y1 + ey - 1])
    rois = np.asarray(rois, F32)
    R = len(rois)
    trans = None
    if cfg.with_trans:
        # shift = trans * trans_std * extent / 16 cells = trans * extent / 128: the step of trans keeps it on the 2^-6 lattice
        ext = cfg.P * cfg.spp * min(cfg.sub_px)
        step = [t for t in (0.5, 1.0, 2.0) if (t * ext) % 2 == 0][0]
        menu = [0, 0, step, -step, 2 * step, -2 * step, 3 * step, -3 * step, 4 * step, -4 * step]
        trans = rng.choice(np.asarray(menu, F32), (R, 2 * cfg.ncls, cfg.part, cfg.part))
        trans[0::4] = 0                            # every fourth roi keeps its class positions under trans
    mult = (rng.integers(1, 5, (R, cfg.od, cfg.P, cfg.P)) * rng.choice([-1, 1], (R, cfg.od, cfg.P, cfg.P))).astype(F32)
    return data, rois, trans, mult


def _ps_sample_class(v, L):
    out = np.empty(v.shape, dtype='U12')
    integer = v == np.floor(v)
    out[v < -0.5] = 'invalid_low'; out[v == -0.5] = 'edge_low'; out[(v > -0.5) & (v < 0)] = 'clamp_low'
    out[(v >= 0) & (v <= L - 1) & integer] = 'int'; out[(v >= 0) & (v <= L - 1) & ~integer] = 'frac'
    out[(v > L - 1) & (v < L - 0.5)] = 'clamp_high'; out[v == L - 0.5] = 'edge_high'; out[v > L - 0.5] = 'invalid_high'
    return out


def psroi_restate(cfg, data, rois, trans, mult=None, mutant=None, dtype=F64, reverse=False, batch_index_base=0, bounds=False):
    """The operator from its definition.  -> dict: top (float32: exact sum, one float32 division), count, and with `mult` grad_out = count * mult,
    grad_data [B,C,H,W], grad_trans (like trans), accumulated in `dtype`; abs_data / abs_trans the sums of |terms| per address; classes the sample
    classes met per axis; lattice the finest power of two every coordinate is a multiple of.  bounds=True (the bounded set: inputs off the
    lattice) skips the lattice bookkeeping and adds the magnitudes PS_BOUND_K multiplies: mag_top, mag_data, mag_trans."""
    assert mutant in (None,) + PS_MUTANTS
    data64 = np.asarray(data, F64)
    P, spp, od, G = cfg.P, cfg.spp, cfg.od, cfg.group
    R = rois.shape[0]
    ch_each = od // cfg.ncls if trans is not None else od
    ctop = np.arange(od)
    cls = ctop // ch_each
    ph = np.arange(P)
    part_idx = np.floor(ph / P * cfg.part).astype(np.int64)
    g_idx = np.clip(np.floor(ph * G / P).astype(np.int64), 0, G - 1)
    cin = (ctop[:, None, None] * G + g_idx[None, :, None]) * G + g_idx[None, None, :]                  # [od,P,P]
    top = np.zeros((R, od, P, P), F32); cnt = np.zeros((R, od, P, P), F32)
    res = {'classes': {'w': set(), 'h': set()}, 'lattice': 1.0}
    gd = np.zeros((PS_B, cfg.C, PS_H, PS_W), dtype); gd_abs = np.zeros(gd.shape, F64)
    gt = None if trans is None else np.zeros(trans.shape, dtype)
    gt_abs = None if trans is None else np.zeros(trans.shape, F64)
    mag_top = np.zeros((R, od, P, P)); mag_data = np.zeros(gd.shape); mag_trans = None if trans is None else np.zeros(trans.shape)
    nloop = min(spp, 4) if mutant == 'spp_cap4' else spp
    samples = [(ih, iw) for ih in range(nloop) for iw in range(nloop)]
    if reverse:
        samples = samples[::-1]
    for n in (range(R - 1, -1, -1) if reverse else range(R)):
        b = int(rois[n, 0]) - batch_index_base
        rnd = lambda v: np.sign(v) * np.floor(np.abs(v) + 0.5)
        sw_, sh_ = rnd(rois[n, 1]) * PS_SCALE - 0.5, rnd(rois[n, 2]) * PS_SCALE - 0.5
        tenth = float(F32(0.1))                    # (the float32 constant both implementations compare with)
        rw = max((rnd(rois[n, 3]) + 1) * PS_SCALE - 0.5 - sw_, tenth); rh = max((rnd(rois[n, 4]) + 1) * PS_SCALE - 0.5 - sh_, tenth)
        bw, bh = rw / P, rh / P
        subw, subh = bw / spp, bh / spp
        if trans is None:
            tx = np.zeros((od, P, P)); ty = np.zeros((od, P, P))
        else:
            t = np.asarray(trans[n], F64).reshape(cfg.ncls, 2, cfg.part, cfg.part)
            tx = t[cls, 0][:, part_idx][:, :, part_idx] * PS_TRANS_STD
            ty = t[cls, 1][:, part_idx][:, :, part_idx] * PS_TRANS_STD
        wstart = (ph * bw + sw_)[None, None, :] + tx * rw
        hstart = (ph * bh + sh_)[None, :, None] + ty * rh
        s = np.zeros((od, P, P)); k = np.zeros((od, P, P), np.int64)
        per_sample = []
        for ih, iw in samples:
            w = wstart + iw * subw + np.zeros_like(hstart); h = hstart + ih * subh + np.zeros_like(wstart)
            for v in (() if bounds else (w[::ch_each], h[::ch_each])):          # (the geometry is per class of channels)
                while not np.array_equal(v / res['lattice'], np.round(v / res['lattice'])):
                    res['lattice'] /= 2
            res['classes']['w'] |= set(np.unique(_ps_sample_class(w[::ch_each], PS_W)))
            res['classes']['h'] |= set(np.unique(_ps_sample_class(h[::ch_each], PS_H)))
            if mutant == 'valid_open':
                ok = ~((w <= -0.5) | (w >= PS_W - 0.5) | (h <= -0.5) | (h >= PS_H - 0.5))
            else:
                ok = ~((w < -0.5) | (w > PS_W - 0.5) | (h < -0.5) | (h > PS_H - 0.5))
            w = np.clip(w, 0, PS_W - 1); h = np.clip(h, 0, PS_H - 1)
            x0 = np.floor(w).astype(np.int64); y0 = np.floor(h).astype(np.int64)
            if mutant == 'floor_plus1':
                x1 = np.minimum(x0 + 1, PS_W - 1); y1 = np.minimum(y0 + 1, PS_H - 1)
            else:
                x1 = np.ceil(w).astype(np.int64); y1 = np.ceil(h).astype(np.int64)
            dx, dy = w - x0, h - y0
            d = data64[b]
            u00, u01, u10, u11 = d[cin, y0, x0], d[cin, y1, x0], d[cin, y0, x1], d[cin, y1, x1]
            val = (1 - dx) * (1 - dy) * u00 + (1 - dx) * dy * u01 + dx * (1 - dy) * u10 + dx * dy * u11
            s += np.where(ok, val, 0.0); k += ok
            mag_top[n] += np.where(ok, np.abs(u00) + np.abs(u01) + np.abs(u10) + np.abs(u11), 0.0)
            # the trans gradient reads the same corners; at an integer coordinate x0 == x1 and its term vanishes (:283-292)
            x1t, y1t = x1, y1
            if mutant == 'trans_onesided':
                x1t = np.minimum(x0 + 1, PS_W - 1); y1t = np.minimum(y0 + 1, PS_H - 1)
            t00, t01, t10, t11 = (u00, u01, u10, u11) if mutant != 'trans_onesided' else (d[cin, y0, x0], d[cin, y1t, x0], d[cin, y0, x1t], d[cin, y1t, x1t])
            per_sample.append((ok, x0, x1, y0, y1, dx, dy, (t11 * dy + t10 * (1 - dy) - t01 * dy - t00 * (1 - dy)),
                               (t11 * dx + t01 * (1 - dx) - t10 * dx - t00 * (1 - dx)),
                               np.abs(t00) + np.abs(t01) + np.abs(t10) + np.abs(t11)))
        if bounds:
            top[n] = np.where(k == 0, 0.0, s / np.maximum(k, 1)).astype(F32)
            mag_top[n] /= np.maximum(k, 1)
        else:
            top[n] = np.where(k == 0, F32(0), s.astype(F32) / np.maximum(k, 1).astype(F32))
            assert np.array_equal(s.astype(F32).astype(F64), s)
        cnt[n] = k
        if mult is None:
            continue
        diff = np.where(k > 0, np.asarray(mult[n], F64), 0.0)           # grad_out / count = mult exactly
        for ok, x0, x1, y0, y1, dx, dy, ex, ey, ua in per_sample:
            m = ok & (k > 0)
            for yy, xx, q in ((y0, x0, (1 - dx) * (1 - dy)), (y1, x0, (1 - dx) * dy), (y0, x1, dx * (1 - dy)), (y1, x1, dx * dy)):
                v = (q * diff)[m]
                np.add.at(gd[b], (cin[m], yy[m], xx[m]), v.astype(dtype)); np.add.at(gd_abs[b], (cin[m], yy[m], xx[m]), np.abs(v))
                if bounds:
                    np.add.at(mag_data[b], (cin[m], yy[m], xx[m]), np.abs(diff[m]))
            if trans is not None:
                ci = np.broadcast_to(cls[:, None, None], m.shape)[m]
                pi = np.broadcast_to(part_idx[None, :, None], m.shape)[m]; pj = np.broadcast_to(part_idx[None, None, :], m.shape)[m]
                vx = (ex * PS_TRANS_STD * diff * rw)[m]; vy = (ey * PS_TRANS_STD * diff * rh)[m]
                if reverse:
                    ci, pi, pj, vx, vy = ci[::-1], pi[::-1], pj[::-1], vx[::-1], vy[::-1]
                np.add.at(gt[n], (2 * ci, pi, pj), vx.astype(dtype)); np.add.at(gt[n], (2 * ci + 1, pi, pj), vy.astype(dtype))
                np.add.at(gt_abs[n], (2 * ci, pi, pj), np.abs(vx)); np.add.at(gt_abs[n], (2 * ci + 1, pi, pj), np.abs(vy))
                if bounds:
                    mx = (ua * PS_TRANS_STD * np.abs(diff) * rw)[m]; my = (ua * PS_TRANS_STD * np.abs(diff) * rh)[m]
                    np.add.at(mag_trans[n], (2 * ci, pi, pj), mx[::-1] if reverse else mx)
                    np.add.at(mag_trans[n], (2 * ci + 1, pi, pj), my[::-1] if reverse else my)
    res.update(top=top, count=cnt, grad_data=gd, grad_trans=gt, abs_data=gd_abs, abs_trans=gt_abs, mag_top=mag_top, mag_data=mag_data, mag_trans=mag_trans)
    return res


def ps_grad_out(count, mult):
    """grad_out = top_count * mult where the bin has samples (grad_out / count is then the integer mult), mult elsewhere (never read)."""
    return np.where(count > 0, count * mult, mult).astype(F32)


def ps_exact_units(cfg, r):
    """Sums of |terms| per address in units of the terms' lattice: below 2^24 every partial sum of every order is an exact float32.
    Data-gradient terms are q * diff (q a product of two coordinates' fractions); trans-gradient terms are
    (fraction * data) * trans_std (2^-3) * diff * roi extent (a multiple of 2^-4)."""
    ud = r['abs_data'] / r['lattice'] ** 2
    ut = None if r['abs_trans'] is None else r['abs_trans'] / (r['lattice'] * 2.0 ** -7)
    return ud, ut


GOLDEN_TOP_CHANNELS = {8: list(range(8)), 128: [0, 63, 64, 127]}       # the 128-channel shape stores the first and last channel of each class


def golden_data_channels(cfg):
    """Input channels whose data gradient the golden file keeps: all of them up to 72, those of GOLDEN_TOP_CHANNELS (group_size 1) beyond."""
    return list(range(cfg.C)) if cfg.C <= 72 else GOLDEN_TOP_CHANNELS[cfg.od]


_cache = {}


def col2im_reference(id_):
    """(case, data, offset, dcol, grad_data, grad_offset) of one exact case, computed once."""
    if id_ not in _cache:
        c = case(id_)
        data, off, dcol = build_operands(c)
        _cache[id_] = (c, data, off, dcol) + col2im_restate(c, data, off, dcol)
    return _cache[id_]


def ps_reference(cfg):
    if cfg.id not in _cache:
        ops = ps_operands(cfg)
        _cache[cfg.id] = ops + (psroi_restate(cfg, *ops),)
    return _cache[cfg.id]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The bounded set: the degenerate roi (x2 < x1: the extent is floored to 0.1, which no lattice holds).  Results are compared with the float64
# restatement under |error| <= k u magnitude, k counted from the kernels' expressions (first order in u = 2^-24), never fitted:
#   coordinates   w = fl(fl(fl(pw bin) + start) + fl(tx roi)) + fl(iw sub)) with bin = fl(roi / P), sub = fl(bin / spp): three additions whose
#                 results stay below 3 (the rois below keep every sample in (1, 3)) err by 3 * 3 u, the small addends (pw bin, tx roi, iw sub: < 0.3 in
#                 all since |trans| <= 8, each carrying at most 3 roundings) by 0.9 u: |dw|, |dh| <= 10 u.  dx = w - floor(w) is exact, so every bilinear weight inherits dw + dh = 20 u
#                 absolutely; no sample sits within 0.2 of an integer, so no floor / ceil decision can flip.
#   forward       a corner term q v errs by |v| 20 u + 4 u q |v| (1 - dx, 1 - dy, their product, the product with v), the sample's 4 terms add
#                 with 3 roundings, the bin's spp^2 samples with spp^2, the division with 1:  k = 20 + 4 + 3 + spp^2 + 1,
#                 magnitude = sum over samples and corners of |v| / count  (every weight is <= 1).
#   data gradient a cell receives n = P^2 spp^2 (bin, sample) terms q diff per channel (all bins of such a roi share 4 cells): weights 20 u, the
#                 per-axis sums of the spp <= 4 form 2 (spp - 1), 1 - d twice, two products and the division 5, the accumulation n:
#                 k = 20 + 2 spp + 3 + n, magnitude = sum of |diff| over those terms.
#   trans gradient a term (u11 dy + u10 (1 - dy) - u01 dy - u00 (1 - dy)) std diff roi: dy errs by 10 u, 1 - dy, four products, three additions,
#                 three more products and the division behind diff 12; n = channels per class * spp^2 terms accumulate:
#                 k = 10 + 12 + n, magnitude = sum of (|u00| + |u01| + |u10| + |u11|) std |diff| roi.
PS_DEGENERATE_ROIS = np.asarray([[0, 45, 33, 42, 31], [1, 29.5, 49, 20, 40]], F32)        # (.5: CUDA round(), half away from zero)
PS_DEGENERATE_CFGS = [(0, 1, False), (0, 1, True), (0, 4, False), (0, 4, True), (0, 5, True), (2, 3, True), (3, 4, True), (3, 5, True)]   # (shape, spp, trans)


def ps_bound_k(cfg):
    n_cell = cfg.P * cfg.P * cfg.spp ** 2
    n_tr = (cfg.od // cfg.ncls) * cfg.spp ** 2
    return {'top': 20 + 4 + 3 + cfg.spp ** 2 + 1, 'grad_data': 20 + 2 * cfg.spp + 3 + n_cell, 'grad_trans': 10 + 12 + n_tr}


def ps_degenerate(k):
    """-> (cfg, data, rois, trans, mult, restatement with magnitudes) of the k-th bounded case."""
    key = ('degenerate', k)
    if key not in _cache:
        shape, spp, with_trans = PS_DEGENERATE_CFGS[k]
        cfg = PsCfg(PS_SHAPES[shape], spp, with_trans)
        data, _, trans, mult = ps_operands(cfg)
        R = len(PS_DEGENERATE_ROIS)
        trans = None if trans is None else trans[:R] + 0
        mult = mult[:R] + 0
        _cache[key] = (cfg, data, PS_DEGENERATE_ROIS, trans, mult, psroi_restate(cfg, data, PS_DEGENERATE_ROIS, trans, mult, bounds=True))
    return _cache[key]


def worst(got, want, bound):
    """Largest |got - want| / bound (0 / 0 counts as 0)."""
    err = np.abs(np.asarray(got, F64) - want)
    return float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max())
