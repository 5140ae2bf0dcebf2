"""Case tables, CPU restatement and error bounds of PSROIPooling (csrc/psroi_pool.hip; psroi_pooling.cu:32-101 forward, :132-194
backward of the reference).  The operator is pinned by known answers (tests/test_psroi_cases_host.py) and by this restatement, like
ROIAlign: the recipe that compiles the reference's own kernels for the checker cannot take a third file.

THE OPERATOR.  Per output element (n, ctop, ph, pw), P = pooled_size, g = group_size (0 = P), everything in float32 with every product
and sum rounded on its own:
    start_w = round(x1) * scale, end_w = (round(x2) + 1) * scale        (C round: halves away from zero), h from y1 / y2 alike
    roi_w = max(end_w - start_w, 0.1), bin_w = roi_w / P
    wstart = clip(floor(pw * bin_w + start_w), 0, W), wend = clip(ceil((pw + 1) * bin_w + start_w), 0, W)
    gw = clamp(floor(float(pw) * g / P), 0, g - 1), c = (ctop * g + gh) * g + gw
    out = 0 for an empty bin, else (sum over the window of data[b][c]) / bin_area;  mapping_channel = c
A roi whose batch index minus batch_index_base is outside [0, B) pools to zeros and gives no gradient.
The bin EDGES are float32 by definition (they decide which integers come out), so both forms below take them in float32; "float64"
refers to the sums and the divisions.  `edges(..., mode=)` also evaluates them in float64 and with the multiply-add contracted, which
is how the host test holds the tables that claim an exact geometry to that claim.

THE TWO FORMS.  psroi_restate(..., dtype=np.float32) follows the documented summation order with float32 operations only:
    forward:  sum from 0, h ascending then w ascending, one division by the cell count;
    backward: every word of grad_in is the sum from 0, in ascending (roi, ph, pw) order, of grad_out / bin_area (one division each) over
              the bins that hold the cell and map to the channel; `grad_in0` (kAddTo) is added to that sum with one addition.
The kernels must reproduce it bit for bit.  dtype=np.float64 does the same in float64: the yardstick of the bounds.

THE BOUNDS (derived, not measured), u = 2^-24 the unit roundoff of float32:
    forward.  A float32 sum of n terms in ANY order has error <= (n - 1) u sum|x| (1 + O(u)) (Higham, Accuracy and Stability, eq. 4.4);
    the division adds one rounding, u |result| <= u sum|x| / area.  Together <= n u sum|x| / area to first order; the bound used is
    n 2^-23 sum|x| / area = 2 n u sum|x| / area, the factor 2 covering the O(u^2) terms (n <= 54 here) and the float64 yardstick's own
    rounding.  A bf16 output adds one rounding to 8 significant bits: 2^-8 (|exact| + the float32 bound).
    backward.  Each contribution carries one division rounding, u |contribution|, and the sum of n_add contributions in any order adds
    (n_add - 1) u sum|contribution|; kAddTo adds one more addition, which the `+ 1` covers: (n_add + 1) 2^-23 sum|contribution|, with
    the prior value counted among the contributions when accumulating.
"""
import numpy as np

F32, F64 = np.float32, np.float64


def c_round(x):
    """C round(): to nearest, halves away from zero.  x float32 -> float32 (exact: |x| + 0.5 is exact in float64)."""
    x = np.asarray(x, F64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(F32)


def _muladd(a, b, c, mode):
    """a * b + c on float32 operands.  'f32': product and sum rounded to float32 one after the other (the operator).  'fma': one rounding
    (the product of two float32 is exact in float64; the float64 sum's own rounding sits 29 bits below float32's).  'f64': float64."""
    if mode == 'f32':
        return F32(F32(a) * F32(b)) + F32(c)
    if mode == 'fma':
        return F32(F64(a) * F64(b) + F64(c))
    return F64(a) * F64(b) + F64(c)


def edges(roi, scale, P, H, W, mode='f32'):
    """Bin edges of one roi row [batch, x1, y1, x2, y2]: integer arrays hs, he, ws, we of length P, clipped to the map."""
    ft = F64 if mode == 'f64' else F32
    scale = ft(F32(scale))
    x1, y1, x2, y2 = (ft(v) for v in c_round(np.asarray(roi[1:5], F32)))
    start_w, start_h = x1 * scale, y1 * scale
    end_w, end_h = (x2 + ft(1)) * scale, (y2 + ft(1)) * scale
    bin_w = max(end_w - start_w, ft(F32(0.1))) / ft(P)
    bin_h = max(end_h - start_h, ft(F32(0.1))) / ft(P)
    p = np.arange(P)

    def span(bin_, start, L):
        s = np.array([np.floor(_muladd(ft(q), bin_, start, mode)) for q in p], F64)
        e = np.array([np.ceil(_muladd(ft(q + 1), bin_, start, mode)) for q in p], F64)
        return np.clip(s, 0, L).astype(np.int64), np.clip(e, 0, L).astype(np.int64)

    hs, he = span(bin_h, start_h, H)
    ws, we = span(bin_w, start_w, W)
    return hs, he, ws, we


def groups(P, g):
    """Group row / column of every bin index: clamp(floor(float(p) * g / P), 0, g - 1) in float32."""
    return np.array([min(max(int(np.floor(F32(F32(p) * F32(g)) / F32(P))), 0), g - 1) for p in range(P)], np.int64)


def psroi_restate(data, rois, scale, output_dim, P, g=0, grad_out=None, grad_in0=None, batch_index_base=0, dtype=F32):
    """data [B, output_dim g g, H, W], rois [R, 5], grad_out [R, output_dim, P, P] or None.  Returns a dict:
    out, mapping [R, output_dim, P, P]; n, sabs: cell count and sum|x| / area of every output element (float64);
    with grad_out: grad_in [B, C, H, W], n_add (contributions per word) and sabs_in (sum |contribution|, the prior value included)."""
    g = P if g == 0 else g
    ft = dtype
    data = np.asarray(data)
    B, C, H, W = data.shape
    assert C == output_dim * g * g
    rois = np.asarray(rois, F32).reshape(-1, 5)
    R = rois.shape[0]
    dat = data.astype(ft)
    a64 = np.abs(data.astype(F64))
    grp = groups(P, g)
    ctop = np.arange(output_dim)
    out = np.zeros((R, output_dim, P, P), ft)
    mapping = np.zeros((R, output_dim, P, P), F32)
    n = np.zeros((R, output_dim, P, P), np.int64)
    sabs = np.zeros((R, output_dim, P, P), F64)
    for ph in range(P):
        for pw in range(P):
            mapping[:, :, ph, pw] = ((ctop * g + grp[ph]) * g + grp[pw])[None]
    bwd = grad_out is not None
    if bwd:
        go = np.asarray(grad_out).astype(ft)
        acc = np.zeros((B, C, H, W), ft)
        n_add = np.zeros((B, C, H, W), np.int64)
        sabs_in = np.zeros((B, C, H, W), F64)
    memo = {}
    for r in range(R):
        b = int(rois[r, 0]) - batch_index_base
        if b < 0 or b >= B:
            continue
        key = rois[r].tobytes()
        if key not in memo:
            hs, he, ws, we = edges(rois[r], scale, P, H, W)
            fw = np.zeros((output_dim, P, P), ft)
            fn = np.zeros((P, P), np.int64)
            fs = np.zeros((output_dim, P, P), F64)
            for ph in range(P):
                for pw in range(P):
                    nh, nw = he[ph] - hs[ph], we[pw] - ws[pw]
                    if nh <= 0 or nw <= 0:
                        continue
                    cs = (ctop * g + grp[ph]) * g + grp[pw]
                    win = dat[b][cs, hs[ph]:he[ph], ws[pw]:we[pw]].reshape(output_dim, -1)       # h ascending, then w ascending
                    s = np.zeros(output_dim, ft)
                    for k in range(win.shape[1]):
                        s = s + win[:, k]
                    fw[:, ph, pw] = s / ft(nh * nw)
                    fn[ph, pw] = nh * nw
                    fs[:, ph, pw] = a64[b][cs, hs[ph]:he[ph], ws[pw]:we[pw]].reshape(output_dim, -1).sum(1) / float(nh * nw)
            memo[key] = (hs, he, ws, we, fw, fn, fs)
        hs, he, ws, we, fw, fn, fs = memo[key]
        out[r], n[r], sabs[r] = fw, fn[None], fs
        if bwd:
            for ph in range(P):
                for pw in range(P):
                    nh, nw = he[ph] - hs[ph], we[pw] - ws[pw]
                    if nh <= 0 or nw <= 0:
                        continue
                    cs = (ctop * g + grp[ph]) * g + grp[pw]
                    v = go[r, :, ph, pw] / ft(nh * nw)
                    acc[b][cs, hs[ph]:he[ph], ws[pw]:we[pw]] += v[:, None, None]
                    n_add[b][cs, hs[ph]:he[ph], ws[pw]:we[pw]] += 1
                    sabs_in[b][cs, hs[ph]:he[ph], ws[pw]:we[pw]] += np.abs(v.astype(F64))[:, None, None]
    res = dict(out=out, mapping=mapping, n=n, sabs=sabs)
    if bwd:
        if grad_in0 is not None:
            g0 = np.asarray(grad_in0).astype(ft)
            acc = g0 + acc
            sabs_in = sabs_in + np.abs(g0.astype(F64))
        res.update(grad_in=acc, n_add=n_add, sabs_in=sabs_in)
    return res


def fwd_bound(ref64, bf16_out=False):
    b = ref64['n'] * 2.0 ** -23 * ref64['sabs']
    if bf16_out:
        b = b + 2.0 ** -8 * (np.abs(ref64['out']) + b)
    return b


def bwd_bound(ref64):
    return (ref64['n_add'] + 1) * 2.0 ** -23 * ref64['sabs_in']


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables
def make_rois(B, H, W, scale, R, seed, exact_P=0):
    """R roi rows over a B x H x W map at `scale`, several of them sharing pixels.  The first rows walk the kinds the kernels can get
    wrong: inside the map with coordinates at .5 (round(2.5) == 3), straddling each border, wholly outside, degenerate (x2 < x1), the
    second image, and batch indices -1 and B; the rest are random.  exact_P > 0: integer coordinates whose extent in cells is a multiple
    of exact_P, so every bin edge is an integer whatever the rounding of the multiply-add."""
    rng = np.random.RandomState(seed)
    iw, ih = W / scale, H / scale                    # image extent
    if exact_P:
        step = exact_P / scale
        rows = []
        for i in range(R):
            x1, y1 = np.floor(rng.uniform(-0.3, 0.8, 2) * [iw, ih])
            kx, ky = rng.randint(1, 3, 2)
            rows.append([i % B, x1, y1, x1 + kx * step - 1, y1 + ky * step - 1])
        if R > 2:
            rows[1][0], rows[2][0] = -1, B
        return np.array(rows, F32).reshape(R, 5)
    kinds = [
        [0, 0.5, 0.5, 0.6 * iw + 0.5, 0.7 * ih - 0.5],                # inside, halves
        [B - 1, -0.4 * iw, 0.2 * ih, 0.3 * iw, 0.6 * ih],             # straddles the left border, last image
        [-1, 0.1 * iw, 0.1 * ih, 0.8 * iw, 0.8 * ih],                 # batch index -1
        [0, 0.5 * iw, -0.5 * ih, 1.4 * iw, 0.4 * ih],                 # top and right borders
        [B, 0.1 * iw, 0.1 * ih, 0.8 * iw, 0.8 * ih],                  # batch index B
        [0, 0.2 * iw, 0.6 * ih, 0.7 * iw, 1.5 * ih],                  # bottom border
        [B - 1, 1.5 * iw, 1.2 * ih, 2.0 * iw, 2.0 * ih],              # wholly outside
        [0, 0.7 * iw, 0.3 * ih, 0.2 * iw, 0.1 * ih],                  # degenerate: x2 < x1, y2 < y1 (the 0.1 clamp)
        [B - 1, -2.5, -0.5, iw + 2.5, ih + 0.5],                      # covers the whole map, halves at negative coordinates
        [0, 0.3 * iw, 0.3 * ih, 0.3 * iw, 0.3 * ih],                  # one pixel wide: with P = 7 all bins land in the same cells
    ]
    rows = kinds[:R]
    while len(rows) < R:
        x1, x2 = np.sort(rng.uniform(-0.2, 1.2, 2)) * iw
        y1, y2 = np.sort(rng.uniform(-0.2, 1.2, 2)) * ih
        rows.append([rng.randint(0, B), np.round(x1 * 2) / 2, np.round(y1 * 2) / 2, np.round(x2 * 2) / 2, np.round(y2 * 2) / 2])
    return np.array(rows, F32).reshape(R, 5)


def make_case(name, output_dim, P, g, H, W, R, scale, seed, B=2, exact=False):
    rng = np.random.RandomState(seed)
    G = P if g == 0 else g
    C = output_dim * G * G
    # values on a 2^-6 grid in [-2, 2): exact in bf16, so one table serves the fp32 and the bf16 layouts
    data = (rng.randint(-128, 128, (B, C, H, W)) / 64.0).astype(F32)
    rois = make_rois(B, H, W, scale, R, seed + 1, exact_P=P if exact else 0)
    grad_out = (rng.randint(-128, 128, (R, output_dim, P, P)) / 64.0).astype(F32)
    grad_in0 = (rng.randint(-128, 128, (B, C, H, W)) / 64.0).astype(F32)
    return dict(name=name, output_dim=output_dim, P=P, g=g, B=B, C=C, H=H, W=W, R=R, scale=scale, data=data, rois=rois,
                grad_out=grad_out, grad_in0=grad_in0, exact=exact)


# (name, output_dim, P, g, H, W, R, scale, exact).  Every value of the grid appears: output_dim {1, 3}; (P, g) in {(1, 1), (3, 3), (7, 7),
# (7, 1), (3, 7), (7, 3)} -- P > g: several bins feed one channel, P < g: channels go unused and get exact zeros backward; maps 1 x 1,
# 5 x 7, 9 x 6; R in {0, 1, 5, 65}; one case more with output_dim 6.  g = 0 stands for g = P once.  Scales 0.3 / 0.0625 * 1.7: edges that round; `exact`: integer edges.
CASE_TABLE = [
    ('p1g1_1x1_r5', 1, 1, 1, 1, 1, 5, 0.5, False),
    ('p3g3_5x7_r65', 3, 3, 3, 5, 7, 65, 0.3, False),
    ('p7g7_9x6_r5', 1, 7, 7, 9, 6, 5, 0.10625, False),
    ('p7g0_5x7_r65', 1, 7, 0, 5, 7, 65, 0.0625, False),
    ('p7g1_9x6_r65', 3, 7, 1, 9, 6, 65, 0.3, False),
    ('p3g7_5x7_r5', 1, 3, 7, 5, 7, 5, 0.3, False),
    ('p7g3_9x6_r65', 3, 7, 3, 9, 6, 65, 0.10625, False),
    ('p7g3_1x1_r1', 1, 7, 3, 1, 1, 1, 0.3, False),
    ('p3g3_9x6_r0', 3, 3, 3, 9, 6, 0, 0.3, False),
    ('p3g7_9x6_r1', 3, 3, 7, 9, 6, 1, 0.0625, False),
    ('exact_p3g3_9x6_r5', 3, 3, 3, 9, 6, 5, 0.5, True),
    ('exact_p1g1_5x7_r65', 3, 1, 1, 5, 7, 65, 1.0, True),
    # beyond the grid: 6 x 49 = 294 channels, more than the 256 one backward workgroup owns, so a cell is shared by two of them
    ('p7g7_5x7_r5_c294', 6, 7, 7, 5, 7, 5, 0.3, False),
]
CASE_NAMES = [c[0] for c in CASE_TABLE]
_cases = {}


def case(name):
    """The case and its two references (float32 in the documented order, float64), computed once and shared: do not modify."""
    if name not in _cases:
        i = CASE_NAMES.index(name)
        _, od, P, g, H, W, R, scale, exact = CASE_TABLE[i]
        c = make_case(name, od, P, g, H, W, R, scale, 100 + 7 * i, exact=exact)
        for key, dt in (('ref32', F32), ('ref64', F64)):
            c[key] = psroi_restate(c['data'], c['rois'], scale, od, P, g, c['grad_out'], dtype=dt)
            c[key + '_acc'] = psroi_restate(c['data'], c['rois'], scale, od, P, g, c['grad_out'], c['grad_in0'], dtype=dt)
        _cases[name] = c
    return _cases[name]


def grid_fold_case():
    """R = 70 000 rois (more than a 65 535-wide grid.y would hold) with output_dim = g = P = 1 on a 2 x 2 map, one image: a 16-row pattern
    repeated, so the restatement's memo keeps the forward cheap; the backward is an ordered sum of up to 70 000 terms per word."""
    rng = np.random.RandomState(5)
    pattern = make_rois(1, 2, 2, 0.5, 16, 9)
    R = 70000
    rois = np.ascontiguousarray(pattern[np.arange(R) % 16])
    data = (rng.randint(-128, 128, (1, 1, 2, 2)) / 64.0).astype(F32)
    grad_out = (rng.randint(-128, 128, (R, 1, 1, 1)) / 64.0).astype(F32)
    return dict(output_dim=1, P=1, g=1, B=1, C=1, H=2, W=2, R=R, scale=0.5, data=data, rois=rois, grad_out=grad_out)


NEW_SYMBOLS = ('relnet_psroi_pool_fwd', 'relnet_psroi_pool_bwd')
