"""Shared by tests/test_grad_accum_cases_host.py and tests/test_gpu_grad_accum_edges.py: the edge cases of the DEFAULT (float-atomic) gradient
accumulation kernels of a training step -- wgrad_streamk_kernel (csrc/wgrad.hip), colsum_add_kernel / colsum_add_bf16x8_kernel /
colsum_add_grouped_kernel (csrc/train_ops.hip), roi_pool_bwd_kernel / roi_pool_bwd_owner_kernel (csrc/roi_pool.hip) -- and of
strided_scatter_kernel: case tables, seeded operand builders, one float64 reference per kernel written from its definition, the bound every GPU
result is held to, float32 emulations in two summation orders and the named mutants (the host file shows that a correct evaluation uses at most
half of each bound and that every mutant exceeds it).  Imports torch / numpy and tests/gemm_cases.py only (never the library), so it loads on a
machine without a GPU.

Reference.  float64 on exactly the bf16 / fp32 values the kernel reads (operands are kept as float32 tensors that hold the rounded values), and the
SAME routine on absolute values gives `mag`, the largest magnitude any partial sum of the element can reach.

Bound (derived as in gemm_cases, not measured).  bf16 x bf16 products are exact in fp32; an fp32 addition, rounded or truncated, errs by at most
2^-23 of its result, and every intermediate result is at most mag, so per element
    |got - ref| <= n_add * 2^-23 * mag
where n_add counts the additions (and other roundings) the kernel's STRUCTURE allows for that element, whatever the order the atomics arrive in:

  wgrad     dW[m][k] = old + s_m^2 sum_p dY[p][m] X[p][k].  A workgroup owns a run of consecutive 64-pixel slabs of a tile and adds their products
            to an MFMA accumulator that starts at 0: over the whole tile at most P additions (the zero rows that pad the last slab add exactly).
            Every share flushes once with one atomic addition into the word; a tile has `slabs` = ceil(P / 64) slabs, hence at most `slabs`
            shares: <= slabs additions, which also take in the old value.  Granting the old value an addition of its own (+ 1) and one rounding
            each to s * s and to s^2 * acc (+ 2; each at most 2^-24 of a term below mag) gives
                n_add = P + slabs + 3.
            mag = |old| + s^2 |dY|^T |X|, s the float32 factor.  Without a row factor the two last roundings do not happen; the formula is kept.
  colsum    out[c] = old + sum_r x[r][c].  Rows are cut into nchunk = min(128, ceil(rows / 512)) chunks of rpb = ceil(rows / nchunk) rows (the grid
            has ny = ceil(rows / rpb) <= nchunk of them); in a chunk each of L row lanes (L = 4: colsum_add_kernel, L = 8: the 16-byte kernels)
            adds ceil(rpb / L) values to 0, the L lane sums are added up, and every chunk issues one atomic addition:
                n_add = ceil(rpb / L) + L + nchunk + 1         (the + 1: the old value)
            mag = |old| + sum_r |x[r][c]|.
  roi       grad_in[b][c][cell] = sum over the (roi, bin) of image b whose argmax[.][c] is the cell of grad_out.  cnt contributions arrive as cnt
            atomic additions to a word that starts at 0 (global memory: scatter form; LDS: owner form); the owner form then flushes its LDS word
            with one more addition into the caller's zeros:
                n_add = cnt (+ 1 for the owner form)
            mag = sum |grad_out| of those contributions.  A cell nothing points to has bound 0: it must come out exactly 0.
Every element of every output is compared; nothing is masked or sampled.  strided_scatter only moves data: bit for bit.

Half of the bound.  The float32 emulations below (ascending, and slab- / chunk-wise as the kernels do it) use at most half of these bounds on
every case: rounding errors of random sign grow like the square root of n_add while the bound grows linearly, and the smallest cases (one or two
additions) are granted an addition more than they perform.  No family needs the exception of train_glue_cases (a formula that grants a rounding
exactly its worst case)."""
import zlib

import numpy as np
import torch

import gemm_cases as GC

F32, BF16, F64, I32 = torch.float32, torch.bfloat16, torch.float64, torch.int32
EPS = 2.0 ** -23
SLAB = 64                  # pixels per slab (kWgBP)
TILE_N = 256               # tile columns (kWgBN)
OWNER_LIST = 1024          # kOwnerList
OWNER_THREADS = 1024       # kOwnerThreads
OWNER_MAX_CELLS = 4608     # kOwnerMaxCells


def seed(id_):
    return zlib.crc32(id_.encode())


def gen(id_):
    return torch.Generator().manual_seed(seed(id_))


def _round(t, dtype):
    return t.to(dtype).to(F32)


def worst(got, want, tol):
    """Largest |got - want| / tol over ALL elements (0 / 0 = 0, any error against a zero tolerance or a non-finite result = inf)."""
    got, want, tol = got.double(), want.double(), tol.double()
    assert got.shape == want.shape == tol.shape, (got.shape, want.shape, tol.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - want).abs()
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float('inf')))
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# wgrad
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _w(id_, Cout, Cin, geom=None, P=None, ks=3, stride=1, dil=1, pad=None, scale=False, xpad=0, dypad=0, dyzero=0, holes=False):
    """geom = (B, Hin, Win): a convolution (ks, stride, dil, pad; pad defaults to dil for 3x3, 0 for 1x1); P: the plain [P, K = Cin] form.
    xpad: x is a channel slice of a parent with that many more channels (NaN); dypad: dy2d a column slice of a parent with that many more columns
    (NaN); dyzero: zero columns of dy2d behind the Cout real ones (the documented padding)."""
    d = dict(id=id_, Cout=Cout, Cin=Cin, conv=geom is not None, ks=ks, stride=stride, dil=dil, scale=scale, xpad=xpad, dypad=dypad, dyzero=dyzero,
             holes=holes)
    if geom is None:
        d.update(ks=1, stride=1, dil=1, pad=0, P=P, K=Cin, Wout=P)
    else:
        B, H, W = geom
        pad = (dil if ks == 3 else 0) if pad is None else pad
        Ho, Wo = (H + 2 * pad - dil * (ks - 1) - 1) // stride + 1, (W + 2 * pad - dil * (ks - 1) - 1) // stride + 1
        d.update(B=B, H=H, W=W, pad=pad, Hout=Ho, Wout=Wo, P=B * Ho * Wo, K=ks * ks * Cin)
    d['slabs'] = -(-d['P'] // SLAB)
    return d


WGRAD_CASES = [
    # Wout at / around the slab width: step_y = 1 step_x = 1 (63), step_y = 1 step_x = 0 (64), step_y = 0 (65, 125, 130)
    _w('W63', 72, 16, (1, 5, 63), scale=True),
    _w('W64', 8, 8, (2, 3, 64), dypad=16),
    _w('W65', 64, 16, (1, 3, 65), xpad=16),
    _w('W125', 136, 8, (1, 2, 125), scale=True),
    _w('W130', 8, 8, (1, 2, 130), xpad=16, dypad=16, dyzero=8),
    # maps so small that a slab crosses several images: the carry loop runs up to 64 times per slab
    _w('S9x3x5', 128, 16, (9, 3, 5), xpad=16),
    _w('S5x2x3', 72, 8, (5, 2, 3), scale=True, dyzero=8),
    _w('S70x1x1', 8, 8, (70, 1, 1), xpad=16, scale=True),
    _w('S3x1x9', 64, 16, (3, 1, 9)),
    # dilation 2: on the 2 x 3 map every tap but the centre row is outside the image
    _w('D2-2x2x3', 8, 8, (2, 2, 3), dil=2, xpad=16),
    _w('D2-2x14x17', 264, 16, (2, 14, 17), dil=2, scale=True),
    # 1x1 stride 2: the pixels stride 2 never reads hold the NaN pattern
    _w('H2-2x9x13', 256, 16, (2, 9, 13), ks=1, stride=2, holes=True),
    _w('H2-2x8x12', 72, 8, (2, 8, 12), ks=1, stride=2, holes=True, xpad=16, scale=True),
    # 7x7 stride 2 pad 3 (the stem's geometry): 49 taps over two tile columns
    _w('K7-1x11x70', 64, 8, (1, 11, 70), ks=7, stride=2, pad=3, xpad=16),
    # the plain form at every pixel count around one and two slabs, over the wave-tile heights and the tile-column widths
    _w('F1', 8, 8, P=1),
    _w('F63', 64, 72, P=63, scale=True),
    _w('F64', 72, 248, P=64, dypad=16),
    _w('F65', 128, 256, P=65, xpad=16),
    _w('F127', 136, 264, P=127, dypad=16, scale=True),
    _w('F128', 256, 8, P=128, dyzero=8),
    _w('F129', 264, 72, P=129, xpad=16, dypad=16),
    _w('F129k', 8, 264, P=129, scale=True),
]
WGRAD_BY_ID = {c['id']: c for c in WGRAD_CASES}
# layers of ONE grouped launch: the 8-row layers run on the 256-row tile the 264-row layer selects; the stream-K shares cut across layers
WGRAD_GROUPS = {'MIX': ('S70x1x1', 'F129', 'F1', 'W64')}
WGRAD_FEW_UNITS = 16                       # cases with at most that many units are flushed at every grid size of wgrad_grids
WGRAD_MUTANTS = {                          # mutant -> cases at which it must exceed the bound
    'last_pixel_dropped': ('W63', 'F65', 'F1', 'S5x2x3', 'K7-1x11x70'),
    'walk_row_off': ('W64', 'W65', 'W125', 'W130'),
    'border_clamped': ('W63', 'S70x1x1', 'D2-2x2x3', 'K7-1x11x70', 'S3x1x9'),
    'taps_transposed': ('W63', 'S9x3x5', 'D2-2x14x17', 'K7-1x11x70'),
    'scale_unsquared': ('W63', 'S70x1x1', 'F63', 'H2-2x8x12'),
}


def wgrad_tile_rows(cases):
    """Rows of the output tile a grouped launch of these layers runs on (64 WM: 128, or 256 when a layer has more than 128 rows)."""
    return 256 if max(c['Cout'] for c in cases) > 128 else 128


def wgrad_units(case, tile_rows=None):
    tile_rows = wgrad_tile_rows([case]) if tile_rows is None else tile_rows
    return -(-case['Cout'] // tile_rows) * -(-case['K'] // TILE_N) * case['slabs']


def wgrad_grids(units):
    return sorted({k for k in (1, 2, 3, 7, units - 1, units, units + 5) if k >= 1})


def share_cuts(units, grid):
    """Unit indices at which the stream-K shares of a `grid`-workgroup launch begin (csrc/wgrad.hip: u = units * block / grid)."""
    g = min(grid, units)
    return {units * i // g for i in range(1, g)}


def wgrad_operands(case):
    """-> dict of CPU float32 tensors holding exactly the values the kernel reads: 'x' [B, H, W, Cin] (NaN where case['holes'] and stride 2 never
    reads) or [P, K], 'dy' [P, Cout], 'scale' [Cout] | None, 'old' [Cout, K] (the accumulator's start value)."""
    g = gen(case['id'])
    if case['conv']:
        x = _round(torch.randn(case['B'], case['H'], case['W'], case['Cin'], generator=g), BF16)
        if case['holes']:
            assert case['ks'] == 1 and case['pad'] == 0
            s = case['stride']
            read = torch.zeros(case['H'], case['W'], dtype=torch.bool)
            read[::s, ::s] = True
            x[:, ~read] = float('nan')
    else:
        x = _round(torch.randn(case['P'], case['K'], generator=g), BF16)
    dy = _round(torch.randn(case['P'], case['Cout'], generator=g), BF16)
    scale = (torch.rand(case['Cout'], generator=g) + 0.5) if case['scale'] else None
    old = torch.randn(case['Cout'], case['K'], generator=g)
    return dict(x=x, dy=dy, scale=scale, old=old)


def wgrad_patches(case, x, mutant=None):
    """The implicit im2col matrix [P, K] (column (r ks + s) Cin + ic; an out-of-image tap is zero) by plain division of the pixel index; the
    plain form returns x.  Mutants: 'walk_row_off' (from pixel 64 on the walk is one output row further down), 'border_clamped' (an out-of-image
    tap reads the clamped border pixel), 'taps_transposed' (tap (r, s) reads what (s, r) should)."""
    if not case['conv']:
        return x
    H, W, Ho, Wo, ks, st, dil, pad = (case[k] for k in ('H', 'W', 'Hout', 'Wout', 'ks', 'stride', 'dil', 'pad'))
    p = torch.arange(case['P'])
    img, rem = p // (Ho * Wo), p % (Ho * Wo)
    y, xx = rem // Wo, rem % Wo
    if mutant == 'walk_row_off':
        assert Wo >= SLAB and case['P'] > SLAB
        y = y + (p >= SLAB).long()
    cols = []
    for r in range(ks):
        for s in range(ks):
            rr, ss = (s, r) if mutant == 'taps_transposed' else (r, s)
            sy, sx = y * st - pad + rr * dil, xx * st - pad + ss * dil
            ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
            if mutant == 'border_clamped':
                ok = torch.ones_like(ok)
            v = x[img, sy.clamp(0, H - 1), sx.clamp(0, W - 1)]
            cols.append(torch.where(ok[:, None], v, torch.zeros_like(v)))
    return torch.cat(cols, 1)


def wgrad_ref64(case, ops_, mutant=None):
    """-> (ref, mag) [Cout, K] float64: old + s^2 dY^T X and |old| + s^2 |dY|^T |X|."""
    X = wgrad_patches(case, ops_['x'].double(), mutant)
    dy = ops_['dy'].double()
    if mutant == 'last_pixel_dropped':
        assert case['P'] % SLAB != 0
        X, dy = X[:-1], dy[:-1]
    s2 = torch.ones(case['Cout'], dtype=F64) if ops_['scale'] is None else ops_['scale'].double() ** 2
    if mutant == 'scale_unsquared':
        s2 = ops_['scale'].double()
    old = ops_['old'].double()
    return old + s2[:, None] * (dy.t() @ X), old.abs() + s2[:, None] * (dy.abs().t() @ X.abs())


def wgrad_bound(case, mag):
    return (case['P'] + case['slabs'] + 3) * EPS * mag


def wgrad_emulate32(case, ops_, order):
    """float32 evaluation.  'ascending': all P products added to one accumulator in pixel order, one flush.  'slabs': an accumulator and a flush
    per 64-pixel slab (every slab a share of its own: the most flushes the stream-K cut allows)."""
    X = wgrad_patches(case, ops_['x'])
    dy = ops_['dy']
    s2 = None if ops_['scale'] is None else (ops_['scale'] * ops_['scale'])[:, None]
    out = ops_['old'].clone()
    acc = torch.zeros_like(out)
    P = case['P']
    for p in range(P):
        acc = acc + dy[p][:, None] * X[p][None, :]                       # the product is exact in float32
        if p == P - 1 or (order == 'slabs' and p % SLAB == SLAB - 1):
            out = out + (acc if s2 is None else s2 * acc)
            acc = torch.zeros_like(out)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------------------------------------------------------------------------
COLSUM_ROWS = (1, 7, 8, 9, 511, 512, 513, 1025, 65536, 65537)
COLSUM_COLS = (1, 7, 8, 63, 64, 65, 72, 256, 264)
# path -> (columns it can be reached with, kernel's row lanes).  'bf16x8': 8 | cols, 8 | ld, 16-byte aligned pointer (the 16-byte kernel);
# 'bf16w': aligned pointer and 8 | ld but a ragged width, 'bf16ld': ld % 8 != 0, 'bf16off': the pointer one element past a 16-byte boundary
# (all three: the scalar kernel).  Widths that are no multiple of 8 cannot reach the 16-byte kernel, widths that are cannot be 'ragged'.
COLSUM_PATHS = {
    'f32': (COLSUM_COLS, 4),
    'bf16x8': (tuple(c for c in COLSUM_COLS if c % 8 == 0), 8),
    'bf16w': (tuple(c for c in COLSUM_COLS if c % 8 != 0), 4),
    'bf16ld': (COLSUM_COLS, 4),
    'bf16off': (COLSUM_COLS, 4),
}


def _cs(path, rows, cols, wide):
    up8 = -(-cols // 8) * 8
    ld = {'f32': cols + (3 if wide else 0), 'bf16x8': cols + (8 if wide else 0), 'bf16w': up8 + (8 if wide else 0), 'bf16ld': up8 + 3,
          'bf16off': up8 + (8 if wide else 0)}[path]
    return dict(id='%s-%dx%d-ld%d' % (path, rows, cols, ld), path=path, rows=rows, cols=cols, ld=ld, dtype=F32 if path == 'f32' else BF16,
                lanes=COLSUM_PATHS[path][1], offset=1 if path == 'bf16off' else 0)


def _colsum_cases():
    cs = []
    for path, (cols, _) in COLSUM_PATHS.items():
        # every row count once per path; the column counts cycle (shifted by one, so that the two largest row counts meet the narrowest widths)
        for i, rows in enumerate(COLSUM_ROWS):
            cs.append(_cs(path, rows, cols[(i + 1) % len(cols)], wide=i % 2 == 0))
    # the 128-chunk cap with more than one column block
    cs += [_cs('f32', 65537, 65, True), _cs('bf16x8', 65537, 264, True), _cs('bf16x8', 65536, 256, False), _cs('bf16ld', 65537, 72, True)]
    return cs


COLSUM_CASES = _colsum_cases()
COLSUM_BY_ID = {c['id']: c for c in COLSUM_CASES}
# queues of the grouped kernel (bf16x8 operands; (rows, cols, ld - cols)): 1, 16 and 17 problems (two launches); the one-block (1, 8) problem lies
# between two multi-block ones, so the block -> problem lookup is crossed by a problem of a single block
_Q = [(1025, 264, 0), (1, 8, 0), (513, 72, 8), (7, 8, 8), (512, 64, 0), (9, 256, 0), (511, 8, 0), (8, 72, 8), (1025, 8, 0), (1, 8, 8), (513, 264, 8),
      (65537, 8, 0), (1, 264, 0), (65536, 64, 8), (8, 8, 0), (1025, 72, 0), (513, 256, 8)]
COLSUM_QUEUES = {'Q1': _Q[2:3], 'Q16': _Q[:16], 'Q17': _Q}
COLSUM_MUTANTS = {'chunk_last_row_dropped': ('f32-513x256-ld259', 'bf16x8-1x64-ld72', 'bf16ld-513x256-ld259', 'bf16off-9x64-ld64')}
COLSUM_QUEUE_MUTANTS = {'group_shifted': ('Q16', 'Q17')}


def colsum_plan(rows, lanes):
    """-> (nchunk, rows per chunk, chunks in the grid, n_add)."""
    nchunk = min(128, -(-rows // 512))
    rpb = -(-rows // nchunk)
    return nchunk, rpb, -(-rows // rpb), -(-rpb // lanes) + lanes + nchunk + 1


def colsum_operands(id_, rows, cols, dtype):
    """-> (x [rows, cols], old [cols]) CPU float32 holding the values the kernel reads."""
    g = gen('colsum-' + id_)
    return _round(torch.randn(rows, cols, generator=g), dtype), torch.randn(cols, generator=g)


def colsum_ref64(x, old, mutant=None, lanes=4):
    xd = x.double()
    if mutant == 'chunk_last_row_dropped':                         # the last row of the first chunk
        _, rpb, _, _ = colsum_plan(x.shape[0], lanes)
        keep = torch.ones(x.shape[0], dtype=torch.bool)
        keep[min(rpb, x.shape[0]) - 1] = False
        xd = xd[keep]
    return old.double() + xd.sum(0), old.double().abs() + xd.abs().sum(0)


def colsum_bound(rows, lanes, mag):
    return colsum_plan(rows, lanes)[3] * EPS * mag


def colsum_emulate32(x, old, lanes, order):
    """'ascending': the rows one by one onto the old value.  'chunks': the kernels' tree -- per chunk, `lanes` strided partial sums, the lane sums
    added from lane 0 up, one addition per chunk onto the old value in ascending chunk order."""
    xs = x.numpy().astype(np.float32)
    out = old.numpy().astype(np.float32).copy()
    rows, cols = xs.shape
    if order == 'ascending':
        for r in range(rows):
            out += xs[r]
        return torch.from_numpy(out)
    _, rpb, ny, _ = colsum_plan(rows, lanes)
    iters = -(-rpb // lanes)
    z = np.zeros((ny, iters * lanes, cols), np.float32)            # zero rows behind a ragged chunk add exactly
    for y in range(ny):
        r0, r1 = y * rpb, min((y + 1) * rpb, rows)
        z[y, :r1 - r0] = xs[r0:r1]
    z = z.reshape(ny, iters, lanes, cols)
    acc = np.zeros((ny, lanes, cols), np.float32)
    for i in range(iters):
        acc += z[:, i]
    t = np.zeros((ny, cols), np.float32)
    for k in range(lanes):
        t += acc[:, k]
    for y in range(ny):
        out += t[y]
    return torch.from_numpy(out)


def colsum_queue_operands(qid):
    return [colsum_operands('%s-%d' % (qid, i), r, c, BF16) for i, (r, c, _) in enumerate(COLSUM_QUEUES[qid])]


def colsum_queue_ref64(qid, operands, mutant=None):
    """-> [(ref, mag)] per problem.  'group_shifted': the second group of 8 columns of a problem (its first where it has one only) holds the sums
    of the NEXT problem's columns of that group, where that problem has them."""
    refs = [colsum_ref64(x, old) for x, old in operands]
    if mutant == 'group_shifted':
        shifted = []
        for i, (ref, mag) in enumerate(refs):
            ref = ref.clone()
            c0 = 8 if ref.numel() >= 16 else 0
            nx, nold = operands[(i + 1) % len(operands)]
            if nx.shape[1] >= c0 + 8 and len(operands) > 1:
                ref[c0:c0 + 8] = operands[i][1].double()[c0:c0 + 8] + nx.double()[:, c0:c0 + 8].sum(0)
            shifted.append((ref, mag))
        refs = shifted
    return refs


# ---------------------------------------------------------------------------------------------------------------------------------------------
# roi pooling backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _r(id_, B, C, hw, R, pooled, dtype, base=0, own=None, gap=False, hot=False, form='cl', levels=None):
    """hw = (H, W).  own: rois of image 0 (the rest is dealt to the other images at random); gap: image 0's rois avoid the list segment
    [1024, 2048); hot: every bin of image 0's rois points at ONE cell in every channel (the contended case).  form: 'cl' = relnet_roi_pool_bwd_cl
    (owner form where it applies, scatter form under relnet_roi_pool_bwd_debug(1)), 'nchw' / 'nhwc' = relnet_roi_pool_bwd_ex with those gradient
    strides, 'fpn' = relnet_roi_pool_fpn_bwd_ex over `levels` = [(H, W)]."""
    levels = [tuple(hw)] if levels is None else [tuple(l) for l in levels]
    return dict(id=id_, B=B, C=C, R=R, PH=pooled[0], PW=pooled[1], dtype=dtype, base=base, own=own, gap=gap, hot=hot, form=form, levels=levels,
                owner=form == 'cl' and B * C // 8 >= 256 and C % 8 == 0 and levels[0][0] * levels[0][1] <= OWNER_MAX_CELLS)


ROI_CASES = [
    # list segments of 1024 rois: R at and around one and two segments; R2049g: image 0 has rois in segments 0 and 2 and none in segment 1
    _r('R1023', 256, 8, (3, 4), 1023, (2, 2), F32),
    _r('R1024', 256, 8, (3, 4), 1024, (2, 2), BF16, base=3),
    _r('R1025', 256, 8, (3, 4), 1025, (2, 2), F32, hot=True),
    _r('R2049g', 256, 8, (3, 4), 2049, (2, 2), BF16, own=300, gap=True),
    # the pair loop: np = n bins (roi, bin) pairs of one image in one segment at 1024, 1028, 2048, 2052 (2 x 2 bins) and 980, 1029, 2058 (7 x 7)
    _r('P256', 256, 8, (3, 4), 1100, (2, 2), F32, own=256),
    _r('P257', 256, 8, (3, 4), 1100, (2, 2), BF16, own=257, hot=True),
    _r('P512', 256, 8, (3, 4), 1100, (2, 2), BF16, own=512, base=3),
    _r('P513', 256, 8, (3, 4), 1100, (2, 2), F32, own=513),
    _r('P20', 29, 72, (4, 5), 60, (7, 7), BF16, own=20),                  # 9 channel groups: no XCD permutation
    _r('P21', 29, 72, (4, 5), 60, (7, 7), F32, own=21, base=3),
    _r('P42', 8, 256, (5, 3), 70, (7, 7), BF16, own=42, hot=True),        # 32 channel groups: permuted
    # the largest map the owner form takes, and one cell more (falls back to the scatter kernel)
    _r('M4608', 256, 8, (64, 72), 300, (2, 2), BF16, own=40),
    _r('M4609', 256, 8, (11, 419), 300, (2, 2), F32, own=40),
    # scatter form only
    _r('X-cl-small', 2, 16, (5, 7), 33, (3, 3), BF16, hot=True),          # B C / 8 < 256: the channels-last entry keeps the scatter kernel
    _r('X-nchw', 2, 5, (5, 7), 33, (3, 3), F32, form='nchw', hot=True),
    _r('X-nchw-300', 3, 300, (2, 3), 9, (2, 2), BF16, form='nchw', base=3),     # more channels than threads
    _r('X-nhwc', 2, 24, (5, 7), 33, (3, 3), BF16, form='nhwc', hot=True),
    _r('X-nhwc-300', 3, 300, (2, 3), 9, (2, 2), F32, form='nhwc'),
    _r('X-fpn2', 2, 16, None, 40, (3, 3), BF16, form='fpn', levels=[(6, 7), (3, 4)], hot=True),
    _r('X-fpn4', 2, 8, None, 64, (2, 2), F32, form='fpn', levels=[(9, 10), (5, 5), (3, 2), (1, 1)], base=3),
]
ROI_BY_ID = {c['id']: c for c in ROI_CASES}
ROI_MUTANTS = {
    'segment_dropped': ('R1025', 'R2049g', 'P513'),
    'tail_pair_dropped': ('P256', 'P257', 'P513', 'P20', 'P21', 'P42'),
    'bin_twice': ('R1023', 'P512', 'X-nchw', 'X-fpn4'),
}


def roi_operands(case):
    """-> dict: 'rois' [R, 5] float32 (column 0 = image + batch_index_base; the box is not read by the backward), 'level' [R] int32 | None,
    'argmax' [R, PH, PW, C] int32 in [-1, cells of the roi's level), 'gout' [R, PH, PW, C] float32 holding values of the case's dtype.
    Synthesised, not produced by a forward: some rois have no valid bin at all (all -1), image 0's are contended where case['hot']."""
    g = gen('roi-' + case['id'])
    B, C, R, PH, PW = case['B'], case['C'], case['R'], case['PH'], case['PW']
    img = torch.randint(0, B, (R,), generator=g)
    if case['own'] is not None:
        img = torch.randint(1, B, (R,), generator=g)
        cand = torch.arange(R)
        if case['gap']:
            cand = cand[(cand < OWNER_LIST) | (cand >= 2 * OWNER_LIST)]
            assert R > 2 * OWNER_LIST
        elif R > OWNER_LIST:
            cand = cand[cand < OWNER_LIST]                      # all of image 0's rois in ONE list segment: np = own * bins
        pick = cand[torch.randperm(cand.numel(), generator=g)[:case['own']]]
        if case['gap']:
            pick[0] = R - 1                                     # at least one behind the empty segment
        img[pick] = 0
    nl = len(case['levels'])
    level = torch.randint(0, nl, (R,), generator=g).to(I32) if case['form'] == 'fpn' else None
    cells = torch.tensor([h * w for h, w in case['levels']])[level.long() if level is not None else torch.zeros(R, dtype=torch.long)]     # [R]
    u = torch.rand(R, PH, PW, C, generator=g)
    argmax = (u * (cells[:, None, None, None] + 1).float()).floor().long() - 1                      # uniform in [-1, cells)
    argmax = torch.minimum(argmax, (cells - 1)[:, None, None, None])
    if case['hot']:
        hot = (cells - 1).clamp_max(5)
        sel = img == 0
        argmax[sel] = hot[sel][:, None, None, None].expand(-1, PH, PW, C)
    argmax[torch.arange(R) % 11 == 7] = -1                      # rois without a single valid bin
    rois = torch.rand(R, 5, generator=g) * 100
    rois[:, 0] = (img + case['base']).float()
    gout = _round(torch.randn(R, PH, PW, C, generator=g), case['dtype'])
    return dict(rois=rois, level=level, argmax=argmax.to(I32), gout=gout)


def owner_tail_mask(n_pairs):
    """Pairs p of a list segment with n_pairs (roi, bin) pairs that the owner kernel handles in its odd tail: thread t walks p = t, t + 2 NT, ...
    two at a time (p, p + NT) while p + NT < np; what is left (p < np <= p + NT) is the tail."""
    p = torch.arange(n_pairs)
    return ((p // OWNER_THREADS) % 2 == 0) & (p + OWNER_THREADS >= n_pairs)


def roi_weights(case, ops_, mutant):
    """[R, PH PW] multiplicity of every (roi, bin): 1, or what the mutant makes of it."""
    R, bins = case['R'], case['PH'] * case['PW']
    w = torch.ones(R, bins, dtype=F64)
    if mutant == 'segment_dropped':
        assert R > OWNER_LIST
        w[OWNER_LIST:2 * OWNER_LIST] = 0
    elif mutant == 'tail_pair_dropped':                         # per image and list segment, the list in ascending roi order
        img = ops_['rois'][:, 0].long() - case['base']
        for base in range(0, R, OWNER_LIST):
            seg = torch.arange(base, min(base + OWNER_LIST, R))
            for b in img[seg].unique().tolist():
                mine = seg[img[seg] == b]
                tail = owner_tail_mask(mine.numel() * bins).view(mine.numel(), bins)
                w[mine] = torch.where(tail, torch.zeros_like(w[mine]), w[mine])
    elif mutant == 'bin_twice':
        r = int((ops_['argmax'].reshape(R, -1) >= 0).any(1).nonzero()[0])
        w[r, 0] = 2
    else:
        assert mutant is None, mutant
    return w


def _roi_scatter(case, ops_, values, dtype, order=None):
    """Per level: [B, C, cells] of `dtype`, the contributions added one by one in `order` (a permutation of the flat (roi, bin, channel) index; None:
    float64 index_add).  values [R, bins, C]."""
    B, C, R = case['B'], case['C'], case['R']
    bins = case['PH'] * case['PW']
    a = ops_['argmax'].reshape(R, bins, C).long()
    img = (ops_['rois'][:, 0].long() - case['base'])[:, None, None].expand(R, bins, C)
    ch = torch.arange(C)[None, None, :].expand(R, bins, C)
    outs = []
    for l, (h, w) in enumerate(case['levels']):
        cells = h * w
        ok = a >= 0
        if ops_['level'] is not None:
            ok = ok & (ops_['level'].long() == l)[:, None, None]
        assert bool((a[ok] < cells).all()) and bool(((img[ok] >= 0) & (img[ok] < B)).all())
        idx = ((img * C + ch) * cells + a)[ok]
        v = values[ok]
        if order is None:
            out = torch.zeros(B * C * cells, dtype=dtype).index_add_(0, idx, v.to(dtype))
        else:
            perm = order(idx.numel())
            o = np.zeros(B * C * cells, np.float32)
            np.add.at(o, idx.numpy()[perm], v.numpy().astype(np.float32)[perm])          # unbuffered: one float32 addition after the other
            out = torch.from_numpy(o)
        outs.append(out.view(B, C, cells))
    return outs


def roi_ref64(case, ops_, mutant=None):
    """-> per level (ref, mag, cnt) [B, C, cells]: grad_in[b, c, argmax] += grad_out in float64, the same on magnitudes, and the number of
    contributions of every element."""
    w = roi_weights(case, ops_, mutant)[:, :, None]
    g = ops_['gout'].reshape(case['R'], -1, case['C']).double()
    ref = _roi_scatter(case, ops_, g * w, F64)
    mag = _roi_scatter(case, ops_, g.abs() * w, F64)
    cnt = _roi_scatter(case, ops_, torch.ones_like(g), F64)
    return list(zip(ref, mag, cnt))


def roi_bound(mag, cnt, owner):
    return (cnt + (1 if owner else 0)) * EPS * mag


def roi_emulate32(case, ops_, order):
    """float32, the contributions one by one: 'ascending' flat (roi, bin, channel) order, 'strided' the order of a 1024-thread walk (pair p taken
    by thread p % 1024: all first pairs of the threads, then all second ones ... read backwards, so that it differs from ascending everywhere)."""
    g = ops_['gout'].reshape(case['R'], -1, case['C'])
    if order == 'ascending':
        perm = lambda n: np.arange(n)
    else:
        perm = lambda n: np.lexsort((np.arange(n), np.arange(n) % OWNER_THREADS))[::-1].copy()
    return _roi_scatter(case, ops_, g, F32, order=perm)


def roi_to_layout(t, channels_last):
    """[R, PH, PW, C] -> the logical [R, C, PH, PW] tensor the wrappers take, in channels-last or dense memory."""
    v = t.permute(0, 3, 1, 2)
    return v if channels_last else v.contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# strided scatter
# ---------------------------------------------------------------------------------------------------------------------------------------------
SCATTER_CASES = [dict(id='%s-%dx%dx%dx%d-s%d%s' % ('bf16' if dt == BF16 else 'f32', B, H, W, C, s, '-mask' if m else ''), B=B, H=H, W=W, C=C, stride=s,
                      dtype=dt, mask=m)
                 for (B, H, W, C, s, dt) in ((1, 1, 1, 8, 2, BF16), (2, 1, 7, 8, 2, BF16), (2, 6, 1, 8, 2, BF16), (2, 7, 7, 8, 2, BF16), (1, 4, 6, 8, 2, BF16),
                                             (3, 3, 3, 8, 1, BF16), (2, 1, 4, 4, 2, F32), (1, 5, 1, 4, 2, F32), (3, 4, 5, 4, 2, F32), (1, 7, 8, 4, 3, F32),
                                             (1, 35, 41, 16, 2, BF16))
                 for m in (False, True)]


def scatter_operands(case):
    """-> (low [B, Ho, Wo, C], mask [B, H, W, C] | None) of the case's dtype.  The mask holds -0.0, +0.0, NaN and negative values next to positive
    ones; low holds -0.0 and a NaN too (the kernel moves bits)."""
    g = gen('scatter-' + case['id'])
    B, H, W, C, s = (case[k] for k in ('B', 'H', 'W', 'C', 'stride'))
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    low = torch.randn(B, Ho, Wo, C, generator=g)
    low.view(-1)[::5] = -0.0
    low.view(-1)[3::17] = float('nan')
    mask = None
    if case['mask']:
        mask = torch.randn(B, H, W, C, generator=g)
        mf = mask.view(-1)
        mf[::4] = -0.0
        mf[1::8] = 0.0
        mf[2::16] = float('nan')
        mask = mask.to(case['dtype'])
    return low.to(case['dtype']), mask


def scatter_ref(case, low, mask):
    """The definition: zeros, out[:, ::s, ::s] = low, and +0 wherever NOT (mask > 0)."""
    s = case['stride']
    out = torch.zeros(case['B'], case['H'], case['W'], case['C'], dtype=low.dtype, device=low.device)
    out[:, ::s, ::s] = low
    if mask is not None:
        out = torch.where(mask > 0, out, torch.zeros_like(out))
    return out


def bits(t):
    return t.contiguous().view(GC.INT_VIEW[t.element_size()])
