"""Shared by tests/test_gemm_cases_host.py and tests/test_gpu_gemm_edges.py: the small / ragged / strided GEMM and convolution cases of
csrc/gemm.hip, their float64 reference, the error bound the GPU results are held to, and guarded device buffers.  Imports torch only (never
the library), so it loads on a machine without a GPU.

Reference.  `ref64` evaluates the definition in float64 on the bf16-rounded operands (bias / shortcut in the precision the kernel reads) and,
by the SAME routine on absolute values, mag = |A| |W|^T + |bias| + |resid|.

Bound (derived, not measured).  bf16 x bf16 products are exact in fp32 (8 + 8 significand bits).  A kernel adds the K_total products, the bias and
the shortcut in SOME order of at most K_total + 2 fp32 additions; each addition, rounded or truncated, errs by at most 2^-23 of its result, and
every intermediate result is at most mag in magnitude (to first order), so
    |got - ref| <= (K_total + 2) * 2^-23 * mag                      per element, fp32 outputs
    |got - ref| <= that + 0.5 * step(ref), step(t) = max(|t|, 2^-126) * 2^-7     bf16 outputs (one rounding to 8 significand bits)
fp32-operand kernels (exact-fp32 MFMA = an fmaf chain) use the same formula.  ReLU and masks are applied to the reference; ReLU is 1-Lipschitz so
the same bound holds behind it, and an element whose pre-activation lies within the bound of 0 may come out on either side: it is accepted when
0 <= got <= |pre| + bound (+ its bf16 rounding)."""
import math
import zlib

import torch

BF16, F32 = torch.bfloat16, torch.float32
GUARD_BYTES = 1 << 20                      # least guard on both sides of every guarded operand
TILE_ROWS = 256                            # tallest tile of csrc/gemm.hip: the guard also holds that many rows of the operand's parent
_PATTERN = {2: 0x7FC1, 4: 0x7FC00001}      # quiet NaN of bf16 / fp32 with a payload no arithmetic produces
_INT = {2: torch.int16, 4: torch.int32}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _g(id_, M, N, K, **kw):
    d = dict(id=id_, kind='gemm', M=M, N=N, K=K, batch=1, a_batched=False, w_batched=False, bias=0, resid=False, relu=False, ldc=None,
             zero_out=False, a_parent=None, a_index=None, w_parent=None, w_index=None, odts=(BF16, F32), splitk=(), knobs=False)
    d.update(kw)
    return d


_S = slice
GEMM_CASES = [
    _g('G1', 1, 8, 64),                                                              # one row, one slab
    _g('G2', 31, 72, 64, bias=1),
    _g('G3', 33, 89, 192, bias=1, relu=True),                                        # ldc = 89: scalar stores; 3 slabs
    _g('G4', 65, 89, 192, ldc=96, resid=True, relu=True),                            # vector stores, ragged last vector, residual prefetch
    _g('G5', 257, 300, 320, ldc=320, zero_out=True, bias=1),                         # pad columns 300..319 stay exactly 0; 5 slabs
] + [
    _g('G6-%dx%d' % (M, K), M, 256, K, resid=True, relu=True, odts=(BF16,))          # row-panel tiles 13 - 15 below one panel
    for M in (64, 70) for K in (64, 128, 256, 512)
] + [
    _g('G7', 300, 1024, 1088, bias=1, relu=True, splitk=(2, 3, 5, 8)),               # 17 slabs
    _g('G8', 70, 136, 128, bias=2),
    _g('G8p', 70, 256, 128, bias=2),                                                 # a per-row bias on a shape the row-panel tiles would take
    _g('G9a', 45, 72, 128, batch=3, a_batched=True, bias=1),
    _g('G9b', 96, 37, 128, batch=3, w_batched=True, ldc=64, zero_out=True,           # broadcast A, W = f[:, :37, :]: the call of the relation module
       w_parent=(3, 50, 128), w_index=(_S(None), _S(0, 37), _S(None))),
    _g('G9c', 45, 72, 128, batch=3, a_batched=True, w_batched=True, resid=True, bias=2),
    _g('G10', 65, 72, 128, a_parent=(65, 256), a_index=(_S(None), _S(64, 192)), w_parent=(72, 256), w_index=(_S(None), _S(64, 192))),
    _g('G11', 1031, 1032, 128, ldc=1040, bias=1, resid=True, relu=True, knobs=True),  # >= 16 tiles: the swizzle x n_loop variants
]

GEMM_F32_CASES = [dict(id='F%dx%dx%d-b%d' % (M, N, K, b), kind='gemm', M=M, N=N, K=K, batch=b, a_batched=b > 1, w_batched=b > 1, bias=1, resid=True,
                       relu=True, ldc=None, zero_out=False, a_parent=None, a_index=None, w_parent=None, w_index=None, odts=(BF16, F32), splitk=(),
                       knobs=False, f32_in=True)
                  for (M, N, K) in ((1, 5, 16), (33, 128, 48), (129, 131, 80)) for b in (1, 2)]

MASK_TILES = (0, 1, 3, 4, 5, 22)
GEMM_MASK_CASES = [dict(id='K%dx%dx%d%s' % (M, N, K, '-res' if r else ''), kind='gemm', M=M, N=N, K=K, batch=1, a_batched=False, w_batched=False, bias=0,
                        resid=r, relu=False, mask=True, ldc=None, zero_out=False, a_parent=None, a_index=None, w_parent=None, w_index=None,
                        odts=(BF16,), splitk=(), knobs=False)
                   for (M, N, K) in ((1, 72, 64), (33, 264, 192), (257, 72, 192)) for r in (False, True)]


def _c(id_, B, H, W, Cin, Cout, R=3, S=3, stride=1, pad=1, dil=1, **kw):
    d = dict(id=id_, kind='conv', B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=S, stride=stride, pad=pad, dil=dil, relu=False, resid=False,
             wfrag=False, views=False, holes=False, abi=False, odts=(BF16, F32), splitk=())
    d.update(kw)
    d['Hout'] = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    d['Wout'] = (W + 2 * pad - dil * (S - 1) - 1) // stride + 1
    d['M'], d['N'], d['K'] = B * d['Hout'] * d['Wout'], Cout, R * S * Cin
    return d


CONV_CASES = [
    _c('C1', 7, 3, 5, 64, 64, relu=True),                                  # five to seventeen 15-pixel images per tile: carries, per-row masks
    _c('C2', 5, 1, 1, 64, 72),                                             # only the centre tap is in bounds; ragged N
    _c('C3', 3, 1, 9, 128, 256),                                           # one filter row; two channel chunks
    _c('C4', 2, 13, 16, 128, 256, pad=2, dil=2, relu=True),                # the P6 map; the window schedule with dilation 2 (324 <= 384 rows)
    _c('C5-9x13', 3, 9, 13, 64, 128, stride=2),
    _c('C5-8x12', 3, 8, 12, 64, 128, stride=2),
    _c('C6-8x12', 2, 8, 12, 128, 64, R=1, S=1, stride=2, pad=0, holes=True),   # the pixels stride 2 never reads hold the NaN pattern
    _c('C6-9x13', 2, 9, 13, 128, 64, R=1, S=1, stride=2, pad=0, holes=True),
    _c('C7-p0', 2, 6, 7, 64, 64, pad=0),                                   # 4 x 5 out
    _c('C7-p2', 2, 6, 7, 64, 64, pad=2),                                   # 8 x 9 out: the outer ring sees only padding
    _c('C8-1x3', 2, 4, 6, 64, 72, R=1, S=3, abi=True),                     # R != S through the C ABI
    _c('C8-3x1', 2, 4, 6, 64, 72, R=3, S=1, abi=True),
] + [
    _c('C9-b%d-k%d' % (B, Cin), B, 5, 7, Cin, 256, R=1, S=1, pad=0, resid=True, relu=True, wfrag=True)    # panel tiles 13 - 15 at 35 / 105 rows
    for B in (1, 3) for Cin in (64, 128, 256, 512)
] + [
    _c('C10-C1', 7, 3, 5, 64, 64, relu=True, resid=True, views=True),      # in_pix > Cin, in_img > H W in_pix, ldc > Cout
    _c('C10-C4', 2, 13, 16, 128, 256, pad=2, dil=2, relu=True, resid=True, views=True),
    _c('C11', 1, 5, 7, 256, 256, resid=True, relu=True, splitk=(2, 3, 8)),                        # split-K epilogue on a ragged single tile
]

CONV_F32_CASES = [dict(_c('%s-c%d-r%d' % (base['id'].replace('C', 'D', 1), cin, relu), base['B'], base['H'], base['W'], cin, base['Cout'], R=base['R'],
                          S=base['S'], stride=base['stride'], pad=base['pad'], dil=base['dil'], relu=relu, resid=relu != 1, odts=(F32,), abi=True),
                       f32_in=True)
                  for base in CONV_CASES if base['id'].split('-')[0] in ('C1', 'C2', 'C5', 'C8') for cin in (16, 48) for relu in (0, 1, 2)]

ALL_CASES = GEMM_CASES + GEMM_F32_CASES + GEMM_MASK_CASES + CONV_CASES + CONV_F32_CASES


def seed(case):
    return zlib.crc32(case['id'].encode())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# operands (CPU): A randn rounded to bf16, W randn / sqrt(K_total) rounded to bf16, bias / resid randn (resid rounded to the output dtype)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _round(t, dtype):
    return t.to(dtype).to(torch.float32)


def operands(case):
    """-> dict of CPU float32 tensors holding exactly the values the kernel reads: 'a' ([batch,] M, K or B, H, W, Cin), 'w' ([batch,] N, K; for a
    convolution the packed [Cout, R S Cin] with k = (r S + s) Cin + ic), 'bias' | None, 'resid32' | None (unrounded), 'mask' | None."""
    g = torch.Generator().manual_seed(seed(case))
    indt = F32 if case.get('f32_in') else BF16
    K = case['K']
    if case['kind'] == 'gemm':
        ashape = ((case['batch'],) if case['a_batched'] else ()) + (case['M'], K)
        wshape = ((case['batch'],) if case['w_batched'] else ()) + (case['N'], K)
        oshape = ((case['batch'],) if case['batch'] > 1 else ()) + (case['M'], case['N'])
        nb = {0: 0, 1: case['N'], 2: case['M']}[case['bias']]
    else:
        ashape = (case['B'], case['H'], case['W'], case['Cin'])
        wshape = (case['Cout'], K)
        oshape = (case['B'], case['Hout'], case['Wout'], case['Cout'])
        nb = case['Cout']
    d = {'a': _round(torch.randn(ashape, generator=g), indt), 'w': _round(torch.randn(wshape, generator=g) / math.sqrt(K), indt)}
    d['bias'] = torch.randn(nb, generator=g) if nb else None
    d['resid32'] = torch.randn(oshape, generator=g) if case['resid'] else None
    d['mask'] = _round(torch.randn(oshape, generator=g), BF16) if case.get('mask') else None
    d['oshape'] = oshape
    return d


def resid_for(ops_, odt):
    return None if ops_['resid32'] is None else _round(ops_['resid32'], odt)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float64 reference from the definition
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _conv_loops64(x, w, case, tap_row_shift=None, ignore_image_boundary=False):
    """Explicit loop definition (cross-correlation, NHWC input, packed weights), all outputs.  x [B,H,W,Cin] float64, w [Cout, R S Cin] float64.
    The two keyword arguments are the MUTATIONS of the host test: tap_row_shift = (r, s): that tap reads the pixels one row further down;
    ignore_image_boundary: a tap above / below the image reads the flattened pixel axis (the neighbouring image) instead of zero."""
    B, H, W, Cin = x.shape
    R, S, st, pad, dil = case['R'], case['S'], case['stride'], case['pad'], case['dil']
    Ho, Wo, Cout = case['Hout'], case['Wout'], case['Cout']
    flat = x.reshape(B * H * W, Cin)
    out = torch.zeros(B, Ho, Wo, Cout, dtype=torch.float64)
    for r in range(R):
        for s in range(S):
            wt = w[:, (r * S + s) * Cin:(r * S + s + 1) * Cin]                   # [Cout, Cin]
            for oy in range(Ho):
                iy = oy * st - pad + r * dil + (1 if tap_row_shift == (r, s) else 0)
                for ox in range(Wo):
                    ix = ox * st - pad + s * dil
                    if ix < 0 or ix >= W:
                        continue
                    if 0 <= iy < H:
                        out[:, oy, ox] += x[:, iy, ix] @ wt.t()
                    elif ignore_image_boundary:
                        for b in range(B):
                            p = (b * H + iy) * W + ix
                            if 0 <= p < B * H * W:
                                out[b, oy, ox] += wt @ flat[p]
    return out


def im2col(case, a):
    """[B,H,W,Cin] -> the implicit GEMM's A matrix [M, R S Cin] (k = (r S + s) Cin + ic, zeros for padded taps); a GEMM operand is returned as is."""
    if case['kind'] != 'conv':
        return a
    B, H, W, Cin = a.shape
    R, S, st, pad, dil = case['R'], case['S'], case['stride'], case['pad'], case['dil']
    Ho, Wo = case['Hout'], case['Wout']
    col = torch.zeros(B, Ho, Wo, R * S, Cin, dtype=a.dtype)
    for r in range(R):
        for s in range(S):
            for oy in range(Ho):
                iy = oy * st - pad + r * dil
                if iy < 0 or iy >= H:
                    continue
                for ox in range(Wo):
                    ix = ox * st - pad + s * dil
                    if 0 <= ix < W:
                        col[:, oy, ox, r * S + s] = a[:, iy, ix]
    return col.reshape(B * Ho * Wo, R * S * Cin)


def _linear64(a, w, bias, resid, case, **mut):
    """A W^T (+ bias) (+ resid) in float64; for a convolution the loop definition."""
    if case['kind'] == 'conv':
        y = _conv_loops64(a, w, case, **mut)
    else:
        y = a @ w.transpose(-1, -2)
        if case['batch'] > 1 and y.dim() == 2:
            y = y.expand(case['batch'], -1, -1).clone()
    if bias is not None:
        y = y + (bias[:, None] if (case['kind'] == 'gemm' and case['bias'] == 2) else bias)
    if resid is not None:
        y = y + resid
    return y


def ref64(case, ops_, odt, **mut):
    """-> (pre, mag): pre-activation reference and its magnitude bound, float64, shape of the output."""
    res_sum = resid_for(ops_, odt) if case['relu'] != 2 else None            # (relu == 2: resid is a ReLU mask, not a summand)
    dbl = lambda t: None if t is None else t.double()
    pre = _linear64(dbl(ops_['a']), dbl(ops_['w']), dbl(ops_['bias']), dbl(res_sum), case, **mut)
    ab = lambda t: None if t is None else t.double().abs()
    mag = _linear64(ab(ops_['a']), ab(ops_['w']), ab(ops_['bias']), ab(res_sum), case)
    return pre, mag


def activate(case, ops_, odt, pre):
    """ReLU / mask of the case applied to a pre-activation tensor (float64)."""
    if case.get('mask'):
        return torch.where(ops_['mask'].to(pre.device) > 0, pre, torch.zeros_like(pre))
    if case['relu'] == 2:
        return torch.where(resid_for(ops_, odt).to(pre.device) > 0, pre, torch.zeros_like(pre))
    return pre.clamp_min(0) if case['relu'] else pre


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bound and acceptance
# ---------------------------------------------------------------------------------------------------------------------------------------------
def bound(mag, k_total):
    return (k_total + 2) * 2.0 ** -23 * mag


def step(t):
    return t.abs().clamp_min(2.0 ** -126) * 2.0 ** -7


def accept(got, want, pre, mag, k_total, bf16_out, relu=False):
    """got: the kernel's output (any float dtype), want = activate(pre): float64.  -> (ok, worst): every element within its tolerance, and the
    largest |got - want| / tolerance (for fp32 outputs the tolerance IS the bound, so worst = err / bound)."""
    good, ratio = accept_map(got, want, pre, mag, k_total, bf16_out, relu)
    return bool(good.all()), float(ratio.max())


def accept_map(got, want, pre, mag, k_total, bf16_out, relu=False):
    """Per element: (accepted, |got - want| / tolerance)."""
    got = got.double()
    bnd = bound(mag, k_total)
    tol = bnd + (0.5 * step(want) if bf16_out else 0)
    err = (got - want).abs()
    good = err <= tol
    if relu is True or relu == 1:                      # pre-activation within the bound of 0: either side
        hi = pre.abs() + bnd
        near = (pre.abs() <= bnd) & (got >= 0) & (got <= hi + (0.5 * step(hi) if bf16_out else 0))
        good = good | near
    good = good & torch.isfinite(got)
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float('inf')))
    return good, ratio


# ---------------------------------------------------------------------------------------------------------------------------------------------
# guarded buffers
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Guarded(object):
    """buf: the flat allocation (pattern everywhere the view does not cover), parent: the dense tensor the view is cut from, view: the operand."""
    def __init__(self, buf, parent, view):
        self.buf, self.parent, self.view = buf, parent, view


def _fill_pattern(buf):
    buf.view(_INT[buf.element_size()]).fill_(_PATTERN[buf.element_size()])


fill_pattern = _fill_pattern            # public names for the other edge-case modules (tests/relation_edge_cases.py)
INT_VIEW = _INT


def guarded(shape, dtype, parent=None, index=None, device='cuda'):
    """One flat buffer filled with a fixed quiet-NaN bit pattern; the operand is `parent_tensor[index]` (default: the dense tensor of `shape`) in the
    middle of it, with max(1 MiB, 256 rows of the parent) of pattern on both sides (256-byte aligned start).  Every element of the parent the view
    does not cover keeps the pattern too.  A read from outside the operand turns outputs into NaN; a store outside it is found by guards_intact; an
    access that is off by up to a 256-row tile lands in memory the test owns."""
    parent = tuple(shape) if parent is None else tuple(parent)
    es = torch.empty((), dtype=dtype).element_size()
    guard = -(-max(GUARD_BYTES // es, TILE_ROWS * parent[-1]) // 128) * 128
    n = 1
    for s in parent:
        n *= s
    buf = torch.empty(2 * guard + n, dtype=dtype, device=device)
    _fill_pattern(buf)
    ptensor = buf[guard:guard + n].view(parent)
    view = ptensor if index is None else ptensor[index]
    assert tuple(view.shape) == tuple(shape), (view.shape, shape)
    return Guarded(buf, ptensor, view)


def guards_intact(buf, view):
    """Everything of `buf` outside `view` still holds the pattern, bit for bit (integer comparison)."""
    it = _INT[buf.element_size()]
    ib = buf.view(it).clone()
    pat = _PATTERN[buf.element_size()]
    ib.as_strided(view.shape, view.stride(), view.storage_offset() - buf.storage_offset()).fill_(pat)
    return bool((ib == pat).all())


def is_pattern_free(view):
    """No element of the view holds the guard pattern (an output fully written)."""
    return not bool((view.contiguous().view(_INT[view.element_size()]) == _PATTERN[view.element_size()]).any())
