"""Shared by tests/test_relation_edge_cases_host.py and tests/test_gpu_relation_edges.py: the pad-edge cases of the relation attention kernels
(csrc/relation.hip, csrc/relation_bwd.hip), their float64 reference, the error bound the forward results are held to, a float32 emulation of the
kernels' algorithm (with switches that make it subtly wrong), and guarded operand buffers.  Imports torch only (never the library), so it loads on
a machine without a GPU; every routine works on the device its arguments live on.

Cases.  (N, M) on both sides of a 32-key tile (31 / 32 / 33), of the 320-key LDS chunk of relation_attention_lds_kernel (320 / 321), of its 16
wavefronts per workgroup (N = 513), M = 1 with N > 1, and the fused kernel's limit of 640 keys; B = 9 makes the fused kernel's image groups of 8
ragged.  Five forward variants (VARIANTS), the dispatch of relnet_relation_attention_kc / relnet_relation_attention_fused.

Operands.  q, k, VW^T, bout, resid are N(0, 1) in float32 rounded to the kernel's input type (resid: the output type); the bias is drawn in the
kernel's own format -- float32 ln G uniform in [-13.9, 0.5] (G from the 1e-6 floor to e^0.5), or fp16 log2 G over the same range -- so the
reference sees the numbers the kernel sees.

Reference.  From the definition in float64, per (image, head): logit_ij = scale q_i . k_j + ln G_ij, p_ij = softmax over j < M,
y_i = sum_j p_ij vw_j + bout, act_i = relu(resid_i + y_i); and A_i = sum_j p_ij |vw_j| + |bout|, the magnitude the rounding errors scale with.

Bound (derived, not measured), per element.
  bf16 variants:  |y - ref| <= (2^-8 + 2^-9) A_i  (+ half a bf16 step of ref for the rounding of the output).  2^-8: the kernels round p_ij to
      bf16 before the second matrix product -- round to nearest with 8 significand bits, a relative error of at most 2^-8, the unit roundoff of
      bf16 -- while the normaliser l_i sums the unrounded fp32 p, so the numerator moves by at most 2^-8 sum_j p_ij |vw_j| <= 2^-8 A_i.
      2^-9 covers every float32 effect: the 64-term dot product (<= 64 2^-24 relative to sum |q||k|, times scale: an absolute logit error
      e <= ~1e-5 for |logit| <= 100, which moves p by the factor exp(e)), the argument error of the exponential (|logit| 2^-24 plus ~2 ulp of the
      hardware exp2), the M-term sums of l and of the accumulator (<= M 2^-24 relative to sum of magnitudes, M <= 700: 4.2e-5) and the final
      multiply / add (2^-23): together below 1e-4 relative to A_i, twenty times inside 2^-9 = 1.95e-3.
  fp32 variant:  |y - ref| <= (M + 64 + 8 max|logit|) 2^-23 A_i: M-term sums, 64-term dot products (their absolute logit error changes p by that
      relative amount), and the exponential's relative error ~ |argument| ulp for arguments up to 2 max|logit| in magnitude.
  activation:  relu is 1-Lipschitz, so the error of y passes through unchanged.  fp32: one more float32 addition, 2^-24 |resid + y|, inside the
      same bound taken around resid + y (A_i + |resid|).  bf16: the LDS and fused kernels round y to bf16, add resid and round again; the streaming
      kernel rounds once.  Tolerance for all: (2^-8 + 2^-9) A_i + half a bf16 step of y + half a bf16 step of resid + y.
  A bf16 step of t is taken as |t| 2^-7 (gemm_cases.step: the upper end of the binade).
tests/test_relation_edge_cases_host.py shows on the CPU that the float32 emulation of the kernels' algorithm stays under half of the bound at every
case, and that each of six subtly wrong variants of it exceeds the tolerance on at least one element.

Guarded buffers (gemm_cases.guarded): every operand is a view in the middle of a buffer filled with a quiet-NaN pattern, >= 1 MiB on both sides."""
import zlib

import torch

import gemm_cases as GC

BF16, F32, F16 = torch.bfloat16, torch.float32, torch.float16
H, D = 16, 1024                            # heads x 64 channels: the configuration the kernels are specialised to
SCALE = 0.125                              # 1 / sqrt(64)
LN2 = 0.6931471805599453
LN_G_RANGE = (-13.9, 0.5)                  # ln G: from just above the reference's floor ln 1e-6 = -13.8 to G = 1.65
FUSED_MAX_KEYS = 640
LDS_CHUNK = 320
LAUNCH = {'stream_f32': 1, 'stream_bf16': 2, 'lds_f16': 3, 'lds_f32': 4, 'fused': 5}     # relnet_relation_attention_last_launch()
VARIANTS = tuple(LAUNCH)
KC_VARIANTS = ('stream_f32', 'stream_bf16', 'lds_f16', 'lds_f32')                         # those that take key_count


def pad32(m):
    return (m + 31) // 32 * 32


# ---------------------------------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (33, 1), (31, 31), (32, 32), (33, 33), (65, 32), (65, 33), (129, 128), (321, 320), (322, 321), (513, 33), (513, 321)]
SHAPES_640 = [(641, 640)]                  # the fused kernel's limit: fused and LDS variants only
SHAPES_B9 = [(33, 33), (322, 321)]         # B = 9: a ragged last group of 8 images in the fused kernel
WAVES_SHAPES = [(65, 33), (322, 321)]      # LDS variants with RELNET_ATTN_WAVES = 1 and 3: several workgroups share one (image, head)

# (want_out, want_act, bout, resid, want_logits on the streaming variants): every legal output combination, bout / resid present and absent
CONFIGS = [
    dict(id='out', out=True, act=False, bout=True, resid=False, logits=True),
    dict(id='act', out=False, act=True, bout=False, resid=True, logits=False),
    dict(id='out+act', out=True, act=True, bout=True, resid=True, logits=True),
    dict(id='out+act-plain', out=True, act=True, bout=False, resid=False, logits=False),
]


def _case(variant, N, M, B=1, waves=None):
    in_dt = F32 if variant == 'stream_f32' else BF16
    bias_dt = F16 if variant == 'lds_f16' else (None if variant == 'fused' else F32)
    d = dict(id='%s-%dx%d-b%d%s' % (variant, N, M, B, '-w%d' % waves if waves else ''), variant=variant, N=N, M=M, B=B, Mpad=pad32(M), waves=waves,
             in_dtype=in_dt, bias_dtype=bias_dt, q_ld=2 * D, k_ld=2 * D, vwt_ld=pad32(M), out_ld=D, resid_ld=D)
    return d


FORWARD_CASES = []
for _v in VARIANTS:
    FORWARD_CASES += [_case(_v, n, m) for (n, m) in SHAPES]
    if _v in ('fused', 'lds_f16', 'lds_f32'):
        FORWARD_CASES += [_case(_v, n, m) for (n, m) in SHAPES_640]
    FORWARD_CASES += [_case(_v, n, m, B=9) for (n, m) in SHAPES_B9]
    if _v in ('lds_f16', 'lds_f32'):
        FORWARD_CASES += [_case(_v, n, m, waves=w) for (n, m) in WAVES_SHAPES for w in (1, 3)]

GUARDED_CASES = [_case(_v, n, m, B=b) for _v in VARIANTS for (n, m, b) in ((33, 1, 1), (65, 33, 2), (322, 321, 1))]

# backward (tests/test_gpu_relation_edges.py): (N, M); the last three of BWD_BF16 put the small-kernel limit N <= 128, Mpad <= 128 on both sides
BWD_F32 = [(1, 1), (33, 1), (33, 32), (33, 33), (65, 33), (128, 128), (129, 97), (160, 129)]
BWD_BF16 = [(33, 32), (65, 33), (128, 128), (129, 97), (160, 129)]
BWD_SMALL = [(1, 1, None), (33, 1, None), (33, 33, None), (128, 128, None), (128, 97, [97, 1, 32, 33, 96])]


def check_case(c):
    """The preconditions of the variant a case names (relnet_relation_attention_kc / _fused): raises AssertionError otherwise."""
    v = c['variant']
    assert v in VARIANTS and 1 <= c['M'] <= c['N'] <= 700 and 1 <= c['B'] <= 9
    assert c['Mpad'] == pad32(c['M']) and c['Mpad'] % 32 == 0 and c['vwt_ld'] >= c['Mpad']
    if v == 'stream_f32':
        assert c['in_dtype'] == F32 and c['bias_dtype'] == F32
        assert c['q_ld'] % 4 == 0 and c['k_ld'] % 4 == 0 and c['vwt_ld'] % 4 == 0            # 16-byte rows of float32
    else:
        assert c['in_dtype'] == BF16
        assert c['q_ld'] % 8 == 0 and c['k_ld'] % 8 == 0 and c['vwt_ld'] % 4 == 0            # 16-byte (q, k) / 8-byte (vwt) rows of bf16
    if v in ('lds_f16', 'lds_f32', 'fused'):
        assert c['out_ld'] % 8 == 0 and c['resid_ld'] % 8 == 0
    if v == 'lds_f16':
        assert c['bias_dtype'] == F16
    if v in ('lds_f32', 'stream_bf16'):
        assert c['bias_dtype'] == F32 and (c['B'] * H * c['N'] * c['Mpad']) % 4 == 0
    if v == 'fused':
        assert c['M'] <= FUSED_MAX_KEYS and c['bias_dtype'] is None
    if c['waves'] is not None:
        assert v in ('lds_f16', 'lds_f32') and 1 <= c['waves'] <= 16
    return True


def seed(case):
    return zlib.crc32(('%dx%d-b%d' % (case['N'], case['M'], case['B'])).encode())      # one set of operands per shape, shared by the variants


# ---------------------------------------------------------------------------------------------------------------------------------------------
# operands (CPU): values as float32 that are exact in the kernel's formats
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _round(t, dtype):
    return t.to(dtype).to(F32)


def operands(case, bias_pad=None):
    """-> dict of CPU float32 tensors holding exactly what the kernel reads: q [B,N,D], k [B,M,D], vwt [B,D,Mpad] (columns >= M zero), bias
    [B,H,N,Mpad] in the natural-log domain AS THE KERNEL SEES IT plus `bias_raw` in the kernel's own format (fp16 log2 G or float32 ln G; None
    for the fused variant, whose bias comes from `boxes`), bout [D], resid [B,N,D].  Pad columns [M, Mpad) of the bias: drawn like the others
    (bias_pad None) or a constant (e.g. NaN)."""
    g = torch.Generator().manual_seed(seed(case))
    B, N, M, Mpad = case['B'], case['N'], case['M'], case['Mpad']
    dt = case['in_dtype']
    o = {}
    o['q'] = _round(torch.randn(B, N, D, generator=g), dt)
    o['k'] = _round(torch.randn(B, M, D, generator=g), dt)
    vwt = torch.zeros(B, D, Mpad)
    vwt[..., :M] = torch.randn(B, D, M, generator=g)
    o['vwt'] = _round(vwt, dt)
    o['bout'] = torch.randn(D, generator=g)
    o['resid'] = _round(torch.randn(B, N, D, generator=g), dt)
    lo, hi = LN_G_RANGE
    u = torch.rand(B, H, N, Mpad, generator=g) * (hi - lo) + lo          # ln G
    if case['bias_dtype'] == F16:
        raw = (u / LN2).to(F16)                                          # fp16 log2 G: what the matrix-core geometry kernel stores
        if bias_pad is not None:
            raw[..., M:] = bias_pad
        o['bias_raw'], o['bias'] = raw, raw.to(torch.float64) * LN2
    else:
        raw = u.clone()
        if bias_pad is not None:
            raw[..., M:] = bias_pad
        o['bias_raw'], o['bias'] = raw, raw.to(torch.float64)
    if case['variant'] == 'fused':
        o['bias_raw'] = o['bias'] = None
        xy = torch.rand(B, N, 2, generator=g) * 500.0
        wh = torch.rand(B, N, 2, generator=g) * 200.0 + 4.0
        o['boxes'] = torch.cat([xy, xy + wh], -1).contiguous()
        # pair_pos_fc1: weights at the scale of the reference's initialisation (E . w has a standard deviation of ~0.11), the bias around 0.25, so that
        # about 1 % of the pairs sit on the 1e-6 floor of log(max(G, 1e-6)) while every row has keys with G ~ 0.25.  With a zero-mean bias and
        # only 33 keys, ~1 % of the (query, head) rows have G < 1e-3 at EVERY key; there the 3e-4 absolute error of an fp16 geometry product is an
        # O(1) change of the logits, for the fused kernel and the two-kernel fp16 path alike ("known limitation"): the
        # conditioning of the reference's formula, not what the edge cases are after
        o['wp'] = torch.randn(H, 64, generator=g) * 0.02
        o['bp'] = 0.25 + torch.randn(H, generator=g) * 0.02
    return o


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float64 reference and bound
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ref64(q, k, vwt, bias, bout, resid, M, key_count=None):
    """From the definition, float64, on the device of the operands.  q [B,N,D], k [B,>=M,D], vwt [B,D,>=M], bias [B,H,N,>=M] (ln G), bout [D] | None,
    resid [B,N,D] | None -> dict(y, act, pre_act, resid, logits [B,N,H,M], A, max_logit) with A = sum_j p |vw_j| + |bout|."""
    return configure(ref64_base(q, k, vwt, bias, M, key_count), bout, resid)


def ref64_base(q, k, vwt, bias, M, key_count=None):
    """The part of the reference that does not depend on bout / resid (computed once per case, shared by the output configurations)."""
    B, N = q.shape[0], q.shape[1]
    f = lambda t: t.to(torch.float64)
    qh = f(q).reshape(B, N, H, 64).permute(0, 2, 1, 3)                       # [B,H,N,64]
    kh = f(k[:, :M]).reshape(B, M, H, 64).permute(0, 2, 1, 3)                # [B,H,M,64]
    vw = f(vwt[..., :M]).reshape(B, H, 64, M).permute(0, 1, 3, 2)            # [B,H,M,64]
    logit = SCALE * qh @ kh.transpose(-1, -2) + f(bias[..., :M])             # [B,H,N,M]
    if key_count is not None:
        col = torch.arange(M, device=q.device)
        live = col[None, :] < torch.as_tensor(key_count, device=q.device).clamp(1, M)[:, None]
        logit = logit.masked_fill(~live[:, None, None, :], float('-inf'))
    p = torch.softmax(logit, -1)
    finite = logit[torch.isfinite(logit)]
    return dict(y=(p @ vw).permute(0, 2, 1, 3).reshape(B, N, D), A=(p @ vw.abs()).permute(0, 2, 1, 3).reshape(B, N, D),
                logits=logit.permute(0, 2, 1, 3).contiguous(), max_logit=float(finite.abs().max()))


def configure(base, bout, resid):
    f = lambda t: t.to(torch.float64)
    y, A = base['y'], base['A']
    if bout is not None:
        y, A = y + f(bout), A + f(bout).abs()
    r = f(resid) if resid is not None else torch.zeros_like(y)
    return dict(y=y, act=torch.relu(r + y), pre_act=r + y, resid=r, logits=base['logits'], A=A, max_logit=base['max_logit'])


def bound(ref, M, bf16):
    """The derived bound on |y - ref| per element (without the rounding of a bf16 output)."""
    if bf16:
        return (2.0 ** -8 + 2.0 ** -9) * ref['A']
    return (M + 64 + 8 * ref['max_logit']) * 2.0 ** -23 * ref['A']


def tolerances(ref, M, bf16):
    """-> (tolerance of y, tolerance of act), per element: the bound plus the output roundings (module docstring)."""
    bnd = bound(ref, M, bf16)
    if bf16:
        t_y = bnd + 0.5 * GC.step(ref['y'])
        return t_y, t_y + 0.5 * GC.step(ref['pre_act'])
    return bnd, (M + 64 + 8 * ref['max_logit']) * 2.0 ** -23 * (ref['A'] + ref['resid'].abs())


def worst_ratio(got, want, tol):
    """Largest |got - want| / tol over the elements (inf for a non-finite element)."""
    got = got.to(torch.float64)
    err = (got - want).abs()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float('inf')))
    return float(ratio.max())


LOGIT_TOL = 1e-4          # the existing float32 tests' bar on the attention logits (tests/test_gpu_relation.py), used for the float64 comparison


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernels' algorithm (CPU), with the switches of the host test's mutants
# ---------------------------------------------------------------------------------------------------------------------------------------------
def emulate(o, case, bf16, use_bout=True, mask_limit=None, pad_bias_zero=False, skip_last_partial=False, half_l=False, drop_key=None,
            round_out=False):
    """Online softmax over key tiles of 32 as relation_attention_kernel runs it: float32 logits, running maximum / normaliser, P rounded to bf16
    before the second product when `bf16` (the normaliser sums the unrounded p), float32 accumulation, 1 / l at the end.  Keys past M read the
    clamped K row M - 1, the bias pad column and the (zero) VW^T pad column, and are masked.  Mutants: mask_limit (keys < mask_limit instead of
    < M survive), pad_bias_zero (the pad columns enter with bias 0, unmasked), skip_last_partial (the tile that holds keys past M is not run),
    use_bout False, half_l (1 / l from the lanes of one 32-lane half: keys with (j mod 8) < 4), drop_key (that key is masked).
    -> y [B,N,D] float32 (rounded to bf16 and back with round_out)."""
    B, N, M, Mpad = case['B'], case['N'], case['M'], case['Mpad']
    qh = o['q'].reshape(B, N, H, 64).permute(0, 2, 1, 3)
    kidx = torch.arange(Mpad).clamp(max=M - 1)
    kh = o['k'][:, kidx].reshape(B, Mpad, H, 64).permute(0, 2, 1, 3)
    vw = o['vwt'].reshape(B, H, 64, Mpad).permute(0, 1, 3, 2)                 # [B,H,Mpad,64], rows >= M zero
    bias = o['bias'].to(F32).clone()
    limit = M if mask_limit is None else mask_limit
    if pad_bias_zero:
        bias[..., M:] = 0.0
        limit = Mpad
    logit = (SCALE * (qh @ kh.transpose(-1, -2))).to(F32) + bias             # [B,H,N,Mpad]
    col = torch.arange(Mpad)
    dead = col >= limit
    if drop_key is not None:
        dead = dead | (col == drop_key)
    logit = torch.where(dead, torch.full_like(logit, float('-inf')), logit)
    ntile = Mpad // 32
    if skip_last_partial and M % 32:
        ntile -= 1
    m_run = torch.full((B, H, N, 1), float('-inf'))
    l_run = torch.zeros(B, H, N, 1)
    acc = torch.zeros(B, H, N, 64)
    lmask = ((col % 8) < 4).to(F32) if half_l else torch.ones(Mpad)
    for t in range(ntile):
        s = logit[..., 32 * t:32 * t + 32]
        m_new = torch.maximum(m_run, s.max(-1, keepdim=True).values)
        alpha = torch.exp(m_run - m_new)
        p = torch.exp(s - m_new)
        l_run = l_run * alpha + (p * lmask[32 * t:32 * t + 32]).sum(-1, keepdim=True)
        pq = p.to(BF16).to(F32) if bf16 else p
        acc = acc * alpha + pq @ vw[:, :, 32 * t:32 * t + 32]
        m_run = m_new
    y = (acc * (1.0 / l_run)).permute(0, 2, 1, 3).reshape(B, N, D)
    if use_bout:
        y = y + o['bout']
    return y.to(BF16).to(F32) if round_out else y


# ---------------------------------------------------------------------------------------------------------------------------------------------
# guarded buffers for the attention operands
# ---------------------------------------------------------------------------------------------------------------------------------------------
K_EXTRA_ROWS = 2           # k is handed over with more than M rows; the extra ones hold NaN


class GuardedOperands(object):
    """Device operands of one case, each a view in the middle of a NaN-pattern buffer: q and k column slices of ONE [B, N + 2, 2 D] buffer (row
    stride 2 D; k has M + 2 rows, the extra ones NaN), resid / out / act [.., :D] of [B, N, D + 64] parents, vwt [.., :Mpad] of a [B, D, Mpad + 32]
    parent, bias / boxes / key_count batch slices [1 : B + 1] of parents with B + 2 images (they have to be dense), logits dense.  Bias columns
    [M, Mpad) are NaN; VW^T columns [M, Mpad) are zero -- the documented contract of that operand, asserted here."""

    def __init__(self, case, o, device='cuda'):
        B, N, M, Mpad = case['B'], case['N'], case['M'], case['Mpad']
        dt = case['in_dtype']
        nan = float('nan')
        self.case = case
        S = slice
        self.qk = GC.guarded((B, N + K_EXTRA_ROWS, 2 * D), dt, device=device)
        gq = self.qk
        self.q = gq.view[:, :N, :D]
        self.k = gq.view[:, :M + K_EXTRA_ROWS, D:]
        GC.fill_pattern(gq.buf)                                              # the parts of the parent neither view covers keep the pattern
        self.q.copy_(o['q'].to(dt))
        self.k.fill_(nan)
        self.k[:, :M].copy_(o['k'].to(dt))
        self.vwt = GC.guarded((B, D, Mpad), dt, parent=(B, D, Mpad + 32), index=(S(None), S(None), S(0, Mpad)), device=device)
        self.vwt.view.copy_(o['vwt'].to(dt))
        assert bool((self.vwt.view[..., M:] == 0).all()), 'VW^T columns [M, Mpad) must be zero: the contract of the operand (ops.relation_attention)'
        self.resid = GC.guarded((B, N, D), dt, parent=(B, N, D + 64), index=(S(None), S(None), S(0, D)), device=device)
        self.resid.view.copy_(o['resid'].to(dt))
        self.bout = GC.guarded((D,), F32, parent=(3, D), index=1, device=device)
        self.bout.view.copy_(o['bout'])
        self.bias = self.boxes = self.wp = self.bp = None
        if case['variant'] == 'fused':
            self.boxes = GC.guarded((B, N, 4), F32, parent=(B + 2, N, 4), index=S(1, B + 1), device=device)
            self.boxes.view.copy_(o['boxes'])
            self.wp = GC.guarded((H, 64), F32, parent=(3, H, 64), index=1, device=device)
            self.wp.view.copy_(o['wp'])
            self.bp = GC.guarded((H,), F32, parent=(3, H), index=1, device=device)
            self.bp.view.copy_(o['bp'])
        else:
            bdt = case['bias_dtype']
            self.bias = GC.guarded((B, H, N, Mpad), bdt, parent=(B + 2, H, N, Mpad), index=S(1, B + 1), device=device)
            self.bias.view.copy_(o['bias_raw'].to(bdt))
            self.bias.view[..., M:] = nan
        self.key_count = GC.guarded((B,), torch.int32, parent=(B + 2,), index=S(1, B + 1), device=device)
        self.out = GC.guarded((B, N, D), dt, parent=(B, N, D + 64), index=(S(None), S(None), S(0, D)), device=device)
        self.act = GC.guarded((B, N, D), dt, parent=(B, N, D + 64), index=(S(None), S(None), S(0, D)), device=device)
        self.logits = GC.guarded((B, N, H, M), F32, device=device)

    def inputs(self):
        return [g for g in (self.qk, self.vwt, self.resid, self.bout, self.bias, self.boxes, self.wp, self.bp, self.key_count) if g is not None]

    def snapshot(self):
        return [g.buf.clone() for g in self.inputs()]

    def inputs_unchanged(self, snap):
        """Bit for bit (integer comparison: NaN patterns compare equal to themselves)."""
        for g, s in zip(self.inputs(), snap):
            it = GC.INT_VIEW[g.buf.element_size()]
            if not torch.equal(g.buf.view(it), s.view(it)):
                return False
        return True

    def reset_outputs(self):
        for g in (self.out, self.act, self.logits):
            GC.fill_pattern(g.buf)
