"""Shared by tests/test_trunk_cases_host.py and tests/test_gpu_trunk_edges.py: the tile-edge cases of the hand-scheduled trunk kernels
(csrc/bottleneck.hip: bottleneck_chain_kernel in its ten instantiations, chain256_roles_kernel, conv3x3_c64_halo_kernel<false / true>;
csrc/stem.hip: stem_fused_kernel and its uint8 twin), a restatement of their host-side launch arithmetic, and their float64 references.  Imports
torch only (never the library), so it loads on a machine without a GPU.  The bound, the acceptance and the guarded buffers are those of
tests/gemm_cases.py (imported, not copied).

Launch plan.  The kernels are persistent: a workgroup walks tiles (resident chain, halo kernels) or lock-step sets of tiles (streamed chain: 8,
roles kernel: 4) and carries LDS-DMA double buffers, weight-ring slots and stage-buffer parities from one to the next.  `plan` restates, per
form, the grid the host launches and how many iterations each workgroup makes, so that the tables below can be CHECKED (on the CPU) to hold a
case on both sides of every edge of that loop: less than a tile, a tile and a set +- one pixel, the grid cap hit exactly, a second iteration in
one and in several workgroups, a third iteration.

References.  Float64 on the bf16 operands, with mag = the same expression on absolute values; accepted through gemm_cases.accept with
K_total = mid (2 mid with the projection shortcut), 4 mid (the second product), 576 (3x3 x 64) and 147 (7x7 x 3)."""
import os
import sys
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_cases import (guarded, guards_intact, is_pattern_free, bound, step, accept, accept_map, fill_pattern,  # noqa: E402,F401
                        BF16, F32)

CUS = 256                      # the grid cap of every persistent trunk kernel: one workgroup per CU
CHUNK = 16384                  # pixels per float64 reference evaluation on the device (no float64 tensor above ~ 300 MB at 2048 channels)


def seed(name):
    return zlib.crc32(str(name).encode())


def _ceil(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# launch plan (bottleneck.hip: relnet_bottleneck_chain / _s2 / _proj, relnet_conv3x3_c64 / _s2)
# ---------------------------------------------------------------------------------------------------------------------------------------------
Plan = namedtuple('Plan', 'grid iters last_set_tiles last_tile_pixels')
# grid: workgroups launched; iters: iterations of the tile / set loop, one entry per workgroup (resident chain: of its wavefront 0, the one that
# makes the most); last_set_tiles: live tiles of the last set (resident chain: of the last group of eight consecutive tiles, one workgroup's
# wavefronts; halo kernels: tiles of the last round over the grid); last_tile_pixels: live pixels of the last tile

SET_TILES = {'resident': 8, 'streamed': 8, 'roles': 4}
HALO_ROWS = {'halo': 8, 'halo_s2': 4}             # output rows of a tile (32 output columns for both)


def out_hw(H, W):
    """Map the stride-2 forms write (and the compact map of the gather form)."""
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def compact_pixels(B, H, W):
    Ho, Wo = out_hw(H, W)
    return B * Ho * Wo


def plan(form, P=None, B=None, H=None, W=None):
    """form: 'resident' (mid 64, also PROJ and the gather form at 64), 'streamed' (mid 128 / 256 / 512, the gather form at 128), 'roles' (mid 256
    with the reduce product): P pixels (the gather form: the compact count).  'halo' / 'halo_s2': B, H, W of the input."""
    if form in HALO_ROWS:
        Ho, Wo = (H, W) if form == 'halo' else out_hw(H, W)
        th = HALO_ROWS[form]
        ty, tx = _ceil(Ho, th), _ceil(Wo, 32)
        ntile = B * ty * tx
        grid = min(ntile, CUS)
        iters = tuple((ntile - wg + grid - 1) // grid for wg in range(grid))
        return Plan(grid, iters, ntile - (max(iters) - 1) * grid, (Ho - th * (ty - 1)) * (Wo - 32 * (tx - 1)))
    S = SET_TILES[form]
    ntile = _ceil(P, 32)
    nset = _ceil(ntile, S)
    if form == 'roles':
        grid = min(nset, CUS)
    else:
        grid = _ceil(ntile, 8) if ntile < 8 * CUS else CUS
    if form == 'resident':                         # per wavefront: tiles t_first = 8 wg + wave, step 8 grid; wavefront 0 of each workgroup
        iters = tuple((ntile - 8 * wg + 8 * grid - 1) // (8 * grid) for wg in range(grid))
    else:                                          # sets wg, wg + grid, ...; idle tiles of the last set still take part
        iters = tuple((nset - wg + grid - 1) // grid for wg in range(grid))
    return Plan(grid, iters, ntile - S * (nset - 1), P - 32 * (ntile - 1))


def second_iteration_pixel(form, P):
    """First pixel of the tile workgroup 0 (wavefront 0) takes in its second iteration."""
    return plan(form, P).grid * SET_TILES[form] * 32


def edge_classes(form, pl):
    """The classes of the issue's table a case belongs to, from its plan alone."""
    n_it = max(pl.iters)
    out = set()
    if form in HALO_ROWS:
        full = HALO_ROWS[form] * 32
        one = pl.grid == 1
        if one and pl.last_tile_pixels == 1:
            out.add('one pixel')
        if one and pl.last_tile_pixels == full:
            out.add('one tile')
        if pl.grid == 4 and pl.last_tile_pixels == 1:
            out.add('one tile + 1 both ways')
        if pl.grid == CUS and n_it == 1 and pl.last_set_tiles == CUS and pl.last_tile_pixels == full:
            out.add('cap exact')
        if n_it == 2 and pl.last_tile_pixels == full:
            out.add('two iterations, full last tile')
        if n_it == 2 and pl.last_tile_pixels < full:
            out.add('two iterations, ragged last tile')
        if n_it == 3:
            out.add('three iterations')
        return out
    S = SET_TILES[form]
    one = pl.grid == 1 and pl.iters == (1,)
    for name, tiles, px in (('one pixel', 1, 1), ('tile - 1', 1, 31), ('tile', 1, 32), ('tile + 1', 2, 1), ('set - 1', S, 31), ('set', S, 32)):
        if one and pl.last_set_tiles == tiles and pl.last_tile_pixels == px:
            out.add(name)
    if pl.grid == 2 and pl.iters == (1, 1) and pl.last_set_tiles == 1 and pl.last_tile_pixels == 1:
        out.add('set + 1')
    if pl.grid == CUS and n_it == 1 and pl.last_set_tiles == S and pl.last_tile_pixels == 32:
        out.add('cap exact')
    if n_it == 2 and pl.iters.count(2) == 1 and pl.last_set_tiles == 1 and pl.last_tile_pixels == 1:
        out.add('one workgroup twice, one live pixel')
    if n_it == 2 and pl.iters.count(2) >= 2 and 1 < pl.last_tile_pixels < 32:
        out.add('several workgroups twice, ragged')
    if n_it == 3:
        out.add('three iterations')
    return out


SMALL_CLASSES = ('one pixel', 'tile - 1', 'tile', 'tile + 1', 'set - 1', 'set', 'set + 1')
TWO_ITER_CLASSES = ('cap exact', 'one workgroup twice, one live pixel', 'several workgroups twice, ragged')
HALO_CLASSES = ('one pixel', 'one tile', 'one tile + 1 both ways', 'cap exact', 'two iterations, full last tile', 'two iterations, ragged last tile',
                'three iterations')

# ---------------------------------------------------------------------------------------------------------------------------------------------
# chain kernels: every instantiation the three entry points launch, and the pixel counts it runs at
# ---------------------------------------------------------------------------------------------------------------------------------------------
_SMALL = (1, 31, 32, 33, 255, 256, 257)
_TWO = (65536, 65537, 65797)
_P = {'resident': _SMALL + _TWO + (131073,),
      'streamed': _SMALL + _TWO + (131073,),
      'streamed-wide': _SMALL + _TWO,              # mid 256 expand-only, mid 512: NP * KSPLIT is even, the ring-slot and stage-buffer parities repeat
                                                   # after one tile; a third iteration is gigabytes of the same state
      'roles': (1, 31, 32, 33, 127, 128, 129, 32768, 32769, 32901, 65537)}


def _form(mid, plan_, pixels, reduce=False, proj=False, gather=False):
    return dict(mid=mid, plan=plan_, P=_P[pixels], reduce=reduce, proj=proj, gather=gather, three=131073 in _P[pixels] or pixels == 'roles')


FORMS = {
    'r64': _form(64, 'resident', 'resident', reduce=True),             # bottleneck_chain_kernel<64, false>
    'e64': _form(64, 'resident', 'resident'),                          # <64, false, false>
    'p64r': _form(64, 'resident', 'resident', reduce=True, proj=True),     # <64, false, true, 1, true>
    'p64e': _form(64, 'resident', 'resident', proj=True),              # <64, false, false, 1, true>
    'r128': _form(128, 'streamed', 'streamed', reduce=True),           # <128, true>
    'e128': _form(128, 'streamed', 'streamed'),                        # <128, true, false>
    'e256': _form(256, 'streamed', 'streamed-wide'),                   # <256, true, false>
    'e512': _form(512, 'streamed', 'streamed-wide'),                   # <512, true, false, 2>
    'r256': _form(256, 'roles', 'roles', reduce=True),                 # chain256_roles_kernel
    'g64': _form(64, 'resident', 'resident', gather=True),             # <64, false, false, 1, false, true>
    'g128': _form(128, 'streamed', 'streamed', gather=True),           # <128, true, false, 1, false, true>
}
DENSE_FORMS = [f for f in FORMS if not FORMS[f]['gather']]
GATHER_FORMS = [f for f in FORMS if FORMS[f]['gather']]
TWO_PRODUCT_OF = {'e64': 'r64', 'e128': 'r128', 'e256': 'r256'}      # expand-only form -> the two-product form with the same x_next bits

# full maps (B, H, W) of the gather form; the classes are those of the compact count B Ho Wo
GATHER_SHAPES = [
    (1, 1, 1),                 # 1
    (1, 8, 12),                # 4 x 6 = 24: less than a tile, even sizes (the last row / column is never read)
    (1, 1, 61),                # 31
    (1, 7, 15),                # 4 x 8 = 32
    (1, 5, 21),                # 3 x 11 = 33
    (2, 9, 13),                # 2 x 35 = 70: an image boundary inside a tile
    (1, 29, 33),               # 15 x 17 = 255
    (1, 31, 32),               # 16 x 16 = 256
    (1, 1, 513),               # 257
    (1, 511, 511),             # 256 x 256 = 65 536: the grid cap exactly
    (1, 1, 131073),            # 65 537: one workgroup iterates twice, for one pixel
    (2, 363, 363),             # 2 x 182 x 182 = 66 248: three workgroups iterate twice, 8 live pixels in the last tile
    (4, 229, 379),             # 4 x 115 x 190 = 87 400: image boundaries at 21 850 (inside tile 682) and 65 550 (inside tile 2048, the first tile
                               # of workgroup 0's second iteration)
    (3, 1, 87381),             # 3 x 43 691 = 131 073: three iterations
]
GATHER_ISOLATION_SHAPE = (4, 229, 379)


def chain_cases(form):
    """-> the case ids of a form: pixel counts (dense forms) or (B, H, W) maps (gather forms)."""
    return list(GATHER_SHAPES) if FORMS[form]['gather'] else list(FORMS[form]['P'])


def case_pixels(form, case):
    return compact_pixels(*case) if FORMS[form]['gather'] else case


def isolation_case(form):
    """One multi-iteration case per form whose second-iteration tile is not the last one."""
    if FORMS[form]['gather']:
        return GATHER_ISOLATION_SHAPE
    return 32901 if form == 'r256' else 65797


def chain_weights(mid, device):
    """W3 [4 mid, mid], Wp (projection, mid 64), W1' [mid, 4 mid] bf16 and the fp32 biases, scaled as tests/test_gpu_bottleneck.py scales them."""
    g = torch.Generator(device=device).manual_seed(seed('weights-%d' % mid))
    r = lambda *s: torch.randn(*s, generator=g, device=device)
    cout = 4 * mid
    d = {'w3': (r(cout, mid) * (0.1 if mid <= 128 else 0.05)).to(BF16), 'b3': r(cout) * 0.1,
         'w1': (r(mid, cout) * 0.05).to(BF16), 'b1': r(mid) * 0.1}
    if mid == 64:
        d['wp'] = (r(cout, mid) * 0.1).to(BF16)
        d['b3p'] = (d['b3'] + r(cout) * 0.1).contiguous()
    return d


def chain_operands(form, case, device):
    """mid2 and the shortcut operand (x, or x_in for the projection forms; the gather form: the full map) as ReLU outputs of randn, bf16."""
    f = FORMS[form]
    mid = f['mid']
    g = torch.Generator(device=device).manual_seed(seed('%s-%s' % (f['mid'], case)))      # one draw per (mid, case): the forms of a width share it
    r = lambda *s: torch.relu(torch.randn(*s, generator=g, device=device)).to(BF16)
    if f['gather']:
        B, H, W = case
        Ho, Wo = out_hw(H, W)
        return {'m2': r(B, Ho, Wo, mid), 'x': r(B, H, W, 4 * mid)}
    d = {'m2': r(case, mid)}
    d['x'] = r(case, 4 * mid)
    if mid == 64:
        d['xin'] = r(case, mid)
    return d


def chain_ref(m2, w3, b3, x=None, xin=None, wp=None):
    """-> (pre, mag), float64 [n, 4 mid]: pre = W3 mid2 + b3 + x, or W3 mid2 + Wp x_in + b3p (the shortcut is not rounded on the way)."""
    def ev(m2, w3, b3, sc, wp):
        y = m2 @ w3.t() + b3
        return y + (sc if wp is None else sc @ wp.t())
    sc = x if xin is None else xin
    d = lambda t: None if t is None else t.double()
    a = lambda t: None if t is None else t.double().abs()
    return ev(d(m2), d(w3), d(b3), d(sc), d(wp)), ev(a(m2), a(w3), a(b3), a(sc), a(wp))


def reduce_ref(xn, w1, b1):
    """The second product from the kernel's OWN x_next (isolates it): -> (pre, mag), float64 [n, mid]."""
    return xn.double() @ w1.double().t() + b1.double(), xn.double().abs() @ w1.double().abs().t() + b1.double().abs()


def bound_share(got, want, mag, k_total):
    """Largest (|got - want| - half a bf16 step) / bound: the part of the fp32 accumulation bound a bf16 output uses beyond its own rounding
    (err / tolerance of a bf16 output approaches 1 for ANY correct evaluation, since the rounding is itself half a step)."""
    return float((((got.double() - want).abs() - 0.5 * step(want)) / bound(mag, k_total).clamp_min(1e-300)).max())


def accept_chain(form, w, m2, sc, xn, m1=None, chunk=CHUNK):
    """x_next (and mid1') of a dense [P, .] case against float64, in chunks of `chunk` pixels.  sc: x, or x_in for the projection forms.
    -> (ok_x, worst_x, ok_m, worst_m); the mid1' pair is (True, 0.0) without the second product."""
    f = FORMS[form]
    mid = f['mid']
    okx = okm = True
    wx = wm = 0.0
    for p0 in range(0, m2.shape[0], chunk):
        s = slice(p0, p0 + chunk)
        if f['proj']:
            pre, mag = chain_ref(m2[s], w['w3'], w['b3p'], xin=sc[s], wp=w['wp'])
        else:
            pre, mag = chain_ref(m2[s], w['w3'], w['b3'], x=sc[s])
        ok, worst = accept(xn[s], pre.clamp_min(0), pre, mag, 2 * mid if f['proj'] else mid, bf16_out=True, relu=True)
        okx, wx = okx and ok, max(wx, worst)
        if m1 is not None:
            pre, mag = reduce_ref(xn[s], w['w1'], w['b1'])
            ok, worst = accept(m1[s], pre.clamp_min(0), pre, mag, 4 * mid, bf16_out=True, relu=True)
            okm, wm = okm and ok, max(wm, worst)
    return okx, wx, okm, wm


# ---------------------------------------------------------------------------------------------------------------------------------------------
# halo 3x3 kernels (C = 64)
# ---------------------------------------------------------------------------------------------------------------------------------------------
HALO_SHAPES = [(1, 1, 1), (1, 1, 33), (1, 9, 1), (1, 8, 32), (1, 9, 33),
               (1, 64, 1024),              # 8 x 32 = 256 tiles
               (1, 65, 1024),              # 9 x 32 = 288
               (1, 57, 1025),              # 8 x 33 = 264
               (1, 152, 864)]              # 19 x 27 = 513: three iterations
HALO_S2_SHAPES = [(1, 1, 1), (1, 7, 63), (1, 8, 64), (1, 9, 65),       # Ho x Wo = 1 x 1, 4 x 32, 4 x 32, 5 x 33
                  (1, 255, 511),           # 128 x 256: 32 x 8 = 256 tiles
                  (1, 263, 511),           # 132 x 256: 33 x 8 = 264
                  (1, 265, 513),           # 133 x 257: 34 x 9 = 306, one live pixel in the last tile
                  (2, 265, 513)]           # 612: three iterations
HALO_SMALL = [s for s in HALO_SHAPES + HALO_S2_SHAPES[1:4] if s[1] <= 9 and s[2] <= 65]


def halo_operands(shape, device):
    B, H, W = shape
    g = torch.Generator(device=device).manual_seed(seed('halo-%s' % (shape,)))
    x = torch.relu(torch.randn(B, H, W, 64, generator=g, device=device)).to(BF16)
    w = (torch.randn(64, 64, 3, 3, generator=g, device=device) * 0.05).to(BF16)          # OIHW
    b = torch.randn(64, generator=g, device=device) * 0.1
    return x, w, b


def halo_ref(x, w, b, stride=1):
    """float64 conv2d(padding 1) of NHWC x with OIHW w: -> (pre, mag) NHWC."""
    ev = lambda x, w, b: F.conv2d(x.permute(0, 3, 1, 2), w, b, stride=stride, padding=1).permute(0, 2, 3, 1).contiguous()
    return ev(x.double(), w.double(), b.double()), ev(x.double().abs(), w.double().abs(), b.double().abs())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fused stem
# ---------------------------------------------------------------------------------------------------------------------------------------------
STEM_TILE = (8, 14)                                # pooled pixels of a workgroup's tile
# The issue's lattice, and W = 63 and 119 beside it: the issue's own W values reach Wp = 2, 15 and 29 only, so Wp % 14 == 2 (16 and 30: two pooled
# columns in the last tile column) needs Wc = 32 and 60.
STEM_H = (7, 8, 9, 10, 11, 37, 38, 39, 40)
STEM_W = (7, 8, 59, 60, 61, 62, 63, 115, 116, 117, 119)


def stem_hw(H, W):
    """-> (Hc, Wc, Hp, Wp): conv1 7x7 / 2, pad 3, then pool1 3x3 / 2 in ceil mode (the last window starts inside the map)."""
    Hc, Wc = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    Hp, Wp = _ceil(Hc - 3, 2) + 1, _ceil(Wc - 3, 2) + 1
    if (Hp - 1) * 2 >= Hc:
        Hp -= 1
    if (Wp - 1) * 2 >= Wc:
        Wp -= 1
    return Hc, Wc, Hp, Wp


def _stem_sizes():
    pairs = [(STEM_H[0], STEM_W[0]), (STEM_H[0], 117), (STEM_H[-1], STEM_W[0]), (STEM_H[-1], 117)]      # the four corners of the issue's lattice
    for i, H in enumerate(STEM_H):                 # every H with (two or) three W, every W two or three times: 30 sizes
        for j in range(3 if i else 2):
            hw = (H, STEM_W[(3 * i + j + 1) % len(STEM_W)])
            if hw not in pairs:
                pairs.append(hw)
    return pairs


STEM_SIZES = _stem_sizes()
STEM_SMALL = [s for s in STEM_SIZES if s[0] <= 11 and s[1] <= 61]
STEM_MEANS = (103.06, 115.90, 123.15)


def stem_extents(H, W):
    """im_info extents of the two images of the uint8 case: the whole canvas, and one that ends inside it (an odd number of rows and columns less
    where there is room for it)."""
    return [[H, W, 1.0], [max(H - 3, 1), max(W - 5, 1), 1.0]]


def stem_operands(size, device):
    """-> fp32 image batch [2, 3, H, W], uint8 canvas [2, H, W, 3], OIHW weights [64, 3, 7, 7] fp32, bias [64]."""
    H, W = size
    g = torch.Generator(device=device).manual_seed(seed('stem-%s' % (size,)))
    img = torch.randn(2, 3, H, W, generator=g, device=device)
    u8 = torch.randint(0, 256, (2, H, W, 3), generator=g, device=device, dtype=torch.uint8)
    w = torch.randn(64, 3, 7, 7, generator=g, device=device) * 0.1
    b = torch.randn(64, generator=g, device=device)
    return img, u8, w, b


def stem_ref(img, w, bias):
    """img [B, 3, H, W] and w [64, 3, 7, 7]: the values the kernel reads (rounded to bf16 by the caller).  -> (want, tol), float64 NHWC
    [B, Hp, Wp, 64]: max_pool(relu(conv + bias)) and the per-conv-pixel tolerance bound(mag, 147) + half a bf16 step of the conv value, pooled
    with the same max-pool (|max a - max b| <= max |a - b|, and the pool of bf16 values is exact)."""
    conv = lambda x, w, b: F.conv2d(x, w, b, stride=2, padding=3)
    ref = conv(img.double(), w.double(), bias.double()).clamp_min(0)
    mag = conv(img.double().abs(), w.double().abs(), bias.double().abs())
    tol = bound(mag, 147) + 0.5 * step(ref)
    pool = lambda t: F.max_pool2d(t, 3, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous()
    return pool(ref), pool(tol)


def stem_accept(got, want, tol):
    """-> (ok, worst err / tolerance)."""
    got = got.double()
    err = (got - want).abs()
    ok = bool(((err <= tol) & torch.isfinite(got)).all())
    ratio = torch.where(torch.isfinite(got), err / tol.clamp_min(1e-300), torch.full_like(err, float('inf')))
    return ok, float(ratio.max())
