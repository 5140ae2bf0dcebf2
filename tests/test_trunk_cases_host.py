"""What tests/test_gpu_trunk_edges.py relies on, checked on the CPU (tests/trunk_cases.py):
  * `plan` against hand-computed launches of csrc/bottleneck.hip, and the case tables against the edge classes: every form of the chain and halo
    kernels keeps a case on both sides of every edge of its persistent loop, so that the tables cannot be thinned later without notice;
  * the stem lattice reaches both sides of the 8 x 14 pooled tile's edges and every parity of the conv map and of the last pooling window;
  * at the small cases, a plain fp32 evaluation of the same bf16 operands passes the acceptance (its share of the tolerance is printed), and the
    same output with two pixels swapped, or with one element moved by two bf16 steps, is rejected."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trunk_cases as TC  # noqa: E402

BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------------------------------
# launch plan
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _p(grid, iters, tiles, px):
    """Plan with the iteration counts given as (count, workgroups) runs."""
    return TC.Plan(grid, tuple(n for n, k in iters for _ in range(k)), tiles, px)


HAND = [
    # streamed: grid = ntile < 2048 ? ceil(ntile / 8) : 256, sets of 8 tiles
    ('streamed', dict(P=1), _p(1, [(1, 1)], 1, 1)),
    ('streamed', dict(P=31), _p(1, [(1, 1)], 1, 31)),
    ('streamed', dict(P=32), _p(1, [(1, 1)], 1, 32)),
    ('streamed', dict(P=33), _p(1, [(1, 1)], 2, 1)),
    ('streamed', dict(P=255), _p(1, [(1, 1)], 8, 31)),
    ('streamed', dict(P=256), _p(1, [(1, 1)], 8, 32)),
    ('streamed', dict(P=257), _p(2, [(1, 2)], 1, 1)),
    ('streamed', dict(P=65536), _p(256, [(1, 256)], 8, 32)),                     # 2048 tiles = 256 sets
    ('streamed', dict(P=65537), _p(256, [(2, 1), (1, 255)], 1, 1)),              # 2049 tiles = 257 sets
    ('streamed', dict(P=65797), _p(256, [(2, 2), (1, 254)], 1, 5)),              # 2057 tiles = 258 sets, 65797 - 32 * 2056 = 5
    ('streamed', dict(P=131073), _p(256, [(3, 1), (2, 255)], 1, 1)),             # 4097 tiles = 513 sets
    ('streamed', dict(P=28125), _p(110, [(1, 110)], 7, 29)),                     # the largest map of tests/test_gpu_bottleneck.py at mid 128: one set each
    # resident: the same grid, tiles per wavefront with step 8 grid
    ('resident', dict(P=257), _p(2, [(1, 2)], 1, 1)),
    ('resident', dict(P=65536), _p(256, [(1, 256)], 8, 32)),
    ('resident', dict(P=65537), _p(256, [(2, 1), (1, 255)], 1, 1)),
    ('resident', dict(P=65797), _p(256, [(2, 2), (1, 254)], 1, 5)),              # tiles 2048 .. 2056: the eight wavefronts of workgroup 0, one of workgroup 1
    ('resident', dict(P=131073), _p(256, [(3, 1), (2, 255)], 1, 1)),
    # roles: sets of 4 tiles, grid = min(nset, 256)
    ('roles', dict(P=127), _p(1, [(1, 1)], 4, 31)),
    ('roles', dict(P=128), _p(1, [(1, 1)], 4, 32)),
    ('roles', dict(P=129), _p(2, [(1, 2)], 1, 1)),
    ('roles', dict(P=32768), _p(256, [(1, 256)], 4, 32)),
    ('roles', dict(P=32769), _p(256, [(2, 1), (1, 255)], 1, 1)),
    ('roles', dict(P=32901), _p(256, [(2, 2), (1, 254)], 1, 5)),                 # 1029 tiles = 258 sets
    ('roles', dict(P=65537), _p(256, [(3, 1), (2, 255)], 1, 1)),                 # 2049 tiles = 513 sets
    ('roles', dict(P=47880), _p(256, [(2, 119), (1, 137)], 1, 8)),               # test_gpu_bottleneck.py's (20, 38, 63): 1497 tiles = 375 sets
    # halo kernels: 8 x 32 (stride 2: 4 x 32 output) tiles, grid = min(ntile, 256)
    ('halo', dict(B=1, H=1, W=1), _p(1, [(1, 1)], 1, 1)),
    ('halo', dict(B=1, H=8, W=32), _p(1, [(1, 1)], 1, 256)),
    ('halo', dict(B=1, H=9, W=33), _p(4, [(1, 4)], 4, 1)),
    ('halo', dict(B=1, H=64, W=1024), _p(256, [(1, 256)], 256, 256)),
    ('halo', dict(B=1, H=65, W=1024), _p(256, [(2, 32), (1, 224)], 32, 32)),     # 288 tiles, the last row of tiles one pixel thick
    ('halo', dict(B=1, H=57, W=1025), _p(256, [(2, 8), (1, 248)], 8, 1)),        # 8 x 33 = 264
    ('halo', dict(B=1, H=152, W=864), _p(256, [(3, 1), (2, 255)], 1, 256)),      # 19 x 27 = 513
    ('halo', dict(B=2, H=150, W=250), _p(256, [(2, 48), (1, 208)], 48, 156)),    # test_gpu_bottleneck.py's largest: 2 x 19 x 8 = 304 tiles
    ('halo_s2', dict(B=1, H=1, W=1), _p(1, [(1, 1)], 1, 1)),
    ('halo_s2', dict(B=1, H=7, W=63), _p(1, [(1, 1)], 1, 128)),
    ('halo_s2', dict(B=1, H=8, W=64), _p(1, [(1, 1)], 1, 128)),
    ('halo_s2', dict(B=1, H=9, W=65), _p(4, [(1, 4)], 4, 1)),
    ('halo_s2', dict(B=1, H=255, W=511), _p(256, [(1, 256)], 256, 128)),
    ('halo_s2', dict(B=1, H=263, W=511), _p(256, [(2, 8), (1, 248)], 8, 128)),   # 33 x 8 = 264
    ('halo_s2', dict(B=1, H=265, W=513), _p(256, [(2, 50), (1, 206)], 50, 1)),   # 34 x 9 = 306
    ('halo_s2', dict(B=2, H=265, W=513), _p(256, [(3, 100), (2, 156)], 100, 1)),     # 612
    ('halo_s2', dict(B=2, H=33, W=49), _p(10, [(1, 10)], 10, 25)),      # test_gpu_quarter_units.py's largest: 2 x 5 x 1 tiles, 1 x 25 live
]


@pytest.mark.parametrize('form,shape,want', HAND, ids=['%s-%s' % (f, '-'.join(str(v) for v in s.values())) for f, s, _ in HAND])
def test_plan_against_hand_computed_launches(form, shape, want):
    assert TC.plan(form, **shape) == want


@pytest.mark.parametrize('form', sorted(TC.FORMS))
def test_every_chain_form_keeps_a_case_in_every_edge_class(form):
    f = TC.FORMS[form]
    have = set()
    for case in TC.chain_cases(form):
        P = TC.case_pixels(form, case)
        assert P * 8 * f['mid'] < 1 << 32
        have |= TC.edge_classes(f['plan'], TC.plan(f['plan'], P))
    need = set(TC.SMALL_CLASSES + TC.TWO_ITER_CLASSES) | ({'three iterations'} if f['three'] else set())
    assert need <= have, (form, sorted(need - have))
    if f['mid'] >= 256 and not f['reduce']:
        assert 'three iterations' not in have                   # (gigabytes, and no state the second iteration has not seen)
    # the isolation case iterates, and the tile workgroup 0 takes second is neither its first nor the last one
    P = TC.case_pixels(form, TC.isolation_case(form))
    q = TC.second_iteration_pixel(f['plan'], P)
    assert max(TC.plan(f['plan'], P).iters) >= 2 and 32 < q < P - 32 and TC.isolation_case(form) in TC.chain_cases(form)


def test_gather_shapes():
    counts = [TC.compact_pixels(*s) for s in TC.GATHER_SHAPES]
    assert counts == [1, 24, 31, 32, 33, 70, 255, 256, 257, 65536, 65537, 66248, 87400, 131073]
    assert (2, 363, 363) in TC.GATHER_SHAPES and min(counts) < 32
    for mid in (64, 128):                                       # the full map is addressed with 32-bit byte offsets too
        assert all(B * H * W * 8 * mid < 1 << 32 for B, H, W in TC.GATHER_SHAPES)
    # an image boundary inside a tile and inside the first tile of workgroup 0's second iteration
    B, H, W = TC.GATHER_ISOLATION_SHAPE
    Ho, Wo = TC.out_hw(H, W)
    bounds = [b * Ho * Wo for b in range(1, B)]
    for form in ('resident', 'streamed'):
        q = TC.second_iteration_pixel(form, B * Ho * Wo)
        assert q == 65536 and any(q < e < q + 32 for e in bounds) and any(e % 32 and e < q for e in bounds)


@pytest.mark.parametrize('form,shapes', [('halo', TC.HALO_SHAPES), ('halo_s2', TC.HALO_S2_SHAPES)])
def test_both_halo_forms_keep_a_case_in_every_edge_class(form, shapes):
    have = set()
    for B, H, W in shapes:
        have |= TC.edge_classes(form, TC.plan(form, B=B, H=H, W=W))
    need = set(TC.HALO_CLASSES) - ({'two iterations, full last tile'} if form == 'halo' else set())      # (dense: 288 and 264 tiles, both ragged)
    assert need <= have, (form, sorted(need - have))


def test_stem_lattice_covers_both_sides_of_the_tile_edges():
    assert [TC.stem_hw(H, 7)[2] for H in TC.STEM_H] == [2, 2, 2, 2, 3, 9, 9, 10, 10]
    assert [TC.stem_hw(7, W)[3] for W in TC.STEM_W] == [2, 2, 15, 15, 15, 15, 16, 29, 29, 29, 30]
    assert 25 <= len(TC.STEM_SIZES) <= 30 and len(set(TC.STEM_SIZES)) == len(TC.STEM_SIZES)
    for corner in ((7, 7), (7, 117), (40, 7), (40, 117)):
        assert corner in TC.STEM_SIZES
    assert set(h for h, _ in TC.STEM_SIZES) == set(TC.STEM_H) and set(w for _, w in TC.STEM_SIZES) == set(TC.STEM_W)
    ty, tx = TC.STEM_TILE
    dims = [TC.stem_hw(H, W) for H, W in TC.STEM_SIZES]
    # one and two pooled rows in a second tile row; one and two pooled columns in a second and in a third tile column
    assert {1, 2} <= {Hp % ty for _, _, Hp, _ in dims if -(-Hp // ty) == 2}
    for cols in (2, 3):
        assert {1, 2} <= {Wp % tx for _, _, _, Wp in dims if -(-Wp // tx) == cols}, cols
    assert any(Hp < ty for _, _, Hp, _ in dims) and any(Wp < tx for _, _, _, Wp in dims)
    # every parity of the conv map, and the last pooling window both complete (2 (n - 1) + 3 == c) and clipped by one, in both directions
    assert {(Hc % 2, Wc % 2) for Hc, Wc, _, _ in dims} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(2 * Hp + 1 - Hc, 2 * Wp + 1 - Wc) for Hc, Wc, Hp, Wp in dims} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for (H, W), (Hc, Wc, Hp, Wp) in zip(TC.STEM_SIZES, dims):   # the size formulas are those of the reference's operators
        y = F.max_pool2d(F.conv2d(torch.zeros(1, 3, H, W), torch.zeros(1, 3, 7, 7), stride=2, padding=3), 3, 2, ceil_mode=True)
        assert tuple(y.shape[2:]) == (Hp, Wp)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the acceptance at the small cases: a plain fp32 evaluation passes, a moved value does not
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _bf(t):
    return t.float().to(BF16)


def _two_steps(t, i):
    """Element i (flat) of a bf16 tensor moved up by two steps of its own exponent."""
    out = t.clone()
    v = out.view(-1)[i].float()
    out.view(-1)[i] = v + 2 * TC.step(v.double()).float() * 1.0001
    assert out.view(-1)[i] != t.view(-1)[i]
    return out


def _swap_rows(t, i, j):
    out = t.clone()
    out[i], out[j] = t[j], t[i]
    return out


@pytest.mark.parametrize('form', TC.DENSE_FORMS)
def test_chain_acceptance_at_the_small_cases(form):
    f = TC.FORMS[form]
    mid = f['mid']
    w = TC.chain_weights(mid, 'cpu')
    for P in [p for p in f['P'] if p <= 257]:
        o = TC.chain_operands(form, P, 'cpu')
        sc = o['xin'] if f['proj'] else o['x']
        # fp32: torch matmul on the bf16 operands, bias and shortcut added in fp32, one rounding to bf16
        acc = o['m2'].float() @ w['w3'].float().t()
        acc = acc + (w['b3p'] + sc.float() @ w['wp'].float().t() if f['proj'] else w['b3'] + sc.float())
        xn = _bf(acc.clamp_min(0))
        m1 = _bf((xn.float() @ w['w1'].float().t() + w['b1']).clamp_min(0)) if f['reduce'] else None
        okx, wx, okm, wm = TC.accept_chain(form, w, o['m2'], sc, xn, m1, chunk=100)
        pre, mag = TC.chain_ref(o['m2'], w['w3'], w['b3p'] if f['proj'] else w['b3'], **(dict(xin=sc, wp=w['wp']) if f['proj'] else dict(x=sc)))
        share = TC.bound_share(xn, pre.clamp_min(0), mag, 2 * mid if f['proj'] else mid)
        print('%-5s P = %3d: fp32 evaluation, worst err / tolerance  x_next %.4f  mid1 %.4f; x_next beyond its bf16 rounding: %.4f of the bound'
              % (form, P, wx, wm, share))
        assert share <= 0.5, (form, P, share)                  # headroom: a correct evaluation stays in the lower half of the bound
        assert okx and okm and wx <= 1.0 and wm <= 1.0, (form, P, wx, wm)
        # one element moved by two bf16 steps
        i = int(xn.float().argmax())
        assert not TC.accept_chain(form, w, o['m2'], sc, _two_steps(xn, i), None)[0], (form, P)
        if m1 is not None:
            j = int(m1.float().argmax())
            assert m1.view(-1)[j] > 0 and not TC.accept_chain(form, w, o['m2'], sc, xn, _two_steps(m1, j))[2], (form, P)
        # two pixels swapped (mid1' is held to the x_next handed in, so its rows are swapped alone)
        if P > 1:
            a, b = P // 2, P - 1
            assert not TC.accept_chain(form, w, o['m2'], sc, _swap_rows(xn, a, b), None)[0], (form, P)
            if m1 is not None:
                assert not TC.accept_chain(form, w, o['m2'], sc, xn, _swap_rows(m1, a, b))[2], (form, P)
        bad = xn.clone()                                        # NaN: an operand read outside its view
        bad[P - 1, 0] = float('nan')
        assert not TC.accept_chain(form, w, o['m2'], sc, bad, None)[0]


@pytest.mark.parametrize('form', TC.GATHER_FORMS)
def test_gather_operands_and_reference_at_the_small_cases(form):
    f = TC.FORMS[form]
    w = TC.chain_weights(f['mid'], 'cpu')
    for shape in [s for s in TC.GATHER_SHAPES if TC.compact_pixels(*s) <= 257]:
        o = TC.chain_operands(form, shape, 'cpu')
        P = TC.compact_pixels(*shape)
        m2 = o['m2'].reshape(P, -1)
        xe = o['x'][:, ::2, ::2].reshape(P, -1)
        assert o['m2'].shape[:3] == o['x'][:, ::2, ::2].shape[:3]
        xn = _bf((m2.float() @ w['w3'].float().t() + w['b3'] + xe.float()).clamp_min(0))
        okx, wx, _, _ = TC.accept_chain(form, w, m2, xe, xn, None)
        assert okx and wx <= 1.0, (form, shape, wx)
        if P > 1:                                               # the shortcut of the next pixel of the full map (an odd one): rejected
            wrong = torch.roll(o['x'], -1, dims=2 if shape[2] > 1 else 1)[:, ::2, ::2].reshape(P, -1)
            bad = _bf((m2.float() @ w['w3'].float().t() + w['b3'] + wrong.float()).clamp_min(0))
            assert not TC.accept_chain(form, w, m2, xe, bad, None)[0], (form, shape)


@pytest.mark.parametrize('shape', TC.HALO_SMALL, ids=['%dx%dx%d' % s for s in TC.HALO_SMALL])
def test_halo_acceptance_at_the_small_cases(shape):
    x, w, b = TC.halo_operands(shape, 'cpu')
    for stride in (1, 2):
        pre, mag = TC.halo_ref(x, w, b, stride)
        assert tuple(pre.shape[1:3]) == ((shape[1], shape[2]) if stride == 1 else TC.out_hw(shape[1], shape[2]))
        y32 = F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), b, stride=stride, padding=1).permute(0, 2, 3, 1).contiguous()
        for relu in (True, False):
            want = pre.clamp_min(0) if relu else pre
            got = _bf(y32.clamp_min(0) if relu else y32)
            ok, worst = TC.accept(got, want, pre, mag, 576, bf16_out=True, relu=relu)
            share = TC.bound_share(got, want, mag, 576)
            print('%s stride %d relu %d: fp32 evaluation, worst err / tolerance %.4f; beyond the bf16 rounding: %.4f of the bound'
                  % (shape, stride, relu, worst, share))
            assert share <= 0.5, (shape, stride, relu, share)
            assert ok and worst <= 1.0, (shape, stride, relu, worst)
            i = int(got.float().abs().argmax())
            assert not TC.accept(_two_steps(got, i), want, pre, mag, 576, bf16_out=True, relu=relu)[0]
            flat = got.reshape(-1, 64)
            if flat.shape[0] > 1:
                sw = _swap_rows(flat, 0, flat.shape[0] - 1).reshape(got.shape)
                assert not TC.accept(sw, want, pre, mag, 576, bf16_out=True, relu=relu)[0]


@pytest.mark.parametrize('size', TC.STEM_SMALL, ids=['%dx%d' % s for s in TC.STEM_SMALL])
def test_stem_acceptance_at_the_small_cases(size):
    img, u8, w, b = TC.stem_operands(size, 'cpu')
    img, w = _bf(img).float(), _bf(w).float()
    want, tol = TC.stem_ref(img, w, b)
    Hc, Wc, Hp, Wp = TC.stem_hw(*size)
    assert tuple(want.shape) == (2, Hp, Wp, 64) and bool((tol > 0).all())
    conv = _bf(F.conv2d(img, w, b, stride=2, padding=3).clamp_min(0))
    assert tuple(conv.shape[2:]) == (Hc, Wc)
    got = F.max_pool2d(conv.float(), 3, 2, ceil_mode=True).permute(0, 2, 3, 1).contiguous().to(BF16)
    ok, worst = TC.stem_accept(got, want, tol)
    print('%s: fp32 evaluation, worst err / tolerance %.4f' % (size, worst))
    assert ok and worst <= 1.0, (size, worst)
    i = int(got.float().argmax())
    assert not TC.stem_accept(_two_steps(got, i), want, tol)[0]
    flat = got.reshape(-1, 64)
    sw = _swap_rows(flat, 0, flat.shape[0] - 1).reshape(got.shape)
    assert not TC.stem_accept(sw, want, tol)[0]


def test_guards_find_a_store_one_tile_off():
    """A row-masked store that is one 32-pixel tile off lands in the guard, and the guard finds it."""
    for C in (64, 2048):
        g = TC.guarded((33, C), BF16, device='cpu')
        g.view.zero_()
        assert TC.guards_intact(g.buf, g.view) and TC.is_pattern_free(g.view)
        first = g.view.storage_offset()
        for p in (first + 33 * C, first + (33 + 31) * C + C - 1, first - 1, first - 32 * C):
            keep = g.buf[p].clone()
            g.buf[p] = 0.0
            assert not TC.guards_intact(g.buf, g.view)
            g.buf[p] = keep
        assert TC.guards_intact(g.buf, g.view)
        g.view[32, C - 1] = float('nan')
        TC.fill_pattern(g.view[32:33])
        assert not TC.is_pattern_free(g.view)
