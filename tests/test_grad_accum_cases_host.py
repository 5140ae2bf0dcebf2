"""CPU-side checks of tests/grad_accum_cases.py (no GPU, no library).  Per kernel family (wgrad, colsum, roi pooling backward, strided scatter):
  * the case tables hold the shapes, paths and edges they are meant to hold (what the GPU file runs is what the tables say);
  * the float64 reference equals an independent statement of the same definition (conv2d autograd, a loop) to 1e-12;
  * the float32 emulation in two summation orders stays at or under HALF of the bound the GPU result is held to, on every case;
  * each named mutant exceeds the bound at the cases named for it, with the operands (seeds) the GPU test uses."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_accum_cases as AC  # noqa: E402

F64 = torch.float64
_ids = lambda cases: [c['id'] for c in cases]
_CACHE = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# wgrad
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _wg(case):
    def make():
        o = AC.wgrad_operands(case)
        return (o,) + AC.wgrad_ref64(case, o)
    return _memo(('wg', case['id']), make)


def test_wgrad_table_holds_the_geometries_tiles_and_views_of_the_issue():
    cs = AC.WGRAD_CASES
    conv = {(c['B'], c['H'], c['W'], c['ks'], c['stride'], c['dil'], c['pad']) for c in cs if c['conv']}
    assert conv >= {(1, 5, 63, 3, 1, 1, 1), (2, 3, 64, 3, 1, 1, 1), (1, 3, 65, 3, 1, 1, 1), (1, 2, 125, 3, 1, 1, 1), (1, 2, 130, 3, 1, 1, 1),
                    (9, 3, 5, 3, 1, 1, 1), (5, 2, 3, 3, 1, 1, 1), (70, 1, 1, 3, 1, 1, 1), (3, 1, 9, 3, 1, 1, 1),
                    (2, 2, 3, 3, 1, 2, 2), (2, 14, 17, 3, 1, 2, 2), (2, 9, 13, 1, 2, 1, 0), (2, 8, 12, 1, 2, 1, 0), (1, 11, 70, 7, 2, 1, 3)}
    assert all(c['Cin'] in (8, 16) for c in cs if c['conv'])
    assert all(c['holes'] for c in cs if c['conv'] and c['ks'] == 1) and [c['Cin'] for c in cs if c['ks'] == 7] == [8]
    assert {c['Wout'] for c in cs if c['conv']} >= {63, 64, 65, 125, 130, 1}
    assert {c['P'] for c in cs if not c['conv']} >= {1, 63, 64, 65, 127, 128, 129}
    assert {c['Cout'] for c in cs} >= {8, 64, 72, 128, 136, 256, 264} and {c['K'] for c in cs} >= {8, 72, 248, 256, 264}
    for key in ('xpad', 'dypad', 'dyzero', 'scale'):
        assert {bool(c[key]) for c in cs} == {False, True}, key
        assert {bool(c[key]) for c in cs if c['conv']} == {False, True}, key
    assert all(c['xpad'] % 8 == 0 and c['dypad'] % 8 == 0 and c['dyzero'] % 8 == 0 and c['Cin'] % 8 == 0 and c['Cout'] % 8 == 0 for c in cs)
    grp = [AC.WGRAD_BY_ID[i] for i in AC.WGRAD_GROUPS['MIX']]
    assert {8, 264} <= {c['Cout'] for c in grp} and AC.wgrad_tile_rows(grp) == 256
    # every mutant case exists, and the pixel-walk mutant sits where the walk matters
    for m, ids in AC.WGRAD_MUTANTS.items():
        assert all(i in AC.WGRAD_BY_ID for i in ids), m
    assert all(AC.WGRAD_BY_ID[i]['Wout'] >= 64 for i in AC.WGRAD_MUTANTS['walk_row_off'])


def test_wgrad_share_cuts_cover_every_unit_boundary():
    """The grids of wgrad_grids place a share boundary at every (tile, slab) unit boundary of every few-unit case, and some of them inside a tile
    (between two slabs), some between tiles and, in the grouped launch, between layers."""
    inside = between = 0
    for c in AC.WGRAD_CASES:
        units = AC.wgrad_units(c)
        assert units <= AC.WGRAD_FEW_UNITS, (c['id'], units)
        cuts = set()
        for g in AC.wgrad_grids(units):
            cuts |= AC.share_cuts(units, g)
        assert cuts == set(range(1, units)), (c['id'], units, sorted(cuts))
        inside += sum(1 for u in cuts if u % c['slabs'])
        between += sum(1 for u in cuts if u % c['slabs'] == 0)
        assert units in AC.wgrad_grids(units) and units + 5 in AC.wgrad_grids(units) and 1 in AC.wgrad_grids(units)
    assert inside > 20 and between >= 4
    grp = [AC.WGRAD_BY_ID[i] for i in AC.WGRAD_GROUPS['MIX']]
    units = [AC.wgrad_units(c, 256) for c in grp]
    total = sum(units)
    cuts = set()
    for g in AC.wgrad_grids(total):
        cuts |= AC.share_cuts(total, g)
    assert cuts == set(range(1, total))


@pytest.mark.parametrize('case', AC.WGRAD_CASES, ids=_ids(AC.WGRAD_CASES))
def test_wgrad_reference_is_conv2d_autograd_and_the_emulations_halve_the_bound(case):
    o, ref, mag = _wg(case)
    assert torch.isfinite(ref).all() and torch.isfinite(mag).all()                  # the NaN holes are never read
    x, dy = o['x'].double(), o['dy'].double()
    s2 = 1.0 if o['scale'] is None else o['scale'].double()[:, None] ** 2
    if case['conv']:
        x = torch.nan_to_num(x, nan=0.0) if case['holes'] else x
        if case['holes']:                                                           # zeroing the holes must not matter: read them back as huge
            big = torch.where(torch.isnan(o['x']), torch.full_like(o['x'], 1e30), o['x']).double()
            assert torch.equal(AC.wgrad_patches(case, big), AC.wgrad_patches(case, x))
        w = torch.zeros(case['Cout'], case['Cin'], case['ks'], case['ks'], dtype=F64, requires_grad=True)
        y = F.conv2d(x.permute(0, 3, 1, 2), w, None, stride=case['stride'], padding=case['pad'], dilation=case['dil'])
        assert tuple(y.shape) == (case['B'], case['Cout'], case['Hout'], case['Wout'])
        (y * dy.view(case['B'], case['Hout'], case['Wout'], case['Cout']).permute(0, 3, 1, 2)).sum().backward()
        want = w.grad.permute(0, 2, 3, 1).reshape(case['Cout'], -1)                 # pack_conv_weight order
    else:
        want = dy.t() @ x
    assert _rel(ref, o['old'].double() + s2 * want) <= 1e-12
    bound = AC.wgrad_bound(case, mag)
    for order in ('ascending', 'slabs'):
        assert AC.worst(AC.wgrad_emulate32(case, o, order), ref, bound) <= 0.5, order


@pytest.mark.parametrize('mutant,cid', [(m, i) for m, ids in sorted(AC.WGRAD_MUTANTS.items()) for i in ids])
def test_wgrad_mutants_exceed_the_bound(mutant, cid):
    case = AC.WGRAD_BY_ID[cid]
    o, ref, mag = _wg(case)
    bad, _ = AC.wgrad_ref64(case, o, mutant)
    assert AC.worst(bad, ref, AC.wgrad_bound(case, mag)) > 1.0


def test_wgrad_pixel_walk_equals_plain_division():
    """The kernel's walk (divide once per share, then + 64 pixels per slab with adds, compares and a carry loop) restated on the host gives the
    (image, y, x) of plain division for every thread row of every slab of every conv case, from every first slab a share can start at."""
    for c in AC.WGRAD_CASES:
        if not c['conv']:
            continue
        Ho, Wo, P = c['Hout'], c['Wout'], c['P']
        step_y, step_x = AC.SLAB // Wo, AC.SLAB - (AC.SLAB // Wo) * Wo
        for s0 in range(c['slabs']):
            for row in range(AC.SLAB):
                p = s0 * AC.SLAB + row
                img, rem = divmod(p, Ho * Wo)
                y, x = divmod(rem, Wo)
                for s in range(s0, c['slabs']):
                    q = s * AC.SLAB + row
                    if q < P:
                        assert (img, y, x) == (q // (Ho * Wo), (q % (Ho * Wo)) // Wo, q % Wo), (c['id'], s0, s, row)
                    y, x = y + step_y, x + step_x
                    if x >= Wo:
                        x -= Wo
                        y += 1
                    while y >= Ho:
                        y -= Ho
                        img += 1


# ---------------------------------------------------------------------------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _csum(case):
    def make():
        x, old = AC.colsum_operands(case['id'], case['rows'], case['cols'], case['dtype'])
        return (x, old) + AC.colsum_ref64(x, old)
    return _memo(('cs', case['id']), make)


def test_colsum_table_holds_every_row_and_column_count_on_every_path():
    cs = AC.COLSUM_CASES
    assert len({c['id'] for c in cs}) == len(cs)
    for path, (cols, lanes) in AC.COLSUM_PATHS.items():
        mine = [c for c in cs if c['path'] == path]
        assert {c['rows'] for c in mine} == set(AC.COLSUM_ROWS), path
        assert {c['cols'] for c in mine} == set(cols), path
        assert {c['ld'] > c['cols'] for c in mine} >= {True}, path
    assert set(AC.COLSUM_PATHS['bf16x8'][0]) | set(AC.COLSUM_PATHS['bf16w'][0]) == set(AC.COLSUM_COLS)
    for c in cs:                                                 # the path the entry point takes is the one the case is named for
        x8 = c['dtype'] == AC.BF16 and c['cols'] % 8 == 0 and c['ld'] % 8 == 0 and c['offset'] == 0
        assert x8 == (c['path'] == 'bf16x8'), c['id']
        assert c['ld'] >= c['cols'] and c['lanes'] == (8 if x8 else 4)
    assert any(c['ld'] % 8 for c in cs if c['path'] == 'bf16ld') and all(c['ld'] % 8 == 0 and c['offset'] == 1 for c in cs if c['path'] == 'bf16off')
    # chunking: 1 chunk up to 512 rows, 2 at 513, 3 at 1025, the cap of 128 at 65536 (512 rows each) and 65537 (513 rows each: 128 chunks in the grid)
    plan = {r: AC.colsum_plan(r, 4)[:3] for r in AC.COLSUM_ROWS}
    assert plan[511] == (1, 511, 1) and plan[512] == (1, 512, 1) and plan[513] == (2, 257, 2) and plan[1025] == (3, 342, 3)
    assert plan[65536] == (128, 512, 128) and plan[65537] == (128, 513, 128)
    assert any(c['rows'] >= 65536 and c['cols'] > 64 for c in cs if c['path'] == 'f32')          # the cap with more than one column block
    assert any(c['rows'] >= 65536 and c['cols'] > 256 for c in cs if c['path'] == 'bf16x8')
    for m, ids in AC.COLSUM_MUTANTS.items():
        assert all(i in AC.COLSUM_BY_ID for i in ids), (m, [i for i in ids if i not in AC.COLSUM_BY_ID])
    q = AC.COLSUM_QUEUES
    assert [len(q[k]) for k in ('Q1', 'Q16', 'Q17')] == [1, 16, 17]
    blocks = lambda r, c: AC.colsum_plan(r, 8)[2] * -(-(c // 8) // 32)
    for k in ('Q16', 'Q17'):
        p = q[k]
        assert any(p[i][:2] == (1, 8) and blocks(*p[i - 1][:2]) > 1 and blocks(*p[i + 1][:2]) > 1 for i in range(1, len(p) - 1)), k
    assert all(c % 8 == 0 and pad % 8 == 0 for p in q.values() for _, c, pad in p)


@pytest.mark.parametrize('case', AC.COLSUM_CASES, ids=_ids(AC.COLSUM_CASES))
def test_colsum_emulations_halve_the_bound(case):
    x, old, ref, mag = _csum(case)
    want = old.double().clone()
    for r in range(0, case['rows'], 4096):                       # an independent statement: block-wise float64 sums
        want += x[r:r + 4096].double().sum(0)
    assert _rel(ref, want) <= 1e-12
    bound = AC.colsum_bound(case['rows'], case['lanes'], mag)
    for order in ('ascending', 'chunks'):
        assert AC.worst(AC.colsum_emulate32(x, old, case['lanes'], order), ref, bound) <= 0.5, order


@pytest.mark.parametrize('qid', sorted(AC.COLSUM_QUEUES))
def test_colsum_queue_emulations_halve_the_bound(qid):
    operands = AC.colsum_queue_operands(qid)
    for (x, old), (ref, mag) in zip(operands, AC.colsum_queue_ref64(qid, operands)):
        bound = AC.colsum_bound(x.shape[0], 8, mag)
        for order in ('ascending', 'chunks'):
            assert AC.worst(AC.colsum_emulate32(x, old, 8, order), ref, bound) <= 0.5, (tuple(x.shape), order)


@pytest.mark.parametrize('mutant,cid', [(m, i) for m, ids in sorted(AC.COLSUM_MUTANTS.items()) for i in ids])
def test_colsum_mutants_exceed_the_bound(mutant, cid):
    case = AC.COLSUM_BY_ID[cid]
    x, old, ref, mag = _csum(case)
    bad, _ = AC.colsum_ref64(x, old, mutant, case['lanes'])
    assert AC.worst(bad, ref, AC.colsum_bound(case['rows'], case['lanes'], mag)) > 1.0


@pytest.mark.parametrize('mutant,qid', [(m, i) for m, ids in sorted(AC.COLSUM_QUEUE_MUTANTS.items()) for i in ids])
def test_colsum_queue_mutants_exceed_the_bound(mutant, qid):
    operands = AC.colsum_queue_operands(qid)
    good = AC.colsum_queue_ref64(qid, operands)
    bad = AC.colsum_queue_ref64(qid, operands, mutant)
    over = [AC.worst(b, r, AC.colsum_bound(x.shape[0], 8, m)) > 1.0 for (x, _), (r, m), (b, _) in zip(operands, good, bad)]
    assert any(over)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# roi pooling backward
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _roi(case):
    def make():
        o = AC.roi_operands(case)
        return o, AC.roi_ref64(case, o)
    return _memo(('roi', case['id']), make)


def _own_pairs(case, o):
    """(roi, bin) pairs of image 0 per list segment."""
    img = o['rois'][:, 0].long() - case['base']
    bins = case['PH'] * case['PW']
    return [int((img[b:b + AC.OWNER_LIST] == 0).sum()) * bins for b in range(0, case['R'], AC.OWNER_LIST)]


def test_roi_table_holds_the_segments_pair_counts_and_forms_of_the_issue():
    by = AC.ROI_BY_ID
    own = [c for c in AC.ROI_CASES if c['owner']]
    assert {c['R'] for c in own} >= {1023, 1024, 1025, 2049}
    assert all(c['B'] * c['C'] // 8 >= 256 for c in own)
    assert {(c['B'], c['C']) for c in own} >= {(29, 72), (256, 8), (8, 256)}
    assert {c['dtype'] for c in own} == {AC.F32, AC.BF16} and {c['base'] for c in own} == {0, 3}
    assert by['M4608']['owner'] and not by['M4609']['owner']
    assert by['M4608']['levels'] == [(64, 72)] and 64 * 72 == AC.OWNER_MAX_CELLS and by['M4609']['levels'] == [(11, 419)]
    assert {c['form'] for c in AC.ROI_CASES} == {'cl', 'nchw', 'nhwc', 'fpn'}
    assert any(c['form'] == 'cl' and not c['owner'] and c['levels'][0][0] * c['levels'][0][1] <= AC.OWNER_MAX_CELLS for c in AC.ROI_CASES)
    nps = {}
    for c in own:
        o, _ = _roi(c)
        nps[c['id']] = _own_pairs(c, o)
        a, img = o['argmax'], o['rois'][:, 0].long() - c['base']
        assert int(a.min()) == -1 and int(a.max()) < c['levels'][0][0] * c['levels'][0][1]
        assert int(img.min()) >= 0 and int(img.max()) < c['B']                        # batch indices inside [0, B) only
        assert bool((a.reshape(c['R'], -1) < 0).all(1).any())                         # rois without a valid bin
    assert [nps[i][0] for i in ('P256', 'P257', 'P512', 'P513')] == [1024, 1028, 2048, 2052]
    assert [nps[i][0] for i in ('P20', 'P21', 'P42')] == [980, 1029, 2058]
    g = nps['R2049g']
    assert len(g) == 3 and g[0] > 0 and g[1] == 0 and g[2] > 0                        # a list segment with none of image 0's rois
    # the odd tail: everything at np <= 1024, four pairs short of everything at 1028, nothing at 2048, the last four at 2052
    assert int(AC.owner_tail_mask(1024).sum()) == 1024 and int(AC.owner_tail_mask(1028).sum()) == 1020
    assert int(AC.owner_tail_mask(2048).sum()) == 0 and AC.owner_tail_mask(2052).nonzero().view(-1).tolist() == [2048, 2049, 2050, 2051]
    for c in AC.ROI_CASES:                                                            # every case: in-range operands
        o, _ = _roi(c)
        img = o['rois'][:, 0].long() - c['base']
        assert int(img.min()) >= 0 and int(img.max()) < c['B'] and int(o['argmax'].min()) >= -1
        if c['hot']:
            assert int((img == 0).sum()) >= 2
    for m, ids in AC.ROI_MUTANTS.items():
        assert all(i in by for i in ids), m


@pytest.mark.parametrize('case', AC.ROI_CASES, ids=_ids(AC.ROI_CASES))
def test_roi_reference_is_the_loop_definition_and_the_emulations_halve_the_bound(case):
    o, refs = _roi(case)
    # the definition as a loop, on a sample of rois (all of them where the operands are small)
    R, C = case['R'], case['C']
    img = (o['rois'][:, 0].long() - case['base']).tolist()
    lv = [0] * R if o['level'] is None else o['level'].tolist()
    pick = range(0, R, -(-o['argmax'].numel() // 40000))
    part = [torch.zeros_like(r[0]) for r in refs]
    a, g = o['argmax'].reshape(R, -1, C), o['gout'].reshape(R, -1, C).double()
    for r in pick:
        for k in range(a.shape[1]):
            for c in range(C):
                if a[r, k, c] >= 0:
                    part[lv[r]][img[r], c, a[r, k, c]] += g[r, k, c]
    sub = dict(o, gout=torch.zeros_like(o['gout']))
    sub['gout'][list(pick)] = o['gout'][list(pick)]
    for (ref, _, _), want in zip(AC.roi_ref64(case, sub), part):
        assert _rel(ref, want) <= 1e-12
    hot = max(float(cnt.max()) for _, _, cnt in refs)
    if case['hot']:
        assert hot >= 2 * case['PH'] * case['PW']                                     # many rois, every bin, one cell
    for order in ('ascending', 'strided'):
        emu = AC.roi_emulate32(case, o, order)
        for (ref, mag, cnt), e in zip(refs, emu):
            assert AC.worst(e, ref, AC.roi_bound(mag, cnt, owner=False)) <= 0.5, order
            assert bool((e[cnt == 0] == 0).all())


@pytest.mark.parametrize('mutant,cid', [(m, i) for m, ids in sorted(AC.ROI_MUTANTS.items()) for i in ids])
def test_roi_mutants_exceed_the_bound(mutant, cid):
    case = AC.ROI_BY_ID[cid]
    o, refs = _roi(case)
    bad = AC.roi_ref64(case, o, mutant)
    assert any(AC.worst(b[0], ref, AC.roi_bound(mag, cnt, owner=True)) > 1.0 for (ref, mag, cnt), b in zip(refs, bad))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# strided scatter
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_scatter_table_and_reference():
    cs = AC.SCATTER_CASES
    assert any(c['H'] == 1 for c in cs) and any(c['W'] == 1 for c in cs) and any(c['H'] == 1 and c['W'] == 1 for c in cs)
    assert {c['H'] % 2 for c in cs} == {0, 1} and {c['W'] % 2 for c in cs} == {0, 1}
    assert {(c['dtype'], c['C']) for c in cs} >= {(AC.BF16, 8), (AC.F32, 4)} and {c['mask'] for c in cs} == {False, True}
    for c in cs:
        low, mask = AC.scatter_operands(c)
        s = c['stride']
        assert tuple(low.shape) == (c['B'], (c['H'] - 1) // s + 1, (c['W'] - 1) // s + 1, c['C'])
        ref = AC.scatter_ref(c, low, mask)
        lb, rb = AC.bits(low), AC.bits(ref)
        if mask is not None and mask.numel() >= 64:
            m = mask.float()
            assert bool(torch.isnan(m).any()) and bool(((m == 0) & torch.signbit(m)).any()) and bool((m > 0).any()) and bool((m < 0).any())
        for b in range(c['B']):                                   # the definition as a loop, on bits
            for h in range(c['H']):
                for w in range(c['W']):
                    for ch in range(c['C']):
                        want = 0
                        if h % s == 0 and w % s == 0 and (mask is None or float(mask[b, h, w, ch]) > 0):
                            want = int(lb[b, h // s, w // s, ch])
                        assert int(rb[b, h, w, ch]) == want
