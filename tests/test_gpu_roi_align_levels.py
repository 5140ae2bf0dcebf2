"""ROIAlign over several maps (relnet_roi_align_levels_fwd / _bwd, ops.roi_align_fpn / roi_align_fpn_bwd): per level bit-identical to
oracle/roi_align.py and to the single-map ops.roi_align; invalid rows (batch index or level out of range) give zeros and no gradient and
touch nothing outside the buffers; no 65 535 limit on the roi count; the separable-patch backward is the adjoint of the forward and equals
float64 autograd of the definition."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cases  # noqa: E402
from oracle import roi_align as ORA  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = (1 / 4.0, 1 / 8.0, 1 / 16.0, 1 / 32.0)


def _ops():
    import relnet_amd  # noqa: F401
    from relnet_amd import ops
    return ops


def _pyramid(B, C, H, W, seed, dtype=np.float32):
    """Four maps of an H x W image at strides 4 .. 32."""
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 1, (B, C, H // s, W // s)).astype(dtype) for s in (4, 8, 16, 32)]


def _rois(n, seed, B, im_h, im_w, max_size=200):
    b = cases.random_boxes(n, seed, im_h, im_w, min_size=4, max_size=max_size)
    rng = np.random.default_rng(seed)
    r = np.hstack([rng.integers(0, B, (n, 1)).astype(np.float32), b]).astype(np.float32)
    r[0] = [0, -20.0, -30.0, 50.0, 40.0]                                # out of the map at the top left
    r[1] = [B - 1, im_w - 30.0, im_h - 20.0, im_w + 60.0, im_h + 50.0]  # ... and at the bottom right
    r[2] = [0, 40.0, 40.0, 40.3, 40.3]                                  # degenerate: smaller than one cell
    r[3] = [B - 1, 0.0, 0.0, im_w - 1.0, im_h - 1.0]                    # the whole image: larger than the coarse maps' footprint bound
    r[4] = [0, 12.0, 30.0, 12.0, 30.0]                                  # zero extent
    return r


def sample_matrix(rois, level, shapes, scales, pooled=(7, 7), sampling_ratio=2, aligned=False):
    """Sparse float64 [R*PH*PW, sum_l B*H_l*W_l] matrix of the definition (oracle sample positions, float64 bilinear weights, 1/count):
    pooled = M @ concat_l(x_l as [B*H_l*W_l, C]).  Rows with an invalid batch index or level stay empty."""
    PH, PW = pooled
    rois = np.asarray(rois, np.float32)
    level = np.zeros(len(rois), np.int64) if level is None else np.asarray(level)
    offs = np.cumsum([0] + [b * h * w for (b, _, h, w) in shapes])
    rows, cols, vals = [], [], []
    for l, (B, _, H, W) in enumerate(shapes):
        sel = np.where((level == l) & (rois[:, 0] >= 0) & (rois[:, 0] < B))[0]
        if not len(sel):
            continue
        _, samples = ORA.roi_align(np.zeros((B, 1, H, W)), rois[sel], pooled, scales[l], sampling_ratio, aligned, dtype=np.float64,
                                   return_samples=True)
        count = {}
        for (r, ph, pw, _, _) in samples:
            count[(r, ph, pw)] = count.get((r, ph, pw), 0) + 1
        for (r, ph, pw, yy, xx) in samples:
            k = ORA._corners(np.float64(yy), np.float64(xx), H, W, np.float64)
            if k is None:
                continue
            yl, xl, yh, xh, w1, w2, w3, w4 = k
            row = (sel[r] * PH + ph) * PW + pw
            b = int(rois[sel[r], 0])
            for (y, x, w) in ((yl, xl, w1), (yl, xh, w2), (yh, xl, w3), (yh, xh, w4)):
                rows.append(row); cols.append(offs[l] + (b * H + y) * W + x); vals.append(float(w) / count[(r, ph, pw)])
    return torch.sparse_coo_tensor(torch.tensor([rows, cols], dtype=torch.int64), torch.tensor(vals, dtype=torch.float64),
                                   (len(rois) * PH * PW, int(offs[-1]))).coalesce()


def _flat(xs):
    """[B,C,H,W] maps -> [sum B*H*W, C] rows in sample_matrix's column order."""
    return torch.cat([x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) for x in xs], 0)


@pytest.mark.parametrize('sampling_ratio,aligned', [(2, False), (0, False), (2, True), (0, True)])
def test_levels_float32_is_the_oracle_bit_for_bit(sampling_ratio, aligned):
    ops = _ops()
    B, C, IH, IW = 2, 16, 160, 224
    xs = _pyramid(B, C, IH, IW, 3)
    rois = _rois(48, 4, B, IH, IW)
    level = np.random.default_rng(5).integers(0, 4, len(rois)).astype(np.int32)
    level[:5] = [0, 1, 2, 3, 3]
    xd = [torch.as_tensor(x).cuda() for x in xs]
    got = ops.roi_align_fpn(xd, SCALES, torch.as_tensor(rois).cuda(), torch.as_tensor(level).cuda(), (7, 7), sampling_ratio, aligned)
    got = got.cpu().numpy()
    for l in range(4):
        sel = np.where(level == l)[0]
        want = ORA.roi_align(xs[l], rois[sel], (7, 7), SCALES[l], sampling_ratio, aligned)
        assert np.array_equal(got[sel], want), l
    # one level, no level table: the single-map operator, bit for bit
    one = ops.roi_align_fpn([xd[2]], [SCALES[2]], torch.as_tensor(rois).cuda(), None, (7, 7), sampling_ratio, aligned)
    ref = ops.roi_align(xd[2], torch.as_tensor(rois).cuda(), (7, 7), SCALES[2], sampling_ratio, aligned)
    assert torch.equal(one, ref)


@pytest.mark.parametrize('sampling_ratio', [2, 0])
def test_levels_bf16_channels_last_equals_roi_align_per_level(sampling_ratio):
    ops = _ops()
    B, C, IH, IW = 2, 64, 160, 224
    xd = [torch.as_tensor(x).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last) for x in _pyramid(B, C, IH, IW, 7)]
    rois = torch.as_tensor(_rois(80, 8, B, IH, IW)).cuda()
    level = torch.as_tensor(np.random.default_rng(9).integers(0, 4, 80).astype(np.int32)).cuda()
    got = ops.roi_align_fpn(xd, SCALES, rois, level, (7, 7), sampling_ratio, channels_last_out=True)
    assert got.permute(0, 2, 3, 1).is_contiguous()
    for l in range(4):
        sel = torch.nonzero(level == l).view(-1)
        want = ops.roi_align(xd[l], rois[sel].contiguous(), (7, 7), SCALES[l], sampling_ratio, channels_last_out=True)
        assert torch.equal(got[sel], want), l
    one = ops.roi_align_fpn([xd[0]], [SCALES[0]], rois, None, (7, 7), sampling_ratio, channels_last_out=True)
    assert torch.equal(one, ops.roi_align(xd[0], rois, (7, 7), SCALES[0], sampling_ratio, channels_last_out=True))


def _carve(n, fill, dtype, guard=4096):
    """A length-n view in the middle of a buffer whose guard regions hold `fill`."""
    buf = torch.full((n + 2 * guard,), fill, dtype=dtype, device='cuda')
    return buf, buf[guard:guard + n]


@pytest.mark.parametrize('dtype,layout', [(torch.float32, 'nchw'), (torch.bfloat16, 'nhwc')])
def test_invalid_rows_pool_to_zeros_and_touch_nothing_else(dtype, layout):
    ops = _ops()
    from relnet_amd import lib
    B, C, IH, IW = 2, 16, 128, 160
    xs = [torch.as_tensor(x).cuda().to(dtype) for x in _pyramid(B, C, IH, IW, 11)]
    if layout == 'nhwc':
        xs = [x.contiguous(memory_format=torch.channels_last) for x in xs]
    rois = _rois(24, 12, B, IH, IW)
    level = np.random.default_rng(13).integers(0, 4, len(rois)).astype(np.int32)
    bad = [(-1, 0), (B, 1), (0, -1), (1, 4), (-1, -1), (B + 5, 7)]      # (batch index, level)
    for i, (b, l) in enumerate(bad):
        rois[6 + 2 * i, 0], level[6 + 2 * i] = b, l
    valid = np.ones(len(rois), bool)
    valid[[6 + 2 * i for i in range(len(bad))]] = False
    rd, ld = torch.as_tensor(rois).cuda(), torch.as_tensor(level).cuda()
    R, PH, PW = len(rois), 7, 7
    sentinel = 1024.0                                                  # (exact in bf16)
    # forward into a guarded output (R, PH, PW, C)
    buf, out = _carve(R * PH * PW * C, sentinel, dtype)
    out.fill_(-7.0)
    o4 = out.view(R, PH, PW, C).permute(0, 3, 1, 2)
    ptrs = (ctypes.c_void_p * 4)(*[x.data_ptr() for x in xs])
    strides = (ctypes.c_long * 16)(*[int(s) for x in xs for s in x.stride()])
    hs = (ctypes.c_int * 4)(*[x.shape[2] for x in xs])
    ws = (ctypes.c_int * 4)(*[x.shape[3] for x in xs])
    sc = (ctypes.c_float * 4)(*SCALES)
    os4 = (ctypes.c_long * 4)(*o4.stride())
    lib.call('relnet_roi_align_levels_fwd', ctypes.addressof(ptrs), ctypes.addressof(strides), ctypes.addressof(hs), ctypes.addressof(ws),
             ctypes.addressof(sc), 4, rd.data_ptr(), ld.data_ptr(), o4.data_ptr(), os4, R, B, C, PH, PW, 2, 0, 0,
             lib.F32 if dtype == torch.float32 else lib.BF16, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = 4096
    assert (buf[:g] == sentinel).all() and (buf[-g:] == sentinel).all()
    assert (o4[torch.as_tensor(~valid)] == 0).all()
    vm = torch.as_tensor(valid).cuda()
    ref = ops.roi_align_fpn(xs, SCALES, rd[vm].contiguous(), ld[vm].contiguous(), channels_last_out=True)
    assert torch.equal(o4[torch.as_tensor(valid)], ref)
    # backward into guarded gradients: the invalid rows add nothing
    go = torch.randn(R, C, PH, PW, device='cuda').to(dtype)
    bufs, gins = [], []
    for x in xs:
        Bx, Cx, Hx, Wx = x.shape
        gb, gv = _carve(Bx * Cx * Hx * Wx, sentinel, torch.float32)
        gv.zero_()
        bufs.append(gb)
        gins.append(gv.view(Bx, Hx, Wx, Cx).permute(0, 3, 1, 2) if layout == 'nhwc' else gv.view(Bx, Cx, Hx, Wx))
    gp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in gins])
    gs = (ctypes.c_long * 16)(*[int(s) for t in gins for s in t.stride()])
    lib.call('relnet_roi_align_levels_bwd', go.data_ptr(), (ctypes.c_long * 4)(*go.stride()), rd.data_ptr(), ld.data_ptr(),
             ctypes.addressof(gp), ctypes.addressof(gs), ctypes.addressof(hs), ctypes.addressof(ws), ctypes.addressof(sc), 4, R, B, C, PH,
             PW, 2, 0, 0, lib.F32 if dtype == torch.float32 else lib.BF16, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for gb in bufs:
        assert (gb[:g] == sentinel).all() and (gb[-g:] == sentinel).all()
    want = ops.roi_align_fpn_bwd(go[vm], rd[vm].contiguous(), ld[vm].contiguous(), [tuple(x.shape) for x in xs], SCALES,
                                 channels_last=(layout == 'nhwc'))
    for a, b_ in zip(gins, want):
        assert float((a - b_).abs().max()) <= 1e-5 * max(float(b_.abs().max()), 1e-30)


def test_more_than_65535_rois():
    ops = _ops()
    B, C, IH, IW = 2, 8, 128, 160
    rng = np.random.default_rng(21)
    R = 70001
    rois = np.zeros((R, 5), np.float32)
    rois[:, 0] = rng.integers(0, B, R)
    xy = rng.uniform(0, 120, (R, 2))
    rois[:, 1:3], rois[:, 3:5] = xy, xy + rng.uniform(2, 60, (R, 2))
    level = torch.as_tensor(rng.integers(0, 4, R).astype(np.int32)).cuda()
    rd = torch.as_tensor(rois).cuda()
    h = R // 2
    for dtype, cl in ((torch.float32, False), (torch.bfloat16, True)):
        xs = [torch.as_tensor(x).cuda().to(dtype) for x in _pyramid(B, C, IH, IW, 22)]
        if cl:
            xs = [x.contiguous(memory_format=torch.channels_last) for x in xs]
        full = ops.roi_align_fpn(xs, SCALES, rd, level, channels_last_out=cl)
        a = ops.roi_align_fpn(xs, SCALES, rd[:h].contiguous(), level[:h].contiguous(), channels_last_out=cl)
        b = ops.roi_align_fpn(xs, SCALES, rd[h:].contiguous(), level[h:].contiguous(), channels_last_out=cl)
        assert torch.equal(full, torch.cat([a, b])), dtype
    # the single-map channels-last entry too (its roi count used to sit on grid.y)
    x = xs[1]
    assert torch.equal(ops.roi_align(x, rd, (7, 7), SCALES[1], 2, channels_last_out=True),
                       torch.cat([ops.roi_align(x, rd[:h].contiguous(), (7, 7), SCALES[1], 2, channels_last_out=True),
                                  ops.roi_align(x, rd[h:].contiguous(), (7, 7), SCALES[1], 2, channels_last_out=True)]))


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('size', ['separable', 'large'])
def test_levels_backward_is_the_adjoint_and_matches_autograd(layout, size):
    """'separable': rois whose footprints take the patch form; 'large': footprints over 64 cells per axis on the fine level (the
    per-sample scatter) next to patch-form rois on the coarse ones."""
    ops = _ops()
    B, C = 2, 16
    IH, IW = (160, 224) if size == 'separable' else (320, 352)
    xs = _pyramid(B, C, IH, IW, 31)
    rois = _rois(32, 32, B, IH, IW, max_size=120 if size == 'separable' else 900)
    level = np.random.default_rng(33).integers(0, 4, len(rois)).astype(np.int32)
    if size == 'large':
        level[:8] = 0
        rois[5:8, 1:] = [[4, 6, 300, 310], [0, 0, 350, 318], [-10, -8, 270, 290]]   # > 64 cells per axis at 1/4
    shapes = [x.shape for x in xs]
    rng = np.random.default_rng(34)
    g = rng.normal(0, 1, (len(rois), C, 7, 7)).astype(np.float32)
    xd = [torch.as_tensor(x).cuda() for x in xs]
    if layout == 'nhwc':
        xd = [x.contiguous(memory_format=torch.channels_last) for x in xd]
    rd, ld, gd = torch.as_tensor(rois).cuda(), torch.as_tensor(level).cuda(), torch.as_tensor(g).cuda()
    for sr in (2, 0):
        y = ops.roi_align_fpn(xd, SCALES, rd, ld, (7, 7), sr)
        gx = ops.roi_align_fpn_bwd(gd, rd, ld, shapes, SCALES, sr, channels_last=(layout == 'nhwc'))
        lhs = float((y.double() * gd.double()).sum())
        rhs = sum(float((x.double() * t.double()).sum()) for x, t in zip(xd, gx))
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (sr, lhs, rhs)
        # float64 autograd through the sparse sample matrix of the definition
        M = sample_matrix(rois, level, shapes, SCALES, (7, 7), sr)
        xt = _flat([torch.as_tensor(x).double() for x in xs]).requires_grad_(True)
        out = torch.sparse.mm(M, xt)                                             # [(r, ph, pw), C]
        gt = torch.as_tensor(g).double().permute(0, 2, 3, 1).reshape(-1, C)
        (out * gt).sum().backward()
        got = _flat([t.cpu().double() for t in gx])
        assert float((got - xt.grad).abs().max()) <= 2e-5 * float(xt.grad.abs().max()), sr
