"""Shared by tests/test_deterministic_cases_host.py and tests/test_gpu_deterministic.py: the inputs of the deterministic training mode's
kernels (TrainConfig.deterministic: relnet_roi_pool_bwd_ordered, relnet_colsum_add[_grouped]_ordered, relnet_reduce_scalar_ordered,
relnet_geometry_bias_bwd_ordered, relnet_lnms_take_bwd_ordered, relnet_wgrad_grouped_ex), numpy float32 restatements that perform the
additions in the order include/relnet_hip.h defines, and the bound a result is held to where only a tree is fixed.  Imports numpy only.

Where the checks come from (U = 2^-24, the unit roundoff of float32):

  defined order   ROI pooling backward: ascending (roi, ph, pw); the take adjoint: ascending flat source index.  The restatement does the
                  same float32 additions one by one from 0 (numpy float32 + float32 is one IEEE addition), so the comparison is bit for bit.
                  The column sums and the scalar reduction have a documented tree as well and are restated here too.
  fixed tree      n float32 terms added in ANY order: |computed - exact| <= gamma_(n-1) sum|x_i|, gamma_k = k U / (1 - k U); to first order
                  (n - 1) U sum|x_i|, which is what `sum_bound` returns, per output word, from the inputs.  bf16 inputs convert to float32
                  exactly, so there is no further term; a scale that is a power of two multiplies exactly.
  order matters   A rerun that gives the same bits proves nothing if every order gives those bits.  Gradient values are therefore
                  +-2^u m with u uniform in {-8..8} and a random mantissa m in [1, 2): sums of such terms round differently in
                  different orders, and `test_deterministic_cases_host.py` asserts that the restatement in REVERSED order differs from
                  the forward order in at least one word on exactly the inputs the GPU tests use."""
import zlib

import numpy as np

U = 2.0 ** -24
F32 = np.float32


def seed(id_):
    return zlib.crc32(id_.encode())


def to_bf16_exact(x):
    """float32 values truncated to the bf16 grid (the low 16 bits cleared): exactly representable in both formats."""
    return (np.ascontiguousarray(x, F32).view(np.uint32) & np.uint32(0xffff0000)).view(F32)


def order_sensitive(rng, shape, bf16=False):
    """+-2^u m, u uniform in {-8, .., 8}, m uniform in [1, 2)."""
    u = rng.integers(-8, 9, shape)
    v = (np.ldexp(rng.uniform(1.0, 2.0, shape), u) * rng.choice([-1.0, 1.0], shape)).astype(F32)
    return to_bf16_exact(v) if bf16 else v


def sum_bound(abs_sum, n):
    """(n - 1) 2^-24 sum|x_i| for an n-term float32 sum in any order (abs_sum, n: arrays or scalars)."""
    return np.maximum(np.asarray(n, np.float64) - 1.0, 0.0) * U * np.asarray(abs_sum, np.float64)


# ---------------------------------------------------------------------------------------------------------
# ROI pooling backward
# ---------------------------------------------------------------------------------------------------------
ROI_H, ROI_W, ROI_B, ROI_R, ROI_SCALE, ROI_P = 6, 8, 2, 24, 1.0 / 16.0, 7
# (id, C, bf16 + NHWC, batch_index_base, every roi on image 1)
ROI_CASES = [('c16-bf16-nhwc-base0', 16, True, 0, False), ('c16-bf16-nhwc-base3', 16, True, 3, False),
             ('c5-f32-nchw-base0', 5, False, 0, False), ('c5-f32-nchw-base3', 5, False, 3, False),
             ('c16-bf16-nhwc-image1', 16, True, 0, True), ('c5-f32-nchw-image1', 5, False, 3, True)]


def roi_case_rois(batch_index_base, image1_only):
    """[24, 5] rois of a 96 x 128 image (maps 6 x 8 at 1 / 16): two whole-map rois; four rois smaller than one cell (both extents round to
    ONE cell: all 49 bins sit on that cell -- 49 contributions to one word per channel); two rois that hang over the map's corner (most bins
    are empty, argmax -1, the rest sit on one cell); three exact duplicates of one roi; 13 random ones.  Images alternate, or all on image 1."""
    rng = np.random.default_rng(seed('roi-rois'))
    boxes = [[0, 0, 127, 95], [0, 0, 127, 95],
             [18, 18, 22, 21], [50, 34, 53, 38], [98, 66, 101, 69], [18, 18, 21, 22],
             [-104, -104, 7, 7], [116, 84, 230, 200],
             [30, 20, 90, 70], [30, 20, 90, 70], [30, 20, 90, 70]]
    while len(boxes) < ROI_R:
        x1, y1 = rng.uniform(0, 100), rng.uniform(0, 70)
        boxes.append([x1, y1, x1 + rng.uniform(10, 90), y1 + rng.uniform(10, 70)])
    rois = np.zeros((ROI_R, 5), F32)
    rois[:, 1:] = np.asarray(boxes, F32)
    img = np.arange(ROI_R) % ROI_B
    img[8:11] = 0                                  # the duplicates are duplicates in every column
    rois[:, 0] = batch_index_base + (1 if image1_only else img)
    return rois


def roi_pool_bwd_ordered_ref(grad_out, argmax, roi_image, B, H, W, reverse=False, stats=False):
    """grad_out [R, C, PH, PW] float32, argmax [R, C, PH, PW] int (cell y W + x, or -1), roi_image [R] (image of each roi, base removed)
    -> [B, C, H W] float32: every word the float32 sum from 0 of its contributions in ascending (reverse: descending) (roi, ph, pw) order.
    stats: also the number of contributions, the float64 sum and the float64 sum of magnitudes of every word."""
    R, C, PH, PW = grad_out.shape
    out = np.zeros((B, C, H * W), F32)
    cnt = np.zeros((B, C, H * W), np.int64)
    s64 = np.zeros((B, C, H * W), np.float64)
    a64 = np.zeros((B, C, H * W), np.float64)
    order = [(r, ph, pw) for r in range(R) for ph in range(PH) for pw in range(PW)]
    cs = np.arange(C)
    for r, ph, pw in (reversed(order) if reverse else order):
        b = int(roi_image[r])
        if b < 0 or b >= B:
            continue
        cell = argmax[r, :, ph, pw]
        ok = cell >= 0
        c_, a_ = cs[ok], cell[ok]
        g = grad_out[r, :, ph, pw][ok].astype(F32)
        out[b, c_, a_] = out[b, c_, a_] + g                    # one float32 addition per word (the channels' targets are distinct)
        cnt[b, c_, a_] += 1
        s64[b, c_, a_] += g.astype(np.float64)
        a64[b, c_, a_] += np.abs(g.astype(np.float64))
    return (out, cnt, s64, a64) if stats else out


# ---------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------
# (id, rows, cols, bf16)
COLSUM_CASES = [('4100x24-bf16', 4100, 24, True), ('1x8-bf16', 1, 8, True), ('257x5-f32', 257, 5, False)]
COLSUM_GROUP_ROWS = [1, 7, 64, 511, 512, 513, 700, 1024, 1025, 33, 2, 4100, 90, 300, 1536, 8, 129]      # 17 problems: two launches
COLSUM_GROUP_COLS = [8, 16, 24, 8, 32, 8, 264, 8, 16, 40, 8, 24, 8, 16, 8, 48, 8]


def colsum_chunks(rows):
    """(number of row chunks, rows per chunk) of the ordered column sum: a function of rows alone."""
    nchunk = min(max((rows + 511) // 512, 1), 128)
    rpb = (rows + nchunk - 1) // nchunk
    return (rows + rpb - 1) // rpb, rpb


def colsum_ordered_ref(x, out0, reverse=False):
    """x [rows, cols] float32 (bf16 values are exact in it), out0 [cols] float32 -> out0 + column sums through the documented tree:
    chunk -> 8 row lanes (rows r0 + l, r0 + l + 8, ..) -> their ascending sum -> ascending sum of the chunk partials -> out0 + that.
    reverse: the rows are fed in reversed order."""
    x = np.ascontiguousarray(x[::-1] if reverse else x, F32)
    rows, cols = x.shape
    chunks, rpb = colsum_chunks(rows)
    total = np.zeros(cols, F32)
    for k in range(chunks):
        r0, r1 = k * rpb, min((k + 1) * rpb, rows)
        part = np.zeros(cols, F32)
        for lane in range(8):
            acc = np.zeros(cols, F32)
            for r in range(r0 + lane, r1, 8):
                acc = acc + x[r]
            part = part + acc
        total = total + part
    return (np.asarray(out0, F32) + total).astype(F32)


def colsum_case(id_, rows, cols, bf16):
    rng = np.random.default_rng(seed('colsum-' + id_))
    return order_sensitive(rng, (rows, cols), bf16), order_sensitive(rng, (cols,))


# ---------------------------------------------------------------------------------------------------------
# scalar reduction
# ---------------------------------------------------------------------------------------------------------
SCALAR_NS = [1, 255, 70001]
SCALAR_SCALE = 0.125              # a power of two: the scaling is exact, the n-term bound needs no extra term


def scalar_case(n):
    rng = np.random.default_rng(seed('scalar-%d' % n))
    return order_sensitive(rng, (n,))


def reduce_scalar_ordered_ref(x, scale, mode):
    """relnet_reduce_scalar_ordered in float32: nb = min(64, ceil(n / 4096)) workgroups of 256 threads; thread t of workgroup b adds
    x[b 256 + t + i nb 256] ascending i; the wavefront's xor butterfly (32, 16, .., 1); ((w0 + w1) + w2) + w3; times the scale (mode 0);
    then the ascending sum of the workgroup values from 0."""
    x = np.asarray(x, F32)
    n = x.size
    v = (x >= 0).astype(F32) if mode else x
    nb = min(max((n + 4095) // 4096, 1), 64)
    stride = nb * 256
    trips = (n + stride - 1) // stride
    pad = np.zeros(trips * stride, F32)
    pad[:n] = v
    acc = np.zeros(stride, F32)
    for i in range(trips):                              # (adding the zero padding is exact)
        acc = acc + pad[i * stride:(i + 1) * stride]
    acc = acc.reshape(nb, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, np.arange(64) ^ o]
    w = acc[:, :, 0]
    part = (((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]) * F32(1.0 if mode else scale)
    t = F32(0.0)
    for k in range(nb):
        t = F32(t + part[k])
    return t


# ---------------------------------------------------------------------------------------------------------
# take adjoint of the learn-NMS branch
# ---------------------------------------------------------------------------------------------------------
TAKE_B, TAKE_N, TAKE_C, TAKE_F = 1, 12, 5, 8


def take_case(bf16):
    """rank_idx [1, 5, 8]: per class the first 8 entries of a permutation of the 12 rois, drawn so that rois 10 and 11 are ranked by no
    class and the others by up to five; d_x [1, 5, 8, 128]."""
    rng = np.random.default_rng(seed('take'))
    rank = np.stack([rng.permutation(10)[:TAKE_F] for _ in range(TAKE_C)])[None].astype(np.int32)
    d_x = order_sensitive(rng, (TAKE_B, TAKE_C, TAKE_F, 128), bf16)
    return d_x, rank


def take_bwd_ordered_ref(d_x, rank_idx, N, reverse=False):
    B, C, F, D = d_x.shape
    out = np.zeros((B * N, D), F32)
    order = [(b, c, f) for b in range(B) for c in range(C) for f in range(F)]
    for b, c, f in (reversed(order) if reverse else order):
        r = int(rank_idx[b, c, f])
        if 0 <= r < N:
            out[b * N + r] = out[b * N + r] + d_x[b, c, f].astype(F32)
    return out


# the new C-ABI entry points (declared in include/relnet_hip.h, bound in lib.py)
NEW_SYMBOLS = ['relnet_roi_pool_bwd_ordered', 'relnet_colsum_ordered_workspace_bytes', 'relnet_colsum_add_ordered',
               'relnet_colsum_add_grouped_ordered', 'relnet_reduce_scalar_workspace_bytes', 'relnet_reduce_scalar_ordered',
               'relnet_geometry_bias_bwd_workspace_bytes', 'relnet_geometry_bias_bwd_ordered', 'relnet_lnms_take_bwd_ordered',
               'relnet_wgrad_grouped_ex']
