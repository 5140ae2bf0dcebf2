"""Shared by tests/test_stem_train_cases_host.py and tests/test_gpu_stem_train.py: the inputs of the stem's backward kernels
(relnet_stem_pool_bwd, relnet_stem_wgrad: a training step whose network.FIXED_PARAMS leaves conv1 trainable) and their restatements.
Imports numpy only.

  pool adjoint    float32, in the kernel's DEFINED order: windows in ascending (ph, pw), each handing d_out * (out > 0) to its first maximum
                  in row-major window order (MXNet's unpool rule and torch's; the reference has no pooling source, so this is a restatement
                  like ROIPooling's), one IEEE float32 addition per window from 0, one rounding to bf16 at the end -> bit for bit.
  conv1 wgrad     float64 by explicit patches of the zero-padded image, with sum|x_i| per word for `deterministic_cases.sum_bound`: the
                  kernel adds n = B Hc Wc float32 products (bf16 x bf16 is exact in float32) in a fixed tree.

The conv maps take their values from a grid of nine bf16 levels, so exact ties are everywhere, and ties are also PLACED: inside one window,
on a pixel shared by two windows and on one shared by four.  One window is all negative under a zero bias (its gradient must vanish), and
one pixel is the first maximum of four windows whose d_out values (2^27, 1, -2^27, 1) sum to 1 in ascending order and to 0 in reversed order."""
import zlib

import numpy as np

F32 = np.float32

#: (Hc, Wc) of the conv map: one window | every border window clipped | odd, more windows | what a 35 x 51 image gives
POOL_CASES = [(3, 3), (4, 4), (7, 5), (18, 26)]
POOL_B, POOL_C = 2, 64
BIG = float(2 ** 27)


def seed(id_):
    return zlib.crc32(id_.encode())


def to_bf16(x):
    """float32 -> nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(F32).reshape(np.shape(x))


def pooled_hw(Hc, Wc):
    """pooling_convention='full', kernel 3, stride 2, no padding; the last window starts inside the map."""
    Ho, Wo = -(-(Hc - 3) // 2) + 1, -(-(Wc - 3) // 2) + 1
    if (Ho - 1) * 2 >= Hc:
        Ho -= 1
    if (Wo - 1) * 2 >= Wc:
        Wo -= 1
    return Ho, Wo


def pool_forward(conv, bias, bf16):
    """relu(maxpool_ceil(conv) + bias) as relnet_stem_bias_relu_pool computes it (bf16: the sum is rounded to bf16 before the ReLU)."""
    B, Hc, Wc, C = conv.shape
    Ho, Wo = pooled_hw(Hc, Wc)
    out = np.empty((B, Ho, Wo, C), F32)
    for ph in range(Ho):
        for pw in range(Wo):
            win = conv[:, 2 * ph:min(2 * ph + 3, Hc), 2 * pw:min(2 * pw + 3, Wc), :]
            out[:, ph, pw, :] = win.reshape(B, -1, C).max(1)
    out = (out + bias.astype(F32)).astype(F32)
    if bf16:
        out = to_bf16(out)
    return np.maximum(out, F32(0))


def pool_backward(conv, out, d_out, bf16, last=False, reverse=False):
    """The adjoint in its defined order.  last: hand the gradient to the LAST maximum instead (the rule the kernel must NOT follow).
    reverse: visit the windows in descending (ph, pw) (an order the kernel must NOT follow)."""
    B, Hc, Wc, C = conv.shape
    Ho, Wo = out.shape[1:3]
    d_conv = np.zeros(conv.shape, F32)
    wins = [(ph, pw) for ph in range(Ho) for pw in range(Wo)]
    for ph, pw in (reversed(wins) if reverse else wins):
        y0, x0 = 2 * ph, 2 * pw
        y1, x1 = min(y0 + 3, Hc), min(x0 + 3, Wc)
        win = conv[:, y0:y1, x0:x1, :].reshape(B, -1, C)
        n = win.shape[1]
        arg = (n - 1 - win[:, ::-1].argmax(1)) if last else win.argmax(1)              # argmax: the first occurrence of the maximum
        g = np.where(out[:, ph, pw, :] > 0, d_out[:, ph, pw, :], F32(0)).astype(F32)
        for k in range(n):
            y, x = y0 + k // (x1 - x0), x0 + k % (x1 - x0)
            d_conv[:, y, x, :] = (d_conv[:, y, x, :] + np.where(arg == k, g, F32(0))).astype(F32)       # one float32 addition
    return to_bf16(d_conv) if bf16 else d_conv


def pool_case(Hc, Wc):
    """-> dict(conv, bias, d_out) float32 arrays on the bf16 grid (so the bf16 and the float32 kernel see the same values)."""
    rng = np.random.default_rng(seed('stem-pool-%dx%d' % (Hc, Wc)))
    B, C = POOL_B, POOL_C
    Ho, Wo = pooled_hw(Hc, Wc)
    conv = (rng.integers(-4, 5, (B, Hc, Wc, C)) / 4.0).astype(F32)                   # nine levels: ties in nearly every window
    bias = (rng.integers(-1, 2, C) / 4.0).astype(F32)
    d_out = to_bf16(np.ldexp(rng.uniform(1.0, 2.0, (B, Ho, Wo, C)), rng.integers(-8, 9, (B, Ho, Wo, C))) * rng.choice([-1.0, 1.0], (B, Ho, Wo, C)))
    # placed ties, image 0, channels 0..31 (the maximum of every window they touch): inside window (0, 0) only
    conv[0, 0, 0, :32] = 4.0; conv[0, 0, 1, :32] = 4.0
    if Wo >= 2:       # pixel (0, 2) is shared by windows (0, 0) and (0, 1); its twin (1, 3) lies in (0, 1) only
        conv[0, 0, 2, :32] = 4.0; conv[0, 1, 3, :32] = 4.0
    if Ho >= 2 and Wo >= 2:
        # channels 32..47: pixel (2, 2) is shared by four windows and tied with (3, 3), which lies in window (1, 1) only
        conv[0, 2, 2, 32:48] = 6.0; conv[0, 3, 3, 32:48] = 6.0
        # channels 48..63: pixel (2, 2) is the only maximum of its four windows, whose gradients cancel differently in another order
        conv[0, 2, 2, 48:] = 8.0
        bias[48:] = 0.0
        for (ph, pw), v in zip(((0, 0), (0, 1), (1, 0), (1, 1)), (BIG, 1.0, -BIG, 1.0)):
            d_out[0, ph, pw, 48:] = v
    # image 1, window (0, 0): every value <= -1, the bias at most 1/4 -> out = 0 on every channel, no gradient leaves this window
    conv[1, 0:3, 0:3, :] = -np.abs(conv[1, 0:3, 0:3, :]) - 1.0
    return dict(conv=conv, bias=bias, d_out=d_out.astype(F32))


# ---------------------------------------------------------------------------------------------------------
# conv1 weight gradient
# ---------------------------------------------------------------------------------------------------------
CHUNK = 4096          # pixels per partial sum of relnet_stem_wgrad (include/relnet_hip.h)
#: (id, B, H, W): conv map 4 x 4, every tap crosses the padding | odd sizes, 19 x 27 | 17 x 241 = one chunk and one pixel
WGRAD_CASES = [('8x8', 2, 8, 8), ('37x53', 2, 37, 53), ('chunk+1', 1, 34, 482)]


def conv_hw(H, W):
    return (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1


def wgrad_case(id_, B, H, W):
    """-> (image [B,3,H,W], d_conv [B,Hc,Wc,64]) float32 on the bf16 grid."""
    rng = np.random.default_rng(seed('stem-wgrad-' + id_))
    Hc, Wc = conv_hw(H, W)
    img = to_bf16(rng.normal(0.0, 1.0, (B, 3, H, W)).astype(F32))
    d = to_bf16((np.ldexp(rng.uniform(1.0, 2.0, (B, Hc, Wc, 64)), rng.integers(-8, 9, (B, Hc, Wc, 64))) * rng.choice([-1.0, 1.0], (B, Hc, Wc, 64))).astype(F32))
    return img, d


def wgrad_float64(img, d_conv):
    """-> (dW [64, 147] float64 with columns (ty, tx, c), sum of |products| per word, terms per word)."""
    B, _, H, W = img.shape
    Hc, Wc = d_conv.shape[1:3]
    pad = np.zeros((B, 3, H + 6, W + 6), np.float64)
    pad[:, :, 3:3 + H, 3:3 + W] = img
    d = d_conv.astype(np.float64)
    dw, ab = np.zeros((64, 7, 7, 3)), np.zeros((64, 7, 7, 3))
    for ty in range(7):
        for tx in range(7):
            patch = pad[:, :, ty:ty + 2 * Hc:2, tx:tx + 2 * Wc:2]                     # [B, 3, Hc, Wc]
            dw[:, ty, tx, :] = np.einsum('bhwo,bchw->oc', d, patch)
            ab[:, ty, tx, :] = np.einsum('bhwo,bchw->oc', np.abs(d), np.abs(patch))
    return dw.reshape(64, 147), ab.reshape(64, 147), B * Hc * Wc
