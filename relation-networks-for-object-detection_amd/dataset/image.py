"""Image pre-processing of `lib/utils/image.py:16-130`: read (BGR), optional mirror, resize so that the short side is
SCALES[i][0] with the long side capped at SCALES[i][1], zero-pad to IMAGE_STRIDE, subtract PIXEL_MEANS and emit RGB-ordered
[1, 3, H, W]; boxes are scaled, rounded and clipped.  cv2 is not installed here: decoding uses Pillow, `.npy` arrays are read
as is, and the resize is a numpy restatement of `cv2.resize(im, None, None, fx=s, fy=s, interpolation=cv2.INTER_LINEAR)`:
plain 2-tap bilinear for up- AND down-scaling (no antialiasing support widening), source coordinate (d + 0.5) / s - 0.5
clamped to the image, and uint8 images come back ROUNDED to uint8 like cv2's output (the mean is subtracted from the rounded
values).  cv2 evaluates the taps in 11-bit fixed point: results can differ by one grey level on a fraction of the pixels --
unpinned (no cv2 here to compare with)."""
import os
import random

import numpy as np


def imread_bgr(path):
    if path.endswith('.npy'):
        im = np.load(path)
        assert im.ndim == 3 and im.shape[2] == 3
        return im
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert('RGB'))
    return rgb[:, :, ::-1]


def _bilinear_axis(n_src, n_dst, scale):
    """cv2 INTER_LINEAR taps of one axis: (left index, right index, weight of the right tap) per destination position."""
    f = (np.arange(n_dst, dtype=np.float64) + 0.5) / scale - 0.5
    i0 = np.floor(f).astype(np.int64)
    w1 = f - i0
    lo = i0 < 0
    i0[lo] = 0; w1[lo] = 0.0
    hi = i0 >= n_src - 1
    i0[hi] = n_src - 1; w1[hi] = 0.0
    return i0, np.minimum(i0 + 1, n_src - 1), w1


def resize_plan(h, w, target_size, max_size, stride=0):
    """The host arithmetic of `resize` (image.py:78-108) for an h x w source: (im_scale, nh, nw, ph, pw) -- the scale, the resized
    size and the size after zero-padding to a multiple of `stride` (= nh, nw for stride 0)."""
    size_min, size_max = min(h, w), max(h, w)
    im_scale = float(target_size) / float(size_min)
    if np.round(im_scale * size_max) > max_size:
        im_scale = float(max_size) / float(size_max)
    nw, nh = int(round(w * im_scale)), int(round(h * im_scale))
    if stride == 0:
        return im_scale, nh, nw, nh, nw
    ph = int(np.ceil(nh / float(stride)) * stride)
    pw = int(np.ceil(nw / float(stride)) * stride)
    return im_scale, nh, nw, ph, pw


def resize(im, target_size, max_size, stride=0):
    """image.py:78-108.  Returns (resized [+ padded] float image, im_scale)."""
    h, w = im.shape[:2]
    im_scale, nh, nw, ph, pw = resize_plan(h, w, target_size, max_size, stride)
    x0, x1, wx = _bilinear_axis(w, nw, im_scale)
    y0, y1, wy = _bilinear_axis(h, nh, im_scale)
    src = im.astype(np.float64)
    top = src[y0][:, x0] * (1.0 - wx)[None, :, None] + src[y0][:, x1] * wx[None, :, None]
    bot = src[y1][:, x0] * (1.0 - wx)[None, :, None] + src[y1][:, x1] * wx[None, :, None]
    out = top * (1.0 - wy)[:, None, None] + bot * wy[:, None, None]
    if im.dtype == np.uint8:                  # cv2 returns the image in the input's type: rounded, saturated
        out = np.clip(np.rint(out), 0, 255)
    out = out.astype(np.float32)
    if stride == 0:
        return out, im_scale
    padded = np.zeros((ph, pw, out.shape[2]), dtype=out.dtype)
    padded[:out.shape[0], :out.shape[1], :] = out
    return padded, im_scale


def transform(im, pixel_means):
    """image.py:110-122: [H, W, 3] BGR -> [1, 3, H, W] in R, G, B order with the means subtracted."""
    t = np.zeros((1, 3, im.shape[0], im.shape[1]), dtype=np.float32)
    for i in range(3):
        t[0, i] = im[:, :, 2 - i] - pixel_means[2 - i]
    return t


def clip_boxes(boxes, im_shape):
    boxes[:, 0::4] = np.maximum(np.minimum(boxes[:, 0::4], im_shape[1] - 1), 0)
    boxes[:, 1::4] = np.maximum(np.minimum(boxes[:, 1::4], im_shape[0] - 1), 0)
    boxes[:, 2::4] = np.maximum(np.minimum(boxes[:, 2::4], im_shape[1] - 1), 0)
    boxes[:, 3::4] = np.maximum(np.minimum(boxes[:, 3::4], im_shape[0] - 1), 0)
    return boxes


def get_image(roidb, config, rng=random, raw=False):
    """image.py:16-45: -> (list of [1,3,H,W] float32 arrays, roidb copies with scaled `boxes` and `im_info`).
    raw=True: no pixel work -- the list holds (decoded uint8 BGR HWC source, flipped, im_scale, nh, nw) per image instead (the resize,
    mirror and transform are left to the device: pack_raw + device_images); `im_info` and the boxes are the same as without it."""
    ims, out = [], []
    for rec in roidb:
        assert os.path.exists(rec['image']), '%s does not exist' % rec['image']
        im = imread_bgr(rec['image'])
        new = dict(rec)
        target_size, max_size = config.SCALES[rng.randrange(len(config.SCALES))]
        if raw:
            assert im.dtype == np.uint8, 'raw images: uint8 sources only (%s is %s)' % (rec['image'], im.dtype)
            im_scale, nh, nw, ph, pw = resize_plan(im.shape[0], im.shape[1], target_size, max_size, config.network.IMAGE_STRIDE)
            ims.append((im, bool(rec['flipped']), im_scale, nh, nw))
            im_info = [ph, pw, im_scale]
        else:
            if rec['flipped']:
                im = im[:, ::-1, :]
            im, im_scale = resize(im, target_size, max_size, stride=config.network.IMAGE_STRIDE)
            t = transform(im, config.network.PIXEL_MEANS)
            ims.append(t)
            im_info = [t.shape[2], t.shape[3], im_scale]
        new['boxes'] = clip_boxes(np.round(rec['boxes'].astype(np.float64).copy() * im_scale), im_info[:2])
        new['im_info'] = im_info
        out.append(new)
    return ims, out


def pack_raw(raws, im_info):
    """The raw-image part of a batch (get_image(raw=True)): a dict of `image_src` (the uint8 sources back to back, flat),
    `image_table` [B,6] int64 (byte offset, h, w, flip, nh, nw), `image_scale` [B] float64 and `canvas_hw`, a host tuple (Hc, Wc):
    the batch maximum of the padded extents im_info[:, :2], which is what tensor_vstack gives the float batch."""
    table = np.zeros((len(raws), 6), dtype=np.int64)
    off = 0
    for i, (im, flip, im_scale, nh, nw) in enumerate(raws):
        table[i] = (off, im.shape[0], im.shape[1], int(flip), nh, nw)
        off += im.size
    src = np.concatenate([np.ascontiguousarray(r[0]).reshape(-1) for r in raws])
    info = np.asarray(im_info)
    canvas = (int(info[:, 0].max()), int(info[:, 1].max()))
    return dict(image_src=src, image_table=table, image_scale=np.array([r[2] for r in raws], dtype=np.float64), canvas_hw=canvas)


def device_images(batch):
    """The uint8 canvas [B,Hc,Wc,3] BGR HWC of a raw-image batch (a loader's batch with raw_images=True, on the GPU): the sources
    resized (and mirrored) by ops.resize_u8 into the top left of their slots, zeros elsewhere.  The detector and the trainers take it
    as `data` with the batch's `im_info`, which gives every image its extent.  No host synchronisation."""
    from .. import ops
    return ops.resize_u8(batch['image_src'], batch['image_table'], batch['image_scale'], batch['canvas_hw'])


def tensor_vstack(tensor_list, pad=0):
    """image.py:tensor_vstack: stack along axis 0, zero-padding every other axis to the largest extent."""
    ndim = len(tensor_list[0].shape)
    dims = [max(t.shape[d] for t in tensor_list) for d in range(1, ndim)]
    n = sum(t.shape[0] for t in tensor_list)
    out = np.full([n] + dims, pad, dtype=tensor_list[0].dtype)
    k = 0
    for t in tensor_list:
        sl = (slice(k, k + t.shape[0]),) + tuple(slice(0, s) for s in t.shape[1:])
        out[sl] = t
        k += t.shape[0]
    return out
