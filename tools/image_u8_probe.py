"""uint8 image input on one MI355X:
    python tools/image_u8_probe.py [images per step for the in-flight part, default 108]
(1) relnet_stem_fused_u8 against relnet_stem_fused per launch (HIP events), 600 x 1000 images, at 108 and 8 images;
(2) relnet_resize_u8 per launch for COCO-sized sources (640 x 480 -> 600 x 800), at 108 and 8 images;
(3) the PCIe-inclusive rate of three captured detector steps in flight (detector.InFlight, RPN branch in line: one queue per step),
    every step first uploading its batch from pinned host memory on its own stream: the fp32 NCHW tensor (tools/pipeline_probe.py
    PROBE_H2D=1), the uint8 600 x 1000 canvas, and the raw 640 x 480 uint8 sources resized inside the captured step.
Every figure is the median of 5 windows after a warm-up, with the min - max of the windows."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import relnet_amd  # noqa: E402,F401
from relnet_amd import backbone, detector, ops  # noqa: E402
from relnet_amd.dataset import image as IMG  # noqa: E402

MEANS = detector.Config.pixel_means
H, W = 600, 1000


def windows(fn, iters, nwin=5, warm=5):
    """ms per call of fn(): device events around `iters` calls, nwin windows."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(nwin):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return out


def fmt(v, unit='ms'):
    return '%.3f %s (windows %.3f - %.3f)' % (float(np.median(v)), unit, min(v), max(v))


def raw_sources(B, g):
    """B 480 x 640 uint8 sources, packed as a loader with raw_images=True ships them (600 x 800 after the resize)."""
    ims = [torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8).numpy() for _ in range(B)]
    raws, info = [], []
    for im in ims:
        s, nh, nw, ph, pw = IMG.resize_plan(480, 640, 600, 1000, 0)
        raws.append((im, False, s, nh, nw))
        info.append([ph, pw, s])
    return IMG.pack_raw(raws, info), np.array(info, np.float32)


def stem_and_resize(p, g):
    w1, b1 = backbone.fold_bn(p['conv1_weight'], p['bn_conv1_gamma'], p['bn_conv1_beta'], p['bn_conv1_moving_mean'],
                              p['bn_conv1_moving_var'])
    w, b = ops.pack_stem_weight(w1, torch.bfloat16, 'cuda'), b1.float().cuda().contiguous()
    for B in (108, 8):
        u8 = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
        im_info = torch.tensor([[H, W, 1.0]] * B).cuda()
        f32 = ops.image_transform_u8(u8, MEANS, im_info)
        assert torch.equal(ops.stem_fused(u8, w, b, im_info, MEANS), ops.stem_fused(f32, w, b))
        it = 20 if B > 8 else 200
        for rep in range(2):          # alternated, twice
            print('B=%d stem fp32 NCHW: %s' % (B, fmt(windows(lambda: ops.stem_fused(f32, w, b), it))), flush=True)
            print('B=%d stem uint8 HWC: %s' % (B, fmt(windows(lambda: ops.stem_fused(u8, w, b, im_info, MEANS), it))), flush=True)
        print('B=%d image_transform_u8 (fp32 out): %s' % (B, fmt(windows(lambda: ops.image_transform_u8(u8, MEANS, im_info), it))),
              flush=True)
        pk, _ = raw_sources(B, g)
        src, tab, sc = (torch.as_tensor(pk[k]).cuda() for k in ('image_src', 'image_table', 'image_scale'))
        print('B=%d resize_u8 640x480 -> 600x800: %s' % (B, fmt(windows(lambda: ops.resize_u8(src, tab, sc, pk['canvas_hw']), it))),
              flush=True)
        del u8, f32, src


def in_flight(p, g, B, kind, n=3):
    """img/s of n captured steps round-robin, each uploading its batch (pinned host -> resident device tensor) on its own stream."""
    cfg = detector.Config()
    dets, steps, res, hosts = [], [], [], []
    if kind == 'raw':
        pk, info = raw_sources(B, g)
        im_info = torch.as_tensor(info).cuda()
    else:
        im_info = torch.tensor([[H, W, 1.0]] * B).cuda()
    for i in range(n):
        det = detector.Detector(p, dtype=torch.bfloat16, device='cuda', relation=True, cfg=cfg,
                                im_hw=pk['canvas_hw'] if kind == 'raw' else (H, W))
        det.overlap_rpn = False
        if kind == 'fp32':
            host = torch.randn(B, 3, H, W, generator=g).pin_memory()
        elif kind == 'u8':
            host = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).pin_memory()
        else:
            host = torch.as_tensor(pk['image_src']).pin_memory()
        dev = host.cuda()
        if kind == 'raw':
            tab, sc = torch.as_tensor(pk['image_table']).cuda(), torch.as_tensor(pk['image_scale']).cuda()
            step = (lambda det=det, dev=dev, tab=tab, sc=sc: det.forward(ops.resize_u8(dev, tab, sc, pk['canvas_hw']), im_info))
        else:
            step = (lambda det=det, dev=dev: det.forward(dev, im_info))
        dets.append(det); steps.append(step); res.append(dev); hosts.append(host)
    with torch.no_grad():
        fl = detector.InFlight(steps)

    def run(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(k):
            i = j % n
            with torch.cuda.stream(fl.streams[i]):
                res[i].copy_(hosts[i], non_blocking=True)
                fl.graphs[i].replay()
        torch.cuda.synchronize()
        return k * B / (time.perf_counter() - t0)

    run(2 * n)
    k = max(24, 600 // B) // n * n
    rates = [run(k) for _ in range(5)]
    mb = hosts[0].numel() * hosts[0].element_size() / B / 1e6
    print('B=%d in flight x%d, upload %s (%.2f MB/image): %s' % (B, n, kind, mb, fmt(rates, 'img/s')), flush=True)
    del fl, dets, steps, res, hosts
    torch.cuda.empty_cache()


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 108
    p = backbone.init_params(seed=1)
    g = torch.Generator().manual_seed(1000)
    print(torch.cuda.get_device_name(0), flush=True)
    stem_and_resize(p, g)
    for kind in ('fp32', 'u8', 'raw', 'fp32'):
        in_flight(p, g, B, kind)


if __name__ == '__main__':
    main()
