#!/usr/bin/env python
"""The exact border lattices of tests/deform_edge_cases.py through the reference's own CUDA kernels (oracle/_ref/libref_cuda.so, built by
oracle/build_ref.py), RUN ON THE MI355X:

    python tests/golden/gen_golden_deform_edges.py [out.npz]        (default tests/golden/ref_cuda_deform_edges.npz)

Only the kernels' outputs are stored (deformable_col2im, deformable_col2im_coord, DeformablePSROIPoolForward / BackwardAcc), next to a checksum
of the regenerated inputs; cases with at most 128 channels.  Every sum of these cases is exact in float32 whatever the order of the atomics, so
the file is reproducible.  The 128-channel pooling shape keeps the pooled values and the data gradient of the first and last
channel of each class only (GOLDEN_TOP_CHANNELS; the channels of a class share their geometry), its trans gradient, which sums over all, whole;
trans-gradient addresses whose sum is not exact in every order (128 channels at spp >= 2, see ps_exact_units) are stored as 0.  tests/test_deform_edge_cases_host.py holds the float64 restatement to this file bit for bit."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import deform_edge_cases as DE  # noqa: E402
from oracle import refcuda as RC  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'ref_cuda_deform_edges.npz')
    Z = {}
    for id_ in DE.GOLDEN_CASES:
        c = DE.case(id_)
        data, off, dcol = DE.build_operands(c)
        kk, pad, st, dil = (DE.K, DE.K), (c.pad, c.pad), (c.stride, c.stride), (c.dil, c.dil)
        gd, go = [], []
        for b in range(c.B):
            col = DE.dcol_to_reference(c, dcol, b)
            gd.append(RC.deformable_col2im(col, off[b], (c.C, c.H, c.W), kk, pad, st, dil, c.dg))
            go.append(RC.deformable_col2im_coord(col, data[b], off[b], kk, pad, st, dil, c.dg))
        Z['col2im_%s_grad_data' % id_] = np.stack(gd)
        Z['col2im_%s_grad_offset' % id_] = np.stack(go)
        Z['col2im_%s_inputs' % id_] = DE.checksum(data, off, dcol)
        print('col2im', id_, np.abs(Z['col2im_%s_grad_data' % id_]).max(), np.abs(Z['col2im_%s_grad_offset' % id_]).max(), flush=True)
    for cfg in DE.ps_configs(max_channels=128):
        data, rois, trans, mult = DE.ps_operands(cfg)
        args = (DE.PS_SCALE, cfg.od, cfg.group, cfg.P, cfg.part, cfg.spp, DE.PS_TRANS_STD)
        top, cnt = RC.psroi_forward(data, rois, trans, *args)
        gi, gt = RC.psroi_backward(DE.ps_grad_out(cnt, mult), cnt, data, rois, trans, *args)
        k = 'psroi_%s_' % cfg.id
        ch = DE.GOLDEN_TOP_CHANNELS[cfg.od]
        Z[k + 'top'], Z[k + 'count'], Z[k + 'grad_data'] = top[:, ch], cnt[:, ch].astype(np.uint8), gi[:, DE.golden_data_channels(cfg)]
        if gt is not None:
            # addresses that collect 2^24 lattice units of |terms| or more are not exact under the kernel's atomics (their last bit moves from run
            # to run): stored as 0, so that the file holds exact results only and regenerates identically
            _, ut = DE.ps_exact_units(cfg, DE.ps_reference(cfg)[-1])
            Z[k + 'grad_trans'] = np.where(ut < 2.0 ** 24, gt, np.float32(0))
        Z[k + 'inputs'] = DE.checksum(data, rois, mult, *([] if trans is None else [trans]))
        print('psroi', cfg.id, np.abs(top).max(), cnt.max(), np.abs(gi).max(), flush=True)
    np.savez_compressed(out, **Z)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
