"""include/relnet_operator_cxx.hpp, PSROIPooling classes: the C++ Param / Prop / Op of `_contrib_PSROIPooling` over the C-ABI.
CPU: the header and tests/cxx/psroi_harness.cpp compile and link against librelnet_hip.so.  GPU: the harness (through ctypes) runs
Prop::InferShape + Op::Forward / Op::Backward on device buffers, bit for bit against the restatement of tests/psroi_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import psroi_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'relation-networks-for-object-detection_amd')
SO = os.path.join(ROOT, 'tests', 'cxx', 'libpsroi_test.so')


def _build():
    import __graft_entry__ as ge
    ge.build()
    src = os.path.join(ROOT, 'tests', 'cxx', 'psroi_harness.cpp')
    hdr = os.path.join(ROOT, 'include', 'relnet_operator_cxx.hpp')
    if os.path.exists(SO) and os.path.getmtime(SO) >= max(os.path.getmtime(src), os.path.getmtime(hdr)):
        return SO
    cmd = [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-std=c++17', '-O2', '-fPIC', '-shared', '-x', 'hip', '--offload-arch=gfx950',
           '-I' + os.path.join(ROOT, 'include'), src, '-o', SO, '-L' + PKG, '-lrelnet_hip', '-Wl,-rpath,' + PKG]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    return SO


def test_header_and_harness_compile_and_link():
    so = _build()
    syms = subprocess.run(['nm', '-D', '--defined-only', so], stdout=subprocess.PIPE).stdout.decode()
    assert 'psroi_pooling' in syms and 'psroi_last_error' in syms


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


@pytest.mark.gpu
def test_cxx_psroi_forward_backward_match_restatement():
    lib = C.CDLL(_build())
    lib.psroi_last_error.restype = C.c_char_p
    lib.psroi_pooling.argtypes = [C.c_void_p] * 7 + [C.c_int] * 8 + [C.c_float, C.c_int, C.c_int]
    c = PC.case('p7g3_9x6_r65')
    d = lambda a: torch.as_tensor(a).cuda().contiguous()
    x, rois, dy = d(c['data']), d(c['rois']), d(c['grad_out'])
    out = torch.full((c['R'], c['output_dim'], c['P'], c['P']), float('nan'), device='cuda')
    mapping = torch.full_like(out, float('nan'))
    gx = d(c['grad_in0'])                                   # kAddTo: accumulated onto the prior contents
    grois = torch.full((c['R'], 5), float('nan'), device='cuda')
    args = (c['B'], c['C'], c['H'], c['W'], c['R'], c['output_dim'], c['P'], c['g'], c['scale'])
    rc = lib.psroi_pooling(_p(x), _p(rois), _p(out), _p(mapping), _p(dy), _p(gx), _p(grois), *args, 3, 1)
    assert rc == 0, (rc, lib.psroi_last_error())
    assert np.array_equal(out.cpu().numpy(), c['ref32']['out'])
    assert np.array_equal(mapping.cpu().numpy(), c['ref32']['mapping'])
    assert np.array_equal(gx.cpu().numpy(), c['ref32_acc']['grad_in'])
    assert float(grois.abs().max()) == 0.0                  # grad_roi = 0 on kWriteTo
    # kWriteTo over NaN: every word written; kNullOp on the rois leaves them alone
    gx.fill_(float('nan')); grois.fill_(7.0)
    rc = lib.psroi_pooling(_p(x), _p(rois), _p(out), _p(mapping), _p(dy), _p(gx), _p(grois), *args, 1, 0)
    assert rc == 0, (rc, lib.psroi_last_error())
    assert np.array_equal(gx.cpu().numpy(), c['ref32']['grad_in']) and float(grois.min()) == 7.0
    # a violated CHECK surfaces as an error, not as an abort: C != output_dim * group_size^2
    rc = lib.psroi_pooling(_p(x), _p(rois), _p(out), _p(mapping), None, None, None, c['B'], c['C'], c['H'], c['W'], c['R'],
                           c['output_dim'] + 1, c['P'], c['g'], c['scale'], 1, 1)
    assert rc == -1 and b'group_size' in lib.psroi_last_error()
