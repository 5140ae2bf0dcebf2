"""CPU checks of the trainable stem (no GPU): the restatements of tests/stem_train_cases.py against torch's own max-pool backward and a
float64 convolution gradient, the assertions that the tie rule and the accumulation order MATTER on exactly the inputs the GPU tests use,
`train.check_fixed_params` through the trainers' constructors, and the declaration / binding of the new entry points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stem_train_cases as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ['%dx%d' % hw for hw in SC.POOL_CASES]


def _case(hw, bf16=True):
    c = SC.pool_case(*hw)
    out = SC.pool_forward(c['conv'], c['bias'], bf16)
    return c, out


@pytest.mark.parametrize('hw', SC.POOL_CASES, ids=IDS)
def test_pool_restatement_matches_torch_autograd(hw):
    """torch's max_pool2d (ceil mode) sends the gradient to the first maximum in row-major order too: the restatement equals autograd of
    relu(max_pool2d(conv) + bias) wherever a pixel gets at most one non-zero term, and within float32 rounding of it everywhere."""
    import torch
    import torch.nn.functional as F
    c, out = _case(hw, bf16=False)
    x = torch.tensor(c['conv']).permute(0, 3, 1, 2).double().requires_grad_(True)
    y = torch.relu(F.max_pool2d(x, 3, 2, 0, ceil_mode=True) + torch.tensor(c['bias']).double().view(1, -1, 1, 1))
    assert tuple(y.shape[2:]) == SC.pooled_hw(*hw)
    assert np.array_equal(y.detach().permute(0, 2, 3, 1).numpy().astype(np.float32), out)
    y.backward(torch.tensor(c['d_out']).permute(0, 3, 1, 2).double())
    want = x.grad.permute(0, 2, 3, 1).numpy()
    got = SC.pool_backward(c['conv'], out, c['d_out'], bf16=False)
    scale = np.abs(c['d_out']).max()
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * 4 * scale
    assert np.count_nonzero(got) > 0 or hw == (3, 3)


@pytest.mark.parametrize('hw', SC.POOL_CASES, ids=IDS)
def test_the_tie_rule_decides_something(hw):
    """"last maximum" gives another array than "first maximum" on these inputs, and the placed ties sit where the docstring says."""
    c, out = _case(hw)
    conv = c['conv']
    first = SC.pool_backward(conv, out, c['d_out'], bf16=True)
    last = SC.pool_backward(conv, out, c['d_out'], bf16=True, last=True)
    assert not np.array_equal(first, last)
    Ho, Wo = SC.pooled_hw(*hw)
    # inside one window: (0, 0) takes window (0, 0)'s gradient on channels 0..31, its twin (0, 1) nothing
    live = out[0, 0, 0, :32] > 0
    assert live.all() and np.array_equal(first[0, 0, 0, :32], SC.to_bf16(c['d_out'][0, 0, 0, :32])) and not first[0, 0, 1, :32].any()
    assert not last[0, 0, 0, :32].any()
    if Wo >= 2:       # shared by two windows: (0, 2) is later than (0, 0) in window (0, 0) and the first maximum of window (0, 1)
        assert np.array_equal(first[0, 0, 2, :32], SC.to_bf16(c['d_out'][0, 0, 1, :32])) and not first[0, 1, 3, :32].any()
    if Ho >= 2 and Wo >= 2:       # shared by four windows: (2, 2) takes all four, (3, 3) none; under "last" (3, 3) takes window (1, 1)'s
        four = c['d_out'][0, 0, 0, 32:48] + c['d_out'][0, 0, 1, 32:48]
        four = (four + c['d_out'][0, 1, 0, 32:48]).astype(np.float32)
        four = (four + c['d_out'][0, 1, 1, 32:48]).astype(np.float32)
        assert np.array_equal(first[0, 2, 2, 32:48], SC.to_bf16(four)) and not first[0, 3, 3, 32:48].any()
        assert np.array_equal(last[0, 3, 3, 32:48], SC.to_bf16(c['d_out'][0, 1, 1, 32:48]))
    # the all-negative window: out is 0 there and nothing flows back to the pixels only it covers
    assert not out[1, 0, 0].any() and not first[1, 0:2, 0:2].any()


@pytest.mark.parametrize('hw', [hw for hw in SC.POOL_CASES if min(SC.pooled_hw(*hw)) >= 2], ids=lambda hw: '%dx%d' % hw)
def test_the_accumulation_order_decides_something(hw):
    """Pixel (2, 2) of image 0, channels 48..63: 2^27 + 1 - 2^27 + 1 is 1 in ascending window order and 0 in descending order."""
    c, out = _case(hw)
    fwd = SC.pool_backward(c['conv'], out, c['d_out'], bf16=True)
    rev = SC.pool_backward(c['conv'], out, c['d_out'], bf16=True, reverse=True)
    assert (fwd[0, 2, 2, 48:] == 1.0).all() and (rev[0, 2, 2, 48:] == 0.0).all()
    assert not np.array_equal(fwd, rev)


@pytest.mark.parametrize('case', SC.WGRAD_CASES, ids=[c[0] for c in SC.WGRAD_CASES])
def test_wgrad_restatement_matches_float64_autograd(case):
    import torch
    import torch.nn.functional as F
    id_, B, H, W = case
    img, d = SC.wgrad_case(*case)
    Hc, Wc = SC.conv_hw(H, W)
    assert d.shape == (B, Hc, Wc, 64)
    if id_ == 'chunk+1':
        assert B * Hc * Wc == SC.CHUNK + 1
    if id_ == '8x8':
        assert (Hc, Wc) == (4, 4)
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(torch.tensor(img).double(), w, stride=2, padding=3)
    (y * torch.tensor(d).double().permute(0, 3, 1, 2)).sum().backward()
    want = w.grad.permute(0, 2, 3, 1).reshape(64, 147).numpy()
    got, ab, n = SC.wgrad_float64(img, d)
    assert n == B * Hc * Wc and np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
    assert (ab >= np.abs(got) - 1e-9).all()


def _trainers():
    sys.path.insert(0, ROOT)
    import relnet_amd  # noqa: F401
    from relnet_amd import train
    return train


@pytest.mark.parametrize('cls,fixed,words', [
    ('Trainer', ['res2', 'bn2', 'gamma', 'beta'], 'conv1 trainable under a fixed res2'),
    ('Trainer', ['conv1', 'res2'], "'gamma' and 'beta' are missing"),
    ('Trainer', [], "'gamma' and 'beta' are missing"),
    ('FPNTrainer', ['gamma', 'beta'], 'lateral gradient of fpn_ft4_1x1 into res2c is missing'),
    ('FPNTrainer', ['conv1', 'bn_conv1', 'gamma', 'beta'], 'lateral gradient of fpn_ft4_1x1 into res2c is missing'),
])
def test_refused_fixed_parameter_lists(cls, fixed, words):
    """The constructors refuse before they touch the parameters or the device."""
    train = _trainers()
    cfg = train.TrainConfig()
    cfg.fixed_params = fixed
    with pytest.raises(ValueError, match=words):
        getattr(train, cls)({}, cfg, device='cpu')


def test_accepted_fixed_parameter_lists():
    train = _trainers()
    from relnet_amd import config as C, dist as D
    shipped = {tuple(C.experiment(name).network.FIXED_PARAMS) for name in C.EXPERIMENTS}
    assert tuple(D.FIXED_PARAMS) in shipped and len(shipped) >= 2
    for fpn in (False, True):
        for fixed in [None] + sorted(shipped):
            cfg = train.TrainConfig()
            cfg.fixed_params, cfg.fpn = (None if fixed is None else list(fixed)), fpn
            assert train.check_fixed_params(cfg) == (False, False)
    cfg = train.TrainConfig()
    cfg.fixed_params = ['conv1', 'bn_conv1', 'gamma', 'beta']
    assert train.check_fixed_params(cfg) == (False, True)
    cfg.fixed_params = ['gamma', 'beta']                                  # the default of the reference's config/config.py
    assert train.check_fixed_params(cfg) == (True, True)
    # ... and the constructor gets past the check: with no parameters it then fails on the first one it reads, not with a ValueError
    for fixed in (None, list(D.FIXED_PARAMS), ['gamma', 'beta']):
        cfg = train.TrainConfig()
        cfg.fixed_params = fixed
        with pytest.raises(KeyError):
            train.Trainer({}, cfg, device='cpu')


def test_symbols_are_declared_and_exported():
    sys.path.insert(0, ROOT)
    import relnet_amd  # noqa: F401
    from relnet_amd import lib, ops
    header = open(os.path.join(ROOT, 'include', 'relnet_hip.h')).read()
    for ret, name in (('int', 'relnet_stem_pool_bwd'), ('int', 'relnet_stem_wgrad'), ('long', 'relnet_stem_wgrad_workspace_bytes')):
        assert name in lib.exported_symbols()
        assert ('%s %s(' % (ret, name)) in header
        assert getattr(lib.load(), name) is not None                       # the built library exports it
    block = header.split("the stem's backward")[1].split('int relnet_stem_wgrad(')[0]          # both declarations cite the reference graph
    assert 'resnet_v1_101_rcnn_base.py:30-36' in block and 'resnet_v1_101_rcnn_base.py:30-31' in block
    assert callable(ops.stem_pool_bwd) and callable(ops.stem_wgrad)
    L = lib.load()
    chunks = lambda b, h, w: L.relnet_stem_wgrad_workspace_bytes(b, h, w) // (64 * 256 * 4)
    assert chunks(1, 17, 241) == 2 and chunks(1, 64, 64) == 1 and chunks(8, 300, 500) == 293      # a function of the shape only
    # argument validation happens before any HIP call
    assert L.relnet_stem_pool_bwd(None, None, None, None, 1, 4, 4, 64, 1, None) != 0 and b'null operand' in L.relnet_last_error()
