"""The last unit of res2 / res3 at the even pixels only (csrc/bottleneck.hip: relnet_bottleneck_chain_s2, relnet_conv3x3_c64_s2;
Backbone.quarter_units): the arithmetic per kept pixel is that of the dense kernels, so every comparison here is bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture
def low_thresholds(monkeypatch):
    import relnet_amd  # noqa: F401
    from relnet_amd import ops
    monkeypatch.setattr(ops, 'CHAIN_MIN_PIXELS', {k: 1 for k in ops.CHAIN_MIN_PIXELS})
    return ops


# (2, 9, 13): odd sizes, 70 compact pixels = two full tiles + a partial one, an image boundary inside a tile; (1, 8, 12): even sizes (the last
# row / column is never read), less than one tile; (3, 21, 35): several lock-step sets; (2, 363, 363): 66 248 compact pixels = 2 071 tiles,
# more than 8 x 256, so some workgroups iterate twice
@pytest.mark.parametrize('shape', [(2, 9, 13), (1, 8, 12), (3, 21, 35), (2, 363, 363)])
@pytest.mark.parametrize('mid', [64, 128])
def test_gather_expand_equals_dense_at_even_pixels(low_thresholds, shape, mid):
    ops = low_thresholds
    B, H, W = shape
    g = torch.Generator(device='cuda').manual_seed(B * 1000 + H + mid)          # (on the device: the largest x is 270 MB)
    m2 = torch.relu(torch.randn(B, H, W, mid, generator=g, device='cuda')).to(BF)
    x = torch.relu(torch.randn(B, H, W, 4 * mid, generator=g, device='cuda')).to(BF)
    w3f = ops.pack_w_frag((torch.randn(4 * mid, mid, generator=g, device='cuda') * 0.1).to(BF))
    b3 = torch.randn(4 * mid, generator=g, device='cuda') * 0.1
    ref = ops.bottleneck_chain(m2, x, w3f, None, b3, None)[0][:, ::2, ::2]
    x0 = x.clone()
    got = ops.bottleneck_chain_s2(m2[:, ::2, ::2].contiguous(), x, w3f, b3)
    assert got.shape == ref.shape and got.is_contiguous()
    assert torch.equal(got, ref)
    assert torch.equal(x, x0)                  # the shortcut operand is only read


@pytest.mark.parametrize('shape', [(2, 9, 13), (1, 8, 12), (2, 33, 49)])
@pytest.mark.parametrize('C', [64, 128])
def test_stride2_3x3_equals_dense_at_even_pixels(shape, C):
    """C = 64: the stride-2 form of the halo kernel against the dense halo kernel; C = 128: the implicit GEMM at stride 2 against
    itself at stride 1."""
    import relnet_amd  # noqa: F401
    from relnet_amd import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(7 * B + H + C)
    x = torch.relu(torch.randn(B, H, W, C, generator=g)).to(BF).cuda()
    w = (torch.randn(C, C, 3, 3, generator=g) * (0.05 if C == 64 else 0.03)).to(BF)
    b = (torch.randn(C, generator=g) * 0.1).cuda()
    wp = ops.pack_conv_weight(w, BF, 'cuda')
    for relu in (True, False):
        if C == 64:
            wf = ops.pack_w_frag(wp, panel_only=False)
            ref = ops.conv3x3_halo(x, wf, b, relu=relu)[:, ::2, ::2]
            got = ops.conv3x3_halo_s2(x, wf, b, relu=relu)
        else:
            ref = ops.conv2d_nhwc(x, wp, b, ksize=3, stride=1, pad=1, relu=relu)[:, ::2, ::2]
            got = ops.conv2d_nhwc(x, wp, b, ksize=3, stride=2, pad=1, relu=relu)
        assert got.shape == ref.shape and torch.equal(got, ref), (shape, C, relu)


def test_backbone_quarter_units_change_no_bit(low_thresholds):
    """2 x 3 x 134 x 198 image: res2 map 33 x 49, res3 map 17 x 25 (both odd).  Switch on: res2c and res3b3 run in the quarter form and
    every output equals the dense trunk's; FPN graphs read the full maps (laterals) and keep the dense path (on a 128 x 192 image: the
    pyramid needs sizes that are multiples of 32)."""
    from relnet_amd import backbone
    p = backbone.init_params(seed=5)
    data = torch.randn(2, 3, 134, 198, generator=torch.Generator().manual_seed(1)).cuda() * 50
    on = backbone.Backbone(p, dtype=BF)
    off = backbone.Backbone(p, dtype=BF)
    assert on.quarter_units
    off.quarter_units = False
    fa, fb = on.forward(data), off.forward(data)
    assert on.last_quarter_units == ['2c', '3b3'] and off.last_quarter_units == []
    assert '2c' in on.last_chain_units and '3b3' in on.last_chain_units
    for k in ('conv4', 'conv5', 'conv_new_1_relu', 'rpn_cls_score', 'rpn_bbox_pred'):
        assert fa[k].shape == fb[k].shape and torch.equal(fa[k], fb[k]), k
    assert tuple(on.forward_res2(data).shape) == (2, 33, 49, 256)          # the trainer's entry still returns the full res2c map
    pf = backbone.init_params(seed=5, fpn=True)
    fb_ = backbone.Backbone(pf, dtype=BF, fpn=True)
    data32 = data[:, :, :128, :192].contiguous()
    ga = fb_.forward(data32)
    assert fb_.quarter_units and fb_.last_quarter_units == [] and '2c' in fb_.last_chain_units
    fb_.quarter_units = False                  # (one instance, toggled: the weights are the same either way)
    gb = fb_.forward(data32)
    assert fb_.last_quarter_units == [] and ga.keys() == gb.keys()
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
