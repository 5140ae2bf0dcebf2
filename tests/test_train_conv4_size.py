"""The size the training step makes its early RPN anchor targets for (train.conv4_hw, before the trunk has run) is the size of
conv4: conv1 7x7 / 2 pad 3, pool1 3x3 / 2 with MXNet's 'full' (ceil) convention, then the stride-2 1x1 convolutions of the
trunk's projection units in res3 and res4 -- here run as torch.nn.functional convolutions and pooling on a zero image."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.mark.parametrize('hw', [(600, 1000), (600, 901), (128, 160), (256, 320), (599, 999), (37, 41), (33, 65), (17, 18),
                                (1000, 600), (801, 1333), (64, 63), (9, 11)])
def test_conv4_size_of_the_early_anchor_targets(hw):
    import relnet_amd  # noqa: F401
    from relnet_amd import train
    from relnet_amd.backbone import unit_names
    x = torch.zeros(1, 3, *hw)
    x = F.conv2d(x, torch.zeros(64, 3, 7, 7), stride=2, padding=3)
    x = F.max_pool2d(x, 3, stride=2, ceil_mode=True)
    for u in unit_names(False):
        stage, stride = u[0], u[5]
        if stage in (3, 4) and stride != 1:
            x = F.conv2d(x[:, :1], torch.zeros(1, 1, 1, 1), stride=stride)
    assert train.conv4_hw(*hw) == tuple(x.shape[2:]), hw
