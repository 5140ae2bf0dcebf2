"""cfg.roi_align together with cfg.dcn is refused at construction: the DCN graph pools with deformable PSROI pooling and has no
ROIPooling to replace (detector.check_pooling).  The check runs before any parameter or device is touched."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _mods():
    import relnet_amd  # noqa: F401
    from relnet_amd import detector, train
    return detector, train


def test_dcn_with_roi_align_is_refused():
    detector, train = _mods()
    cfg = detector.Config()
    cfg.dcn, cfg.roi_align = True, True
    with pytest.raises(ValueError, match='roi_align'):
        detector.Detector({}, cfg=cfg, device='cpu')
    tcfg = train.TrainConfig()
    tcfg.dcn, tcfg.roi_align = True, True
    with pytest.raises(ValueError, match='roi_align'):
        train.Trainer({}, tcfg, device='cpu')


def test_roi_align_and_dcn_alone_pass_the_check():
    detector, _ = _mods()
    for dcn, align in ((True, False), (False, True), (False, False)):
        cfg = detector.Config()
        cfg.dcn, cfg.roi_align = dcn, align
        detector.check_pooling(cfg)
