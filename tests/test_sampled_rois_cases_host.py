"""Host checks of the sampled ROI minibatch (TRAIN.BATCH_ROIS > 0): the numpy restatement of tests/sampled_rois_cases.py against the
reference's own sample_rois (tests/golden/sampled_rois.npz), the selection rule, and the plumbing (C-ABI symbol, CustomOp shapes,
trainer configuration and refusals)."""
import os

import numpy as np
import pytest

import sampled_rois_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'sampled_rois.npz'))


@pytest.fixture(scope='module')
def results():
    """The restatement on every case, for both seeds: computed once, shared, never changed."""
    return {name: tuple(SC.sample(SC.case(name), s) for s in SC.SEEDS) for name in SC.CASES}


@pytest.mark.parametrize('name', list(SC.CASES))
def test_restatement_equals_the_reference_run(gold, results, name):
    """Rows, labels, weights and keep_index bit for bit.  The targets' dx / dy columns bit for bit too; dw / dh within 1 ulp of a value below
    ~2 / 0.2 (rtol 3e-7, atol 1e-6, the bound tests/test_oracle_golden.py puts on the same pair): the reference run took numpy's float32 log,
    whose last bit depends on the SIMD path numpy picks, the restatement (like the kernel) pins the correctly rounded one."""
    got = results[name][0]
    for k in ('rois_out', 'label', 'bbox_weight', 'keep_index'):
        np.testing.assert_array_equal(got[k], gold[name + '/' + k], err_msg=k)
    bt, want = got['bbox_target'], gold[name + '/bbox_target']
    assert bt.dtype == want.dtype == np.float32 and bt.shape == want.shape
    np.testing.assert_array_equal(bt[..., 0::4], want[..., 0::4])
    np.testing.assert_array_equal(bt[..., 1::4], want[..., 1::4])
    np.testing.assert_array_equal(bt != 0, want != 0)
    np.testing.assert_allclose(bt, want, rtol=3e-7, atol=1e-6)


@pytest.mark.parametrize('name', list(SC.CASES))
def test_every_selection_is_valid(results, name):
    c = SC.case(name)
    fg_rois = SC.fg_rois_per_image(c['fg_fraction'], c['R'])
    for b, p in enumerate(results[name][0]['per_image']):
        nr = c['N'] if c['num_rois'] is None else int(c['num_rois'][b])
        M = nr + (int(c['num_gt'][b]) if c['append_gt'] else 0)
        keep = p['keep_index']
        assert keep.shape == (c['R'],) and keep.min() >= 0 and keep.max() < M
        n_fg, n_bg = min(fg_rois, len(p['fg'])), 0
        n_bg = min(c['R'] - n_fg, len(p['bg']))
        fg_part, bg_part = keep[:n_fg], keep[n_fg:n_fg + n_bg]
        assert set(fg_part) <= set(p['fg']) and set(bg_part) <= set(p['bg'])
        assert (np.diff(fg_part) > 0).all() and (np.diff(bg_part) > 0).all()              # distinct, ascending
        for stream, members, take, chosen in p['picks']:
            assert len(chosen) == take == len(set(chosen)) and set(chosen) <= set(members) and (np.diff(chosen) > 0).all()
            w = SC.words(SC.SEEDS[0], b, stream, members)
            assert len(set(w.tolist())) == len(members)                                    # the words are unique
            assert SC.words(SC.SEEDS[0], b, stream, chosen).max() < np.sort(w)[take]        # ... and the chosen ones the smallest
        pos = n_fg + n_bg
        t = 0
        while pos < c['R']:                     # padding rounds: each distinct within itself, drawn from all M
            gap = min(M, c['R'] - pos)
            part = keep[pos:pos + gap]
            assert (np.diff(part) > 0).all()
            pos, t = pos + gap, t + 1
        assert t == {'short': 1, 'tiny': 3}.get(name, t)


def test_case_properties(results, gold):
    """What each small case is there for (tests/sampled_rois_cases.py CASES)."""
    per = lambda name: results[name][0]['per_image'][0]
    sizes = lambda name: (len(per(name)['fg']), len(per(name)['bg']))
    assert sizes('exact-fit') == (2, 6) and per('exact-fit')['n_choice'] == 0 and int(gold['exact-fit/n_choice'][0]) == 0
    np.testing.assert_array_equal(gold['exact-fit/keep_index'][0], [12, 13, 0, 2, 4, 6, 8, 10])     # the reference's own order
    assert sizes('many-fg') == (9, 6) and sizes('many-bg') == (2, 11) and sizes('both') == (8, 7)
    s = per('short')
    assert sizes('short') == (3, 3) and len(set(s['keep_index'][5:]) - set(s['fg']) - set(s['bg'])) > 0      # a neither-set row was padded in
    t = per('tiny')['keep_index']
    assert len(set(t)) == 2 and len(t) == 8
    e = per('edges')
    assert list(e['fg']) == [3] and list(e['bg']) == [8]                   # IoU exactly 0.5 is fg (not bg), exactly 0.1 is bg at BG_THRESH_LO 0.1
    assert e['label'][0] == 4 and e['label'][1] == 0
    assert SC.overlaps(np.array([[0, 0, 9, 4.]]), np.array([[0, 0, 9, 9.]]))[0, 0] == 0.5
    assert SC.overlaps(np.array([[0, 0, 9, 0.]]), np.array([[0, 0, 9, 9.]]))[0, 0] == 0.1
    assert per('no-append')['keep_index'].max() < 12
    cs = results['class-specific'][0]
    assert cs['bbox_target'].shape == (1, 8, 20) and (cs['bbox_weight'][0, 0].reshape(5, 4).sum(1) > 0).tolist().index(True) == int(cs['label'][0, 0])
    bt = results['batch'][0]
    assert [len(p['fg']) for p in bt['per_image']][2] == 0 and (bt['label'][2] == 0).all() and (bt['bbox_weight'][2] == 0).all()
    assert bt['keep_index'][1].max() < 8                                   # num_rois 7 + one gt row: rows 7 .. 11 of image 1 are never candidates
    assert (bt['rois_out'][1, :, 0] == 1).all()
    for name in ('large', 'limit'):
        assert len(per(name)['fg']) > 128 and len(per(name)['bg']) > 384 and (results[name][0]['label'] > 0).sum() == 128
    lim = SC.case('limit')
    assert lim['N'] + lim['gt'].shape[1] == SC.LIMIT


@pytest.mark.parametrize('name', SC.SAMPLED)
def test_two_seeds_give_different_subsets(results, name):
    a, b = results[name]
    assert not np.array_equal(a['keep_index'], b['keep_index'])


def test_key32_extends_the_anchor_hash():
    """Stream 0 is the anchor sampler's hash (oracle/anchors.py restates it); other streams differ."""
    from oracle import anchors as OA
    idx = np.arange(0, 5000, 7)
    k0 = SC.key32(SC.SEEDS[0], 3, 0, idx)
    np.testing.assert_array_equal(k0, np.asarray(OA.anchor_key(SC.SEEDS[0], 3, idx), dtype=np.uint32))
    assert (SC.key32(SC.SEEDS[0], 3, 1, idx) != k0).mean() > 0.99
    assert len(set(k0.tolist())) == len(idx)


def test_fg_rois_rounding():
    assert [SC.fg_rois_per_image(0.25, r) for r in (10, 6, 128)] == [2, 2, 32]             # round half to even, as np.round in the reference
    assert [int(round(0.25 * r)) for r in (10, 6, 128)] == [2, 2, 32]                      # what ops.proposal_target computes


def test_symbol_is_declared_and_exported():
    import relnet_amd  # noqa: F401
    from relnet_amd import lib
    name = 'relnet_proposal_target_sample'
    assert name in lib.exported_symbols()
    assert ('int %s(' % name) in open(os.path.join(ROOT, 'include', 'relnet_hip.h')).read()
    assert getattr(lib.load(), name) is not None                           # the built library exports it


@pytest.mark.parametrize('batch_rois,rows', [(-1, 15), (-2, 12), (-128, 128), (128, 128)])
def test_custom_op_infer_shape(batch_rois, rows):
    import relnet_amd  # noqa: F401
    from relnet_amd import operator_py
    prop = operator_py.get_prop('proposal_target')(num_classes='2', batch_images='1', batch_rois=str(batch_rois), fg_fraction='0.25')
    ins, outs = prop.infer_shape([(12, 5), (3, 5)])[:2]
    assert outs == [(rows, 5), (rows,), (rows, 8), (rows, 8)] and ins == [(12, 5), (3, 5)]
    prop.create_operator(None, ins, None)                                  # every form constructs


def test_train_config_and_refusals():
    import relnet_amd  # noqa: F401
    from relnet_amd import train
    cfg = train.TrainConfig()
    assert cfg.batch_rois == -1 and (cfg.fg_fraction, cfg.fg_thresh, cfg.bg_thresh_lo) == (0.25, 0.5, 0.0)
    train.check_batch_rois(cfg)                                            # today's setting passes, relation graph or not
    e = train.TrainConfig.from_experiment('rcnn_end2end_relation_8epoch', train=True)
    assert e.batch_rois == -1 and e.fg_fraction == 0.25 and e.bg_thresh_lo == 0.0
    for flag in ('relation', 'learn_nms'):
        cfg = train.TrainConfig()
        cfg.batch_rois, cfg.relation, cfg.learn_nms = 128, False, False
        train.check_batch_rois(cfg)
        setattr(cfg, flag, True)
        with pytest.raises(ValueError, match='BATCH_ROIS'):
            train.check_batch_rois(cfg)
    cfg = train.TrainConfig()
    cfg.batch_rois, cfg.relation = -2, False
    with pytest.raises(ValueError, match='BATCH_ROIS'):
        train.check_batch_rois(cfg)


def test_from_experiment_divides_by_batch_images(monkeypatch):
    """TRAIN.BATCH_ROIS counts a whole BATCH_IMAGES batch (proposal_target.py:60): the config tree's defaults are 128 rois over 2 images."""
    import relnet_amd  # noqa: F401
    from relnet_amd import config, train
    name = 'rcnn_end2end_relation_8epoch'
    real = config.experiment

    def patched(n):
        e = real(n)
        e.TRAIN.BATCH_ROIS, e.TRAIN.BATCH_IMAGES, e.TRAIN.BG_THRESH_LO = 128, 2, 0.1
        return e
    monkeypatch.setattr(config, 'experiment', patched)
    c = train.TrainConfig.from_experiment(name, train=True)
    assert c.batch_rois == 64 and c.bg_thresh_lo == 0.1
