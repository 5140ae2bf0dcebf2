#!/usr/bin/env python
"""Build the reference's graphs by running ITS OWN graph files (relation_rcnn/symbols/*.py, imported unchanged from
/root/reference) on the `relnet_amd.mx` facade, and store them as JSON fixtures under tests/golden/symbols/.

Needs a reference checkout; the tests do not: the `-m gpu` tests load these fixtures with `mx.sym.load`, bind them on the GPU
and compare with the hand-wired Detector and the oracle, and tests/test_mx_facade.py holds the facade to RECORD
(tests/golden/reference_graphs.json, written here too): for all ten shipped experiments, the symbol their YAML names and the
signature of both graphs (argument / auxiliary counts and digests, outputs, the inferred rois shape), and the digest of
every fixture's text.

    python tests/golden/gen_symbol_json.py [--ref <reference checkout>] [--check]
"""
import argparse
import hashlib
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

#: (experiment, is_train, entry) -> fixture name
FIXTURES = [('rcnn_end2end_8epoch', False), ('rcnn_end2end_relation_8epoch', False), ('rcnn_end2end_relation_8epoch', True),
            ('rcnn_end2end_relation_learn_nms_8epoch', False), ('rcnn_dcn_end2end_relation_8epoch', False),
            ('rcnn_fpn_relation_8epoch', False)]
RECORD = os.path.join(HERE, 'reference_graphs.json')


def _sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def signature(sym, infer_rois):
    """What the tests compare a graph by: counts and digests of its argument / auxiliary names, its outputs, and (test graphs
    of the single-scale experiments) the rois shape inferred at one 600x1000 image."""
    args, aux = sym.list_arguments(), sym.list_auxiliary_states()
    sig = {'n_arguments': len(args), 'arguments_sha256': _sha('\n'.join(args)), 'n_aux': len(aux), 'aux_sha256': _sha('\n'.join(aux)),
           'outputs': sym.list_outputs(), 'rois_output': None}
    if infer_rois:
        _, out, _ = sym.infer_shape(data=(1, 3, 600, 1000), im_info=(1, 3))
        sig['rois_output'] = list(dict(zip(sym.list_outputs(), out))['rois_output'])
    return sig


def record(ref):
    from relnet_amd import config as C
    rec = {'experiments': {}, 'fixtures': {}}
    for name in sorted(C.EXPERIMENTS):
        yaml_cfg = C.update_config(os.path.join(ref, 'experiments', 'relation_rcnn', 'cfgs',
                                                'resnet_v1_101_coco_trainvalminus_%s.yaml' % name), C._defaults())
        rec['experiments'][name] = {'yaml_symbol': yaml_cfg.symbol, 'graphs': {
            mode: signature(build(ref, name, mode == 'train'), mode == 'test' and 'fpn' not in name) for mode in ('test', 'train')}}
    for name, is_train in FIXTURES:
        rec['fixtures']['%s_%s.json' % (name, 'train' if is_train else 'test')] = _sha(_text(build(ref, name, is_train)))
    return rec


def _text(sym):
    return json.dumps(json.loads(sym.tojson()), separators=(',', ':'))


def build(ref, name, is_train):
    import relnet_amd  # noqa: F401
    from relnet_amd import mx, config as C, py2compat
    mx.install()
    py2compat.add_source_dir(os.path.join(ref, 'relation_rcnn', 'symbols'))
    cfg = C.experiment(name)
    mx.sym.reset_names()
    mod = importlib.import_module(cfg.symbol)
    net = getattr(mod, cfg.symbol)()
    sym = net.get_symbol_rcnn(cfg, is_train=is_train) if 'fpn' in name else net.get_symbol(cfg, is_train=is_train)
    return sym


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    ap.add_argument('--check', action='store_true', help='compare with the committed fixtures instead of writing')
    a = ap.parse_args()
    out = os.path.join(HERE, 'symbols')
    os.makedirs(out, exist_ok=True)
    for name, is_train in FIXTURES:
        text = _text(build(a.ref, name, is_train))
        path = os.path.join(out, '%s_%s.json' % (name, 'train' if is_train else 'test'))
        if a.check:
            assert open(path).read() == text, path
            print('same', path)
        else:
            with open(path, 'w') as f:
                f.write(text)
            print('wrote %s (%d bytes, %d nodes)' % (path, len(text), len(json.loads(text)['nodes'])))
    rec = json.dumps(record(a.ref), indent=1, sort_keys=True) + '\n'
    if a.check:
        assert open(RECORD).read() == rec, RECORD
        print('same', RECORD)
    else:
        with open(RECORD, 'w') as f:
            f.write(rec)
        print('wrote %s' % RECORD)


if __name__ == '__main__':
    main()
