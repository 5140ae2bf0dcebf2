"""The guarded optimizer step on two ranks that share cuda:0 and exchange over gloo (tools/dist_guard_check.py): a NaN that only rank 1
produces reaches both ranks through the all-reduce, both skip and keep equal, unchanged weights; the clean step after it moves both and
keeps them equal.  The one place the bucketed branch of Trainer.update() runs with a guard."""
import ast
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def test_two_ranks_skip_together_and_stay_equal():
    from importlib import import_module
    launch = import_module('relation-networks-for-object-detection_amd.launch')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes', '1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(launch.free_port()), os.path.join(ROOT, 'tools', 'dist_guard_check.py')]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    line = [l for l in out.splitlines() if l.startswith('DIST_GUARD_CHECK')]
    assert line, out[-2000:]
    res = ast.literal_eval(line[-1][len('DIST_GUARD_CHECK'):].strip())
    print(res)
    # the bucketed branch ran: five buckets, waited for in launch order, statistics after each wait
    assert res['launch_order'] == [4, 3, 2, 1, 0] and res['update_order'] == [4, 3, 2, 1, 0], res
    assert res['step1_skipped_on_all_ranks'] and res['step1_weights_unchanged_on_all_ranks'] and res['step1_equal_across_ranks'], res
    assert res['step2_applied_on_all_ranks'] and res['step2_weights_moved_on_all_ranks'] and res['step2_equal_across_ranks'], res
    assert res['step2_same_norm_on_all_ranks'] and res['work_copy_is_rounded_master'] and res['step_count'] == 2, res
