"""chain256_roles_kernel (csrc/bottleneck.hip, relnet_bottleneck_chain at mid 256 with the reduce product) carries the bits it carried before its
step structure was rewritten (64-channel steps, W1' fragments from registers): SHA-256 of the raw bytes of x_next and mid1' on the seeded `r256`
operands of tests/trunk_cases.py, out of place and in place over the shortcut, against constants recorded from the kernel of commit f1dc4e7
("Train conv1 and res2 when FIXED_PARAMS leaves them trainable"), the last one with 32-channel steps and W1' through LDS.

tests/test_gpu_trunk_edges.py pins x_next of this form to the expand-only kernel bit for bit but holds mid1' only to a float64 tolerance; this
file is the pin for mid1': every accumulator must see the same operands in the same order (pass ascending, then kk = 0..3) with the same
rounding points.

P = 1 (one pixel), 129 (a second set with one live pixel), 32901 (258 sets: a second iteration in two workgroups, ragged last tile) and
65537 (a third iteration).  The largest case has ~ 170 MB of operands; every case runs in well under a second."""
import hashlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trunk_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu

PARENT = 'f1dc4e7'
#: P -> (sha256 of x_next [P, 1024] bf16, sha256 of mid1' [P, 256] bf16), from the kernel of PARENT (out of place; in place gave the same there)
SHA = {
    1: ('fae9f56161ba87d02dabeca8b9fd295fe315c50955f3b55828878d45f4cfb202', '7bdea3b606cf79179526d3ac4c645fdb6a3dbbe7d290ea35085bdb5354d14efb'),
    129: ('276d5e13957b1135a59b6dc99459972f512fe19099080e5a882512d7453a2276', 'b911989f343090bad80e8360d5084c3d33b9311f4b9d904d5e8b455c3f884c95'),
    32901: ('60194746694c06efb3650d65fc602edd0e013a86f6dd61ad8da40f4f62ffb77a', '855ad669f4d8202df54bcabd40ca3afcb11429f2f3edaf0f8495e907bf923a08'),
    65537: ('0cc548581d4e742ccb505c85dc5494f5f299aecce2fb9e5812285751a8934dc1', 'f707220be98cda7c710ebd4c225061a3c3a24b2bc667b5ee4db77e857784af65'),
}


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


_STATE = {}


def _setup():
    if not _STATE:
        import relnet_amd  # noqa: F401
        from relnet_amd import ops, lib
        lib.load()
        w = TC.chain_weights(256, 'cuda')
        _STATE.update(ops=ops, w3f=ops.pack_w_frag(w['w3']), w1f=ops.pack_chain_w1(w['w1']), b3=w['b3'], b1=w['b1'])
    return _STATE


def run_case(P, inplace):
    """-> (sha256 of x_next, sha256 of mid1') of the seeded r256 case through ops.bottleneck_chain."""
    s = _setup()
    o = TC.chain_operands('r256', P, 'cuda')
    x = o['x']
    xn, m1 = s['ops'].bottleneck_chain(o['m2'], x, s['w3f'], s['w1f'], s['b3'], s['b1'], inplace=inplace)
    torch.cuda.synchronize()
    assert (xn.data_ptr() == x.data_ptr()) == inplace
    assert tuple(xn.shape) == (P, 1024) and tuple(m1.shape) == (P, 256)
    return sha(xn), sha(m1)


@pytest.mark.parametrize('inplace', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('P', sorted(SHA))
def test_chain256_outputs_carry_the_bits_of_the_parent_kernel(P, inplace):
    got = run_case(P, inplace)
    print('r256 P = %6d %s: x_next %s  mid1 %s' % (P, 'in place' if inplace else 'out of place', got[0], got[1]))
    assert got[0] == SHA[P][0], ('x_next differs from the kernel of %s' % PARENT, P, inplace)
    assert got[1] == SHA[P][1], ('mid1_next differs from the kernel of %s' % PARENT, P, inplace)
