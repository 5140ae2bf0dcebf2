"""TrainMetrics.get(reduce=True) over two gloo ranks on the CPU: the accumulator copy is summed over the ranks (int64 counts and
float64 sums: exact), reduce=False stays local, and the local accumulator is left as it was."""
import os
import socket

import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


def _fill(rank):
    """(counts, sums) a rank's step kernels would have left: distinct per rank, sums that are not exactly representable sums."""
    g = torch.Generator().manual_seed(7 + rank)
    return torch.randint(0, 1 << 40, (16,), generator=g), torch.rand(8, generator=g, dtype=torch.float64) * 1e3


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import sys
    import types
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import relnet_amd  # noqa: F401
    from relnet_amd import dist as D, metric as M
    D.init(backend='gloo')
    tm = M.TrainMetrics(types.SimpleNamespace(learn_nms=True), device='cpu')
    c, s = _fill(rank)
    tm.counts.copy_(c); tm.sums.copy_(s)
    local = tm.get_counts()
    summed = tm.get_counts(reduce=True)
    names, values = tm.get(reduce=True)
    q.put((rank, local, summed, names, values, tm.get_counts()))
    D.fence()
    torch.distributed.destroy_process_group()


def test_reduce_sums_both_ranks_and_local_stays_local():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import relnet_amd  # noqa: F401
    from relnet_amd import metric as M
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (c0, s0), (c1, s1) = _fill(0), _fill(1)
    want_sum, want = [], {0: [], 1: []}
    for n in res[0][3]:
        slot, is_int, inst = M._SLOTS[n]
        for r, (c, s) in ((0, (c0, s0)), (1, (c1, s1))):
            want[r].append((int(c[slot]) if is_int else float(s[slot]), int(c[inst])))
        want_sum.append((int(c0[slot] + c1[slot]) if is_int else float(s0[slot] + s1[slot]), int(c0[inst] + c1[inst])))
    for rank, local, summed, names, values, after in res:
        assert names == M.RPN_NAMES + M.RCNN_NAMES + M.NMS_NAMES
        assert local == want[rank] and after == want[rank]                 # reduce=False is local; reducing changed nothing locally
        assert summed == want_sum                                          # equal, not close: integer and float64 sums of two values
        assert values == [s / n for s, n in want_sum]
