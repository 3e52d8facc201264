"""`reduce_over_ranks` of `eqxvision_amd.metrics` on CPU: two gloo processes with different counters whose sums pass 2^24 (where the
fp32 all-reduce of `dist.all_reduce_sum_` stops being exact) and 2^32; both ranks must end with the exact integer sum."""
import os
import socket

import numpy as np
import torch
import torch.multiprocessing as mp

C = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _matrix(rank):
    m = np.arange(C * C, dtype=np.int64).reshape(C, C) * (rank + 1)
    m[0, 0] = 2 ** 24 + 1 + rank              # the sum 2^25 + 3 is odd: fp32 cannot hold it
    m[1, 2] = 2 ** 32 + 5 + 7 * rank
    m[2, 1] = 2 ** 40 * (rank + 1) + 1
    return m


def _counts(rank):
    return np.array([2 ** 24 + 1 + rank, 2 ** 33 + 3 * rank, 2 ** 34 + 1], np.int64)


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from eqxvision_amd import dist as D
    from eqxvision_amd import metrics as M
    D.init_from_env("gloo")
    cm = M.ConfusionMatrix(C, device="cpu")
    cm.mat.copy_(torch.from_numpy(_matrix(rank)))
    cm.reduce_over_ranks()
    acc = M.TopK((1, 5), device="cpu")
    acc.counts.copy_(torch.from_numpy(_counts(rank)))
    acc.reduce_over_ranks()
    q.put((rank, cm.mat.numpy().copy(), acc.counts.numpy().copy(), cm.compute()["mean_iou"]))
    torch.distributed.destroy_process_group()


def test_reduce_over_ranks_is_exact_gloo():
    from eqxvision_amd import metrics as M
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in ps]
    res = [q.get(timeout=120) for _ in range(world)]
    [p.join(60) for p in ps]
    want, want_counts = _matrix(0) + _matrix(1), _counts(0) + _counts(1)
    assert want[0, 0] == 2 ** 25 + 3 and np.float32(want[0, 0]) != want[0, 0] and want[1, 2] > 2 ** 32
    assert sorted(r for r, *_ in res) == [0, 1]
    for _, mat, counts, miou in res:
        assert mat.dtype == np.int64 and np.array_equal(mat, want)
        assert np.array_equal(counts, want_counts)
        assert miou == M.metrics_from_matrix(want)["mean_iou"]
