"""Staged training, data parallel (CPU, gloo, world_size 2): the exchange of a staged pass -- an early bucket
(allreduce_begin), the rest of the trainable slices (allreduce_begin_rest with ranges) and the tail
(allreduce_gradient_and_stats with ranges) -- sums exactly the trainable slices: both ranks end with the same trainable
values, and a frozen slice, which each rank fills with its own marker here, is never exchanged."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3000
RANGES = [(250, 1000), (1100, 3000)]   # frozen: [0, 250) (two blocks) and [1000, 1100) (the anchor nets)
EARLY = (1100, 3000)                   # the classification net's bucket, started before the backbone's


def _grad(rank):
    g = np.random.RandomState(rank).randn(N).astype(np.float32)
    mask = np.zeros(N, bool)
    for lo, hi in RANGES:
        mask[lo:hi] = True
    g[~mask] = 1000.0 + rank            # a value an exchange would change
    return g


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from frcnn_amd import objective as OBJ
    g = torch.from_numpy(_grad(rank))
    pending = [OBJ.allreduce_begin(g, *EARLY)]
    pending = OBJ.allreduce_begin_rest(g, pending, RANGES)
    assert sorted((p[0], p[1]) for p in pending) == [(250, 1000), EARLY]
    tot = OBJ.allreduce_gradient_and_stats(g, np.arange(8.0) * (rank + 1), pending, RANGES)
    np.save(os.path.join(out_dir, "g%d.npy" % rank), g.numpy())
    np.save(os.path.join(out_dir, "t%d.npy" % rank), tot)
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_staged_exchange_sums_the_trainable_slices_only(tmp_path):
    import torch.multiprocessing as mp
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    g0, g1 = np.load(tmp_path / "g0.npy"), np.load(tmp_path / "g1.npy")
    want = _grad(0) + _grad(1)
    for lo, hi in RANGES:
        assert np.array_equal(g0[lo:hi], g1[lo:hi]) and np.array_equal(g0[lo:hi], want[lo:hi])
    for rank, g in ((0, g0), (1, g1)):
        assert np.all(g[:250] == 1000.0 + rank) and np.all(g[1000:1100] == 1000.0 + rank)
    assert np.load(tmp_path / "t0.npy").tolist() == (np.arange(8.0) * 3).tolist()
