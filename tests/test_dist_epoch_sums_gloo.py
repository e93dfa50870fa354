"""CPU, world_size 2 over gloo: distributed.allreduce_epoch_sums, the once-per-epoch fp64 SUM of the two epoch accumulators
(training and validation rows) that gives every rank the same logs -- the function Trainer.fit calls with backend nccl (= RCCL)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ubdvss_amd import distributed as ud, keras_metrics


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _rank_sums(rk):
    """what rank rk's accumulators could hold after an epoch: seen, non-finite count, eleven weighted sums; two rows"""
    rng = np.random.default_rng(100 + rk)
    sums = rng.random((2, 2 + len(keras_metrics.EPOCH_VALUES))) * 10
    sums[:, 0] = [6 + rk, 3 + rk]
    sums[:, 1] = [rk, 0]
    return sums


def _worker(rk, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rk), WORLD_SIZE=str(world), LOCAL_RANK=str(rk))
    ud.init_from_env(backend="gloo")
    torch.set_num_threads(1)
    t = torch.from_numpy(_rank_sums(rk).copy())
    out = ud.allreduce_epoch_sums(t)
    assert out.dtype == torch.float64
    np.save(os.path.join(out_dir, f"r{rk}.npy"), out.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_epoch_sums_allreduce_two_ranks(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0, r1 = np.load(tmp_path / "r0.npy"), np.load(tmp_path / "r1.npy")
    assert np.array_equal(r0, r1)                                  # every rank forms its logs from the same sums
    assert np.array_equal(r0, _rank_sums(0) + _rank_sums(1))       # two fp64 terms: the sum is exact in either order
    logs = keras_metrics.epoch_logs_from_sums(r0[0], True)
    assert logs["loss"] == (_rank_sums(0) + _rank_sums(1))[0, 2] / 13


def test_epoch_sums_single_process_and_dtype():
    t = torch.from_numpy(_rank_sums(0).copy())
    assert ud.allreduce_epoch_sums(t) is t and np.array_equal(t.numpy(), _rank_sums(0))
    with pytest.raises(ValueError, match="float64"):
        ud.allreduce_epoch_sums(t.float())
