"""Multi-process harness of bench.py on CPU (gloo, world_size 2): the
replica timing takes the max time and the summed work over ranks."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    elapsed = [0.5, 0.75][rank]
    iters = [30, 34][rank]
    dist.barrier()
    out = bench.reduce_over_ranks(dist, elapsed, iters, "cpu")
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_reduce_over_ranks_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        assert res[r] == (0.75, 64.0)


def test_reduce_single_process():
    import bench
    assert bench.reduce_over_ranks(None, 0.2, 7, "cpu") == (0.2, 7.0)


def test_dump_outputs_writes_the_align_results(tmp_path):
    """--dump-outputs: the pose, the Hessian and the result's scalar fields as float .npy files."""
    import numpy as np
    import bench
    from dynamic_direct_lidar_odometry_amd import GicpResult
    pose = np.arange(16, dtype=np.float32).reshape(4, 4)
    res = GicpResult(converged=1, nr_iterations=3, iterations_run=3, lm_trials=4, num_correspondences=131000,
                     final_cost=0.125, lm_lambda=1e-9, device_ms=7.0)
    for i in range(36):
        res.final_hessian[i] = i + 0.5
    d = tmp_path / "dump"
    bench.dump_outputs(str(d), pose, res)
    assert sorted(p.name for p in d.iterdir()) == ["final_hessian.npy", "pose.npy", "result.npy"]
    p = np.load(d / "pose.npy")
    assert p.dtype == np.float32 and (p == pose).all()
    h = np.load(d / "final_hessian.npy")
    assert h.dtype == np.float64 and (h == (np.arange(36) + 0.5).reshape(6, 6)).all()
    r = np.load(d / "result.npy")
    assert r.dtype == np.float64 and len(r) == len(bench.RESULT_FIELDS)
    assert dict(zip(bench.RESULT_FIELDS, r)) == {"converged": 1, "nr_iterations": 3, "iterations_run": 3,
                                                 "lm_failed": 0, "lm_trials": 4, "num_correspondences": 131000,
                                                 "final_cost": 0.125, "lm_lambda": 1e-9}
