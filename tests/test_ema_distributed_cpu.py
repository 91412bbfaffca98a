"""Weight EMA across ranks on CPU (world size 2, gloo, host-emulated kernels; pattern of tests/test_finetune_distributed_cpu.py): with and
without ZeRO-1 the averaged parameters and the counters are identical on both ranks, and the ZeRO-1 run's average - made behind the parameter
all-gather, over the whole active range on every rank - is bitwise the unsharded run's."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _worker(rank, world, port):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import ctypes
    import build_emu
    from transfuser_amd import _lib
    _lib._install_test_backend(ctypes.CDLL(build_emu.build()))
    import model_cases as mc
    from transfuser_amd.train import Engine
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    cfg = mc.tiny_config(n_layer=1)
    batch = mc.small_batch(2, 32, 64, 64, 40, seed=70 + rank)            # each rank its own micro-batch

    def run(zero):
        prod, _ = mc.build_pair(cfg, "regnety_tiny", "cpu", seed=5)
        prod.train()
        eng = Engine(prod, cfg, lr=1e-3, cuts=(3,), zero_redundancy_optimizer=zero, ema_decay=0.5)
        for _ in range(2):
            eng.train_step(batch)
        assert eng.ema.state.tolist() == [0.5, 2.0, 2.0, 0.5], eng.ema.state.tolist()
        return eng

    full, shard = run(False), run(True)
    opt = shard.optimizer
    assert shard.zero and 0 < opt.hi - opt.lo < shard.arena.active_numel and shard.ema.flat.numel() == shard.arena.active_numel
    assert torch.equal(full.arena.params, shard.arena.params)
    n = full.arena.active_numel
    assert not torch.equal(full.ema.flat, full.arena.params[:n])         # the average lags the live weights
    for eng, what in ((full, "unsharded"), (shard, "ZeRO-1")):
        both = [torch.zeros_like(eng.ema.flat) for _ in range(world)]
        dist.all_gather(both, eng.ema.flat.contiguous())
        assert torch.equal(both[0], both[1]), "%s: the averaged parameters differ between the ranks" % what
    assert torch.equal(full.ema.flat, shard.ema.flat), "ZeRO-1 average differs from the unsharded run's in %d elements" % int((full.ema.flat != shard.ema.flat).sum())
    assert torch.equal(full.ema.buf_flat, shard.ema.buf_flat)            # each rank's own BatchNorm statistics, the same in both runs
    with shard.ema_weights():                                            # a swap needs no collective: every rank holds the whole average
        assert torch.equal(shard.arena.params[:n], full.ema.flat)
    assert torch.equal(full.arena.params, shard.arena.params)
    dist.destroy_process_group()


def test_ema_identical_on_both_ranks_with_and_without_zero1_gloo():
    port = 41500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)
