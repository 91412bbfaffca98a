"""Fine-tuning across ranks on CPU (world size 2, gloo, host-emulated kernels; pattern of tests/test_accum_clip_distributed_cpu.py): a ZeRO-1
sharded optimizer with parameter groups, a frozen trunk and an active clip ends two steps with the bits of the unsharded two-rank run, and the
frozen parameters keep their initial bits on both ranks."""
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
    import finetune_cases as ft
    import model_cases as mc
    from transfuser_amd.train import Engine
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    cfg = mc.tiny_config(n_layer=1)
    batch = mc.small_batch(2, 32, 64, 64, 40, seed=60 + rank)            # each rank its own micro-batch

    def run(zero):
        prod, _ = mc.build_pair(cfg, "regnety_tiny", "cpu", seed=5)
        prod.train()
        init = {n: p.detach().clone() for n, p in prod.named_parameters()}
        eng = Engine(prod, cfg, lr=1e-3, cuts=(3,), zero_redundancy_optimizer=zero, freeze=[ft.PREFIX], param_groups=ft.BOTH, max_grad_norm=0.05)
        for _ in range(2):
            eng.train_step(batch)
        assert float(eng.optimizer.state[0]) == 2.0 and float(eng.optimizer.grad_norm) > 0.05      # the clip is active
        return eng, init

    full, init = run(False)
    shard, _ = run(True)
    opt = shard.optimizer
    assert shard.zero and 0 < opt.hi - opt.lo < shard.arena.active_numel and opt.lo % 64 == 0 and opt.exp_avg.numel() == opt.hi - opt.lo
    assert (rank == 0) == (opt.lo == 0)                                   # rank 1's tile table starts at a non-zero tile
    assert [(n, o) for n, _, o in full.arena.layout] == [(n, o) for n, _, o in shard.arena.layout]
    assert torch.equal(full.arena.params, shard.arena.params), "ZeRO-1 shard + groups + freeze differs from the unsharded run: %d elements" % int(
        (full.arena.params != shard.arena.params).sum())
    assert float(full.optimizer.grad_norm) == float(opt.grad_norm)
    moved = 0
    for n, p in shard.model.named_parameters():
        if ft.under(n):
            assert torch.equal(p.detach(), init[n]), "frozen %s moved on rank %d" % (n, rank)
        else:
            moved += int(not torch.equal(p.detach(), init[n]))
    assert moved > 0
    both = [torch.zeros_like(shard.arena.params) for _ in range(world)]
    dist.all_gather(both, shard.arena.params)
    assert torch.equal(both[0], both[1])                                  # replicas stay in lock-step
    dist.destroy_process_group()


def test_zero1_shard_with_groups_and_frozen_trunk_gloo():
    port = 39500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)
