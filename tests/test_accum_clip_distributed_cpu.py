"""Gradient accumulation across ranks on CPU (world size 2, gloo, host-emulated kernels; pattern of tests/test_distributed_cpu.py): two ranks x
accumulate=2 compute what one rank x accumulate=4 computes on the same four micro-batches, and only the window's last micro-batch all-reduces
(DistributedDataParallel's no_sync on the others)."""
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
    alone = [dist.new_group([r]) for r in range(world)][rank]            # a world of one inside the same process: the single-rank reference
    cfg = mc.tiny_config(n_layer=1)
    micro = [mc.small_batch(2, 32, 64, 64, 40, seed=40 + i) for i in range(4)]

    def run(group, k, mine):
        prod, _ = mc.build_pair(cfg, "regnety_tiny", "cpu", seed=5)
        prod.train()
        eng = Engine(prod, cfg, lr=1e-4, group=group, cuts=(), accumulate=k, max_grad_norm=1.0)
        calls = []
        inner = eng.reducer._reduce_range
        eng.reducer._reduce_range = lambda lo, hi: (calls.append((lo, hi)), inner(lo, hi))[1]
        for i, b in enumerate(mine):
            assert float(eng.optimizer.state[0]) == 0.0 and calls == [], (i, calls)      # no update, no all-reduce inside the window
            eng.train_step(b)
        assert float(eng.optimizer.state[0]) == 1.0
        grads = {n: (p.grad.detach() * eng.grad_scale()).clone() for n, p, _ in eng.arena.layout}
        return eng, grads, float(eng.optimizer.grad_norm), calls

    # rank r takes micro-batches r and r + 2: together the two ranks see all four, as DistributedSampler would deal them
    eng2, g2, norm2, calls2 = run(None, 2, [micro[rank], micro[rank + 2]])
    assert eng2.reducer.world == 2 and eng2.grad_scale() == 0.25            # deferred 1 / world x the window's 1 / k
    assert len(calls2) == 1, calls2                                          # exactly one all-reduce per window
    eng1, g1, norm1, calls1 = run(alone, 4, micro)
    assert eng1.reducer.world == 1 and eng1.grad_scale() == 0.25 and calls1 == []
    assert g1.keys() == g2.keys()
    for n in g1:      # the same fp32 sums in another order: 1e-5 of the tensor's max (determinism_cases.check_mode_agreement)
        err = (g2[n] - g1[n]).abs().max().item() / max(g1[n].abs().max().item(), 1e-6)
        assert err < 1e-5, (n, err)
    assert abs(norm2 - norm1) <= 1e-5 * norm1, (norm2, norm1)
    both = [torch.zeros_like(eng2.arena.params) for _ in range(world)]
    dist.all_gather(both, eng2.arena.params)
    assert torch.equal(both[0], both[1])                                     # replicas stay in lock-step
    dist.destroy_process_group()


def test_two_ranks_times_two_equals_one_rank_times_four_gloo():
    port = 37500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)
