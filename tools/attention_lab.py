#!/usr/bin/env python
"""In-graph per-launch time of the fused attention kernels (csrc/attention.cpp) at the four GPT stages of the bench configuration (B = 10, T = 174, 4 heads,
C = 72 / 216 / 576 / 1512, attn_pdrop 0.1), against the algorithmic FLOPs (forward 4 T^2 hs per head, backward 2.5x).  python tools/attention_lab.py
--long: other anchor grids (T = 196 / 366 / 768 / 1024, the column-chunked kernels), fused forward + backward against the unfused path of the same build."""
import os, sys, torch
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from transfuser_amd import ops
dev = "cuda"
REP = 20


def graph_time(fn, rep=REP):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(rep): fn()
        g.replay(); torch.cuda.synchronize()
        best = 1e30
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s); g.replay(); e1.record(s); e1.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e3 / rep)
    return best


def unfused(qkv, dy, B, T, C, nh, drop):
    """Forward + backward of the path a Block takes when ops.attention_supported is false (functions._gpt_block_fwd / _bwd): three batched GEMMs
    + softmax(+dropout) forward, five GEMMs + softmax backward, the probabilities and their dropped copy kept in between."""
    import math
    from transfuser_amd import functions as F
    hs, alpha = C // nh, 1.0 / math.sqrt(C // nh)
    att, Tp, att_d = F._attn_fwd(qkv, B, T, C, nh, drop=drop)
    F._attn_ctx(att_d, qkv, B, T, C, nh, Tp)
    dqkv, datt = torch.empty_like(qkv), torch.empty_like(att)
    k, q, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    sq, sp, sy = (T * 3 * C, hs), (nh * T * Tp, T * Tp), (T * C, hs)
    ops.gemm(dy, v, datt, T, T, hs, C, 3 * C, Tp, batch=B * nh, inner=nh, sa=sy, sb=sq, sc=sp)
    ops.gemm(att_d, dy, dqkv[:, 2 * C:], T, hs, T, Tp, C, 3 * C, a_trans=True, b_trans=True, batch=B * nh, inner=nh, sa=sp, sb=sy, sc=sq)
    ops.softmax_dropout_bwd_(att, datt, B * nh * T, T, Tp, *drop)
    ops.gemm(datt, k, dqkv[:, C:2 * C], T, hs, T, Tp, 3 * C, 3 * C, b_trans=True, alpha=alpha, batch=B * nh, inner=nh, sa=sp, sb=sq, sc=sq)
    ops.gemm(datt, q, dqkv[:, :C], T, hs, T, Tp, 3 * C, 3 * C, a_trans=True, b_trans=True, alpha=alpha, batch=B * nh, inner=nh, sa=sp, sb=sq, sc=sq)
    return dqkv


if "--long" in sys.argv:      # T > 192: the column-chunked kernels against the unfused path of the same build, forward + backward of one Block's attention
    seed = torch.zeros(1, dtype=torch.int32, device=dev)
    drop = (seed, 7, 0.1)
    print("# (B, nh, T, hs): fused forward + backward us | unfused (8 batched GEMMs + softmax fwd / bwd) us, in-graph, best of 5 replays of %d; saved for the backward" % REP)
    for B, nh, T, hs in ((10, 4, 196, 18), (10, 4, 366, 144), (10, 4, 480, 54), (10, 4, 768, 54), (10, 4, 1024, 378)):
        C = nh * hs
        qkv = torch.randn(B * T, 3 * C, device=dev) * 0.5
        dy = torch.randn(B * T, C, device=dev)
        assert ops.attention_supported(T, C, nh)

        def fused():
            y, lse = ops.attention_fwd(qkv, B, T, C, nh, drop=drop)
            return ops.attention_bwd(qkv, dy, lse, B, T, C, nh, drop=drop, y=y)
        Tp = (T + 3) // 4 * 4
        head = "(%d, %d, %4d, %3d): fused %7.1f us, saves %.3f MB (log-sum-exp)" % (B, nh, T, hs, graph_time(fused), B * nh * T * 4 / 1e6)
        if T > 512:      # tf_softmax_*_f32 hold a row in registers, n <= 512: beyond, the fused kernels are the only attention path
            print(head + " | unfused: does not exist (row softmax kernels take n <= 512); P and drop(P) would be %.1f MB" % (2 * B * nh * T * Tp * 4 / 1e6), flush=True)
            continue
        err = float((fused() - unfused(qkv, dy, B, T, C, nh, drop)).abs().max())
        tun = graph_time(lambda: unfused(qkv, dy, B, T, C, nh, drop))
        print(head + " | unfused %7.1f us, saves %.1f MB (P and drop(P)); max |dqkv difference| %.1e" % (tun, 2 * B * nh * T * Tp * 4 / 1e6, err), flush=True)
    sys.exit(0)
B, T, nh = 10, 174, 4
if "--pmc" in sys.argv:       # eager launches for the counter passes of tools/pmc_attention.sh: the widest and the narrowest stage only
    seed = torch.zeros(1, dtype=torch.int32, device=dev)
    for C in (1512, 576, 72):
        qkv = torch.randn(B * T, 3 * C, device=dev) * 0.5
        dy = torch.randn(B * T, C, device=dev)
        for _ in range(6):
            y, lse = ops.attention_fwd(qkv, B, T, C, nh, drop=(seed, 7, 0.1))
            ops.attention_bwd(qkv, dy, lse, B, T, C, nh, drop=(seed, 7, 0.1))
    torch.cuda.synchronize()
    sys.exit(0)
seed = torch.zeros(1, dtype=torch.int32, device=dev)
print("# C (hs): forward us (TF/s) | backward dq + dkv us (TF/s), in-graph, best of 5 replays of %d" % REP)
tot = 0.0
for C in (72, 216, 576, 1512):
    qkv = torch.randn(B * T, 3 * C, device=dev) * 0.5
    dy = torch.randn(B * T, C, device=dev)
    y, lse = ops.attention_fwd(qkv, B, T, C, nh, drop=(seed, 7, 0.1))
    tf = graph_time(lambda: ops.attention_fwd(qkv, B, T, C, nh, drop=(seed, 7, 0.1)))
    tb2 = graph_time(lambda: ops.attention_bwd(qkv, dy, lse, B, T, C, nh, drop=(seed, 7, 0.1)))                # two dependent launches (rounds 3-5)
    tb = graph_time(lambda: ops.attention_bwd(qkv, dy, lse, B, T, C, nh, drop=(seed, 7, 0.1), y=y))            # D = dY . Y, then both halves as one grid
    fl = 4.0 * T * T * (C // nh) * nh * B
    tot += 4 * (tf + tb)
    print("C = %4d (hs %3d): forward %6.1f us (%5.1f TF/s) | backward %6.1f us (%5.1f TF/s); as two dependent launches %6.1f us" %
          (C, C // nh, tf, fl / tf / 1e6, tb, 2.5 * fl / tb / 1e6, tb2), flush=True)
print("# 4 layers per stage, forward + backward: %.2f ms per training step" % (tot / 1e3))
