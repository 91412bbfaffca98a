"""Fused self-attention beyond one column chunk (192 < T <= 1024, the column-chunked kernels of csrc/attention.cpp): shared checks of
tests/test_attention_long_emu.py (host emulator) and tests/test_attention_long_gpu.py (MI355X).  References are PyTorch on the CPU with the
product's own dropout masks, compared with kernel_cases.close at the project's TOL = 1e-3."""
import math

import pytest
import torch

import kernel_cases as kc
import model_cases as mc
from transfuser_amd import ops

# (B, nh, T, hs, p): each the smallest shape at which its property can go wrong
PARITY_CASES = [(1, 2, 193, 18, 0.1),      # second chunk with ONE live column, Tp = 196, ragged 16-channel chunk of hs
                (1, 1, 384, 6, 0.0),       # exactly two full chunks, hs below one channel chunk
                (1, 1, 385, 6, 0.1),       # three chunks, the last with one column; last row tile with one live row
                (2, 2, 200, 24, 0.1),      # mask index across the chunk boundary with B > 1, nh > 1
                (1, 1, 193, 258, 0.1)]     # row operand staged in LDS in the backward (hs >= 256)
PARITY_CASES_GPU = [(2, 4, 366, 144, 0.1), (1, 1, 1024, 34, 0.0), (1, 1, 1000, 384, 0.1)]
# (B, nh, T, hs, p, f): the key third of every token row t with t % 7 == 3 is multiplied by f - row maxima in EVERY chunk, so the online softmax's
# rescale of the phase-B accumulators really runs; f = 64 makes a chunk's exp(S - m) underflow to exact zeros
SKEW_CASES = [(1, 2, 400, 18, 0.1, 8.0), (1, 2, 400, 18, 0.0, 64.0)]
SKEW_CASES_GPU = [(1, 4, 366, 54, 0.1, 8.0)]
REPRO_CASE = (2, 2, 200, 24, 0.1)
CHUNK = 192


def check_parity(dev, B, nh, T, hs, p, skew=None):
    """kernel_cases.check_fused_attention restated for T > 192: only the one-grid backward (ops.attention_bwd with y) exists there.  y, the
    log-sum-exp and dK / dQ / dV against PyTorch on the CPU, all finite."""
    C = nh * hs
    qkv = kc.R(B * T, 3 * C, dev="cpu", scale=0.7)
    if skew is not None:
        rows = (torch.arange(B * T) % T) % 7 == 3
        qkv[rows, :C] *= skew
    qkv.requires_grad_(True)
    k, q, v = [qkv[:, j * C:(j + 1) * C].view(B, T, nh, hs).transpose(1, 2) for j in range(3)]
    s = (q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(hs))
    if skew is not None:         # the input must keep exercising the rescale: asserted on the reference's scores before the product is looked at
        sd = s.detach().reshape(-1, T)
        late = float((sd.argmax(-1) >= CHUNK).float().mean())
        assert 0.1 <= late <= 0.9, late
        cmax = torch.stack([c.max(-1).values for c in sd.split(CHUNK, dim=-1)], -1)
        spread = float((cmax.max(-1).values - cmax.min(-1).values).max())
        if skew >= 64:
            assert spread > 104, spread                       # exp(-104) is 0 in fp32
    att = torch.softmax(s, dim=-1)
    seed = torch.full((1,), 777, dtype=torch.int32, device=dev)
    site = 13
    Tp = (T + 3) // 4 * 4
    if p > 0:
        mask = ops.dropout(torch.ones(B * nh, T, Tp, device=dev), seed, site, p)[:, :, :T].reshape(B, nh, T, T).cpu()
        assert 0.5 * p < float((mask == 0).float().mean()) < 1.5 * p + 0.02
        att = att * mask
    y = (att @ v).transpose(1, 2).contiguous().view(B * T, C)
    dy = kc.R(B * T, C, seed=9, dev="cpu")
    (g,) = torch.autograd.grad(y, qkv, dy)
    drop = (seed, site, p) if p > 0 else None
    qd = qkv.detach().to(dev)
    assert ops.attention_supported(T, C, nh)
    yh, lse = ops.attention_fwd(qd, B, T, C, nh, drop)
    dq = ops.attention_bwd(qd, dy.to(dev), lse, B, T, C, nh, drop, y=yh)
    for t in (yh, lse, dq):
        assert bool(torch.isfinite(t).all())
    kc.close(yh, y, what="fused attention fwd")
    kc.close(lse.view(B, nh, T), torch.logsumexp(s.detach(), -1), what="fused attention log-sum-exp")
    kc.close(dq[:, C:2 * C], g[:, C:2 * C], what="fused attention dQ")
    kc.close(dq[:, :C], g[:, :C], what="fused attention dK")
    kc.close(dq[:, 2 * C:], g[:, 2 * C:], what="fused attention dV")


def check_reproducible(dev):
    """Forward and backward twice: bitwise equal (every output tile has one owner), and no launch of a float-atomic kernel form."""
    B, nh, T, hs, p = REPRO_CASE
    C = nh * hs
    qkv, dy = kc.R(B * T, 3 * C, dev=dev, scale=0.7), kc.R(B * T, C, seed=9, dev=dev)
    drop = (torch.full((1,), 777, dtype=torch.int32, device=dev), 13, p)
    assert ops.attention_supported(T, C, nh)
    before = ops.float_atomic_launches()
    runs = []
    for _ in range(2):
        y, lse = ops.attention_fwd(qkv, B, T, C, nh, drop)
        runs.append((y, lse, ops.attention_bwd(qkv, dy, lse, B, T, C, nh, drop, y=y)))
    assert ops.float_atomic_launches() == before
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def check_predicate(dev):
    assert ops.attention_supported(1024, 72, 4)
    assert not ops.attention_supported(1025, 72, 4)
    assert not ops.attention_supported(400, 4 * 386, 4)
    assert not ops.attention_supported(400, 4 * 19, 4)
    with pytest.raises(RuntimeError):
        ops.attention_fwd(torch.zeros(1025, 3 * 72, device=dev), 1, 1025, 72, 4)
    # the older two-launch backward (no y) stays at T <= 192 and says so
    qkv = torch.zeros(200, 3 * 72, device=dev)
    with pytest.raises(RuntimeError, match="tf_attention_bwd_y_f32"):
        ops.attention_bwd(qkv, torch.zeros(200, 72, device=dev), torch.zeros(4 * 200, device=dev), 1, 200, 72, 4)


class count_fused_forwards:
    """Counts the calls of ops.attention_fwd (functions._gpt_block_fwd looks it up on the module at call time)."""

    def __enter__(self):
        self.n, self._orig = 0, ops.attention_fwd

        def counted(*a, **k):
            self.n += 1
            return self._orig(*a, **k)
        ops.attention_fwd = counted
        return self

    def __exit__(self, *exc):
        ops.attention_fwd = self._orig


def long_anchors(cfg):
    """6 x 22 image + 8 x 8 LiDAR anchors: T = 196 tokens."""
    cfg.img_vert_anchors, cfg.img_horz_anchors, cfg.lidar_vert_anchors, cfg.lidar_horz_anchors = 6, 22, 8, 8
    cfg.img_anchors, cfg.lidar_anchors = 6 * 22, 8 * 8
    return cfg


def check_gpt_stage(dev, C=72, B=2, n_layer=1, p=0.1, tol=1e-3):
    """model_cases.check_dropout_gpt_stage on a non-default anchor grid (T = 196): one fusion stage, product kernels vs the oracle GPT with the
    same masks - outputs, input gradients, every parameter gradient; the Block must take the fused attention path."""
    from oracle import transfuser_cpu as otf
    import transfuser_amd.transfuser as ptf
    torch.manual_seed(0)
    cfg = long_anchors(mc.full_config(dropout=p))
    cfg.n_layer = n_layer
    og = otf.GPT(C, cfg, use_velocity=False)
    with torch.no_grad():
        og.pos_emb.normal_(0, 0.05)
        for n, q in og.named_parameters():
            if n.endswith(".bias") or n.endswith("ln1.weight") or n.endswith("ln2.weight") or n.endswith("ln_f.weight"):
                q.add_(torch.randn_like(q) * 0.05)
    pg = ptf.GPT(C, cfg.n_head, cfg.block_exp, n_layer, cfg.img_vert_anchors, cfg.img_horz_anchors, cfg.lidar_vert_anchors, cfg.lidar_horz_anchors,
                 cfg.seq_len, p, p, p, cfg, use_velocity=False).to(dev)
    assert pg.pos_emb.shape[1] == 196
    pg.load_state_dict(og.state_dict(), strict=True)
    pg.seed = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    og.train(); pg.train()
    dropped = []
    assert mc.install_product_masks(pg, og, pg.seed, dev, dropped) == 1 + 3 * n_layer
    pool_i = torch.nn.AdaptiveAvgPool2d((cfg.img_vert_anchors, cfg.img_horz_anchors))
    pool_l = torch.nn.AdaptiveAvgPool2d((cfg.lidar_vert_anchors, cfg.lidar_horz_anchors))
    xi, xl = torch.randn(B, C, 12, 22), torch.randn(B, C, 8, 8)
    xio, xlo = xi.clone().requires_grad_(True), xl.clone().requires_grad_(True)
    fx, fy = og(pool_i(xio), pool_l(xlo), None)
    yi = xio + torch.nn.functional.interpolate(fx, size=(12, 22), mode='bilinear', align_corners=False)
    yl = xlo + torch.nn.functional.interpolate(fy, size=(8, 8), mode='bilinear', align_corners=False)
    di, dl = torch.randn_like(yi), torch.randn_like(yl)
    (yi * di).sum().add((yl * dl).sum()).backward()
    xip = xi.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
    xlp = xl.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
    with count_fused_forwards() as cnt:
        yip, ylp = pg(xip, xlp, None)
        torch.autograd.backward([yip, ylp], [di.permute(0, 2, 3, 1).contiguous().to(dev), dl.permute(0, 2, 3, 1).contiguous().to(dev)])
    assert cnt.n == n_layer, cnt.n

    def rel(a, b):
        return (a.detach().cpu().float() - b.detach()).abs().max().item() / max(b.detach().abs().max().item(), 1e-6)
    assert len(dropped) == 1 + 3 * n_layer and all(0.05 < d < 0.15 for d in dropped), dropped
    assert rel(yip.permute(0, 3, 1, 2), yi) <= tol and rel(ylp.permute(0, 3, 1, 2), yl) <= tol
    assert rel(xip.grad.permute(0, 3, 1, 2), xio.grad) <= tol and rel(xlp.grad.permute(0, 3, 1, 2), xlo.grad) <= tol
    pgo = dict(og.named_parameters())
    for n, q in pg.named_parameters():
        if "attn.key.bias" in n:
            continue                                       # exact gradient is 0 (softmax shift invariance): only round-off on both sides
        assert rel(q.grad, pgo[n].grad) <= tol, (n, rel(q.grad, pgo[n].grad))


def check_tiny_model(dev="cuda"):
    """The whole tiny model on the 6 x 22 + 8 x 8 grid (T = 196 at all four stages, hs = 6 / 12 / 18 / 24) against the oracle; then one Engine train
    step eager and one captured: finite, equal losses, every Block through the fused attention."""
    import transfuser_amd.transfuser as ptf
    from transfuser_amd.train import Engine
    cfg = long_anchors(mc.tiny_config(n_layer=1))
    ptf.GPT._site_base = 0
    prod, ref = mc.build_pair(cfg, "regnety_tiny", dev)
    batch = mc.small_batch(2, 32, 64, 64, 40)
    with count_fused_forwards() as cnt:
        lp, lr = mc.run_pair(prod, ref, cfg, batch, dev)
    assert cnt.n == 4 * cfg.n_layer, cnt.n
    mc.compare(prod, ref, lp, lr)
    bd = {k: v.to(dev) for k, v in batch.items()}
    losses = []
    for use_graph in (False, True):
        ptf.GPT._site_base = 0
        prod, _ = mc.build_pair(cfg, "regnety_tiny", dev)
        prod.train()
        eng = Engine(prod, cfg, lr=1e-3, use_graph=use_graph, autotune=False)
        with count_fused_forwards() as cnt:
            losses.append(float(eng.train_step(bd)[0]))
            torch.cuda.synchronize()
        # eager: one forward; captured: the engine's warm-up steps and the capture itself, 4 stages x n_layer each
        assert cnt.n >= 4 * cfg.n_layer and cnt.n % (4 * cfg.n_layer) == 0 and (use_graph or cnt.n == 4 * cfg.n_layer), cnt.n
    assert all(math.isfinite(v) for v in losses), losses
    assert abs(losses[0] - losses[1]) <= 1e-5 * max(1.0, abs(losses[0])), losses
