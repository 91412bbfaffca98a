"""Weight EMA, the measurements of its pull request, one visit, same-lease alternating rounds:
(a) `python bench.py` of a parent checkout (--parent DIR, built) vs this tree with the default arguments (no average), three pairs: the
    no-regression claim, and the only gate;
(b) the launches alone at the full arena size (168 M floats), event-timed beside tf_adamw_f32 in the same run: tf_ema_apply_f32 (byte model:
    12 / 28 of AdamW's time), tf_swap_f32 (16 / 28), and tf_ema_apply_multi_f32 / tf_swap_multi_f32 over the flagship model's float buffers;
(c) B = 10 fp32 captured step with ema_decay = 0.9999, ema_every 1 and 4, vs no average.
Event / wall-clock timing, warm-up, no profiler.  `python tools/ema_bench.py [--parent DIR] [--out profiles/ema_ab.txt]` on an MI355X; what it
prints is also written to --out."""
import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


class Tee:
    def __init__(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.f, self.out = open(path, "w"), sys.stdout

    def write(self, s):
        self.out.write(s)
        self.f.write(s)
        self.f.flush()

    def flush(self):
        self.out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit; without it part (a) is skipped")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip_calls", action="store_true", help="skip part (b)")
    ap.add_argument("--skip_step", action="store_true", help="skip part (c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_ab.txt"))
    args = ap.parse_args()
    sys.stdout = Tee(args.out)
    if args.parent:
        from accum_clip_bench import bench_pairs
        bench_pairs(os.path.abspath(args.parent), args.pairs, args.steps, args.warmup)

    import torch
    from transfuser_amd import ops
    from transfuser_amd.train import _ALIGN
    dev = torch.device("cuda", 0)
    ops.L().tf_build_id.restype = __import__("ctypes").c_char_p
    print("build id %s" % ops.L().tf_build_id().decode())

    def event_ms(fn, iters=10, warm=3):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    from transfuser_amd.config import GlobalConfig
    from transfuser_amd.model import LidarCenterNet

    def flagship():
        cfg = GlobalConfig()
        cfg.n_layer = 4
        cfg.use_target_point_image = True
        cfg.embd_pdrop = cfg.attn_pdrop = cfg.resid_pdrop = 0.1
        torch.manual_seed(0)
        model = LidarCenterNet(cfg, dev, "transFuser", "regnety_032", "regnety_032", use_velocity=False)
        model.train()
        return cfg, model

    if not args.skip_calls:
        bench_calls(torch, ops, dev, event_ms, flagship, 168 * 1000 * 1000 // _ALIGN * _ALIGN)
    if args.skip_step:
        return
    bench_step(torch, ops, dev, flagship, args)


def bench_calls(torch, ops, dev, event_ms, flagship, n):
    p, g, m, v = (torch.randn(n, device=dev) * s for s in (1.0, 1e-3, 1e-4, 1e-8))
    v.abs_()
    e = p.clone()
    state = torch.tensor([0.0, 1e-4], device=dev)
    st = torch.tensor([0.9999, 0.0, 0.0, 0.0], device=dev)
    ops.ema_tick_(st)                                   # coef = 1 - decay: the apply launches below all update
    _, model = flagship()
    live = [b for b in model.buffers() if b.is_floating_point()]
    avg = [b.detach().clone() for b in live]
    table = ops.ema_table(zip(avg, live))
    print("(b) per call, ms, three alternating rounds; flat ranges of %.1f M floats, table of %d buffers / %d floats (largest %d)"
          % (n / 1e6, table[1], table[2], max(b.numel() for b in live)))
    rows = {"tf_adamw_f32 (28 B / parameter)": lambda: ops.adamw_(p, g, m, v, state),
            "tf_ema_apply_f32 (12 B / parameter)": lambda: ops.ema_apply_(e, p, st),
            "tf_swap_f32 (16 B / parameter)": lambda: ops.swap_(e, p),
            "tf_ema_tick_f32": lambda: ops.ema_tick_(st),
            "tf_ema_apply_multi_f32, the model's float buffers": lambda: ops.ema_apply_multi_(table, st),
            "tf_swap_multi_f32, the model's float buffers": lambda: ops.swap_multi_(table)}
    res = {k: [] for k in rows}
    for _ in range(3):
        for k, fn in rows.items():
            res[k].append(event_ms(fn))
    for k, t in res.items():
        print("  %-52s %s  mean %.4f" % (k, "  ".join("%8.4f" % x for x in t), sum(t) / 3))
    mean = lambda k: sum(res[k]) / 3
    a = mean("tf_adamw_f32 (28 B / parameter)")
    for k, model_ratio in (("tf_ema_apply_f32 (12 B / parameter)", 12 / 28), ("tf_swap_f32 (16 B / parameter)", 16 / 28)):
        print("  %s / tf_adamw_f32 = %.3f (byte model %.3f), %.2f TB/s" % (k.split(" ")[0], mean(k) / a, model_ratio, int(k.split("(")[1].split(" ")[0]) * n / mean(k) / 1e9))


def bench_step(torch, ops, dev, flagship, args):
    from transfuser_amd.data import synthetic_batch
    from transfuser_amd.train import Engine
    hist_fn = lambda pts: ops.lidar_hist(torch.from_numpy(pts).to(dev)[None])[0].cpu().numpy()
    batch = {k: t.to(dev) for k, t in synthetic_batch(10, 256, 704, seed=0, hist_fn=hist_fn).items()}

    def engine(**kw):      # bench.py's flagship workload: transFuser, regnety_032 trunks, B = 10, 256 x 704, fp32, captured
        cfg, model = flagship()
        eng = Engine(model, cfg, lr=cfg.lr, use_graph=True, precision="fp32", **kw)
        for _ in range(args.warmup):
            eng.train_step(batch)
        torch.cuda.synchronize()
        return eng

    def step_ms(eng, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            eng.train_step(batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    engines = {"no average": engine(), "ema_decay 0.9999, ema_every 1": engine(ema_decay=0.9999), "ema_decay 0.9999, ema_every 4": engine(ema_decay=0.9999, ema_every=4)}
    print("(c) B = 10 fp32 graph step, ms per step, three alternating rounds (active arena %.1f M floats)" % (engines["no average"].arena.active_numel / 1e6))
    res = {k: [] for k in engines}
    for _ in range(3):
        for k, eng in engines.items():
            res[k].append(step_ms(eng, args.steps))
    for name, t in res.items():
        print("  %-32s %s  mean %.3f" % (name, "  ".join("%8.3f" % x for x in t), sum(t) / len(t)))


if __name__ == "__main__":
    main()
