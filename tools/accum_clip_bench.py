"""Gradient accumulation and global-norm clipping, the measurements of their pull request, one visit, same-lease alternating pairs:
(a) `python bench.py` of a parent checkout (--parent DIR, built) vs this tree with the default arguments, three pairs: the no-regression claim;
(b) B = 10 fp32 graph step with max_grad_norm set vs without, three alternating rounds, beside the event-timed cost of the unchanged
    adamw_kernel launch and of the gradient-norm launch on the same arena: the clip must add less than one adamw_kernel launch;
(c) ms per micro-batch at accumulate=8 vs the k = 1 step (report only).
Event / wall-clock timing, warm-up, no profiler.  `python tools/accum_clip_bench.py [--parent DIR]` on an MI355X."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def bench_pairs(parent, pairs, steps, warmup):
    print("(a) bench.py --gpus 1 --steps %d --warmup %d, parent vs branch, alternating" % (steps, warmup), flush=True)
    rows = {"parent": [], "branch": []}
    env = {k: v for k, v in os.environ.items() if k != "TF_HIP_LIB"}
    for i in range(pairs):
        for name, tree in (("parent", parent), ("branch", ROOT)):
            r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                               cwd=tree, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stderr[-2000:])
                raise SystemExit("bench.py of the %s tree failed (%d)" % (name, r.returncode))
            line = json.loads(r.stdout.strip().splitlines()[-1])
            rows[name].append(line["value"])
            print("  pair %d %-6s %9.3f %s" % (i, name, line["value"], line.get("unit", "")), flush=True)
    for name, v in rows.items():
        print("  %-6s values %s  mean %.3f  spread %.3f" % (name, "  ".join("%.3f" % x for x in v), sum(v) / len(v), max(v) - min(v)))
    print("  branch - parent (means) %+.3f" % (sum(rows["branch"]) / pairs - sum(rows["parent"]) / pairs), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit; without it part (a) is skipped")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.parent:
        bench_pairs(os.path.abspath(args.parent), args.pairs, args.steps, args.warmup)

    import torch
    from transfuser_amd import ops
    from transfuser_amd.config import GlobalConfig
    from transfuser_amd.data import synthetic_batch
    from transfuser_amd.model import LidarCenterNet
    from transfuser_amd.train import Engine
    dev = torch.device("cuda", 0)
    ops.L().tf_build_id.restype = __import__("ctypes").c_char_p
    print("build id %s" % ops.L().tf_build_id().decode())
    hist_fn = lambda pts: ops.lidar_hist(torch.from_numpy(pts).to(dev)[None])[0].cpu().numpy()
    batch = {k: v.to(dev) for k, v in synthetic_batch(10, 256, 704, seed=0, hist_fn=hist_fn).items()}

    def engine(**kw):      # bench.py's flagship workload: transFuser, regnety_032 trunks, B = 10, 256 x 704, fp32, captured
        cfg = GlobalConfig()
        cfg.n_layer = 4
        cfg.use_target_point_image = True
        cfg.embd_pdrop = cfg.attn_pdrop = cfg.resid_pdrop = 0.1
        torch.manual_seed(0)
        model = LidarCenterNet(cfg, dev, "transFuser", "regnety_032", "regnety_032", use_velocity=False)
        model.train()
        eng = Engine(model, cfg, lr=cfg.lr, use_graph=True, precision="fp32", **kw)
        for _ in range(max(args.warmup, 2 * eng.accumulate)):
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

    plain, clip = engine(), engine(max_grad_norm=1.0)
    print("(b) B = 10 fp32 graph step, ms per step, three alternating rounds (arena %.1f M floats)" % (plain.arena.numel / 1e6))
    res = {"no clip": [], "max_grad_norm=1": []}
    for _ in range(3):
        res["no clip"].append(step_ms(plain, args.steps))
        res["max_grad_norm=1"].append(step_ms(clip, args.steps))
    for name, v in res.items():
        print("  %-16s %s  mean %.3f" % (name, "  ".join("%8.3f" % t for t in v), sum(v) / len(v)))
    added = sum(res["max_grad_norm=1"]) / 3 - sum(res["no clip"]) / 3
    a, o = plain.arena, plain.optimizer
    n = a.active_numel
    t_adamw = event_ms(lambda: ops.adamw_(a.params[:n], a.grads[:n], o.exp_avg, o.exp_avg_sq, o.state))
    parts = torch.empty(ops.grad_sumsq_parts(n), dtype=torch.float32, device=dev)
    t_sumsq = event_ms(lambda: ops.grad_sumsq(a.grads[:n], parts))
    t_clip = event_ms(lambda: clip.optimizer.step())
    print("  adamw_kernel launch alone %.3f ms; grad_sumsq launch alone %.3f ms; sumsq + clipping AdamW %.3f ms" % (t_adamw, t_sumsq, t_clip))
    print("  added by the clip: %.3f ms per step (step delta), %.3f ms (launch delta); bound = the adamw_kernel launch, %.3f ms: %s"
          % (added, t_clip - t_adamw, t_adamw, "within" if max(added, t_clip - t_adamw) <= t_adamw else "EXCEEDED"))
    k1 = sum(res["no clip"]) / 3
    del clip
    acc = engine(accumulate=8)
    v = [step_ms(acc, 16) for _ in range(3)]
    print("(c) accumulate=8: ms per micro-batch %s  mean %.3f  vs the k = 1 step %.3f (report only)" % ("  ".join("%8.3f" % t for t in v), sum(v) / 3, k1))


if __name__ == "__main__":
    main()
