"""What the flow-matching head costs at inference, same process, alternating windows:
    python tools/flow_bench.py [--model fastvlm-0.5b] [--chunk 50] [--steps 10] [--time-dim 64] [--env-steps 40] [--reps 100] [--rounds 5] [--out FILE.json]
control    = FastVLAPolicy.select_action at B = 1 on synthetic weights, chunk_size = --chunk, n_action_steps = 1 (the backbone and the head on every call):
             `regression` is today's head, `flow` the flow head sampling with --steps Euler steps; milliseconds per ENVIRONMENT step over --env-steps calls
sampler    = fv_head_flow_sample alone (FastVLAEngine.head_flow_sample, explicit noise) on the model's head dimensions at B = 1 and B = 64: the
             conditioning once, then three launches per step
naive      = the composition the sampler replaces, at the same B: --steps x (x and phi(t_i) written into the saved activations by fv_head_flow_prepare,
             fv_head_forward -- the whole head, conditioning recomputed every step --, x <- x + dt v as one torch axpy).  fv_head_flow_prepare stands in
             for the write of x and phi(t_i), which costs the composition one launch per step however it is done: 10 launches per step in all
Times: host clock around windows that end in a device synchronise; the median of --rounds rounds with its spread (max - min).  The figures to read:
`sampler.b1_ms` against `naive.b1_ms` (and b64) with their spreads, and `control.flow_minus_regression_ms` against `control.regression_spread_ms`.
Written to profiles/flow_bench.json unless --out names another file."""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "vla-from-fastvlm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from fastvla_hip import FastVLAEngine, arch  # noqa: E402

A = 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--time-dim", type=int, default=64)
    ap.add_argument("--env-steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/flow_bench.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    K, N, E = args.chunk, args.steps, args.time_dim
    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731

    def window(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / reps

    def measure(cases, reps):
        rounds = []
        for _ in range(args.rounds):       # alternating windows: other work shares the machine
            rounds.append({k: round(window(fn, reps), 5) for k, fn in cases.items()})
        out = {"rounds": rounds}
        for k in cases:
            xs = [r[k] for r in rounds]
            out[k + "_ms"], out[k + "_spread_ms"] = med(xs), round(max(xs) - min(xs), 5)
        return out

    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    g = torch.Generator().manual_seed(1)
    img, st = torch.rand(3, 336, 336, generator=g), torch.randn(A, generator=g)
    pols, cases = {}, {}
    for name, kw in (("regression", {"action_head": "regression"}), ("flow", {"action_head": "flow", "flow_steps": N, "flow_time_dim": E})):
        torch.manual_seed(3)
        pol = FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{args.model}:5", dropout=0.0), chunk_size=K, n_action_steps=1, **kw).to(dev)
        pol.eval()
        pol.reset()
        pols[name] = pol
        cases[name] = lambda pol=pol: pol.select_action(img, st, "pick up the red cube", dev)
    res = {"model": args.model, "chunk": K, "action_dim": A, "flow_steps": N, "time_dim": E, "env_steps_per_window": args.env_steps, "reps_per_window": args.reps,
           "control": {"unit": "ms per environment step at B = 1", **measure(cases, args.env_steps)}}
    c = res["control"]
    c["flow_minus_regression_ms"] = round(c["flow_ms"] - c["regression_ms"], 5)
    c["flow_minus_regression_per_round_ms"] = [round(r["flow"] - r["regression"], 5) for r in c["rounds"]]
    cfg, feat = pols["flow"].config, pols["flow"].model.backbone.output_dim
    for pol in pols.values():
        pol.reset()
        pol.model.backbone.engine().close()

    # the head alone, on the model's head dimensions (no backbone weights are loaded: the head entry points do not need them)
    m = arch.ModelConfig("head", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    eng = FastVLAEngine(m, state_dim=cfg.state_dim, action_dim=K * A, hidden_dim=cfg.hidden_dim, fusion_dim=cfg.fusion_dim, max_batch=64)
    eng.set_head_flow(E)
    flat = (torch.randn(eng.head_numel(), generator=g) * 0.02).to(dev)
    for k, v in eng.head_views(flat).items():
        if k in ("state_projection.0.weight", "fusion.1.weight"):
            v.fill_(1.0)
    dt = -1.0 / N
    ts = [float(torch.tensor(1.0 - i / N, dtype=torch.float32)) for i in range(N)]
    scases, ncases, check = {}, {}, {}
    for B in (1, 64):
        pooled, states = torch.randn(B, feat, generator=g).to(dev), torch.randn(B, cfg.state_dim, generator=g).to(dev)
        noise, saved = torch.randn(B, K * A, generator=g).to(dev), eng.head_saved(B)
        tvec = [torch.full((B,), t, device=dev) for t in ts]

        def sampler(pooled=pooled, states=states, noise=noise):
            return eng.head_flow_sample(flat, pooled, states, steps=N, noise=noise)

        def naive(pooled=pooled, states=states, noise=noise, saved=saved, tvec=tvec):
            x = noise
            for i in range(N):
                eng.head_flow_prepare(x, saved, noise=x, t=tvec[i])      # t x + (1 - t) x == x: writes x and phi(t_i) into the saved activations
                v, _ = eng.head_forward(flat, pooled, states, saved=saved)
                x = torch.add(x, v, alpha=dt)
            return x

        scases[f"b{B}"], ncases[f"b{B}"] = sampler, naive
        a, b = sampler(), naive()
        torch.cuda.synchronize()
        check[f"b{B}"] = float((a - b).norm() / b.norm())
    res["sampler"] = {"unit": f"ms per fv_head_flow_sample call, {N} steps (host-enqueued back to back)", **measure(scases, args.reps)}
    res["naive"] = {"unit": f"ms per {N} x (fv_head_flow_prepare + fv_head_forward + axpy)", **measure(ncases, args.reps)}
    res["sampler_vs_naive_rel_l2"] = check
    for B in (1, 64):
        res[f"naive_over_sampler_b{B}"] = round(res["naive"][f"b{B}_ms"] / res["sampler"][f"b{B}_ms"], 3)
    eng.close()
    print(json.dumps(res))
    out = Path(args.out) if args.out else ROOT / "profiles" / "flow_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
