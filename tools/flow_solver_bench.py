"""What the flow head's higher-order integrators (fv_head_set_flow_solver) cost and buy at inference, same process, alternating windows:
    python tools/flow_solver_bench.py [--model fastvlm-0.5b] [--chunk 50] [--time-dim 64] [--reps 100] [--rounds 5] [--parent-checkout DIR] [--out FILE.json]
legs       = every solver at a comparable budget of network evaluations -- Euler N = 10 (10), midpoint N = 5 (10), Heun N = 5 (10), RK4 N = 3 (12) -- on the
             model's head dimensions (explicit noise) at B = 1 and B = 64, for
             `plain`   fv_head_flow_sample (conditioning once, 3 launches per evaluation)
             `guided`  fv_head_flow_sample_guided, "exp" weights with inference delay 0 and execution horizon 10, shift 10 (8 launches per evaluation)
             ONE handle runs all of them (it reserved the two rows; the solver is switched between windows, a host-only call); the Euler leg of the same run
             is the yardstick for time
error      = each leg's distance (worst row against the RMS row norm) from a float64 RK4 N = 160 reference on the same inputs
             (tests/flow_solver_util.py; the B = 1 inputs are row 0 of the B = 64 inputs: rows never meet).  The head is UNTRAINED (random weights ~
             1 / sqrt(fan-in)): its field follows phi(t) down to the embedding's shortest period, 0.004 of the unit interval, which ten evaluations do not
             resolve with any solver -- `reference.distance_from_twice_the_steps` says how far the reference itself is from converged.  The accuracy a
             smooth field buys is the float64 table of tests/test_flow_solver_host.py; this file is about time
digest     = tools/rtc_bench.py --digest (a flow policy that asks for nothing new) on this build and, with --parent-checkout, on a built checkout of the parent
             commit, each in a process of its own: they must be identical
Times: host clock around windows that end in a device synchronise; the median of --rounds rounds with its spread (max - min).  The figures to read:
`ms_per_eval` of every leg against Euler's with the spreads, and `error` against Euler's.  Written to profiles/flow_solver_bench.json unless --out names
another file."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "vla-from-fastvlm_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

A = 14
LEGS = (("euler", 10), ("midpoint", 5), ("heun", 5), ("rk4", 3))
REF = ("rk4", 160)


def digest_of(checkout: Path) -> str:
    """tools/rtc_bench.py --digest of a built checkout, in a fresh process"""
    out = subprocess.run([sys.executable, str(checkout / "tools" / "rtc_bench.py"), "--digest"], check=True, capture_output=True, text=True, cwd=str(checkout))
    return json.loads(out.stdout.strip().splitlines()[-1])["digest"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--time-dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-checkout", default=None, help="root of a built checkout of the parent commit: its digest is recorded beside this build's")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/flow_solver_bench.py measures on the GPU: no HIP device visible")
    digests = {"this_build": digest_of(ROOT)}      # (before this process opens the device)
    if args.parent_checkout:
        digests["parent_build"] = digest_of(Path(args.parent_checkout).resolve())
        digests["identical"] = digests["parent_build"] == digests["this_build"]
    old = ROOT / "profiles" / "rtc_bench.json"
    if old.is_file() and "digest" in json.loads(old.read_text()):
        digests["recorded_in_rtc_bench_json"] = json.loads(old.read_text())["digest"]

    import flow_solver_util as su
    import flow_util as fu
    import rtc_util as ru
    from fastvla_hip import FastVLAEngine, _lib, arch
    from fastvla_hip.rtc import prefix_weights
    from vla_fastvlm.fastvla import FastVLAConfig
    dev = torch.device("cuda", 0)
    K, E = args.chunk, args.time_dim
    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
    cfg, feat = FastVLAConfig(), arch.preset(args.model).llm.hidden
    dims = (feat, cfg.state_dim, cfg.hidden_dim, cfg.fusion_dim, K, A, E)
    m = arch.ModelConfig("head", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    eng = FastVLAEngine(m, state_dim=cfg.state_dim, action_dim=K * A, hidden_dim=cfg.hidden_dim, fusion_dim=cfg.fusion_dim, max_batch=64)
    eng.set_head_flow(E)
    d, s, shift = 0, min(10, K - 1), min(10, K - 1)
    weights = prefix_weights(K, d, s, "exp")
    eng.set_head_flow_guidance(weights, ru.BETA)
    eng.set_head_flow_solver("rk4")      # reserves the two rows; every window below names its own solver

    # weights ~ 1 / sqrt(fan-in) (tests/flow_util.sampler_case's recipe: every layer's output stays O(1)), one observation set for B = 64 whose row 0 is B = 1
    g = torch.Generator().manual_seed(1)
    shapes = fu.flow_head_shapes(feat, cfg.state_dim, K * A, cfg.hidden_dim, cfg.fusion_dim, E)
    p = {k: (torch.randn(*sh, generator=g) / (sh[-1] ** 0.5 if len(sh) > 1 else 10.0)) + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0)
         for k, sh in shapes.items()}
    flat = torch.zeros(eng.head_numel(), device=dev)
    for k, v in eng.head_views(flat).items():
        v.copy_(p[k])
    pooled, states = torch.randn(64, feat, generator=g), torch.randn(64, cfg.state_dim, generator=g)
    noise, other = torch.randn(64, K * A, generator=g), torch.randn(64, K * A, generator=g)
    prev = fu.euler_sample(p, pooled, states, other, 10, E).float()      # a plausible previous chunk: the sample of another start noise
    Y, W = ru.targets(prev, ru.prefix_weights_ref(K, d, s, "exp"), K, A, shift)
    t0 = time.perf_counter()
    ref = {"plain": su.rk_sample(p, pooled, states, noise, REF[1], E, REF[0]),
           "guided": su.guided_rk(p, pooled, states, noise, REF[1], E, Y, W, ru.BETA, REF[0])[0]}
    # how far the reference itself still moves when its step is halved (the plain sampler): what "distance from the reference" can resolve
    ref_self = fu.worst_row_vs_rms(su.rk_sample(p, pooled, states, noise, 2 * REF[1], E, REF[0]), ref["plain"])
    ref_seconds = round(time.perf_counter() - t0, 1)

    def window(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / reps

    res = {"model": args.model, "head_dims": dict(zip(("feat", "state", "hidden", "fusion", "chunk", "action_dim", "time_dim"), dims)),
           "reps_per_window": args.reps, "rounds": args.rounds, "reference": {"solver": REF[0], "steps": REF[1], "dtype": "float64", "seconds": ref_seconds,
                                                                            "distance_from_twice_the_steps": float(f"{ref_self:.4e}")},
           "guidance": {"schedule": "exp", "inference_delay": d, "execution_horizon": s, "shift": shift, "max_guidance_weight": ru.BETA},
           "unit": "ms per sampler call (host-enqueued back to back); error: worst row against the RMS row norm of the float64 reference", "digest": digests}
    for sampler in ("plain", "guided"):
        for B in (1, 64):
            po, st, no, pv = pooled[:B].to(dev), states[:B].to(dev), noise[:B].to(dev).contiguous(), prev[:B].to(dev).contiguous()
            legs, errs = {}, {}
            for solver, N in LEGS:
                if sampler == "plain":
                    fn = lambda N=N: eng.head_flow_sample(flat, po, st, steps=N, noise=no)      # noqa: E731
                else:
                    fn = lambda N=N: eng.head_flow_sample_guided(flat, po, st, pv, shift=shift, steps=N, noise=no)[0]      # noqa: E731
                legs[solver] = (N, fn)
                eng.set_head_flow_solver(solver)
                out = fn()
                torch.cuda.synchronize()
                errs[solver] = fu.worst_row_vs_rms(out.cpu(), ref[sampler][:B])
            rounds = []
            for _ in range(args.rounds):       # alternating windows: other work shares the machine
                r = {}
                for solver, (N, fn) in legs.items():
                    eng.set_head_flow_solver(solver)
                    r[solver] = round(window(fn, args.reps), 5)
                rounds.append(r)
            entry = {"rounds": rounds}
            for solver, (N, _) in legs.items():
                xs = [r[solver] for r in rounds]
                evals = N * _lib.FLOW_SOLVER_STAGES[solver]
                entry[solver] = {"steps": N, "evaluations": evals, "ms": med(xs), "spread_ms": round(max(xs) - min(xs), 5), "ms_per_eval": round(med(xs) / evals, 5),
                                 "error": float(f"{errs[solver]:.4e}")}
            for solver in legs:
                e = entry[solver]
                e["ms_per_eval_over_euler"] = round(e["ms_per_eval"] / entry["euler"]["ms_per_eval"], 4)
                e["euler_error_over_error"] = round(entry["euler"]["error"] / e["error"], 2)
            res[f"{sampler}_b{B}"] = entry
    eng.close()
    print(json.dumps(res))
    out = Path(args.out) if args.out else ROOT / "profiles" / "flow_solver_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
