"""What temporal ensembling costs in the B = 1 control loop, same process, alternating windows:
    python tools/ensemble_bench.py [--model fastvlm-0.5b] [--chunk 50] [--coeff 0.01] [--env-steps 40] [--reps 200] [--rounds 5] [--out FILE.json]
queue      = FastVLAPolicy.select_action with chunk_size = --chunk and n_action_steps = 1 on synthetic weights: today's every-step loop (the backbone and the
             head on every call, row 0 served), milliseconds per ENVIRONMENT step over --env-steps calls
ensemble   = the same policy with temporal_ensemble_coeff = --coeff: the same backbone and head on every call, then fv_ensemble_step over the (1, K, A) chunk
kernel     = fv_ensemble_step alone (TemporalEnsembler.step into a preallocated output) at n_env = 1 and 64, K = --chunk, A = 14, over --reps calls
Times: host clock around windows that end in a device synchronise; the median of --rounds rounds with its spread (max - min).  The figure to read is
`ensemble_minus_queue_ms` against `queue_spread_ms`, the same run's run-to-run spread of the leg it is taken from, and against `kernel.n_env1_ms`.
Written to profiles/temporal_ensemble_bench.json unless --out names another file."""
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
from fastvla_hip import TemporalEnsembler  # noqa: E402

A = 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--coeff", type=float, default=0.01)
    ap.add_argument("--env-steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ensemble_bench.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    K = args.chunk
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
    for name, kw in (("queue", {}), ("ensemble", {"temporal_ensemble_coeff": args.coeff})):
        torch.manual_seed(3)
        pol = FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{args.model}:5", dropout=0.0), chunk_size=K, n_action_steps=1, **kw).to(dev)
        pol.eval()
        pol.reset()
        pols[name] = pol
        cases[name] = lambda pol=pol: pol.select_action(img, st, "pick up the red cube", dev)      # (the ensembler lives on across the windows: steady state)
    res = {"model": args.model, "chunk": K, "action_dim": A, "coeff": args.coeff, "env_steps_per_window": args.env_steps, "kernel_reps_per_window": args.reps,
           "control": {"unit": "ms per environment step at B = 1", **measure(cases, args.env_steps)}}
    c = res["control"]
    c["ensemble_minus_queue_ms"] = round(c["ensemble_ms"] - c["queue_ms"], 5)
    c["ensemble_minus_queue_per_round_ms"] = [round(r["ensemble"] - r["queue"], 5) for r in c["rounds"]]

    eng = pols["queue"].model.backbone.engine()
    kcases, keep = {}, []
    for n_env in (1, 64):
        ens = TemporalEnsembler(eng, n_env, K, A, args.coeff)
        chunks, out = torch.randn(n_env, K, A, generator=g).to(dev), torch.empty(n_env, A, device=dev)
        kcases[f"n_env{n_env}"] = lambda ens=ens, chunks=chunks, out=out: ens.step(chunks, out=out)
        keep.append(ens)
    res["kernel"] = {"unit": "ms per fv_ensemble_step call (host-enqueued back to back)", **measure(kcases, args.reps)}
    for ens in keep:
        ens.close()
    for pol in pols.values():
        pol.reset()
        pol.model.backbone.engine().close()
    print(json.dumps(res))
    out = Path(args.out) if args.out else ROOT / "profiles" / "temporal_ensemble_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
