"""What the flow head's training-time distributions cost (fv_head_set_flow_time), same process, alternating windows:
    python tools/flow_time_bench.py [--model fastvlm-0.5b] [--chunk 50] [--time-dim 64] [--batch 32] [--reps 10] [--rounds 5] [--legs prepare,step] [--out FILE.json]
prepare    = fv_head_flow_prepare ALONE -- the one launch the setting changes -- on the model's head dimensions at B = --batch with S = 1 and 8 draws, for
             uniform  (the handle as it always was: the plain kernel instance), beta15_1 = Beta(1.5, 1) on (0.001, 1) (pi0; the closed form u^(1/a)),
             beta2_5 = Beta(2, 5) (the general inversion: Newton on a continued fraction, in double, by every thread of the row's block) and
             strat = uniform with strata (S = 8 only; S = 1 launches the plain instance); microseconds per launch
step       = FastVLAPolicy.fused_train_step, head-only (frozen backbone), on synthetic weights at B = --batch with flow_time_dist "uniform", "pi0" and
             "beta:2,5"; milliseconds per optimiser step
Times: host clock around windows that end in a device synchronise; the median of --rounds rounds with its spread (max - min).  No bar is fixed in advance: every
leg is read against the uniform leg of the same run, the difference against that leg's own spread.  Written to profiles/flow_time_bench.json unless --out names
another file."""
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
PREPARE_LEGS = {"uniform": None, "beta15_1": dict(dist="beta", a=1.5, b=1.0, t_lo=0.001, t_hi=1.0), "beta2_5": dict(dist="beta", a=2.0, b=5.0),
                "strat": dict(dist="uniform", stratify=True)}
STEP_LEGS = {"uniform": {}, "pi0": dict(flow_time_dist="pi0"), "beta2_5": dict(flow_time_dist="beta:2,5")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--time-dim", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--prepare-reps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="prepare,step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/flow_time_bench.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    K, E, B = args.chunk, args.time_dim, args.batch
    legs = set(args.legs.split(","))
    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731

    def window(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / reps

    def measure(cases, reps, scale=1.0, unit="ms"):
        rounds = []
        for _ in range(args.rounds):       # alternating windows: other work shares the machine
            rounds.append({k: round(scale * window(fn, reps), 5) for k, fn in cases.items()})
        out = {"rounds": rounds}
        for k in cases:
            xs = [r[k] for r in rounds]
            out[f"{k}_{unit}"], out[f"{k}_spread_{unit}"] = med(xs), round(max(xs) - min(xs), 5)
        for k in cases:
            if k != "uniform":
                out[f"{k}_minus_uniform_{unit}"] = round(out[f"{k}_{unit}"] - out[f"uniform_{unit}"], 5)
        return out

    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    cfg0 = FastVLAConfig(vlm_model_name=f"synthetic:{args.model}:5", dropout=0.0)
    res = {"model": args.model, "chunk": K, "action_dim": A, "time_dim": E, "batch": B, "rounds": args.rounds}
    g = torch.Generator().manual_seed(1)

    if "prepare" in legs:
        # the noising launch alone, on the model's head dimensions (no backbone weights are loaded: the head entry points do not need them)
        feat = arch.preset(args.model).llm.hidden
        m = arch.ModelConfig("head", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                             arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
        targets = torch.randn(B, K * A, generator=g).to(dev)
        res["prepare"] = {"unit": f"microseconds per fv_head_flow_prepare at B = {B} (host clock over {args.prepare_reps} back-to-back launches)", "feat": feat}
        for S in (1, 8):
            engines, cases = [], {}
            for name, tm in PREPARE_LEGS.items():
                if name == "strat" and S == 1:
                    continue
                eng = FastVLAEngine(m, state_dim=cfg0.state_dim, action_dim=K * A, hidden_dim=cfg0.hidden_dim, fusion_dim=cfg0.fusion_dim, max_batch=B)
                eng.set_head_flow(E)
                if S > 1:
                    eng.set_head_flow_draws(S)
                if tm is not None:
                    eng.set_head_flow_time(**tm)
                saved = eng.head_saved(B)

                def launch(eng=eng, saved=saved):
                    return eng.head_flow_prepare(targets, saved, seed=7, offset=3)

                engines.append(eng)
                cases[name] = launch
            res["prepare"][f"s{S}"] = r = measure(cases, args.prepare_reps, scale=1e3, unit="us")
            print(f"[flow_time_bench] prepare S={S}:", {k: v for k, v in r.items() if k != "rounds"}, file=sys.stderr, flush=True)
            for eng in engines:
                eng.close()

    if "step" in legs:
        batch = {"images": torch.rand(B, 3, 336, 336, generator=g).to(dev), "states": torch.randn(B, A, generator=g).to(dev),
                 "actions": torch.randn(B, K, A, generator=g).to(dev), "tasks": ["pick up the red cube"] * B}
        pols, cases = [], {}
        for name, kw in STEP_LEGS.items():
            torch.manual_seed(3)
            pol = FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{args.model}:5", dropout=0.0), chunk_size=K, action_head="flow", flow_time_dim=E,
                                flow_seed=11, **kw).to(dev)
            pol.train()

            def step(pol=pol):
                return pol.fused_train_step(batch, lr=1e-5)

            pols.append(pol)
            cases[name] = step
        res["step"] = {"unit": f"ms per head-only optimiser step at B = {B}", **measure(cases, args.reps)}
        print("[flow_time_bench] step:", {k: v for k, v in res["step"].items() if k != "rounds"}, file=sys.stderr, flush=True)
        for pol in pols:
            pol.model.backbone.engine().close()
    print(json.dumps(res))
    out = Path(args.out) if args.out else ROOT / "profiles" / "flow_time_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
