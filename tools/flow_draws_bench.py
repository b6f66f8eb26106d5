"""What several noise draws per observation cost, and what they replace, same process, alternating windows:
    python tools/flow_draws_bench.py [--model fastvlm-0.5b] [--chunk 50] [--time-dim 64] [--batch 32] [--reps 10] [--rounds 5] [--legs head,steps] [--out FILE.json]
head       = fv_head_flow_prepare + fv_head_forward + fv_head_mse_backward on the model's head dimensions at B = --batch with S = 1, 2, 4, 8, 16 draws
             (one engine per S: the setting sizes the saved activations); milliseconds per call of the three
steps      = FastVLAPolicy.fused_train_step on synthetic weights at B = --batch, flow head, on three routes -- head-only (frozen backbone), rank-16 LoRA
             and full fine-tuning of decoder + projector -- in three forms each:
               s1      one step with one draw (today's step)
               s8      one step with flow_noise_draws = 8: eight draws for one backbone pass
               accum8  what s8 replaces: eight accumulated single-draw micro-steps of the same batch (grad_accum_steps = 8), the optimiser on the eighth
             milliseconds per optimiser step
Times: host clock around windows that end in a device synchronise; the median of --rounds rounds with its spread (max - min).  The figures to read:
`steps.<route>.s8_ms` against `steps.<route>.accum8_ms` (the feature has a point only if s8 is below accum8), `s8_ms - s1_ms` against `head.s8_ms - head.s1_ms`,
and every difference against the spreads beside it.  Written to profiles/flow_draws_bench.json unless --out names another file."""
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
DRAWS = (1, 2, 4, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--time-dim", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--head-reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="head,steps")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/flow_draws_bench.py measures on the GPU: no HIP device visible")
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
    cfg0 = FastVLAConfig(vlm_model_name=f"synthetic:{args.model}:5", dropout=0.0)
    res = {"model": args.model, "chunk": K, "action_dim": A, "time_dim": E, "batch": B, "rounds": args.rounds}
    g = torch.Generator().manual_seed(1)

    if "head" in legs:
        # the head alone, on the model's head dimensions (no backbone weights are loaded: the head entry points do not need them)
        feat = arch.preset(args.model).llm.hidden
        m = arch.ModelConfig("head", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                             arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
        pooled, states = torch.randn(B, feat, generator=g).to(dev), torch.randn(B, cfg0.state_dim, generator=g).to(dev)
        targets = torch.randn(B, K * A, generator=g).to(dev)
        engines, cases = [], {}
        for S in DRAWS:
            eng = FastVLAEngine(m, state_dim=cfg0.state_dim, action_dim=K * A, hidden_dim=cfg0.hidden_dim, fusion_dim=cfg0.fusion_dim, max_batch=B)
            eng.set_head_flow(E)
            eng.set_head_flow_draws(S)
            eng.set_head_loss("mse", 1.0, K)
            flat = (torch.randn(eng.head_numel(), generator=torch.Generator().manual_seed(2)) * 0.02).to(dev)
            for k, v in eng.head_views(flat).items():
                if k in ("state_projection.0.weight", "fusion.1.weight"):
                    v.fill_(1.0)
            saved, grads = eng.head_saved(B), torch.zeros_like(flat)

            def step(eng=eng, flat=flat, saved=saved, grads=grads):
                u = eng.head_flow_prepare(targets, saved, seed=7, offset=3)
                v, _ = eng.head_forward(flat, pooled, states, saved=saved, normalized_actions=True)
                return eng.head_backward(flat, v, u, saved, flat_grads=grads)

            engines.append(eng)
            cases[f"s{S}"] = step
        res["head"] = {"unit": f"ms per fv_head_flow_prepare + fv_head_forward + fv_head_mse_backward at B = {B}", "hidden_dim": cfg0.hidden_dim,
                       "fusion_dim": cfg0.fusion_dim, "feat": feat, **measure(cases, args.head_reps)}
        for eng in engines:
            eng.close()
        print("[flow_draws_bench] head:", {k: v for k, v in res["head"].items() if k.endswith("_ms")}, file=sys.stderr, flush=True)

    if "steps" in legs:
        batch = {"images": torch.rand(B, 3, 336, 336, generator=g).to(dev), "states": torch.randn(B, A, generator=g).to(dev),
                 "actions": torch.randn(B, K, A, generator=g).to(dev), "tasks": ["pick up the red cube"] * B}
        res["steps"] = {"unit": f"ms per optimiser step at B = {B} (accum8: eight single-draw micro-steps of the same batch)"}
        for route, ckw, bkw in (("head_only", {}, None), ("lora_r16", {"freeze_backbone": False}, {"lora_rank": 16}), ("full", {"freeze_backbone": False}, {})):
            pols, cases = [], {}
            for name, S, accum in (("s1", 1, 1), ("s8", 8, 1), ("accum8", 1, 8)):
                torch.manual_seed(3)
                pol = FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{args.model}:5", dropout=0.0, **ckw), chunk_size=K, action_head="flow",
                                    flow_time_dim=E, flow_seed=11, flow_noise_draws=S).to(dev)
                pol.train()
                if bkw is not None:
                    pol.enable_backbone_training(**bkw)

                def step(pol=pol, accum=accum):
                    for _ in range(accum):
                        out = pol.fused_train_step(batch, lr=1e-5, grad_accum_steps=accum)
                    return out

                pols.append(pol)
                cases[name] = step
            r = measure(cases, args.reps)
            r["s8_minus_s1_ms"] = round(r["s8_ms"] - r["s1_ms"], 5)
            r["accum8_over_s8"] = round(r["accum8_ms"] / r["s8_ms"], 3)
            res["steps"][route] = r
            print(f"[flow_draws_bench] {route}:", {k: v for k, v in r.items() if k != "rounds"}, file=sys.stderr, flush=True)
            for pol in pols:
                pol.model.backbone.engine().close()
            del pols, cases
            torch.cuda.empty_cache()
    print(json.dumps(res))
    out = Path(args.out) if args.out else ROOT / "profiles" / "flow_draws_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
