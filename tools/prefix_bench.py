"""What action-prefix conditioning costs, same process, alternating windows (tools/rtc_bench.py's method):
    python tools/prefix_bench.py [--model fastvlm-0.5b] [--chunk 50] [--max-delay 12] [--steps 10] [--time-dim 64] [--env-steps 40] [--reps 100] [--rounds 5] [--out FILE.json]
sampler    = the head alone on the model's head dimensions (explicit noise) at B = 1 and B = 64:
             `plain`     fv_head_flow_sample on a plain flow head (conditioning once, 3 launches per step): the yardstick, the parent commit's code
             `guided`    fv_head_flow_sample_guided on the same head, "exp" weights with inference delay 0 and execution horizon 10, shift 10 (8 per step)
             `prefix`    fv_head_flow_sample_prefix on a prefix-width head, every row's delay = --max-delay, shift 10 (3 per step)
             `plain_w`   fv_head_flow_sample on the prefix-width head (what the wider row stride costs the plain sampler)
control    = FastVLAPolicy.select_action at B = 1 on synthetic weights, chunk_size = --chunk, n_action_steps = 10: no rtc, rtc by guidance, rtc by prefix --
             milliseconds per ENVIRONMENT step over --env-steps calls (the backbone and the sampler run on every tenth)
train      = the head-only train step (prepare, forward, loss + backward, clip + AdamW) at B = 64 with and without prefix mode
Times: host clock around windows that end in a device synchronise; the median of --rounds rounds with its spread (max - min).  The figures to read:
`prefix_over_plain_b1` / `_b64` against the run's own spread, `guided_over_plain_*`, `control.*_minus_plain_ms`, `train.prefix_over_plain`.
Written to profiles/flow_prefix_bench.json unless --out names another file."""
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

A = 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--max-delay", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--time-dim", type=int, default=64)
    ap.add_argument("--env-steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/prefix_bench.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    from fastvla_hip import FastVLAEngine, arch
    from fastvla_hip.rtc import prefix_weights
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    K, D, N, E, n_exec = args.chunk, args.max_delay, args.steps, args.time_dim, 10
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

    g = torch.Generator().manual_seed(1)
    img, st = torch.rand(3, 336, 336, generator=g), torch.randn(A, generator=g)
    pols, cases = {}, {}
    for name, kw in (("plain", {}), ("guidance", {"rtc": True}), ("prefix", {"rtc": True, "rtc_method": "prefix", "flow_prefix_max_delay": D})):
        torch.manual_seed(3)
        pol = FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{args.model}:5", dropout=0.0), chunk_size=K, n_action_steps=n_exec, action_head="flow",
                            flow_steps=N, flow_time_dim=E, **kw).to(dev)
        pol.eval()
        pol.reset()
        pols[name] = pol
        cases[name] = lambda pol=pol: pol.select_action(img, st, "pick up the red cube", dev)
    res = {"model": args.model, "chunk": K, "max_delay": D, "action_dim": A, "flow_steps": N, "time_dim": E, "n_action_steps": n_exec,
           "env_steps_per_window": args.env_steps, "reps_per_window": args.reps,
           "control": {"unit": f"ms per environment step at B = 1, a plan on every {n_exec}th", **measure(cases, args.env_steps)}}
    c = res["control"]
    for name in ("guidance", "prefix"):
        c[f"{name}_minus_plain_ms"] = round(c[f"{name}_ms"] - c["plain_ms"], 5)
        c[f"{name}_minus_plain_per_round_ms"] = [round(r[name] - r["plain"], 5) for r in c["rounds"]]
    cfg, feat = pols["plain"].config, pols["plain"].model.backbone.output_dim
    for pol in pols.values():
        pol.reset()
        pol.model.backbone.engine().close()

    # the head alone, on the model's head dimensions (no backbone weights are loaded: the head entry points do not need them)
    m = arch.ModelConfig("head", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))

    def engine(prefix, guided=False):
        e = FastVLAEngine(m, state_dim=cfg.state_dim, action_dim=K * A, hidden_dim=cfg.hidden_dim, fusion_dim=cfg.fusion_dim, max_batch=64)
        e.set_head_flow(E)
        if prefix:
            e.set_head_flow_prefix(K, D)
        if guided:
            e.set_head_flow_guidance(prefix_weights(K, 0, n_exec, "exp"), 5.0)
        e.set_head_loss("mse", 1.0, K)
        return e

    def params(e):
        flat = (torch.randn(e.head_numel(), generator=g) * 0.02).to(dev)
        for k, v in e.head_views(flat).items():
            if k in ("state_projection.0.weight", "fusion.1.weight"):
                v.fill_(1.0)
        return flat

    plain, wide = engine(False, guided=True), engine(True)
    fp, fw = params(plain), params(wide)
    scases = {}
    for B in (1, 64):
        pooled, states = torch.randn(B, feat, generator=g).to(dev), torch.randn(B, cfg.state_dim, generator=g).to(dev)
        noise, prev = torch.randn(B, K * A, generator=g).to(dev), torch.randn(B, K * A, generator=g).to(dev)
        delays, out = torch.full((B,), D, dtype=torch.int32, device=dev), torch.empty(B, K * A, device=dev)
        scases[f"plain_b{B}"] = lambda pooled=pooled, states=states, noise=noise: plain.head_flow_sample(fp, pooled, states, steps=N, noise=noise)
        scases[f"guided_b{B}"] = lambda pooled=pooled, states=states, noise=noise, prev=prev, out=out: plain.head_flow_sample_guided(
            fp, pooled, states, prev, shift=n_exec, steps=N, noise=noise, chunk_out=out)[0]
        scases[f"prefix_b{B}"] = lambda pooled=pooled, states=states, noise=noise, prev=prev, out=out, delays=delays: wide.head_flow_sample_prefix(
            fw, pooled, states, prev, delays, shift=n_exec, steps=N, noise=noise, chunk_out=out)[0]
        scases[f"plain_w_b{B}"] = lambda pooled=pooled, states=states, noise=noise: wide.head_flow_sample(fw, pooled, states, steps=N, noise=noise)
    res["sampler"] = {"unit": f"ms per sampler call, {N} steps (host-enqueued back to back)", **measure(scases, args.reps)}
    for B in (1, 64):
        for k in ("prefix", "guided", "plain_w"):
            res[f"{k}_over_plain_b{B}"] = round(res["sampler"][f"{k}_b{B}_ms"] / res["sampler"][f"plain_b{B}_ms"], 3)
        res[f"plain_spread_over_plain_b{B}"] = round(res["sampler"][f"plain_b{B}_spread_ms"] / res["sampler"][f"plain_b{B}_ms"], 3)

    # the head-only train step
    B = 64
    pooled, states = torch.randn(B, feat, generator=g).to(dev), torch.randn(B, cfg.state_dim, generator=g).to(dev)
    targets = torch.randn(B, K * A, generator=g).to(dev)
    tcases = {}
    for name, e, flat in (("plain", plain, fp.clone()), ("prefix", wide, fw.clone())):
        mm, vv, saved, it = torch.zeros_like(flat), torch.zeros_like(flat), e.head_saved(B), [0]

        def step(e=e, flat=flat, mm=mm, vv=vv, saved=saved, it=it):
            it[0] += 1
            u = e.head_flow_prepare(targets, saved, seed=7, offset=it[0])
            v, _ = e.head_forward(flat, pooled, states, saved=saved, normalized_actions=True)
            _, grads = e.head_backward(flat, v, u, saved)
            e.adamw_step(flat, grads, mm, vv, it[0], lr=1e-5)
        tcases[name] = step
    res["train"] = {"unit": f"ms per head-only train step at B = {B}", **measure(tcases, args.reps)}
    res["train"]["prefix_over_plain"] = round(res["train"]["prefix_ms"] / res["train"]["plain_ms"], 3)
    plain.close(), wide.close()
    out = Path(args.out) if args.out else ROOT / "profiles" / "flow_prefix_bench.json"
    print(json.dumps(res))
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
