"""What real-time chunking (the guided flow sampler) costs at inference, same process, alternating windows:
    python tools/rtc_bench.py [--model fastvlm-0.5b] [--chunk 50] [--steps 10] [--time-dim 64] [--env-steps 40] [--reps 100] [--rounds 5] [--out FILE.json]
    python tools/rtc_bench.py --digest
sampler    = the head alone on the model's head dimensions (explicit noise) at B = 1 and B = 64:
             `unguided`  fv_head_flow_sample (conditioning once, 3 launches per step)
             `guided`    fv_head_flow_sample_guided, "exp" weights with inference delay 0 and execution horizon 10, shift 10 (conditioning once, 8 per step)
             `zero`      the guided sampler with every weight 0 (the same launches; what the machinery costs when nothing guides)
control    = FastVLAPolicy.select_action at B = 1 on synthetic weights, chunk_size = --chunk, n_action_steps = 10, with and without rtc: milliseconds per
             ENVIRONMENT step over --env-steps calls (the backbone and the sampler run on every tenth)
Times: host clock around windows that end in a device synchronise; the median of --rounds rounds with its spread (max - min).  The figures to read:
`guided_over_unguided_b1` / `_b64` and `control.rtc_minus_plain_ms` against `control.plain_spread_ms`.
Written to profiles/rtc_bench.json unless --out names another file (an existing "digest" entry is kept).

--digest: sha256 over the actions of a flow policy WITHOUT rtc (synthetic:tiny, chunk 8, n_action_steps 3, 7 select_action calls, one reset in between):
the value recorded in profiles/rtc_bench.json was produced by the build before real-time chunking existed; a build that prints another has changed what a
policy that does not ask for rtc computes.  Uses nothing the earlier build lacks."""
import argparse
import hashlib
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


def digest(dev) -> str:
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    torch.manual_seed(3)
    pol = FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:tiny:77", hidden_dim=48, fusion_dim=64, dropout=0.0), chunk_size=8, n_action_steps=3,
                        action_head="flow", flow_time_dim=6, flow_seed=77).to(dev)
    g = torch.Generator().manual_seed(5)
    img, st = torch.rand(3, 72, 96, generator=g).to(dev), torch.randn(A, generator=g).to(dev)
    h = hashlib.sha256()
    for i in range(7):
        if i == 4:
            pol.reset()
        h.update(pol.select_action(img, st, "open drawer", dev).cpu().numpy().tobytes())
    h.update(pol.select_action_chunk(img, st, "open drawer", dev).cpu().numpy().tobytes())
    pol.model.backbone.engine().close()
    return h.hexdigest()


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
    ap.add_argument("--digest", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rtc_bench.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    if args.digest:
        print(json.dumps({"digest": digest(dev)}))
        return
    from fastvla_hip import FastVLAEngine, arch
    from fastvla_hip.rtc import prefix_weights
    K, N, E, n_exec = args.chunk, args.steps, args.time_dim, 10
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
    for name, kw in (("plain", {}), ("rtc", {"rtc": True})):
        torch.manual_seed(3)
        pol = FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{args.model}:5", dropout=0.0), chunk_size=K, n_action_steps=n_exec, action_head="flow",
                            flow_steps=N, flow_time_dim=E, **kw).to(dev)
        pol.eval()
        pol.reset()
        pols[name] = pol
        cases[name] = lambda pol=pol: pol.select_action(img, st, "pick up the red cube", dev)
    res = {"model": args.model, "chunk": K, "action_dim": A, "flow_steps": N, "time_dim": E, "n_action_steps": n_exec, "env_steps_per_window": args.env_steps,
           "reps_per_window": args.reps, "control": {"unit": f"ms per environment step at B = 1, a plan on every {n_exec}th", **measure(cases, args.env_steps)}}
    c = res["control"]
    c["rtc_minus_plain_ms"] = round(c["rtc_ms"] - c["plain_ms"], 5)
    c["rtc_minus_plain_per_round_ms"] = [round(r["rtc"] - r["plain"], 5) for r in c["rounds"]]
    cfg, feat = pols["rtc"].config, pols["rtc"].model.backbone.output_dim
    for pol in pols.values():
        pol.reset()
        pol.model.backbone.engine().close()

    # the head alone, on the model's head dimensions (no backbone weights are loaded: the head entry points do not need them)
    m = arch.ModelConfig("head", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    engs = {}
    for name, w in (("guided", prefix_weights(K, 0, n_exec, "exp")), ("zero", [0.0] * K)):
        engs[name] = FastVLAEngine(m, state_dim=cfg.state_dim, action_dim=K * A, hidden_dim=cfg.hidden_dim, fusion_dim=cfg.fusion_dim, max_batch=64)
        engs[name].set_head_flow(E)
        engs[name].set_head_flow_guidance(w, 5.0)
    eng = engs["guided"]
    flat = (torch.randn(eng.head_numel(), generator=g) * 0.02).to(dev)
    for k, v in eng.head_views(flat).items():
        if k in ("state_projection.0.weight", "fusion.1.weight"):
            v.fill_(1.0)
    scases, check = {}, {}
    for B in (1, 64):
        pooled, states = torch.randn(B, feat, generator=g).to(dev), torch.randn(B, cfg.state_dim, generator=g).to(dev)
        noise, prev = torch.randn(B, K * A, generator=g).to(dev), torch.randn(B, K * A, generator=g).to(dev)
        out = torch.empty(B, K * A, device=dev)

        def unguided(pooled=pooled, states=states, noise=noise):
            return eng.head_flow_sample(flat, pooled, states, steps=N, noise=noise)

        def guided(which, pooled=pooled, states=states, noise=noise, prev=prev, out=out):
            return engs[which].head_flow_sample_guided(flat, pooled, states, prev, shift=n_exec, steps=N, noise=noise, chunk_out=out)[0]

        scases[f"unguided_b{B}"] = unguided
        scases[f"guided_b{B}"] = lambda guided=guided: guided("guided")
        scases[f"zero_b{B}"] = lambda guided=guided: guided("zero")
        a, b = unguided(), guided("zero")
        torch.cuda.synchronize()
        check[f"b{B}"] = bool(torch.equal(a, b))
    res["sampler"] = {"unit": f"ms per sampler call, {N} steps (host-enqueued back to back)", **measure(scases, args.reps)}
    res["zero_weights_equal_unguided_bits"] = check
    for B in (1, 64):
        res[f"guided_over_unguided_b{B}"] = round(res["sampler"][f"guided_b{B}_ms"] / res["sampler"][f"unguided_b{B}_ms"], 3)
        res[f"zero_over_unguided_b{B}"] = round(res["sampler"][f"zero_b{B}_ms"] / res["sampler"][f"unguided_b{B}_ms"], 3)
    for e in engs.values():
        e.close()
    out = Path(args.out) if args.out else ROOT / "profiles" / "rtc_bench.json"
    if out.is_file():
        old = json.loads(out.read_text())
        if "digest" in old:
            res["digest"] = old["digest"]
    print(json.dumps(res))
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
