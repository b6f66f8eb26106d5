"""What several samples per observation cost (fv_head_flow_sample_multi), one process, alternating windows:
    python tools/flow_samples_bench.py [--model fastvlm-0.5b] [--chunk 50] [--steps 10] [--time-dim 64] [--reps 100] [--rounds 5] [--parent-checkout DIR] [--out FILE.json]
The head alone on the model's head dimensions (0.5B: feat 896, hid 1024, fus 1024, K = 50, A = 14, E = 64), N = --steps Euler steps, drawn noise, at B = 1 and 64:
    `plain_b{B}`         fv_head_flow_sample on this build
    `multi_b{B}_s{S}`    fv_head_flow_sample_multi, S = 1, 2, 4, 8, 16 candidates, select = medoid, every optional output asked for
    `multi_b{B}_s1_bare` the same entry point with S = 1 and no optional output: nothing to choose or report, the final stage writes the result itself
    `separate_b{B}_s{S}` S single fv_head_flow_sample calls at the candidates' offsets: what one multi-sample call replaces
    `select_b{B}_s{S}`   the selection kernel alone (fv_op_flow_select) on S candidates: its share of the call
    `parent_plain_b{B}`  --parent-checkout DIR (the root of a BUILT checkout of the parent commit): fv_head_flow_sample of THAT build, measured by a second
                         process that this one starts once and asks for a window each round, between its own windows -- the same box, alternating
    `served_plain_b{B}`  with --parent-checkout: fv_head_flow_sample of THIS build measured the same way, by a process of its own on a handle without candidates
Times: host clock around windows of --reps calls that end in a device synchronise; the median of --rounds rounds with its spread (max - min).
The conditions, stated before the run:
    (1) multi_b{B}_s1_bare and plain_b{B} each lie inside the min .. max of parent_plain_b{B}'s rounds, at B = 1 and 64
    (2) multi_b{B}_s{S} < separate_b{B}_s{S} at every S > 1
    (3) multi_b1_s{S} / multi_b1_s1 for S = 2 .. 8 is REPORTED (no figure is required)
Written to profiles/flow_samples_bench.json unless --out names another file."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
A, SAMPLES, BATCHES = 14, (1, 2, 4, 8, 16), (1, 64)
SEED, OFFSET = 7, (1 << 62) + 1


def setup(checkout: Path, args, samples: int):
    """-> (torch, engine, flat, {B: (pooled, states)}) on the package and library of `checkout`"""
    for p in (str(checkout), str(checkout / "vla-from-fastvlm_amd")):
        sys.path.insert(0, p)
    import torch
    from fastvla_hip import FastVLAEngine, arch
    if not torch.cuda.is_available():
        raise SystemExit("tools/flow_samples_bench.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    dims = arch.preset(args.model) if hasattr(arch, "preset") else None
    feat = dims.llm.hidden
    m = arch.ModelConfig("head", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    eng = FastVLAEngine(m, state_dim=A, action_dim=args.chunk * A, hidden_dim=1024, fusion_dim=1024, max_batch=max(BATCHES))
    eng.set_head_flow(args.time_dim)
    if samples > 1:
        eng.set_head_flow_samples(samples)
    g = torch.Generator().manual_seed(1)
    flat = (torch.randn(eng.head_numel(), generator=g) * 0.02).to(dev)
    for k, v in eng.head_views(flat).items():
        if k in ("state_projection.0.weight", "fusion.1.weight"):
            v.fill_(1.0)
    obs = {B: (torch.randn(B, feat, generator=g).to(dev), torch.randn(B, A, generator=g).to(dev)) for B in BATCHES}
    return torch, eng, flat, obs, feat


def window(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def serve(args):
    """the second process: the plain sampler of the checkout it was started on; one window per line read ("b1" / "b64"), "quit" ends it"""
    torch, eng, flat, obs, _ = setup(Path(args.serve).resolve(), args, 1)
    print("ready", flush=True)
    for line in sys.stdin:
        key = line.strip()
        if key == "quit":
            break
        pooled, states = obs[int(key[1:])]
        print(round(window(torch, lambda: eng.head_flow_sample(flat, pooled, states, steps=args.steps, seed=SEED, offset=OFFSET), args.reps), 5), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--time-dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-checkout", default=None, help="root of a built checkout of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--serve", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        serve(args)
        return
    torch, eng, flat, obs, feat = setup(ROOT, args, max(SAMPLES))
    from fastvla_hip import _lib
    K, N, da = args.chunk, args.steps, args.chunk * A
    ops = _lib.load_testops()
    stream = torch.cuda.current_stream().cuda_stream
    cases = {}
    for B in BATCHES:
        pooled, states = obs[B]
        cases[f"plain_b{B}"] = lambda pooled=pooled, states=states: eng.head_flow_sample(flat, pooled, states, steps=N, seed=SEED, offset=OFFSET)
        for S in SAMPLES:
            cases[f"multi_b{B}_s{S}"] = lambda pooled=pooled, states=states, S=S: eng.head_flow_sample_multi(flat, pooled, states, samples=S, select="medoid", steps=N,
                                                                                                              seed=SEED, offset=OFFSET)
            if S == 1:      # the call of a caller who wants one sample and no report: the single-sample call's launches
                cases[f"multi_b{B}_s1_bare"] = lambda pooled=pooled, states=states: eng.head_flow_sample_multi(flat, pooled, states, samples=1, select="first", steps=N,
                                                                                                            seed=SEED, offset=OFFSET, extras=False)
                continue

            def separate(pooled=pooled, states=states, S=S):
                for s in range(S):
                    eng.head_flow_sample(flat, pooled, states, steps=N, seed=SEED, offset=OFFSET + (s << 56))

            cases[f"separate_b{B}_s{S}"] = separate
            cand = torch.randn(S * B, da, device=flat.device)
            outs = [torch.empty(B, da, device=flat.device), torch.empty(B, da, device=flat.device), torch.empty(S * B, da, device=flat.device),
                    torch.empty(B, dtype=torch.int32, device=flat.device), torch.empty(B, S, device=flat.device), torch.empty(B, da, device=flat.device)]

            def select(cand=cand, outs=outs, B=B, S=S):
                _lib.check(ops.fv_op_flow_select(cand.data_ptr(), B, S, da, _lib.FLOW_SELECTS["medoid"], None, 0, None, None, K, None, None,
                                                 *(o.data_ptr() for o in outs), stream), "fv_op_flow_select")

            cases[f"select_b{B}_s{S}"] = select
    def start(checkout):
        c = subprocess.Popen([sys.executable, str(Path(__file__).resolve()), "--serve", str(Path(checkout).resolve()), "--model", args.model,
                              "--chunk", str(K), "--steps", str(N), "--time-dim", str(args.time_dim), "--reps", str(args.reps)],
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        if c.stdout.readline().strip() != "ready":
            raise SystemExit(f"the process of checkout {checkout} did not start")
        return c

    # (a process of its own has its own device addresses, and a handle without candidates a smaller workspace: `served_plain` is THIS build measured the way
    # the parent build is, so that the pair differs in the build alone)
    child, twin = (start(args.parent_checkout), start(ROOT)) if args.parent_checkout else (None, None)

    def served_window(c, B):
        c.stdin.write(f"b{B}\n")
        c.stdin.flush()
        return float(c.stdout.readline())

    rounds = []
    for _ in range(args.rounds):       # alternating windows: other work shares the machine
        r = {}
        for k, fn in cases.items():
            r[k] = round(window(torch, fn, args.reps), 5)
            if child and k.startswith("plain_b"):
                r["parent_" + k] = served_window(child, int(k[7:]))
                r["served_" + k] = served_window(twin, int(k[7:]))
        rounds.append(r)
    for c in (child, twin):
        if c:
            c.stdin.write("quit\n")
            c.stdin.flush()
            c.wait(timeout=60)
    eng.close()
    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
    res = {"model": args.model, "head": {"feat": feat, "hid": 1024, "fus": 1024, "chunk": K, "action_dim": A, "time_dim": args.time_dim}, "flow_steps": N,
           "reps_per_window": args.reps, "unit": "ms per call (host-enqueued back to back)", "rounds": rounds}
    for k in rounds[0]:
        xs = [r[k] for r in rounds]
        res[k + "_ms"], res[k + "_spread_ms"] = med(xs), round(max(xs) - min(xs), 5)
    cond = {}
    if child:
        for B in BATCHES:
            xs = [r[f"parent_plain_b{B}"] for r in rounds]
            lo, hi = min(xs), max(xs)
            cond[f"1_b{B}"] = {"parent_min_ms": lo, "parent_max_ms": hi, "plain_ms": res[f"plain_b{B}_ms"], "multi_s1_ms": res[f"multi_b{B}_s1_bare_ms"], "multi_s1_with_outputs_ms": res[f"multi_b{B}_s1_ms"],
                               "served_plain_ms": res[f"served_plain_b{B}_ms"], "plain_inside": lo <= res[f"plain_b{B}_ms"] <= hi,
                               "multi_s1_inside": lo <= res[f"multi_b{B}_s1_bare_ms"] <= hi, "served_plain_inside": lo <= res[f"served_plain_b{B}_ms"] <= hi}
    cond["2"] = {f"b{B}_s{S}": {"multi_ms": res[f"multi_b{B}_s{S}_ms"], "separate_ms": res[f"separate_b{B}_s{S}_ms"],
                                 "cheaper": res[f"multi_b{B}_s{S}_ms"] < res[f"separate_b{B}_s{S}_ms"]} for B in BATCHES for S in SAMPLES if S > 1}
    cond["3_b1_cost_over_s1"] = {f"s{S}": round(res[f"multi_b1_s{S}_ms"] / res["multi_b1_s1_ms"], 3) for S in SAMPLES if S > 1}
    cond["3_b64_cost_over_s1"] = {f"s{S}": round(res[f"multi_b64_s{S}_ms"] / res["multi_b64_s1_ms"], 3) for S in SAMPLES if S > 1}
    res["conditions"] = cond
    print(json.dumps({k: v for k, v in res.items() if k != "rounds"}))
    out = Path(args.out) if args.out else ROOT / "profiles" / "flow_samples_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
