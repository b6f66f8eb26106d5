"""What action chunks cost in the head and buy in the control loop, same process, alternating windows:
    python tools/chunk_bench.py [--model fastvlm-0.5b] [--batch 64] [--chunk 50] [--reps 20] [--rounds 3] [--env-steps 40] [--out FILE.json]
head       = fv_head_forward + fv_head_mse_backward at the model's head dimensions (feat = llm hidden, hidden = fusion = 1024, A = 14), B = --batch, for a head
             K * A wide with K = 1 and K = --chunk, each with the plain MSE (the single-block kernel, whatever K) and with the masked L1 (chunk_loss_kernel + fold)
loss       = the chunked loss kernel + its fold alone (fv_op_chunk_loss) on (B, K, A)
control    = FastVLAPolicy.select_action at B = 1 on synthetic weights, milliseconds per ENVIRONMENT step over --env-steps calls: K = 1 (today's loop), then
             K = --chunk with n_action_steps 1 and 10 (the backbone runs on every n-th call; the other calls pop a queued row)
Times: host clock around windows of --reps calls that end in a device synchronise; the median of --rounds rounds with its spread (max - min).  Every figure is
to be read against the same run's K = 1 leg.  The head engine carries no weights.  Written to profiles/action_chunk_bench.json unless --out names another file."""
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
from fastvla_hip import FastVLAEngine, _lib, arch  # noqa: E402

A = 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--env-steps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/chunk_bench.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    model = arch.preset(args.model)
    B = args.batch
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
            rounds.append({k: round(window(fn, reps), 4) for k, fn in cases.items()})
        out = {"rounds": rounds}
        for k in cases:
            xs = [r[k] for r in rounds]
            out[k + "_ms"], out[k + "_spread_ms"] = med(xs), round(max(xs) - min(xs), 4)
        return out

    res = {"model": args.model, "batch": B, "action_dim": A, "chunk": args.chunk, "reps_per_window": args.reps, "head": {}, "control": {}}
    g = torch.Generator().manual_seed(1)
    ops = _lib.load_testops()
    cases, keep = {}, []
    for K in (1, args.chunk):
        da = K * A
        eng = FastVLAEngine(model, state_dim=A, action_dim=da, hidden_dim=1024, fusion_dim=1024, max_batch=B, max_text_tokens=8)
        flat = (torch.randn(eng.head_numel(), generator=g) * 0.02).to(dev)
        pooled, states = torch.randn(B, model.llm.hidden, generator=g).to(dev), torch.randn(B, A, generator=g).to(dev)
        tgt = torch.randn(B, da, generator=g).to(dev)
        pad = torch.zeros(B, K, dtype=torch.bool)
        for b in range(B):
            pad[b, K - (b % (K + 1)):] = b % (K + 1) > 0
        pad_dev = pad.to(dev)
        grads, saved = torch.zeros(eng.head_numel(), device=dev), eng.head_saved(B)
        act = eng.head_forward(flat, pooled, states, saved=saved)[0]
        gbuf, part, out3, pad8 = torch.zeros(B, da, device=dev), torch.zeros(768, device=dev), torch.zeros(3, device=dev), pad_dev.to(torch.uint8)

        def step(eng=eng, flat=flat, pooled=pooled, states=states, tgt=tgt, saved=saved, grads=grads, pad=None):
            a, _ = eng.head_forward(flat, pooled, states, saved=saved, normalized_actions=True)
            eng.head_backward(flat, a, tgt, saved, flat_grads=grads, pad=pad)

        def mse_step(eng=eng, step=step):
            if eng.head_loss["kind"] != "mse":
                eng.set_head_loss("mse", 1.0, eng.head_loss["chunk"])
            step()

        def l1_step(eng=eng, step=step, K=K, pad_dev=pad_dev):
            if eng.head_loss["kind"] != "l1":
                eng.set_head_loss("l1", 1.0, K)
            step(pad=pad_dev)

        def loss_alone(act=act, tgt=tgt, pad8=pad8, gbuf=gbuf, part=part, out3=out3, da=da):
            _lib.check(ops.fv_op_chunk_loss(act.data_ptr(), tgt.data_ptr(), pad8.data_ptr(), gbuf.data_ptr(), part.data_ptr(), 768, out3.data_ptr(),
                                            out3[1:].data_ptr(), B * da, A, 1, 1.0, 1.0, torch.cuda.current_stream().cuda_stream), "fv_op_chunk_loss")

        cases.update({f"K{K}_mse_step": mse_step, f"K{K}_l1_masked_step": l1_step, f"K{K}_chunk_loss_alone": loss_alone})
        keep.append(eng)
    res["head"] = measure(cases, args.reps)
    for K in (1, args.chunk):
        h = res["head"]
        h[f"K{K}_l1_over_mse"] = round(h[f"K{K}_l1_masked_step_ms"] / h[f"K{K}_mse_step_ms"], 4)
    res["head"]["wide_over_narrow_mse"] = round(res["head"][f"K{args.chunk}_mse_step_ms"] / res["head"]["K1_mse_step_ms"], 4)
    for eng in keep:
        eng.close()

    # ---- the control loop: select_action per environment step
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    img, st = torch.rand(3, 336, 336, generator=g), torch.randn(A, generator=g)
    cases = {}
    for K, n in ((1, 1), (args.chunk, 1), (args.chunk, min(10, args.chunk))):
        torch.manual_seed(3)
        pol = FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{args.model}:5", dropout=0.0), chunk_size=K, n_action_steps=n).to(dev)
        pol.eval()

        def env_step(pol=pol):
            pol.select_action(img, st, "pick up the red cube", dev)

        def run(pol=pol, env_step=env_step, n=n):       # whole refill periods only: a window starts and ends on an empty queue
            pol.reset()
            for _ in range(n):
                env_step()

        cases[f"K{K}_n{n}"] = (run, n, pol)
    rounds = []
    for _ in range(args.rounds):
        rounds.append({k: round(window(run, max(1, args.env_steps // n)) / n, 4) for k, (run, n, _) in cases.items()})
    c = {"rounds": rounds, "unit": "ms per environment step"}
    for k in cases:
        xs = [r[k] for r in rounds]
        c[k + "_ms"], c[k + "_spread_ms"] = med(xs), round(max(xs) - min(xs), 4)
    base = c["K1_n1_ms"]
    for k in cases:
        c[k + "_over_K1"] = round(c[k + "_ms"] / base, 4)
    res["control"] = c
    for _, _, pol in cases.values():
        pol.model.backbone.engine().close()
    print(json.dumps(res))
    out = Path(args.out) if args.out else ROOT / "profiles" / "action_chunk_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
