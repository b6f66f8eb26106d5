"""What the step guard costs in the fused optimiser call, and proof that a run without it kept its bits.
    python tools/step_guard_bench.py [--repeats 7] [--reps 10] [--out profiles/step_guard_bench.json]
    python tools/step_guard_bench.py --digest [--checkout DIR]
Timing: the optimiser call alone over the FastVLM-0.5B master and over the rank-16 LoRA trainable buffer, plain (fv_adamw_clip_step) against guarded
(fv_adamw_clip_step_guarded, healthy gradients: every step is applied), in ONE process, in alternating windows of `reps` back-to-back calls between device
events, `repeats` windows per leg: median and spread (max - min) per leg.  The guard adds one one-block launch and one scalar load per block, nothing per
element; the cost of one one-block launch (fv_step_guard_observe) is measured in the same run.  Acceptance, stated with the numbers and not tuned:
    guarded median - plain median <= spread of the plain windows + one one-block launch
--digest: sha256 of the master after 3 full-decoder steps at B = 32 (FastVLM-0.5B, synthetic weights, fixed seeds) with the guard OFF, through calls that exist
without the feature; --checkout DIR runs a built checkout of the parent commit with this very script: equal digests say the default path kept its bits."""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent


def _use_checkout(root) -> None:
    for p in (str(root), str(Path(root) / "vla-from-fastvlm_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _stats(xs):
    xs = sorted(xs)
    return {"ms": round(xs[len(xs) // 2], 5), "min_ms": round(xs[0], 5), "max_ms": round(xs[-1], 5), "spread_ms": round(xs[-1] - xs[0], 5)}


def _engine(args):
    from fastvla_hip import FastVLAEngine, arch, weights
    model = arch.preset(args.model)
    eng = FastVLAEngine(model, max_batch=args.batch, max_text_tokens=args.tokens, llm_precision=1)
    eng.load_weights(weights.init_backbone(model, seed=1234))
    return eng


def digest(args) -> dict:
    """3 whole full-decoder steps, guard off: forward / backward, fv_adamw_clip_step over the master, commit -> sha256 of the master"""
    dev = torch.device("cuda", 0)
    eng = _engine(args)
    B, T = args.batch, args.tokens
    gen = torch.Generator().manual_seed(1)
    images = torch.rand(B, 3, 336, 336, generator=gen).to(dev)
    ids, lens = torch.randint(0, 151643, (B, T), generator=gen), torch.full((B,), T)
    states, targets = torch.randn(B, 14, generator=gen).to(dev), torch.randn(B, 14, generator=gen).to(dev)
    eng.train_begin()
    _, total, _ = eng.train_layout()
    hn = eng.head_numel()
    _, tower_out = eng.vision_forward(eng.preprocess(images), return_tower_out=True)
    tower_out = tower_out.clone()
    flat = torch.zeros(total, device=dev)
    eng.train_export_params(flat)
    for k, t in eng.head_views(flat[:hn]).items():
        t.copy_(torch.randn(t.shape, generator=gen) * 0.02 + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0))
    eng.train_commit(flat)
    ws = eng.train_workspace(B, T)
    g, m, v = (torch.zeros_like(flat) for _ in range(3))
    for step in (1, 2, 3):
        eng.train_forward_backward(flat, tower_out, ids, lens, states, targets, ws, training=True, dropout_p=0.1, seed=7, offset=step, flat_grads=g)
        eng.adamw_step(flat, g, m, v, step, lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, grad_scale=1.0 / eng.train_loss_scale())
        eng.train_commit(flat)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for lo in range(0, total, 1 << 26):
        h.update(flat[lo: lo + (1 << 26)].cpu().numpy().tobytes())
    eng.close()
    return {"full_decoder_b32_p_after_3_steps": h.hexdigest(), "numel": int(total), "model": args.model, "batch": B}


def bench(args) -> dict:
    from fastvla_hip import StepGuard
    dev = torch.device("cuda", 0)
    eng = _engine(args)
    eng.train_begin()
    eng.train_lora_begin(args.rank, None, "all")
    _, total, _ = eng.train_layout()
    _, ltotal = eng.train_lora_layout()
    hp = dict(lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, grad_scale=1.0 / eng.train_loss_scale())
    guard = StepGuard(eng, init_delta_log2=0, min_delta_log2=-12, max_delta_log2=12)
    res = {"model": args.model, "rank": args.rank, "repeats": args.repeats, "reps_per_window": args.reps, "optimizer": {}}
    res["one_block_launch"] = _stats([_window(guard.observe, 200) for _ in range(args.repeats)])
    launch = res["one_block_launch"]["ms"]
    for name, n in ((f"lora_rank{args.rank}", ltotal), ("full_master", total)):
        p = torch.empty(n, device=dev).normal_(0, 0.02)
        g = torch.empty(n, device=dev).normal_(0, 1.0)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        norm = torch.zeros(1, device=dev)
        calls = {"plain": lambda: eng.adamw_step(p, g, m, v, 1, grad_norm_out=norm, **hp),
                 "guarded": lambda: eng.adamw_step(p, g, m, v, 1, grad_norm_out=norm, guard=guard, **hp)}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        xs = {"plain": [], "guarded": []}
        for _ in range(args.repeats):      # alternating windows: drift of the clocks lands on both legs
            for leg in ("plain", "guarded"):
                xs[leg].append(_window(calls[leg], args.reps))
        entry = {"numel": int(n), "plain": _stats(xs["plain"]), "guarded": _stats(xs["guarded"])}
        entry["guarded_minus_plain_ms"] = round(entry["guarded"]["ms"] - entry["plain"]["ms"], 5)
        entry["bound_ms"] = round(entry["plain"]["spread_ms"] + launch, 5)
        entry["within_bound"] = entry["guarded_minus_plain_ms"] <= entry["bound_ms"]
        res["optimizer"][name] = entry
        del p, g, m, v
        torch.cuda.empty_cache()
    st = guard.state()
    res["guard_state_after"] = {k: st[k] for k in ("applied", "skipped_nonfinite", "skipped_saturated", "delta_log2")}
    guard.close()
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkout", default=None, help="root of a built checkout to run in place of this one (the parent commit's: --digest only)")
    ap.add_argument("--digest", action="store_true", help="only the guard-off digest of 3 full-decoder steps")
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.checkout and not args.digest:
        raise SystemExit("--checkout goes with --digest: the guarded legs exist in this build only")
    _use_checkout(args.checkout or ROOT)
    if not torch.cuda.is_available():
        raise SystemExit("tools/step_guard_bench.py measures on the GPU: no HIP device visible")
    res = {"digest": digest(args)} if args.digest else bench(args)
    res["checkout"] = "other" if args.checkout else "this"
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
