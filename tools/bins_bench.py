"""What the binned action head costs: its two kernels alone, and the head-only training step against the regression head.
    python tools/bins_bench.py [--parent-checkout DIR] [--model fastvlm-0.5b] [--batch 32] [--chunk 8] [--bins 256] [--reps 200] [--steps 10] [--rounds 5] [--out FILE.json]
kernels    = fv_op_bins_loss (loss kernel + fold) and fv_op_bins_decode alone at (B, K, A, Nb) = (--batch, --chunk, 14, --bins), enqueued back to back, timed with
             device events over --reps launches per window: microseconds per launch, the bytes the launch has to move -- loss: the logits read and the gradient
             written, 2 n Nb 4; decode: the logits read, n Nb 4 -- and bytes over time as a share of the 8.0 TB/s HBM peak.  At this size the logits (3.7 MB)
             stay in the caches: the figure is the launch, not HBM.
step       = FastVLAPolicy.fused_train_step on synthetic --model weights at B = --batch, chunk_size = --chunk, frozen backbone: `head` steps on features
             prepared once (the head's forward, loss, backward and the fused AdamW: what the head type changes), `train` is the whole step with the frozen
             backbone's forward.  Legs: `bins` (this build), `regression` (this build) and, with --parent-checkout DIR -- the root of a BUILT checkout of the
             parent commit --, `parent_regression`: the regression head of the parent build.  Every leg is a process of its own that stays up; the windows
             ALTERNATE between the legs (other work shares the machine), --steps steps per window, --rounds rounds; median and spread (max - min) per leg.
Written to profiles/action_bins_bench.json unless --out names another file."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
A = 14
HBM_PEAK = 8.0e12


def worker(checkout: Path, head: str, args) -> None:
    """one leg: builds its policy from `checkout`'s package and library, then answers every line on stdin with one JSON line of window times"""
    for p in (str(checkout), str(checkout / "vla-from-fastvlm_amd")):
        sys.path.insert(0, p)
    import torch
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    dev = torch.device("cuda", 0)
    kw = {"action_head": "bins", "action_bins": args.bins, "action_bins_range": (-3.0, 3.0)} if head == "bins" else {}
    torch.manual_seed(3)
    pol = FastVLAPolicy(FastVLAConfig(vlm_model_name=f"synthetic:{args.model}:5", dropout=0.0), chunk_size=args.chunk, **kw).to(dev)
    pol.train()
    g = torch.Generator().manual_seed(1)
    B, K = args.batch, args.chunk
    batch = {"images": torch.rand(B, 3, 336, 336, generator=g).to(dev), "states": torch.randn(B, A, generator=g).to(dev),
             "actions": torch.randn(B, K, A, generator=g).clamp(-2.9, 2.9).to(dev), "tasks": ["pick up the red cube"] * B}
    skw = dict(lr=1e-4, weight_decay=1e-4, max_grad_norm=1.0)
    prep = pol.prepare_batch(batch)
    for _ in range(3):      # warm-up of both forms
        pol.fused_train_step(prepared=prep, **skw)
        pol.fused_train_step(batch, **skw)
    torch.cuda.synchronize()
    import fastvla_hip
    lib = fastvla_hip.library_path().resolve()      # (named relative to its checkout: which build the leg ran is the point, not where it lay)
    print(json.dumps({"ready": head, "checkout": "this build" if checkout.resolve() == ROOT else "--parent-checkout", "lib": str(lib.relative_to(checkout.resolve())),
                      "head_numel": int(pol.model._flat.numel())}), flush=True)

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.steps, float(out["loss"])

    for line in sys.stdin:
        if line.strip() == "quit":
            break
        h, lh = window(lambda: pol.fused_train_step(prepared=prep, **skw))
        t, lt = window(lambda: pol.fused_train_step(batch, **skw))
        print(json.dumps({"head_ms": round(h, 5), "train_ms": round(t, 5), "loss": lt}), flush=True)
    pol.model.backbone.engine().close()


def kernels(args) -> dict:
    for p in (str(ROOT), str(ROOT / "vla-from-fastvlm_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    from fastvla_hip import _lib
    lib = _lib.load_testops()
    dev = torch.device("cuda", 0)
    B, K, nb = args.batch, args.chunk, args.bins
    n = B * K * A
    g = torch.Generator().manual_seed(2)
    z = (torch.rand(n, nb, generator=g) * 16 - 8).to(dev)
    t = (torch.rand(n, generator=g) * 6 - 3).to(dev)
    w = np.float32((3.0 - -3.0) / nb)
    rng = torch.tensor([-3.0, 3.0, float(w)], device=dev)
    grad, act = torch.empty_like(z), torch.empty(n, device=dev)
    part, out = torch.empty(4 * ((n + 3) // 4), device=dev), torch.empty(5, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def loss(sigma):
        _lib.check(lib.fv_op_bins_loss(z.data_ptr(), t.data_ptr(), None, None, None, rng.data_ptr(), 1, sigma, 0, grad.data_ptr(), part.data_ptr(), part.numel(),
                                       out.data_ptr(), out[1:].data_ptr(), n, nb, K * A, K, 1.0, st), "fv_op_bins_loss")

    def decode(mode):
        _lib.check(lib.fv_op_bins_decode(z.data_ptr(), rng.data_ptr(), 1, mode, act.data_ptr(), None, n, nb, K * A, None, None, st), "fv_op_bins_decode")

    cases = {"loss_hard": (lambda: loss(0.0), 2 * n * nb * 4), "loss_hl_gauss": (lambda: loss(0.75), 2 * n * nb * 4), "decode_argmax": (lambda: decode(0), n * nb * 4),
             "decode_mean": (lambda: decode(1), n * nb * 4)}
    rounds = []
    for _ in range(args.rounds):
        row = {}
        for name, (fn, _bytes) in cases.items():
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            row[name] = round(1e3 * e0.elapsed_time(e1) / args.reps, 4)
        rounds.append(row)
    res = {"unit": "microseconds per launch (loss: kernel + fold), device events, launches enqueued back to back", "shape": [B, K, A, nb], "groups": n, "rounds": rounds}
    for name, (_fn, nbytes) in cases.items():
        xs = sorted(r[name] for r in rounds)
        med = xs[len(xs) // 2]
        res[name] = {"us": med, "spread_us": round(xs[-1] - xs[0], 4), "bytes": nbytes, "gb_per_s": round(nbytes / (med * 1e-6) / 1e9, 1),
                     "share_of_hbm_peak": round(nbytes / (med * 1e-6) / HBM_PEAK, 4)}
    return res


def read_record(p, name):
    """the next JSON line of a leg's stdout (the package prints notes of its own there)"""
    while True:
        line = p.stdout.readline()
        if not line:
            raise SystemExit(f"tools/bins_bench.py: the {name} leg ended early (exit {p.wait()})")
        if line.startswith("{"):
            return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-checkout", default=None)
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=2, default=None, metavar=("CHECKOUT", "HEAD"))
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), args.worker[1], args)
    res = {"model": args.model, "batch": args.batch, "chunk": args.chunk, "action_dim": A, "bins": args.bins, "steps_per_window": args.steps,
           "launches_per_window": args.reps, "kernels": kernels(args)}
    legs = [("bins", ROOT, "bins"), ("regression", ROOT, "regression")]
    if args.parent_checkout:
        legs.append(("parent_regression", Path(args.parent_checkout).resolve(), "regression"))
    common = ["--model", args.model, "--batch", str(args.batch), "--chunk", str(args.chunk), "--bins", str(args.bins), "--steps", str(args.steps)]
    procs = {}
    try:
        for name, checkout, head in legs:      # one after the other: a leg is up and warm before the next one starts
            p = subprocess.Popen([sys.executable, str(Path(__file__).resolve()), "--worker", str(checkout), head, *common], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            procs[name] = p
            res.setdefault("legs", {})[name] = read_record(p, name)
        rounds = []
        for _ in range(args.rounds):
            row = {}
            for name, p in procs.items():
                p.stdin.write("go\n")
                p.stdin.flush()
                row[name] = read_record(p, name)
            rounds.append(row)
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
                p.wait(timeout=60)
            except Exception:
                p.kill()
    step = {"unit": "ms per step; head = on prepared features, train = with the frozen backbone's forward", "rounds": rounds}
    for name in procs:
        for key in ("head_ms", "train_ms"):
            xs = sorted(r[name][key] for r in rounds)
            step[f"{name}_{key}"] = xs[len(xs) // 2]
            step[f"{name}_{key[:-3]}_spread_ms"] = round(xs[-1] - xs[0], 5)
    for base in (n for n in ("regression", "parent_regression") if n in procs):
        for key in ("head_ms", "train_ms"):
            step[f"bins_minus_{base}_{key}"] = round(step[f"bins_{key}"] - step[f"{base}_{key}"], 5)
    res["step"] = step
    print(json.dumps(res))
    out = Path(args.out) if args.out else ROOT / "profiles" / "action_bins_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
