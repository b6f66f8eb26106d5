"""The headline step of bench.py (literal mode, fastvlm-0.5b, B = 64, T = 64) on the MISS path of prompt reuse: one id of the prompt is flipped before every
step, so every literal call's probe misses, the decoder runs and the commit stores key and rows.  Against bench.py's own figure with FASTVLA_PROMPT_REUSE=0
this prices the probe and commit launches; `--same` flips the id of a scratch copy instead (the same extra launch per step, every call after the first hits).

    python tools/prompt_miss_bench.py --steps 50 --warmup 5 [--same]      -> one JSON line
"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--image", type=int, default=336)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--same", action="store_true", help="flip an id of a scratch copy: the prompt stays, every call after the first hits")
    args = ap.parse_args()
    from fastvla_hip import FastVLAEngine, arch, weights
    dev = torch.device("cuda", 0)
    model = arch.preset(args.model)
    B, T = args.batch, args.tokens
    eng = FastVLAEngine(model, state_dim=14, action_dim=14, hidden_dim=1024, fusion_dim=1024, device=dev, max_batch=B, max_text_tokens=T,
                        llm_precision=arch.default_llm_precision(model))
    eng.load_weights(weights.init_backbone(model, seed=args.seed))
    flat = torch.zeros(eng.head_numel(), dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(4321)
    for k, v in eng.head_views(flat).items():
        if v.ndim == 2:
            v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) / (v.shape[1] ** 0.5))
        elif k in ("state_projection.0.weight", "fusion.1.weight"):
            v.fill_(1.0)
    torch.manual_seed(1234)
    images = torch.rand(B, 3, args.image, args.image, device=dev)
    ids = torch.randint(0, min(151643, model.llm.vocab), (B, T), device=dev, dtype=torch.int32)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    states = torch.randn(B, 14, device=dev)
    scratch = ids.clone()

    def step():
        (scratch if args.same else ids)[0, 0:1].bitwise_xor_(1)
        act, _ = eng.head_forward(flat, eng.backbone(images, ids, lens), states)
        return act

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    c0, h0 = eng.prompt_reuse_stats()
    t = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t
    c1, h1 = eng.prompt_reuse_stats()
    print(json.dumps({"metric": "prompt_reuse_step_ms", "mode": "same prompt" if args.same else "one id flipped per step", "ms_per_step": round(1e3 * el / args.steps, 3),
                      "steps": args.steps, "literal_calls": c1 - c0, "hits": h1 - h0, "batch": B, "tokens": T, "model": args.model}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
