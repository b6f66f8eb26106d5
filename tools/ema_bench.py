"""What an EMA of the trainable weights costs at the three buffer sizes the project trains (FastVLM-0.5B, B = 32): head ~3 M floats, rank-16 LoRA trainable
buffer ~15 M, full master ~0.5 G.
    python tools/ema_bench.py [--checkout DIR] [--repeats 5] [--reps 20] [--no-steps] [--out FILE.json]
    python tools/ema_bench.py --digest [--checkout DIR]
Three legs, for the optimiser call alone (device events around `reps` back-to-back calls after a warm-up call, `repeats` such measurements, median and range)
and for the whole training step (device events around `steps` steps):
    off    fv_adamw_clip_step / fv_adamw_clip_step_groups, no average                                32 bytes per element
    fused  fv_adamw_clip_step_ema: the average moves in the same pass                                 40 bytes per element
    lerp   `off` followed by torch.Tensor.lerp_ on the average, the unfused alternative               44 bytes per element
`off` uses only calls that exist without the feature: --checkout DIR measures a built checkout of the PARENT commit with this very script (legs off only; its
range over the repeats is the run-to-run spread the other figures are read against).  GB/s = bytes per element x numel / time.
--digest: sha256 of (p, m, v) after 3 head-only updates (`tiny`) and 3 rank-4 LoRA updates (`small`) of a policy that never switches EMA on (FASTVLA_EMA_* unset):
equal digests from this build and from the parent's say the default path kept its bits (tests/test_gpu_ema.py compares with profiles/ema_bench.json)."""
import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
BYTES = {"off": 32, "fused": 40, "lerp": 44}


def _use_checkout(root) -> None:
    for p in (str(root), str(Path(root) / "vla-from-fastvlm_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


def default_path_digests(dev: str = "cuda:0") -> dict:
    """{"head_only", "lora_rank4"}: sha256 over the bytes of p, m, v after 3 updates; the package that is importable decides which build is measured"""
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    for k in ("FASTVLA_EMA_DECAY", "FASTVLA_EMA_WARMUP", "FASTVLA_EMA_UPDATE_AFTER"):
        if os.environ.get(k):
            raise RuntimeError(f"{k} is set: the digests are those of a run that does not switch EMA on")
    out = {}
    for name, model, enable in (("head_only", "tiny:77", None), ("lora_rank4", "small:41", dict(lora_rank=4, lora_alpha=8.0))):
        torch.manual_seed(31)
        cfg = FastVLAConfig(vlm_model_name=f"synthetic:{model}", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=enable is None)
        pol = FastVLAPolicy(cfg).to(dev)
        pol.train()
        if enable is not None:
            pol.enable_backbone_training(**enable)
        g = torch.Generator().manual_seed(6)
        for _ in range(3):
            batch = {"images": torch.rand(2, 3, 96, 128, generator=g).to(dev), "states": torch.randn(2, 14, generator=g).to(dev),
                     "actions": torch.randn(2, 14, generator=g).to(dev), "tasks": ["pick up the red cube", "open the drawer"]}
            pol.fused_train_step(batch, lr=1e-3, weight_decay=1e-2)
        torch.cuda.synchronize()
        p = pol._unfrozen.trainable if pol._unfrozen is not None else pol.model._flat
        h = hashlib.sha256()
        for t in (p, pol._opt_state["m"], pol._opt_state["v"]):
            h.update(t.detach().cpu().numpy().tobytes())
        out[name] = h.hexdigest()
        pol.model.backbone.engine().close()
    return out


def _events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _measure(fn, reps, repeats):
    fn()
    torch.cuda.synchronize()
    xs = sorted(_events(fn, reps) for _ in range(repeats))
    return {"ms": round(xs[len(xs) // 2], 5), "min_ms": round(xs[0], 5), "max_ms": round(xs[-1], 5), "spread_ms": round(xs[-1] - xs[0], 5)}


def bench(args) -> dict:
    from fastvla_hip import FastVLAEngine, _lib, arch, lora, optim, weights
    have_ema = "fv_adamw_clip_step_ema" in _lib.SIGNATURES
    legs = ["off"] + (["fused", "lerp"] if have_ema else [])
    dev = torch.device("cuda", 0)
    model = arch.preset(args.model)
    B, T = args.batch, args.tokens
    eng = FastVLAEngine(model, max_batch=B, max_text_tokens=T, llm_precision=1)
    eng.load_weights(weights.init_backbone(model, seed=1234))
    hn = eng.head_numel()
    w = 1e-3      # float32(1 - 0.999) up to rounding: any weight in (0, 1) runs the same instructions
    res = {"model": args.model, "batch": B, "rank": args.rank, "legs": legs, "bytes_per_element": {k: BYTES[k] for k in legs}, "repeats": args.repeats,
           "reps_per_measurement": args.reps, "steps_per_measurement": args.steps, "ema_weight": w, "optimizer": {}, "step": {}}
    gen = torch.Generator().manual_seed(1)
    images = torch.rand(B, 3, 336, 336, generator=gen).to(dev)
    ids, lens = torch.randint(0, 151643, (B, T), generator=gen), torch.full((B,), T)
    states, targets = torch.randn(B, 14, generator=gen).to(dev), torch.randn(B, 14, generator=gen).to(dev)
    hp = dict(lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, grad_scale=1.0)
    cnt = {"i": 0}

    def opt(leg, p, g, m, v, e):
        cnt["i"] += 1
        if leg == "fused":
            eng.adamw_step(p, g, m, v, cnt["i"], ema=e, ema_weight=w, **hp)
        else:
            eng.adamw_step(p, g, m, v, cnt["i"], **hp)
            if leg == "lerp":
                e.lerp_(p, w)

    def run_mode(name, step, p, bufs):
        p0 = p.clone()
        res["step"][name] = {}
        for leg in legs:
            p.copy_(p0)
            for b in bufs[:2]:
                b.zero_()
            bufs[2].copy_(p0)
            cnt["i"] = 0
            step(leg)
            torch.cuda.synchronize()
            xs = sorted(_events(lambda: step(leg), args.steps) for _ in range(args.repeats))
            res["step"][name][leg] = {"ms": round(xs[len(xs) // 2], 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4), "spread_ms": round(xs[-1] - xs[0], 4)}
        p.copy_(p0)

    if not args.no_steps:
        # head-only, the flagship step: frozen backbone forward (the reference-literal one), head forward / backward, the optimiser over the head buffer --
        # measured BEFORE the handle enters training mode
        hflat = (torch.randn(hn, generator=gen) * 0.02).to(dev)
        for k, t in eng.head_views(hflat).items():
            if k in ("state_projection.0.weight", "fusion.1.weight"):
                t.add_(1.0)
        hm, hv, he = torch.zeros_like(hflat), torch.zeros_like(hflat), hflat.clone()

        def head_step(leg):
            pooled = eng.backbone(images, ids, lens, splice=False)
            act, saved = eng.head_forward(hflat, pooled, states, training=False)
            _, hg = eng.head_backward(hflat, act, targets, saved)
            opt(leg, hflat, hg, hm, hv, he)

        run_mode("head", head_step, hflat, (hm, hv, he))
    eng.train_begin()
    eng.train_lora_begin(args.rank, None, "all")
    tensors, total, _ = eng.train_layout()
    lt, ltotal = eng.train_lora_layout()
    hp["grad_scale"] = 1.0 / eng.train_loss_scale()

    # ---- the optimiser call alone
    sizes = {"head": hn, f"lora_rank{args.rank}": ltotal, "full_master": total}
    for name, n in sizes.items():
        p = torch.empty(n, device=dev).normal_(0, 0.02)
        g = torch.empty(n, device=dev).normal_(0, 1.0)
        m, v, e = torch.zeros_like(p), torch.zeros_like(p), p.clone()
        norm = torch.zeros(1, device=dev)
        reps = args.reps if n < (1 << 26) else max(3, args.reps // 2)
        calls = {"off": lambda: eng.adamw_step(p, g, m, v, 1, grad_norm_out=norm, **hp)}
        if have_ema:
            calls["fused"] = lambda: eng.adamw_step(p, g, m, v, 1, grad_norm_out=norm, ema=e, ema_weight=w, **hp)
            calls["lerp"] = lambda: (eng.adamw_step(p, g, m, v, 1, grad_norm_out=norm, **hp), e.lerp_(p, w))
        entry = {"numel": n, "single": {}}
        for leg in legs:
            r = _measure(calls[leg], reps, args.repeats)
            r["gb_s"] = round(BYTES[leg] * n / r["ms"] / 1e6, 1)
            entry["single"][leg] = r
        if name == "full_master":      # the grouped kernel under a full fine-tuning table (decoder x 0.1, layer decay 0.9, no decay on vectors)
            groups, _ = optim.build_param_groups(tensors, weight_decay=hp["weight_decay"], total=n, lr_scales={"decoder": 0.1}, layer_decay=0.9, no_decay=("vectors",))
            table = eng.adamw_groups(groups, n)
            gn = torch.zeros(len(groups), device=dev)
            gcalls = {"off": lambda: eng.adamw_step(p, g, m, v, 1, grad_norm_out=norm, groups=table, group_norms_out=gn, **hp)}
            if have_ema:
                gcalls["fused"] = lambda: eng.adamw_step(p, g, m, v, 1, grad_norm_out=norm, groups=table, group_norms_out=gn, ema=e, ema_weight=w, **hp)
                gcalls["lerp"] = lambda: (eng.adamw_step(p, g, m, v, 1, grad_norm_out=norm, groups=table, group_norms_out=gn, **hp), e.lerp_(p, w))
            entry["grouped"] = {"groups": len(groups)}
            for leg in legs:
                r = _measure(gcalls[leg], reps, args.repeats)
                r["gb_s"] = round(BYTES[leg] * n / r["ms"] / 1e6, 1)
                entry["grouped"][leg] = r
            table.close()
        res["optimizer"][name] = entry
        del p, g, m, v, e
        torch.cuda.empty_cache()
    if args.no_steps:
        eng.close()
        return res

    # ---- the whole training step (the frozen tower runs once, outside: the same work in every leg)
    pix = eng.preprocess(images)
    _, tower_out = eng.vision_forward(pix, return_tower_out=True)
    tower_out = tower_out.clone()
    flat = torch.zeros(total, device=dev)
    eng.train_export_params(flat)
    for k, t in eng.head_views(flat[:hn]).items():
        t.copy_(torch.randn(t.shape, generator=gen) * 0.02 + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0))
    front = next(t["offset"] for t in lt if ".lora_" in t["name"])
    lflat = torch.zeros(ltotal, device=dev)
    lflat[:front].copy_(flat[:front])
    lora.init_adapters(lflat, lt, seed=0)
    ws = eng.train_workspace(B, T)
    grads = torch.zeros_like(flat)
    # rank-16 LoRA (projected): forward / backward, projection, the optimiser over the trainable buffer, adapted commit
    lg, lm, lv, le = (torch.zeros_like(lflat) for _ in range(4))

    def lora_step(leg):
        eng.train_forward_backward(flat, tower_out, ids, lens, states, targets, ws, training=True, dropout_p=0.1, seed=7, offset=cnt["i"] + 1, flat_grads=grads)
        eng.train_lora_project(grads, lflat, lg)
        opt(leg, lflat, lg, lm, lv, le)
        eng.train_lora_commit(flat, lflat)

    run_mode(f"lora_rank{args.rank}", lora_step, lflat, (lm, lv, le))
    # full fine-tuning: forward / backward, the optimiser over the whole master, commit
    fm, fv, fe = (torch.zeros_like(flat) for _ in range(3))

    def full_step(leg):
        eng.train_forward_backward(flat, tower_out, ids, lens, states, targets, ws, training=True, dropout_p=0.1, seed=7, offset=cnt["i"] + 1, flat_grads=grads)
        opt(leg, flat, grads, fm, fv, fe)
        eng.train_commit(flat)

    eng.train_commit(flat)
    run_mode("full_master", full_step, flat, (fm, fv, fe))
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkout", default=None, help="root of a built checkout to measure in place of this one (the parent commit's: legs off only)")
    ap.add_argument("--digest", action="store_true", help="only the off-by-default digests")
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-steps", action="store_true", help="the optimiser call alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _use_checkout(args.checkout or ROOT)
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_bench.py measures on the GPU: no HIP device visible")
    res = {"digests": default_path_digests()} if args.digest else bench(args)
    res["checkout"] = "other" if args.checkout else "this"
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
