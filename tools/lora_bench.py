"""Full fine-tuning step against the two LoRA steps (projected, direct) of the unfrozen decoder, same process, same inputs, alternating windows -- and the LoRA kernels alone:
    python tools/lora_bench.py [--model fastvlm-0.5b] [--batch 32] [--tokens 64] [--rank 16] [--steps 6] [--rounds 3] [--out FILE.json]
full step = fv_train_forward_backward + fv_adamw_clip_step over the whole master + fv_train_commit               (tools/train_unfrozen_bench.py --no-tower)
LoRA step = fv_train_forward_backward + fv_train_lora_project + fv_adamw_clip_step over the trainable buffer + fv_train_lora_commit
direct    = fv_train_lora_forward_backward (dA, dB straight from activations and output gradients; no full gradient buffer) + the same AdamW + commit
The frozen tower runs once, outside the windows (it is the same work in both modes).  Times: host clock around windows that end in a device synchronise;
kernels alone: device events around repeated launches.  GB/s = the bytes the algorithm needs (computed from the shapes below) over that time.
Memory: the torch allocator's peak while a mode's buffers are the only ones alive (the library's own allocations -- weights, operand copies -- are the same
in both modes and not in that figure).
--rslora: every LoRA mode runs with s = alpha / sqrt(rank).  --dora: a DoRA step (fv_train_lora_begin_ex FV_LORA_DORA: the projected LoRA step with the row-norm
pass in its commit and the magnitude gradient in its projection) joins the alternating windows, on a second engine over the same weights (a handle holds one
adapter mode), and its projection / commit / row-norm times join kernels_ms; every other figure is measured as without it.
--groups: ONLY the optimiser step, single-group (fv_adamw_clip_step) against grouped (fv_adamw_clip_step_groups), in alternating windows of the same process over
two buffers -- the full master under a full fine-tuning table (decoder x 0.1, layer decay 0.9, no decay on vectors) and the rank-r trainable buffer under a LoRA+
table (lora_B x 16, no decay on vectors: hundreds of groups) -- written to profiles/optim_groups_bench.json unless --out names another file."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "vla-from-fastvlm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from fastvla_hip import FastVLAEngine, _lib, arch, lora, optim, weights  # noqa: E402


def groups_bench(args, eng, dev):
    """single-group against grouped optimiser step over the full master and over the LoRA trainable buffer; host clock around windows that end in a device
    synchronise, the four (buffer, entry) windows alternating within a round.  GB/s counts 32 bytes per element for both entries: the norm pass reads the
    gradient (4), the update reads p, g, m, v and writes p, m, v (28).  Every call passes step = 1 while m and v move on: the bias corrections are host-side
    scalars, so the kernels' work does not depend on the step number."""
    tensors, total, _ = eng.train_layout()
    lt, ltotal = eng.train_lora_layout()
    hp = dict(lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, grad_scale=1.0 / eng.train_loss_scale())
    cases = {"full_master": (tensors, total, dict(lr_scales={"decoder": 0.1}, layer_decay=0.9, no_decay=("vectors",))),
             f"lora_rank{args.rank}_trainable": (lt, ltotal, dict(lora_plus_ratio=16, no_decay=("vectors",)))}
    bufs, res = {}, {"model": args.model, "rank": args.rank, "reps_per_window": args.kernel_reps, "bytes_per_element": 32, "buffers": {}}
    for name, (layout, n, opts) in cases.items():
        groups, _ = optim.build_param_groups(layout, weight_decay=hp["weight_decay"], total=n, **opts)
        table = eng.adamw_groups(groups, n)
        p = torch.empty(n, device=dev).normal_(0, 0.02)
        gr = torch.empty(n, device=dev).normal_(0, 1.0)
        bufs[name] = (p, gr, torch.zeros_like(p), torch.zeros_like(p), table, torch.zeros(len(groups), device=dev))
        segs = sum((x["end"] - x["begin"] + _lib.FV_ADAMW_SEGMENT - 1) // _lib.FV_ADAMW_SEGMENT for x in groups)
        res["buffers"][name] = {"numel": n, "groups": len(groups), "segments": segs, "options": optim.normalize_options(**opts), "rounds": []}
    norm = torch.zeros(1, device=dev)

    def window(fn, k):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    for _ in range(args.rounds):
        for name, (p, gr, m, v, table, gn) in bufs.items():
            k = args.kernel_reps if p.numel() < (1 << 26) else max(3, args.kernel_reps // 2)
            plain = window(lambda: eng.adamw_step(p, gr, m, v, 1, grad_norm_out=norm, **hp), k)
            grouped = window(lambda: eng.adamw_step(p, gr, m, v, 1, grad_norm_out=norm, groups=table, group_norms_out=gn, **hp), k)
            res["buffers"][name]["rounds"].append({"single_ms": round(plain, 4), "grouped_ms": round(grouped, 4)})
    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
    for name, b in res["buffers"].items():
        for key in ("single", "grouped"):
            xs = [r[key + "_ms"] for r in b["rounds"]]
            b[key + "_ms"] = med(xs)
            b[key + "_spread_ms"] = round(max(xs) - min(xs), 4)
            b[key + "_gb_s"] = round(32.0 * b["numel"] / b[key + "_ms"] / 1e6, 1)
    print(json.dumps(res))
    out = Path(args.out) if args.out else ROOT / "profiles" / "optim_groups_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    for b in bufs.values():
        b[4].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--targets", default="all")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--dora", action="store_true", help="also measure the DoRA step (a second engine in the same process)")
    ap.add_argument("--rslora", action="store_true", help="s = alpha / sqrt(rank) in every LoRA mode")
    ap.add_argument("--groups", action="store_true", help="only the optimiser step: single-group against grouped AdamW (profiles/optim_groups_bench.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lora_bench.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    model = arch.preset(args.model)
    B, T = args.batch, args.tokens
    eng = FastVLAEngine(model, max_batch=B, max_text_tokens=T, llm_precision=1)
    eng.load_weights(weights.init_backbone(model, seed=1234))
    eng.train_begin()
    eng.train_lora_begin(args.rank, None, args.targets, rslora=args.rslora)
    _, total, _ = eng.train_layout()
    lt, ltotal = eng.train_lora_layout()
    front = next(t["offset"] for t in lt if ".lora_" in t["name"])
    if args.groups:
        groups_bench(args, eng, dev)
        eng.close()
        return
    g = torch.Generator().manual_seed(1)
    images = torch.rand(B, 3, 336, 336, generator=g).to(dev)
    ids = torch.randint(0, 151643, (B, T), generator=g)
    lens = torch.full((B,), T)
    states, targets = torch.randn(B, 14, generator=g).to(dev), torch.randn(B, 14, generator=g).to(dev)
    _, tower_out = eng.vision_forward(eng.preprocess(images), return_tower_out=True)
    tower_out = tower_out.clone()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base_mem = torch.cuda.memory_allocated()

    flat = torch.zeros(total, device=dev)
    eng.train_export_params(flat)
    for k, v in eng.head_views(flat[: eng.head_numel()]).items():
        v.copy_(torch.randn(v.shape, generator=g) * 0.02 + (1.0 if k in ("state_projection.0.weight", "fusion.1.weight") else 0.0))
    master0 = flat.clone().cpu()
    ws = eng.train_workspace(B, T)
    lflat = torch.zeros(ltotal, device=dev)
    lflat[:front].copy_(flat[:front])
    lora.init_adapters(lflat, lt, seed=0)
    for name, v in lora.adapter_views(lflat, lt).items():      # B != 0: the projection and the commit do real work
        if name.endswith(".lora_B.weight"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.01).to(dev))
    lflat0 = lflat.clone()
    lg, lm, lv = torch.zeros_like(lflat), torch.zeros_like(lflat), torch.zeros_like(lflat)
    n = {"full": 0, "lora": 0, "direct": 0}
    hp = dict(lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, grad_scale=1.0 / eng.train_loss_scale())

    def direct_step():
        n["direct"] += 1
        loss = eng.train_lora_forward_backward(flat, lflat, tower_out, ids, lens, states, targets, ws, training=True, dropout_p=0.1, seed=7, offset=n["direct"],
                                               lora_grads=lg)[1]
        eng.adamw_step(lflat, lg, lm, lv, n["direct"], **hp)
        eng.train_lora_commit(flat, lflat)
        return loss

    def fb(off):
        return eng.train_forward_backward(flat, tower_out, ids, lens, states, targets, ws, training=True, dropout_p=0.1, seed=7, offset=off, flat_grads=grads)[1]

    def lora_step():
        n["lora"] += 1
        loss = fb(n["lora"])
        eng.train_lora_project(grads, lflat, lg)
        eng.adamw_step(lflat, lg, lm, lv, n["lora"], **hp)
        eng.train_lora_commit(flat, lflat)
        return loss

    def window(step, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            loss = step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k, float(loss)

    # ---- direct LoRA mode alone in memory (the full-size gradient buffer does not exist yet): its peak, then its warm-up
    window(direct_step, args.warmup)
    mem_direct = torch.cuda.max_memory_allocated() - base_mem
    # ---- projected LoRA mode: the full gradient buffer joins
    torch.cuda.reset_peak_memory_stats()
    grads = torch.zeros_like(flat)
    lflat.copy_(lflat0); lm.zero_(); lv.zero_(); eng.train_lora_commit(flat, lflat)
    window(lora_step, args.warmup)
    mem_lora = torch.cuda.max_memory_allocated() - base_mem
    # ---- full mode: Adam's moments over the whole master join
    torch.cuda.reset_peak_memory_stats()
    before_full = torch.cuda.memory_allocated()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)

    def full_step():
        n["full"] += 1
        loss = fb(n["full"])
        eng.adamw_step(flat, grads, m, v, n["full"], **hp)
        eng.train_commit(flat)
        return loss

    def to_full():       # the same starting point for every window of a mode
        flat.copy_(master0.to(dev)); eng.train_commit(flat)

    def to_lora():
        flat.copy_(master0.to(dev)); lflat.copy_(lflat0); eng.train_lora_commit(flat, lflat)

    to_full()
    window(full_step, args.warmup)
    mem_full = torch.cuda.max_memory_allocated() - base_mem - (lflat.numel() * 4 * 5)     # (the LoRA mode's five small buffers are alive too: taken out)
    # ---- DoRA (--dora): its own engine over the same weights, master and inputs; magnitudes start as the row norms of W0, so with lora_B != 0 they differ from
    # the norms of W0 + s B A and every kernel does its real work
    eng_d = None
    if args.dora:
        eng_d = FastVLAEngine(model, max_batch=B, max_text_tokens=T, llm_precision=1)
        eng_d.load_weights(weights.init_backbone(model, seed=1234))
        eng_d.train_begin()
        eng_d.train_lora_begin(args.rank, None, args.targets, dora=True, rslora=args.rslora)
        dt, dtotal = eng_d.train_lora_layout()
        dflat = torch.zeros(dtotal, device=dev)
        dflat[:front].copy_(flat[:front])
        dnamed = lora.adapter_views(dflat, dt)
        for name, view in lora.adapter_views(lflat0, lt).items():
            dnamed[name].copy_(view)
        zeroB = dflat.clone()
        for name, view in lora.adapter_views(zeroB, dt).items():
            if name.endswith(".lora_B.weight"):
                view.zero_()
        eng_d.train_lora_init_magnitude(flat, zeroB)
        for name, view in lora.adapter_views(zeroB, dt).items():
            if name.endswith(".lora_magnitude_vector.weight"):
                dnamed[name].copy_(view)
        del zeroB
        dflat0 = dflat.clone()
        dg, dm_, dv_ = torch.zeros_like(dflat), torch.zeros_like(dflat), torch.zeros_like(dflat)
        ws_d = eng_d.train_workspace(B, T)
        n["dora"] = 0

        def dora_step():
            n["dora"] += 1
            loss = eng_d.train_forward_backward(flat, tower_out, ids, lens, states, targets, ws_d, training=True, dropout_p=0.1, seed=7, offset=n["dora"], flat_grads=grads)[1]
            eng_d.train_lora_project(grads, dflat, dg)
            eng_d.adamw_step(dflat, dg, dm_, dv_, n["dora"], **hp)
            eng_d.train_lora_commit(flat, dflat)
            return loss

        def to_dora():
            flat.copy_(master0.to(dev)); dflat.copy_(dflat0); eng_d.train_lora_commit(flat, dflat)

        to_dora()
        window(dora_step, args.warmup)
    rounds = []
    for _ in range(args.rounds):       # alternating windows: other work shares the host
        to_full()
        f_ms, f_loss = window(full_step, args.steps)
        to_lora()
        l_ms, l_loss = window(lora_step, args.steps)
        to_lora()
        d_ms, d_loss = window(direct_step, args.steps)
        rounds.append({"full_ms": round(f_ms, 2), "lora_ms": round(l_ms, 2), "lora_direct_ms": round(d_ms, 2), "full_loss": f_loss, "lora_loss": l_loss,
                       "lora_direct_loss": d_loss})
        if eng_d is not None:
            to_dora()
            o_ms, o_loss = window(dora_step, args.steps)
            rounds[-1].update({"dora_ms": round(o_ms, 2), "dora_loss": o_loss})
    to_lora()

    # ---- the kernels alone
    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    fb(1)
    shp = lora.logical_shapes(model)
    names = lora.parse_targets(args.targets)
    L, r = model.llm.layers, args.rank
    adapted = L * sum(shp[t][0] * shp[t][1] for t in names)                   # elements of dW' / W0 under adapters
    adapters = sum(t["numel"] for t in lt if ".lora_" in t["name"])
    passes = (r + 31) // 32
    partial = L * sum(((shp[t][0] + 127) // 128) * r * shp[t][1] for t in names)      # dA partial sums: written once, read once
    proj_bytes = 4.0 * (adapted * passes + 2 * partial + 3 * adapters) + 8.0 * front
    mats = sum(t["numel"] for t in eng.train_layout()[0] if t["rows"] > 1 and t["bucket"] > 0)
    vecs = sum(t["numel"] for t in eng.train_layout()[0] if t["rows"] == 1 and t["bucket"] > 0)
    embed = model.llm.vocab * model.llm.hidden
    commit_bytes = 4.0 * mats + 2.0 * mats + 2.0 * (mats - embed - model.llm.hidden * model.tower.out_dim) + 8.0 * vecs   # fp32 in, bf16 rows out, one transposed copy out
    t_proj = timed(lambda: eng.train_lora_project(grads, lflat, lg), args.kernel_reps)
    t_lcommit = timed(lambda: eng.train_lora_commit(flat, lflat), args.kernel_reps)
    t_commit = timed(lambda: eng.train_commit(flat), args.kernel_reps)
    t_merge = timed(lambda: eng.train_lora_merge(grads, lflat), args.kernel_reps)     # (into the gradient buffer: a scratch target of the master's size)
    t_adam_full = timed(lambda: eng.adamw_step(flat, grads, m, v, 1, **hp), max(3, args.kernel_reps // 4))
    t_adam_lora = timed(lambda: eng.adamw_step(lflat, lg, lm, lv, 1, **hp), args.kernel_reps)
    # the direct backward's kernels alone (csrc/lora_direct_kernels.hip), through the test-only op library: the four packed tensors of ONE layer at this step's
    # row count, on random operands, times the layer count
    t_direct = None
    try:
        ops = _lib.load_testops()
        l_ = model.llm
        H, I, qd, kd = l_.hidden, l_.inter, l_.heads * l_.head_dim, l_.kv_heads * l_.head_dim
        R = B * (model.tower.num_tokens + T)
        tmask = lora.target_mask(args.targets)
        packs = [(1, tmask & 7, (qd, kd, kd), qd + 2 * kd, H, 2), (0, tmask >> 3 & 1, (H, 0, 0), H, qd, 2), (2, tmask >> 4 & 3, (I, I, 0), 2 * I, H, 2),
                 (0, tmask >> 6 & 1, (H, 0, 0), H, I, 3)]
        nfl = C.c_size_t()
        _lib.check(ops.fv_op_lora_direct_scratch_floats(R, r, max(2 * I, qd + 2 * kd, H), C.byref(nfl)), "fv_op_lora_direct_scratch_floats")
        scratch = torch.empty(nfl.value, device=dev)
        calls = []
        for kind, pm, outs, Np, K, xk in packs:
            if not pm:
                continue
            dY = (torch.randn(R, Np, device=dev) * 0.1).to(torch.float16)
            X = torch.randn(R, 2 * K if xk == 2 else K, device=dev).to(torch.bfloat16 if xk == 2 else torch.float16)
            ao, bo, off = [0, 0, 0], [0, 0, 0], 0
            for p_ in range(3):
                if outs[p_] and pm >> p_ & 1:
                    ao[p_] = off; off += r * K
                    bo[p_] = off; off += outs[p_] * r
            par, out = torch.randn(off, device=dev) * 0.01, torch.zeros(off, device=dev)
            calls.append((kind, pm, Np, K, (C.c_int64 * 3)(*ao), (C.c_int64 * 3)(*bo), dY, X, xk, 2 * K if xk == 2 else K, K if xk == 2 else 0, par, out))

        def direct_kernels():
            st_ = torch.cuda.current_stream().cuda_stream
            for kind, pm, Np, K, ao, bo, dY, X, xk, ldx, lo_off, par, out in calls:
                _lib.check(ops.fv_op_lora_direct(kind, pm, r, Np, K, qd, kd, ao, bo, dY.data_ptr(), X.data_ptr(), xk, ldx, lo_off, R, par.data_ptr(), out.data_ptr(), 1.0,
                                                 scratch.data_ptr(), scratch.numel(), st_), "fv_op_lora_direct")

        t_direct = L * timed(direct_kernels, max(3, args.kernel_reps // 4))
        del calls, scratch
    except (OSError, AttributeError) as exc:      # (the op library is test infrastructure: a tree without it still measures the steps)
        print(f"[lora_bench] direct kernels alone not measured: {exc}", file=sys.stderr)
    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
    res = {"model": args.model, "batch": B, "tokens": model.tower.num_tokens + T, "rank": r, "targets": list(names), "steps_per_window": args.steps, "rounds": rounds,
           "full_ms_per_step": med([x["full_ms"] for x in rounds]), "lora_ms_per_step": med([x["lora_ms"] for x in rounds]),
           "lora_direct_ms_per_step": med([x["lora_direct_ms"] for x in rounds]),
           "full_numel": total, "trainable_numel": ltotal, "adapter_numel": adapters, "exchange_mb": {"full": round(total * 4 / 1e6, 1), "lora": round(ltotal * 4 / 1e6, 1)},
           "torch_peak_gb": {"lora_direct": round(mem_direct / 1e9, 2), "lora": round(mem_lora / 1e9, 2), "full": round(mem_full / 1e9, 2)},
           "kernels_ms": {"lora_direct_all_layers": None if t_direct is None else round(t_direct, 3), "lora_project": round(t_proj, 3), "lora_commit": round(t_lcommit, 3), "commit": round(t_commit, 3), "lora_merge": round(t_merge, 3),
                          "adamw_full": round(t_adam_full, 3), "adamw_lora": round(t_adam_lora, 3)},
           "hbm_gb_s": {"lora_project": round(proj_bytes / t_proj / 1e6, 1), "lora_commit": round(commit_bytes / t_lcommit / 1e6, 1), "commit": round(commit_bytes / t_commit / 1e6, 1)},
           "bytes_gb": {"lora_project": round(proj_bytes / 1e9, 3), "commit": round(commit_bytes / 1e9, 3)}}
    if args.rslora:
        res["rslora"] = True
    if eng_d is not None:
        to_dora()
        eng_d.train_forward_backward(flat, tower_out, ids, lens, states, targets, ws_d, training=True, dropout_p=0.1, seed=7, offset=1, flat_grads=grads)
        t_dproj = timed(lambda: eng_d.train_lora_project(grads, dflat, dg), args.kernel_reps)
        t_dcommit = timed(lambda: eng_d.train_lora_commit(flat, dflat), args.kernel_reps)
        scratch_m = dflat.clone()
        t_norm = timed(lambda: eng_d.train_lora_init_magnitude(flat, scratch_m), args.kernel_reps)
        res["dora_ms_per_step"] = med([x["dora_ms"] for x in rounds])
        res["dora_trainable_numel"] = dtotal
        res["kernels_ms"].update({"dora_project": round(t_dproj, 3), "dora_commit": round(t_dcommit, 3), "dora_row_norms": round(t_norm, 3)})
        # DoRA's projection reads the adapted master rows once more (dm), its commit once more (the row-norm pass)
        res["hbm_gb_s"].update({"dora_project": round((proj_bytes + 4.0 * adapted) / t_dproj / 1e6, 1), "dora_commit": round((commit_bytes + 4.0 * adapted) / t_dcommit / 1e6, 1),
                                "dora_row_norms": round(4.0 * adapted / t_norm / 1e6, 1)})
        eng_d.close()
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
