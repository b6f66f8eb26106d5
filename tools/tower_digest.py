"""The bits the FastViT-HD tower's forward puts out at inference and in training, as one sha256 per leg, and the profiler's cost model as plain
numbers -- for comparing two builds of the library:
    python tools/tower_digest.py [--parent-checkout DIR] [--timeout 900] [--out FILE.json]
Every checkout (this one, then --parent-checkout: the root of a BUILT checkout of the parent commit) runs in a fresh process of its own, one after the
other, each under --timeout seconds; the first failure stops the tool.  The inputs are seeded here; the package and the library are the checkout's own.
Configurations:
  tiny B=1, tiny B=3 mb=2   preset `tiny` (256^2): sides 64 and 32 take the depthwise pair march, side 16 two depthwise launches; two attention
                            stages; tower_microbatch = 2 leaves a ragged last micro-batch
  small B=2                 preset `small` (384^2)
  full B=1, 2, 4            the `fastvlm-0.5b` tower (1024^2): the 32x32x16 ConvFFN cut into ranges at few row tiles and in one launch above them, the
                            fused stems, the STASH instances in training
Every tower stands under the 2-layer 256-wide decoder of tests/test_gpu_train_tower.py (the training entry points need its head_dim of 64).
Legs of a configuration (each digest runs over the raw bytes of the outputs named, in that order):
  forward / taps / unit_taps / images   vision_forward (tokens, tower_out), every vision_forward_taps and vision_forward_unit_taps tap, and
                            vision_forward_images from a u8 source (an error text where the library refuses the model) -- then all four again under
                            set_batch_invariant(True)
  train_forward             train_tower_forward's tower_out and every train_tower_unit_outputs tensor
  train_backward            the tower slice of flat_grads after one train_tower_backward on a seeded d_tower_out (the stash the backward reads)
  train_unit <n>            (tiny only) train_tower_unit of every unit, teacher-forced with the inference walk's taps: y, g_in, the tower slice
Numbers of a configuration: workspace_bytes, fv_train_tower_workspace_bytes, and from fv_profile one vision_forward and one train_tower_forward: per
family launches / flops / bytes and the GEMM list's (m, n, k, epi, launches).  Times are not compared.
`identical` says whether every leg and every number of the two builds agrees; written to profiles/tower_digest.json unless --out names another file."""
import argparse
import hashlib
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
VT = "model.vision_tower.vision_tower.model."
SEED = 4321


def worker(checkout: Path) -> dict:
    for p in (str(checkout), str(checkout / "vla-from-fastvlm_amd")):
        sys.path.insert(0, p)
    import torch
    import fastvla_hip
    from fastvla_hip import FastVLAEngine, arch, weights
    dev = torch.device("cuda", 0)
    legs, numbers = {}, {}

    def digest(*outs):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for o in outs:
            h.update(o.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
        return h.hexdigest()

    def profiled(eng, fn):
        eng.profile(True)
        fn()
        fams, gemms = eng.profile_read()
        eng.profile(False)
        return {"families": {k: [v["launches"], v["flops"], v["bytes"]] for k, v in fams.items() if v["launches"]},
                "gemms": [[g["m"], g["n"], g["k"], g["epi"], g["launches"]] for g in gemms]}

    def configuration(label, model, w, B, microbatch=0, every_unit=False):
        print(f"[{checkout.name}] {label}", file=sys.stderr, flush=True)
        eng = FastVLAEngine(model, state_dim=14, action_dim=14, hidden_dim=64, fusion_dim=64, max_batch=B, max_text_tokens=16, tower_microbatch=microbatch,
                            llm_precision=1)
        eng.load_weights(w)
        S = model.tower.image_size
        g = torch.Generator().manual_seed(SEED + B)
        src = torch.randint(0, 256, (B, 3, S // 2 + 7, S // 2 + 40), dtype=torch.uint8, generator=g).to(dev)
        pix = eng.preprocess(src)
        taps = None
        for inv in (False, True):
            eng.set_batch_invariant(inv)
            tag = f"{label} batch_invariant " if inv else f"{label} "
            legs[tag + "forward"] = digest(*eng.vision_forward(pix, return_tower_out=True))
            tok, tout, t = eng.vision_forward_taps(pix)
            legs[tag + "taps"] = digest(tok, tout, *t)
            tok, tout, t = eng.vision_forward_unit_taps(pix)
            legs[tag + "unit_taps"] = digest(tok, tout, *t)
            taps = taps or t
            try:
                legs[tag + "images"] = digest(*eng.vision_forward_images(src, return_tower_out=True))
            except RuntimeError as e:      # (the library refuses a model without the fused stem: the refusal is the record)
                legs[tag + "images"] = f"refused: {e}"
        eng.set_batch_invariant(False)
        num = {"workspace_bytes": eng.workspace_bytes(B, 16, False), "vision_forward": profiled(eng, lambda: eng.vision_forward(pix))}
        eng.train_begin()
        eng.train_tower_begin()
        tensors, total, _ = eng.train_layout()
        first = min(t["offset"] for t in tensors if t["name"].startswith(VT))
        tws = eng.train_tower_workspace(B)
        num["train_tower_workspace_bytes"] = tws.numel() - 256
        tower_out = eng.train_tower_forward(pix, tws)
        legs[f"{label} train_forward"] = digest(tower_out, *eng.train_tower_unit_outputs(B, tws))
        grads = torch.zeros(total, dtype=torch.float32, device=dev)
        dto = (torch.randn(tuple(tower_out.shape), generator=g) * 4.0).to(device=dev, dtype=torch.float16)
        eng.train_tower_backward(pix, dto, tws, grads)
        legs[f"{label} train_backward"] = digest(grads[first:])
        num["train_tower_forward"] = profiled(eng, lambda: eng.train_tower_forward(pix, tws))
        if every_unit:
            units = eng.tower_units()
            shapes = [(B, sd, sd, ch) for _, _, sd, ch in units] + [tuple(tower_out.shape)]
            for n, shape in enumerate(shapes):
                grads.zero_()
                y, g_in = eng.train_tower_unit(n, pix if n == 0 else taps[n - 1], torch.randn(shape, generator=g) * 1e-2, tws, grads, 1024.0)
                legs[f"{label} train_unit {n}"] = digest(y, *([] if g_in is None else [g_in]), grads[first:])
        numbers[label] = num
        eng.close()

    llm = arch.LLMConfig(hidden=256, layers=2, heads=4, kv_heads=2, head_dim=64, inter=640, vocab=1024)   # (training needs head_dim 64: `tiny`'s own has 32)
    tiny, small, full = (arch.ModelConfig("tower-" + n, llm, arch.preset(n).tower) for n in ("tiny", "small", "fastvlm-0.5b"))
    w = weights.init_backbone(tiny, seed=51)
    configuration("tiny B=1", tiny, w, 1, every_unit=True)
    configuration("tiny B=3 mb=2", tiny, w, 3, microbatch=2, every_unit=True)
    configuration("small B=2", small, weights.init_backbone(small, seed=51), 2)
    w = weights.init_backbone(full, seed=51)
    for B in (1, 2, 4):
        configuration(f"full B={B}", full, w, B)
    return {"library": str(Path(fastvla_hip.library_path()).resolve().relative_to(checkout.resolve())), "legs": legs, "numbers": numbers}


def run(checkout: Path, timeout: int) -> dict:
    out = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--worker", str(checkout)], check=True, stdout=subprocess.PIPE, text=True, timeout=timeout)
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-checkout", default=None, help="root of a built checkout of the parent commit")
    ap.add_argument("--timeout", type=int, default=900, help="seconds each checkout's process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(worker(Path(args.worker).resolve())))
        return
    res = {"this_build": run(ROOT, args.timeout)}
    if args.parent_checkout:
        res["parent_build"] = run(Path(args.parent_checkout).resolve(), args.timeout)
        a, b = res["this_build"], res["parent_build"]
        res["differing_legs"] = sorted(k for k in set(a["legs"]) | set(b["legs"]) if a["legs"].get(k) != b["legs"].get(k))
        res["differing_numbers"] = sorted(f"{c}: {k}" for c in set(a["numbers"]) | set(b["numbers"])
                                          for k in set(a["numbers"].get(c, {})) | set(b["numbers"].get(c, {}))
                                          if a["numbers"].get(c, {}).get(k) != b["numbers"].get(c, {}).get(k))
        res["identical"] = not res["differing_legs"] and not res["differing_numbers"]
    out = Path(args.out) if args.out else ROOT / "profiles" / "tower_digest.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k.startswith("differing") or k == "identical"}))
    if args.parent_checkout and not res["identical"]:
        raise SystemExit(f"{len(res['differing_legs'])} legs and {len(res['differing_numbers'])} numbers differ between the two builds")


if __name__ == "__main__":
    main()
