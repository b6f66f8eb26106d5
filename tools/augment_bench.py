"""The letterbox against the augmented letterbox, same process, same inputs, alternating windows:
    python tools/augment_bench.py [--model fastvlm-0.5b] [--batch 32] [--side 336] [--reps 20] [--rounds 3] [--out FILE.json]
plain      = fv_preprocess                                             (B x 3 x side x side -> B x S x S x 4 bf16)
augmented  = fv_augment_draw + fv_preprocess_augmented                 (the preset `default`: 90 % crop, brightness / contrast / saturation 0.8 .. 1.2)
draw       = fv_augment_draw alone                                     (one block per image; the contrast range makes it read every pixel for the gray mean)
and, to say where a difference lies, fv_preprocess_augmented alone over three fixed tables: identity rows (the table read and the window arithmetic, colour
skipped), the drawn windows with colour skipped, the drawn table in full.  u8 and f32 sources.  Both letterbox forms write the same B x S x S x 8 bytes; GB/s
counts those plus the source once.  Times: host clock around windows of --reps calls that end in a device synchronise; the median of --rounds rounds with
its spread (max - min).  The engine carries no weights: the calls read nothing but image_size from the handle.  Written to profiles/augment_bench.json unless
--out names another file."""
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
from fastvla_hip import FastVLAEngine, arch, augment  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="fastvlm-0.5b")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--side", type=int, default=336)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/augment_bench.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda", 0)
    model = arch.preset(args.model)
    B, S = args.batch, model.tower.image_size
    eng = FastVLAEngine(model, max_batch=B, max_text_tokens=8)
    opts = augment.preset("default")
    g = torch.Generator().manual_seed(1)
    f32 = torch.rand(B, 3, args.side, args.side, generator=g).to(dev)
    sources = {"u8": (f32 * 255).to(torch.uint8), "f32": f32}
    n = {"offset": 0}

    def window(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / args.reps

    def draw(img):
        n["offset"] += 1
        return eng.augment_draw(opts, img, seed=7, offset=n["offset"])

    res = {"model": args.model, "batch": B, "source": [3, args.side, args.side], "image_size": S, "options": augment.record(opts), "reps_per_window": args.reps,
           "out_mb": round(B * S * S * 8 / 1e6, 1), "dtypes": {}}
    for name, img in sources.items():
        ident = torch.zeros(B, augment.SAMPLE_FLOATS, device=dev)
        ident[:, 2], ident[:, 3], ident[:, 4], ident[:, 8], ident[:, 12] = args.side, args.side, 1.0, 1.0, 1.0
        full = eng.augment_draw(opts, img, seed=7, offset=0)
        crop = full.clone()
        crop[:, 4:16] = ident[:, 4:16]
        crop[:, 16] = 0.0                                       # (the int32 flag 0 and the float 0.0 share their bits)
        assert torch.equal(eng.preprocess_augmented(img, ident), eng.preprocess(img))
        cases = {"plain": lambda: eng.preprocess(img), "augmented": lambda: eng.preprocess_augmented(img, draw(img)), "draw": lambda: draw(img),
                 "store_identity_rows": lambda: eng.preprocess_augmented(img, ident), "store_crop_only": lambda: eng.preprocess_augmented(img, crop),
                 "store_crop_and_colour": lambda: eng.preprocess_augmented(img, full)}
        rounds = []
        for _ in range(args.rounds):       # alternating windows: other work shares the machine
            rounds.append({k + "_ms": round(window(fn), 4) for k, fn in cases.items()})
        med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
        d = {"rounds": rounds}
        nbytes = B * S * S * 8 + img.numel() * img.element_size()
        for k in cases:
            xs = [r[k + "_ms"] for r in rounds]
            d[k + "_ms"], d[k + "_spread_ms"] = med(xs), round(max(xs) - min(xs), 4)
            if k != "draw":
                d[k + "_gb_s"] = round(nbytes / med(xs) / 1e6, 1)
        d["augmented_over_plain"] = round(d["augmented_ms"] / d["plain_ms"], 4)
        d["augmented_over_plain_rounds"] = [round(r["augmented_ms"] / r["plain_ms"], 4) for r in rounds]
        res["dtypes"][name] = d
    print(json.dumps(res))
    out = Path(args.out) if args.out else ROOT / "profiles" / "augment_bench.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
