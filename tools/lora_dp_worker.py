"""One rank of a data-parallel LoRA training step (fv_train_lora_*; vla_fastvlm/training/unfrozen.py) -- the worker tests/test_gpu_lora.py starts once alone and
twice as two gloo ranks on one GPU (under RCCL on a multi-GPU node: torchrun --nproc-per-node N tools/lora_dp_worker.py --out DIR).  Every rank builds the same
`small` policy in LoRA mode with the same non-zero adapters, takes its slice of ONE fixed batch, runs FastVLAPolicy.fused_train_step -- forward/backward,
projection onto the adapters (--direct: adapter gradients straight from the backward instead), ONE all-reduce of the trainable buffer, clip + AdamW, adapted
commit -- and writes its reduced gradient and updated buffers to --out.  --dora / --rslora: the adapters' variants (with lora_B != 0 the magnitudes, which
start as the row norms of W0, differ from the norms of W0 + s B A: every magnitude has a gradient)."""
import argparse
import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "vla-from-fastvlm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def fixed_batch(B, dev):
    g = torch.Generator().manual_seed(6)
    return {"images": torch.rand(B, 3, 96, 128, generator=g).to(dev), "states": torch.randn(B, 14, generator=g).to(dev),
            "actions": torch.randn(B, 14, generator=g).to(dev), "tasks": ["pick up the red cube", "open the drawer", "push", "stack the blocks"][:B]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--backend", default="gloo")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rank-dim", type=int, default=8)
    ap.add_argument("--direct", action="store_true", help="the direct LoRA backward (fv_train_lora_forward_backward): no full-size gradient buffer, no projection")
    ap.add_argument("--dora", action="store_true", help="weight-decomposed LoRA: a trained magnitude per output row (projected backward only)")
    ap.add_argument("--rslora", action="store_true", help="rank-stabilised scaling: s = alpha / sqrt(rank)")
    args = ap.parse_args()
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(args.backend, rank=rank, world_size=world)
    from fastvla_hip import lora
    from vla_fastvlm.fastvla import FastVLAConfig, FastVLAPolicy
    torch.manual_seed(5)
    pol = FastVLAPolicy(FastVLAConfig(vlm_model_name="synthetic:small:41", hidden_dim=64, fusion_dim=64, dropout=0.0, freeze_backbone=False)).to(dev)
    pol.train()
    st = pol.enable_backbone_training(lora_rank=args.rank_dim, lora_direct=args.direct, **({"lora_dora": True} if args.dora else {}),
                                      **({"lora_rslora": True} if args.rslora else {}))
    assert (st.g is None) == bool(args.direct)
    # lora_B != 0, the same on every rank: with PEFT's B = 0 start every dA would be exactly zero
    g = torch.Generator().manual_seed(17)
    for name, v in lora.adapter_views(st.lflat, st.lora_tensors).items():
        if name.endswith(".lora_B.weight"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.05).to(dev))
    st.commit()
    master0 = st.flat.clone()
    batch = fixed_batch(args.batch, dev)
    per = args.batch // world
    mine = {k: v[rank * per:(rank + 1) * per] for k, v in batch.items()}
    out = pol.fused_train_step(mine, lr=1e-3, weight_decay=0.0)
    torch.cuda.synchronize()
    front = st.front
    torch.save({"grads": st.lg.cpu() / world / st.eng.train_loss_scale(), "lflat": st.lflat.cpu(), "loss": float(out["loss"]), "grad_norm": float(out["grad_norm"]),
                "payload": st.whole.last_numel, "trainable": int(st.lflat.numel()), "full": int(st.flat.numel()), "moments": int(st.m.numel()),
                "master_unchanged": bool(torch.equal(st.flat[front:], master0[front:])), "bucketed": list(st.bucketed.launched), "world": world},
               Path(args.out) / f"rank{rank}.pt")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    pol.model.backbone.engine().close()


if __name__ == "__main__":
    main()
