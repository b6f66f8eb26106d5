"""sha256 of loss + flat gradients of fv_head_mse_backward (the plain MSE path) on a fixed seed, at three head widths:
    python tools/head_backward_digest.py [CHECKOUT]
CHECKOUT: the root of a built checkout whose fastvla_hip package and library are measured (default: this one).  Run once for this build and once for a
built checkout of the parent commit, on the same machine: equal digests say the default path kept its bits (DESIGN section 7 records them)."""
import hashlib
import sys
from pathlib import Path

import torch

root = sys.argv[1] if len(sys.argv) > 1 else str(Path(__file__).resolve().parent.parent)
sys.path.insert(0, root + "/vla-from-fastvlm_amd")
from fastvla_hip import FastVLAEngine, arch  # noqa: E402

DEV = "cuda:0"
for da, B in ((14, 8), (56, 8), (700, 64)):
    m = arch.ModelConfig("h", arch.LLMConfig(hidden=96, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                         arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
    eng = FastVLAEngine(m, state_dim=14, action_dim=da, hidden_dim=64, fusion_dim=80, max_batch=B)
    g = torch.Generator().manual_seed(1234)
    flat = (torch.randn(eng.head_numel(), generator=g) * 0.1).to(DEV)
    pooled, states, tgt = torch.randn(B, 96, generator=g).to(DEV), torch.randn(B, 14, generator=g).to(DEV), torch.randn(B, da, generator=g).to(DEV)
    act, saved = eng.head_forward(flat, pooled, states)
    loss, grads = eng.head_backward(flat, act, tgt, saved)
    torch.cuda.synchronize()
    h = hashlib.sha256(loss.cpu().numpy().tobytes() + grads.cpu().numpy().tobytes()).hexdigest()
    print(f"head_mse_backward da={da} B={B} sha256={h} loss={float(loss)!r}")
    eng.close()
