"""Host-side wrapper around one fv_handle: torch owns device memory and streams, the library does the arithmetic.

One engine per process / GPU (one process per GPU under torch.distributed).  Everything here is plumbing: allocate
buffers with torch's caching allocator, hand raw pointers and the current HIP stream to libfastvla_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from .arch import ModelConfig
from .select import check_flow_samples

HEAD_KEYS = (
    "state_projection.0.weight", "state_projection.0.bias", "state_projection.1.weight", "state_projection.1.bias",
    "fusion.0.weight", "fusion.0.bias", "fusion.1.weight", "fusion.1.bias", "fusion.4.weight", "fusion.4.bias",
    "action_head.weight", "action_head.bias",
)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _bucket_trampoline(bucket_cb):
    """-> (the C callback that hands a finished gradient bucket to bucket_cb(bucket, offset, numel), the dict its first exception is kept in under "exc": it
    must not unwind through the C frames, so the caller raises it once the library call has returned)"""
    err = {}

    def _cb(_user, bucket, off, numel):
        if bucket_cb is not None:
            try:
                bucket_cb(int(bucket), int(off), int(numel))
            except Exception as exc:
                err.setdefault("exc", exc)

    return _lib.BUCKET_CB(_cb), err


def _train_tensors(arr):
    """fv_train_tensor records -> the dicts train_layout() and train_lora_layout() hand out"""
    return [dict(name=t.name.decode(), offset=t.offset, numel=t.numel, rows=t.rows, cols=t.cols, bucket=t.bucket, packing=t.packing) for t in arr]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class AdamWGroups:
    """Owner of one fv_adamw_groups table (FastVLAEngine.adamw_groups).  ONE step may be in flight per table: it holds the step's partial sums."""

    def __init__(self, engine: "FastVLAEngine", groups, n: int):
        arr = (_lib.AdamWGroup * max(1, len(groups)))()
        for i, g in enumerate(groups):
            if isinstance(g, dict):
                g = (g["begin"], g["end"], g.get("lr_scale", 1.0), g.get("weight_decay", 0.0), g.get("frozen", False))
            arr[i] = _lib.AdamWGroup(int(g[0]), int(g[1]), float(g[2]), float(g[3]), int(bool(g[4])), 0)
        self._engine, self.n, self.n_groups = engine, int(n), len(groups)
        out = C.c_void_p()
        with torch.cuda.device(engine.device):
            _lib.check(engine.lib.fv_adamw_groups_create(engine.h, arr, len(groups), int(n), C.byref(out)), "fv_adamw_groups_create", engine.h)
        self._h = out.value

    def handle(self) -> int:
        if not self._h:
            raise _lib.FastVLAHipError("this parameter-group table has been closed")
        return self._h

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self._engine, "h", None):      # (after the engine's fv_destroy only the host record is left: dropped with this object)
            _lib.check(self._engine.lib.fv_adamw_groups_destroy(self._engine.h, h), "fv_adamw_groups_destroy", self._engine.h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check_head_loss(kind, beta, chunk, action_dim: Optional[int] = None):
    """-> (kind, beta, chunk) validated; ValueError for an unknown loss name, a beta that is not a positive finite number, chunk < 1 or a chunk that does
    not divide the head's output width."""
    import math
    if kind not in _lib.LOSS_KINDS:
        raise ValueError(f"unknown action loss '{kind}': one of {sorted(_lib.LOSS_KINDS)}")
    beta = float(beta)
    if not (beta > 0.0 and math.isfinite(beta)):
        raise ValueError(f"action loss beta must be a positive finite number, got {beta}")
    if int(chunk) != chunk or int(chunk) < 1:
        raise ValueError(f"chunk size must be an integer >= 1, got {chunk}")
    if action_dim is not None and action_dim % int(chunk):
        raise ValueError(f"chunk size {chunk} does not divide the head's output width {action_dim}")
    return str(kind), beta, int(chunk)


def check_loss_weights(dim_w, step_w, A: int, K: int) -> Optional[dict]:
    """-> {"dim": [A floats] or None, "step": [K floats] or None}, or None when both are None; ValueError for a wrong length or a negative / non-finite value"""
    import math

    def vec(v, n, name):
        if v is None:
            return None
        v = [float(x) for x in (v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else list(v))]
        if len(v) != n:
            raise ValueError(f"{name} must have {n} values, got {len(v)}")
        bad = [x for x in v if not (math.isfinite(x) and x >= 0.0)]
        if bad:
            raise ValueError(f"{name} must be finite and >= 0, got {bad[0]}")
        return v

    w = {"dim": vec(dim_w, A, "action_dim_weights"), "step": vec(step_w, K, "action_step_weights")}
    return None if w["dim"] is None and w["step"] is None else w


def check_head_bins(bins, range, sigma=0.0, decode="argmax", action_dim: Optional[int] = None, chunk: int = 1) -> dict:
    """-> {"bins", "range": [[lo, hi], ...] (one pair, or one per action dimension), "sigma", "decode"} validated as fv_head_set_bins validates them; ValueError
    for bins outside 2 .. 1024, a range that is not (lo, hi) or a list of such pairs with finite lo < hi, a negative or non-finite sigma, an unknown decode
    name and -- with action_dim = A and chunk = K given -- a list whose length is neither 1 nor A, or K * A * bins above the head's widest output."""
    import math
    if isinstance(bins, bool) or not isinstance(bins, int) and not (isinstance(bins, float) and bins == int(bins)) or not 2 <= int(bins) <= _lib.HEAD_BINS_MAX:
        raise ValueError(f"action_bins must be an integer 2 .. {_lib.HEAD_BINS_MAX}, got action_bins={bins!r} (action_head='bins')")
    bins = int(bins)
    try:
        pairs = [list(range)] if len(range) == 2 and not hasattr(range[0], "__len__") else [list(p) for p in range]
        pairs = [[float(lo), float(hi)] for lo, hi in pairs]
    except (TypeError, ValueError):
        raise ValueError(f"action_bins_range must be (lo, hi) or one such pair per action dimension, got action_bins_range={range!r}") from None
    for lo, hi in pairs:
        if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
            raise ValueError(f"action_bins_range needs finite lo < hi in every pair, got lo={lo!r}, hi={hi!r} (action_bins_range={range!r})")
    try:
        sigma = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"action_bins_sigma must be a finite number >= 0, got action_bins_sigma={sigma!r}") from None
    if not (math.isfinite(sigma) and sigma >= 0.0):
        raise ValueError(f"action_bins_sigma must be a finite number >= 0 (in units of the bin width), got action_bins_sigma={sigma!r} with action_bins={bins}")
    key = decode.strip().lower() if isinstance(decode, str) else decode
    if key not in _lib.BINS_DECODES:
        raise ValueError(f"action_bins_decode must be one of {list(_lib.BINS_DECODES)}, got action_bins_decode={decode!r} (action_head='bins')")
    if action_dim is not None:
        A, K = int(action_dim), int(chunk)
        if len(pairs) not in (1, A):
            raise ValueError(f"action_bins_range must hold one (lo, hi) pair or one per action dimension: got {len(pairs)} pairs with action_dim={A}")
        if K * A * bins > _lib.HEAD_BINS_MAX_WIDTH:
            raise ValueError(f"chunk_size * action_dim * action_bins must not exceed {_lib.HEAD_BINS_MAX_WIDTH} (the head's linear kernels take one output per "
                             f"block row). Got chunk_size={K}, action_dim={A}, action_bins={bins}.")
    return dict(bins=bins, range=pairs, sigma=sigma, decode=key)


def bins_ranges_from_stats(stats: dict, *, mode: str = "min_max", margin: float = 0.05, num_std: float = 3.0):
    """Dataset statistics of the action (LeRobot's {"min", "max", "mean", "std"}, A values each, un-normalised) -> A (lo, hi) pairs in the NORMALISED space the
    head works in ((a - mean) / std).  mode "min_max": the observed extremes, widened by `margin` of their span on either side; "std": +- num_std everywhere.
    A dimension that never moves (std or span 0) gets (-1, 1)."""
    if mode not in ("min_max", "std"):
        raise ValueError(f"mode must be 'min_max' or 'std', got {mode!r}")
    vec = lambda k: [float(x) for x in torch.as_tensor(stats[k], dtype=torch.float64).reshape(-1).tolist()]      # noqa: E731
    mean, std = vec("mean"), vec("std")
    if mode == "std":
        return [(-float(num_std), float(num_std)) for _ in mean]
    out = []
    for lo, hi, m, sd in zip(vec("min"), vec("max"), mean, std):
        if not sd > 0.0 or not hi > lo:
            out.append((-1.0, 1.0))
            continue
        nlo, nhi = (lo - m) / sd, (hi - m) / sd
        pad = float(margin) * (nhi - nlo)
        out.append((nlo - pad, nhi + pad))
    return out


FLOW_DRAWS_MAX = 16          # include/fastvla_hip.h FV_FLOW_DRAWS_MAX
FLOW_DRAW_SHIFT = 56         # draw s of a step at offset o draws at o + (s << 56): bits 56 .. 59 of a flow offset number the draws


def check_flow_draws(draws) -> int:
    """-> the number of noise draws per observation, validated: an integer 1 .. 16 (ValueError otherwise)"""
    if isinstance(draws, bool) or not isinstance(draws, int) and not (isinstance(draws, float) and draws == int(draws)):
        raise ValueError(f"flow_noise_draws must be an integer 1 .. {FLOW_DRAWS_MAX}, got {draws!r}")
    if not 1 <= int(draws) <= FLOW_DRAWS_MAX:
        raise ValueError(f"flow_noise_draws must be an integer 1 .. {FLOW_DRAWS_MAX}, got {draws!r}")
    return int(draws)


def check_flow_solver(name) -> str:
    """-> the solver's name in lower case; ValueError for anything but the keys of _lib.FLOW_SOLVERS"""
    key = name.strip().lower() if isinstance(name, str) else name
    if key not in _lib.FLOW_SOLVERS:
        raise ValueError(f"flow_solver must be one of {list(_lib.FLOW_SOLVERS)}, got {name!r}")
    return key


def check_flow_time(dist, a, b, t_lo, t_hi, stratify) -> dict:
    """-> set_head_flow_time's arguments, validated as fv_head_set_flow_time validates them (ValueError otherwise): dist a key of _lib.FLOW_TIME_SPEC_DISTS,
    finite a / b (a Beta's inside _lib.FLOW_BETA_RANGE), 0 <= t_lo < t_hi <= 1, stratify a bool"""
    import math
    key = dist.strip().lower() if isinstance(dist, str) else dist
    if key not in _lib.FLOW_TIME_SPEC_DISTS:
        raise ValueError(f"flow time dist must be one of {list(_lib.FLOW_TIME_SPEC_DISTS)}, got {dist!r}")
    a, b, t_lo, t_hi = float(a), float(b), float(t_lo), float(t_hi)
    if not all(math.isfinite(x) for x in (a, b, t_lo, t_hi)):
        raise ValueError(f"flow time a, b and range must be finite, got {(a, b, t_lo, t_hi)}")
    lo, hi = _lib.FLOW_BETA_RANGE
    if key == "beta" and not (lo <= a <= hi and lo <= b <= hi):
        raise ValueError(f"flow time Beta({a:g}, {b:g}): both parameters must lie in [{lo:g}, {hi:g}]")
    if not 0.0 <= t_lo < t_hi <= 1.0:
        raise ValueError(f"flow time range must be 0 <= lo < hi <= 1, got ({t_lo:g}, {t_hi:g})")
    if not isinstance(stratify, (bool, int)) or stratify not in (0, 1):
        raise ValueError(f"flow time stratify must be a bool, got {stratify!r}")
    return dict(dist=key, a=a, b=b, t_lo=t_lo, t_hi=t_hi, stratify=bool(stratify))


def flow_draw_offset(offset: int, s: int) -> int:
    """the Philox offset draw s of a step at `offset` draws at: a single-draw call at this offset gives draw s's rows.  ValueError when the step's offset
    already uses the draw bits or s is outside 0 .. 15."""
    if not 0 <= int(s) < FLOW_DRAWS_MAX:
        raise ValueError(f"draw index must be 0 .. {FLOW_DRAWS_MAX - 1}, got {s}")
    if (int(offset) >> FLOW_DRAW_SHIFT) & (FLOW_DRAWS_MAX - 1):
        raise ValueError(f"offset {int(offset):#x} has bits {FLOW_DRAW_SHIFT} .. {FLOW_DRAW_SHIFT + 3} set: they number the draws")
    return int(offset) + (int(s) << FLOW_DRAW_SHIFT)


class FastVLAEngine:
    def __init__(self, model: ModelConfig, *, state_dim: int = 14, action_dim: int = 14, hidden_dim: int = 1024,
                 fusion_dim: int = 1024, device: Optional[torch.device] = None, max_batch: int = 64,
                 max_text_tokens: int = 64, tower_microbatch: int = 0, llm_precision: int = 1):
        self.lib = _lib.load()  # raises if the HIP library is missing: no fallback
        if not torch.cuda.is_available():
            raise _lib.FastVLAHipError("no HIP device visible: the FastVLA HIP path needs an MI355X (no CPU fallback)")
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.type != "cuda":
            raise _lib.FastVLAHipError(f"FastVLAEngine needs a cuda (ROCm) device, got {self.device}")
        self.model = model
        self.head_dims = dict(feat=model.llm.hidden, ds=state_dim, da=action_dim, hid=hidden_dim, fus=fusion_dim)
        d = _lib.ModelDesc()
        l, t = model.llm, model.tower
        d.llm_hidden, d.llm_layers, d.llm_heads, d.llm_kv_heads = l.hidden, l.layers, l.heads, l.kv_heads
        d.llm_head_dim, d.llm_inter, d.llm_vocab = l.head_dim, l.inter, l.vocab
        d.rope_theta, d.rms_eps = l.rope_theta, l.rms_eps
        d.tower_stages = len(t.layers)
        for i in range(len(t.layers)):
            d.tower_layers[i], d.tower_dims[i], d.tower_is_attn[i] = t.layers[i], t.dims[i], int(i in t.attn_stages)
        d.tower_mlp_ratio, d.tower_head_dim, d.tower_se_rd, d.tower_out_dim = t.mlp_ratio, t.head_dim, t.se_rd, t.out_dim
        d.ln_eps, d.bn_eps, d.image_size = t.ln_eps, t.bn_eps, t.image_size
        d.state_dim, d.action_dim, d.hidden_dim, d.fusion_dim = state_dim, action_dim, hidden_dim, fusion_dim
        d.max_batch, d.max_text_tokens, d.tower_microbatch = max_batch, max_text_tokens, tower_microbatch
        d.llm_precision = int(llm_precision)
        self.llm_precision = int(llm_precision)
        self.desc = d
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fv_create(C.byref(d), self.device.index or 0, C.byref(h)), "fv_create")
        self.h = h
        self._ws: Optional[torch.Tensor] = None
        self._side: Optional[torch.cuda.Stream] = None
        # FASTVLA_FUSED_LETTERBOX=1: backbone() hands raw images to the stem (fv_vision_forward_images) instead of letterboxing first
        self.fused_letterbox = os.environ.get("FASTVLA_FUSED_LETTERBOX", "0") == "1" and model.tower.dims[0] == 96
        self.overlap_streams = os.environ.get("FASTVLA_OVERLAP", "1") == "1"
        # An image's tower tokens must not depend on the batch it is evaluated in once they are CONSUMED (splice mode: the small-batch kernel forms put 1.7e-2
        # between an observation alone and the same observation inside a batch).  FASTVLA_BATCH_INVARIANT=1 / 0 fixes the choice; unset, the numerics follow the
        # mode: tokens_consumed(True) -- the host side calls it whenever the tower output feeds the decoder -- switches the large-batch forms on, literal mode
        # (tokens computed and dropped) keeps the fast small-batch forms.
        env = os.environ.get("FASTVLA_BATCH_INVARIANT")
        self._invariant_policy: Optional[bool] = None if env in (None, "") else env == "1"
        self._invariant_on = False
        if self._invariant_policy:
            self.set_batch_invariant(True)
        # FASTVLA_PROMPT_REUSE=0: the literal call recomputes the decoder every time (fv_set_prompt_reuse; on by default in the library)
        if os.environ.get("FASTVLA_PROMPT_REUSE", "1") == "0":
            self.set_prompt_reuse(False)
        offs = (C.c_int64 * 13)()
        _lib.check(self.lib.fv_head_layout(self.h, C.byref(offs)), "fv_head_layout")
        self.head_offsets = list(offs)
        self.head_loss = dict(kind="mse", beta=1.0, chunk=1)      # set_head_loss
        self.head_loss_weights: Optional[dict] = None             # set_head_loss_weights: {"dim": A floats or None, "step": K floats or None}, None = off
        self._pad_keep: Optional[torch.Tensor] = None
        self.head_flow: Optional[dict] = None                     # set_head_flow: None = the regression head
        self.head_bins: Optional[dict] = None                     # set_head_bins: None = no binned head
        self.head_flow_guidance: Optional[dict] = None            # set_head_flow_guidance: None = the unguided sampler only
        self.head_flow_time = None                                # set_head_flow_time: the training time's distribution beyond set_head_flow's own (None: off)
        self.head_flow_draws = 1                                  # set_head_flow_draws: noise draws per observation in the training forms
        self.head_flow_prefix: Optional[dict] = None              # set_head_flow_prefix: None = no action-prefix conditioning
        self.head_flow_solver = "euler"                           # set_head_flow_solver: the integrator of all three samplers
        self.head_flow_samples: Optional[dict] = None             # set_head_flow_samples: None = one sample per observation
        self.head_flow_solver_rows = False                        # True once a higher-order solver was named: the workspace plan holds its two rows
        self.loaded = False

    def close(self):
        if getattr(self, "h", None):
            for t in list(getattr(self, "_group_tables", ())):      # parameter-group tables (and temporal ensemblers) go before the handle
                t.close()
            self.lib.fv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- frozen weights
    def load_weights(self, state: Dict[str, torch.Tensor]) -> None:
        keep, descs = [], (_lib.TensorDesc * len(state))()
        for i, (k, v) in enumerate(state.items()):
            t = v.detach().to("cpu")
            if t.dtype not in (torch.float32, torch.bfloat16):
                t = t.float()
            t = t.contiguous()
            keep.append(t)
            nm = k.encode()
            keep.append(nm)
            descs[i].name = nm
            descs[i].data = t.data_ptr()
            descs[i].dtype = _lib.FV_F32 if t.dtype == torch.float32 else _lib.FV_BF16
            descs[i].ndim = max(t.ndim, 1)
            if t.ndim > 4:
                raise ValueError(f"{k}: rank > 4")
            for j, s in enumerate(t.shape if t.ndim else (1,)):
                descs[i].shape[j] = s
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fv_load_weights(self.h, descs, len(state)), "fv_load_weights", self.h)
        self.loaded = True

    def load_weights_streaming(self, provider) -> None:
        """Pack the frozen weights pulling ONE tensor at a time: provider(name) -> torch.Tensor (f32 or bf16, on the CPU or on
        this engine's device) or None when the checkpoint has no such key.  Nothing but the tensor being packed is alive on
        the host side, and bf16 tensors are copied as they are (fv_load_weights_cb)."""
        keep = {}

        def cb(_user, name, out):
            try:
                t = provider(name.decode())
            except Exception as exc:  # an exception must not unwind through the C frames
                keep["exc"] = exc
                return 1
            if t is None:
                return 1
            t = t.detach()
            if t.dtype not in (torch.float32, torch.bfloat16):
                t = t.float()
            if t.device.type == "cuda" and t.device != self.device:
                t = t.to(self.device)
            t = t.contiguous()
            if t.ndim > 4:
                keep["exc"] = ValueError(f"{name.decode()}: rank > 4")
                return 1
            if t.device.type == "cuda":
                # the library copies with blocking calls on the null stream: whatever produced t on torch's current stream
                # (a generator, a dtype cast, a .to(device)) must have finished before the pointer is handed over
                torch.cuda.current_stream(t.device).synchronize()
            keep["t"] = t  # alive until the next call
            d = out.contents
            d.data = t.data_ptr()
            d.dtype = _lib.FV_F32 if t.dtype == torch.float32 else _lib.FV_BF16
            d.ndim = max(t.ndim, 1)
            for j, n in enumerate(t.shape if t.ndim else (1,)):
                d.shape[j] = n
            d.device = int(t.device.type == "cuda")
            return 0

        fn = _lib.TENSOR_PROVIDER(cb)
        with torch.cuda.device(self.device):
            torch.cuda.synchronize(self.device)
            rc = self.lib.fv_load_weights_cb(self.h, fn, None)
        if "exc" in keep:
            raise keep["exc"]
        _lib.check(rc, "fv_load_weights_cb", self.h)
        self.loaded = True

    # ---------------------------------------------------------------- workspace
    def workspace_bytes(self, B: int, T: int, splice: bool) -> int:
        n = C.c_size_t()
        _lib.check(self.lib.fv_workspace_bytes(self.h, B, T, int(splice), C.byref(n)), "fv_workspace_bytes")
        return n.value

    def ensure_workspace(self, B: int, T: int, splice: bool) -> None:
        need = self.workspace_bytes(B, T, splice)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.fv_bind_workspace(self.h, *self._aligned(self._ws)), "fv_bind_workspace")

    # ---------------------------------------------------------------- frozen backbone
    IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # reference model/fastvlm_adapter.py:468-469,475-476

    def preprocess(self, images: torch.Tensor, pad_value: float = 0.0, resize_with_padding: bool = True, normalize_imagenet: bool = False,
                   range_heuristic: bool = True) -> torch.Tensor:
        """letterbox (+ the reference's `_maybe_normalize_imagenet`, :463-477, when asked; range_heuristic = its torchvision branch, which is what an installed
        reference runs: torchvision is one of its dependencies)."""
        images, dt = self._augment_source(images)
        B, Cc, H, W = images.shape
        S = self.model.tower.image_size
        pix = torch.empty(B, S, S, 4, dtype=torch.bfloat16, device=self.device)
        if normalize_imagenet:
            import ctypes
            mean, std = (ctypes.c_float * 3)(*self.IMAGENET_MEAN), (ctypes.c_float * 3)(*self.IMAGENET_STD)
            _lib.check(self.lib.fv_preprocess_normalized(self.h, images.data_ptr(), dt, B, Cc, H, W, float(pad_value), int(resize_with_padding), mean, std,
                                                         int(range_heuristic), pix.data_ptr(), _stream()), "fv_preprocess_normalized")
            return pix
        _lib.check(self.lib.fv_preprocess(self.h, images.data_ptr(), dt, B, Cc, H, W, float(pad_value),
                                          int(resize_with_padding), pix.data_ptr(), _stream()), "fv_preprocess")
        return pix

    # ---------------------------------------------------------------- image augmentation (fastvla_hip/augment.py)
    def _augment_source(self, images: torch.Tensor):
        """-> (images on the device, contiguous, uint8 as it is and everything else fp32; the library's type code): what every entry point that reads source images takes"""
        if images.ndim != 4:
            raise ValueError(f"(B,C,H,W) expected, but got shape {tuple(images.shape)}")
        if images.dtype == torch.uint8:
            dt = _lib.FV_U8
        else:
            images = images.to(torch.float32)
            dt = _lib.FV_F32
        return images.to(self.device).contiguous(), dt

    def augment_draw(self, options: Dict, images: Optional[torch.Tensor] = None, *, shape: Optional[Tuple[int, int, int, int]] = None, seed: int = 0,
                     offset: int = 0, sample_base: int = 0) -> torch.Tensor:
        """Draw one fv_augment_sample per image on the device (fv_augment_draw; no host synchronisation) -> the table, a (B, 20) fp32 tensor whose column
        16 holds the int32 `colour` flag.  options: fastvla_hip.augment.normalize_options' dict.  images (B,C,H,W) f32 | u8, or -- when contrast is (1, 1),
        the only option that reads pixels -- shape=(B, C, H, W) alone.  Row b is a function of (seed, offset, sample_base + b) and the options."""
        from . import augment as _aug
        cfg = _aug.config_struct(options)
        ptr, dt = None, _lib.FV_F32
        if images is not None:
            images, dt = self._augment_source(images)
            shape, ptr = tuple(images.shape), images.data_ptr()
        if shape is None:
            raise ValueError("augment_draw needs the images or their shape")
        B, Cc, H, W = (int(v) for v in shape)
        table = torch.empty(max(B, 0), _aug.SAMPLE_FLOATS, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_augment_draw(self.h, C.byref(cfg), ptr, dt, B, Cc, H, W, int(seed), int(offset), int(sample_base), table.data_ptr(), _stream()),
                   "fv_augment_draw", self.h)
        return table

    def preprocess_augmented(self, images: torch.Tensor, table: torch.Tensor, pad_value: float = 0.0, resize_with_padding: bool = True,
                             value_max: Optional[float] = None) -> torch.Tensor:
        """preprocess() sampling through `table` (augment_draw's, or B hand-made 80-byte rows): crop window + colour map per image
        (fv_preprocess_augmented).  value_max: the clamp's upper end; default 255 for uint8 images, 1 otherwise."""
        from . import augment as _aug
        images, dt = self._augment_source(images)
        B, Cc, H, W = images.shape
        if table.device != self.device or table.dtype != torch.float32 or not table.is_contiguous() or tuple(table.shape) != (B, _aug.SAMPLE_FLOATS):
            raise ValueError(f"the table must be a contiguous ({B}, {_aug.SAMPLE_FLOATS}) fp32 tensor on {self.device}, got {tuple(table.shape)} {table.dtype} on {table.device}")
        if value_max is None:
            value_max = 255.0 if dt == _lib.FV_U8 else 1.0
        S = self.model.tower.image_size
        pix = torch.empty(B, S, S, 4, dtype=torch.bfloat16, device=self.device)
        _lib.check(self.lib.fv_preprocess_augmented(self.h, images.data_ptr(), dt, B, Cc, H, W, float(pad_value), int(resize_with_padding), table.data_ptr(),
                                                    float(value_max), pix.data_ptr(), _stream()), "fv_preprocess_augmented", self.h)
        return pix

    def vision_forward(self, pix: torch.Tensor, return_tower_out: bool = False):
        B = pix.shape[0]
        t, l = self.model.tower, self.model.llm
        self.ensure_workspace(B, 1, False)
        tok = torch.empty(B, t.num_tokens, l.hidden, dtype=torch.float32, device=self.device)
        tout = torch.empty(B, t.num_tokens, t.out_dim, dtype=torch.bfloat16, device=self.device) if return_tower_out else None
        _lib.check(self.lib.fv_vision_forward(self.h, pix.data_ptr(), B, tok.data_ptr(), _ptr(tout), _stream()),
                   "fv_vision_forward")
        return (tok, tout) if return_tower_out else tok

    def vision_forward_images(self, images: torch.Tensor, pad_value: float = 0.0, resize_with_padding: bool = True,
                              return_tower_out: bool = False):
        """preprocess() + vision_forward() as ONE call (fv_vision_forward_images): the stem samples the source images itself, the
        letterboxed 1024^2 frame never exists in HBM.  Same tokens, bit for bit."""
        images, dt = self._augment_source(images)
        B, Cc, H, W = images.shape
        t, l = self.model.tower, self.model.llm
        self.ensure_workspace(B, 1, False)
        tok = torch.empty(B, t.num_tokens, l.hidden, dtype=torch.float32, device=self.device)
        tout = torch.empty(B, t.num_tokens, t.out_dim, dtype=torch.bfloat16, device=self.device) if return_tower_out else None
        _lib.check(self.lib.fv_vision_forward_images(self.h, images.data_ptr(), dt, B, Cc, H, W, float(pad_value), int(resize_with_padding),
                                                     tok.data_ptr(), _ptr(tout), _stream()), "fv_vision_forward_images", self.h)
        return (tok, tout) if return_tower_out else tok

    def vision_forward_taps(self, pix: torch.Tensor):
        """-> (tokens f32, tower_out bf16, [stem, stage0, ...] NHWC bf16): per-stage activation maps for the parity tests."""
        B = pix.shape[0]
        t, l = self.model.tower, self.model.llm
        self.ensure_workspace(B, 1, False)
        tok = torch.empty(B, t.num_tokens, l.hidden, dtype=torch.float32, device=self.device)
        tout = torch.empty(B, t.num_tokens, t.out_dim, dtype=torch.bfloat16, device=self.device)
        side = t.image_size // 4
        taps = [torch.empty(B, side, side, t.dims[0], dtype=torch.bfloat16, device=self.device)]
        for i, c in enumerate(t.dims):
            taps.append(torch.empty(B, side >> i, side >> i, c, dtype=torch.bfloat16, device=self.device))
        arr = (C.c_void_p * len(taps))(*[x.data_ptr() for x in taps])
        _lib.check(self.lib.fv_vision_forward_taps(self.h, pix.data_ptr(), B, tok.data_ptr(), tout.data_ptr(), arr, len(taps),
                                                   _stream()), "fv_vision_forward_taps", self.h)
        return tok, tout, taps

    UNIT_KINDS = ("stem", "cpe", "block", "down")

    def tower_units(self):
        """-> [(kind, stage, side, channels)] of every tower unit in execution order (fv_vision_unit_info)."""
        out, u = [], 0
        k, st, sd, ch = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        while self.lib.fv_vision_unit_info(self.h, u, C.byref(k), C.byref(st), C.byref(sd), C.byref(ch)) == 0:
            out.append((self.UNIT_KINDS[k.value], st.value, sd.value, ch.value))
            u += 1
        return out

    def vision_forward_unit_taps(self, pix: torch.Tensor):
        """-> (tokens f32, tower_out bf16, [output of unit 0, 1, ...] NHWC bf16): unit u's input is taps[u - 1], so the parity
        test feeds each oracle unit the ENGINE's own input (teacher forcing)."""
        B = pix.shape[0]
        t, l = self.model.tower, self.model.llm
        self.ensure_workspace(B, 1, False)
        tok = torch.empty(B, t.num_tokens, l.hidden, dtype=torch.float32, device=self.device)
        tout = torch.empty(B, t.num_tokens, t.out_dim, dtype=torch.bfloat16, device=self.device)
        taps = [torch.empty(B, sd, sd, ch, dtype=torch.bfloat16, device=self.device) for _, _, sd, ch in self.tower_units()]
        arr = (C.c_void_p * len(taps))(*[x.data_ptr() for x in taps])
        _lib.check(self.lib.fv_vision_forward_unit_taps(self.h, pix.data_ptr(), B, tok.data_ptr(), tout.data_ptr(), arr, len(taps),
                                                        _stream()), "fv_vision_forward_unit_taps", self.h)
        return tok, tout, taps

    def llm_pooled(self, ids: torch.Tensor, lens: torch.Tensor, img_tokens: Optional[torch.Tensor] = None,
                   pool_mode: int = 0) -> torch.Tensor:
        B, T = ids.shape
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        lens = lens.to(device=self.device, dtype=torch.int32).contiguous()
        ni = 0 if img_tokens is None else img_tokens.shape[1]
        self.ensure_workspace(B, T, img_tokens is not None)
        pooled = torch.empty(B, self.model.llm.hidden, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_llm_forward_pooled(self.h, ids.data_ptr(), lens.data_ptr(), _ptr(img_tokens), ni, B, T,
                                                  pool_mode, pooled.data_ptr(), _stream()), "fv_llm_forward_pooled")
        return pooled

    def set_batch_invariant(self, on: bool = True) -> None:
        """fv_set_batch_invariant: the tower keeps the large-batch kernel forms at every batch size, so an image evaluated alone gets the tokens it
        gets inside a batch (bit for bit); costs ~0.9 ms per one-observation step.  FASTVLA_BATCH_INVARIANT=1 switches it on at creation."""
        _lib.check(self.lib.fv_set_batch_invariant(self.h, int(bool(on))), "fv_set_batch_invariant", self.h)
        self._invariant_on = bool(on)

    def set_prompt_reuse(self, on: bool = True) -> None:
        """fv_set_prompt_reuse: literal-mode calls keep the pooled rows of the last prompt on the device and return them while (ids, lens) stay the same."""
        _lib.check(self.lib.fv_set_prompt_reuse(self.h, int(bool(on))), "fv_set_prompt_reuse", self.h)

    def prompt_reuse_stats(self) -> Tuple[int, int]:
        """(literal calls that used the prompt slot, how many of them hit) since the engine was created.  Synchronises the device."""
        calls, hits = C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.fv_prompt_reuse_stats(self.h, C.byref(calls), C.byref(hits)), "fv_prompt_reuse_stats", self.h)
        return int(calls.value), int(hits.value)

    def tokens_consumed(self, consumed: bool) -> None:
        """The caller says whether the tower tokens of the calls that follow feed the decoder (splice mode) or are dropped (the literal reference): unless
        FASTVLA_BATCH_INVARIANT pins the choice, batch invariance of the tower follows that."""
        if self._invariant_policy is None and bool(consumed) != self._invariant_on:
            self.set_batch_invariant(bool(consumed))

    def fp16_saturations(self, reset: bool = False) -> int:
        """How many 8-value activation groups the fp16 single-pass projections (llm_precision >= 2) had to clamp to +-65504 since the
        last reset (fv_llm_fp16_saturations): 0 in a healthy model; non-zero means the fp16 budget does not hold for this checkpoint /
        input and the engine should be rebuilt with llm_precision=1.  Synchronises the device."""
        n = C.c_uint64()
        _lib.check(self.lib.fv_llm_fp16_saturations(self.h, C.byref(n), int(reset)), "fv_llm_fp16_saturations", self.h)
        return int(n.value)

    # ---------------------------------------------------------------- image-prefix reuse
    def llm_prefix(self, img_tokens: torch.Tensor) -> torch.Tensor:
        """(B, Ni, H) f32 image tokens -> the decoder's prefix cache: every layer's un-rotated [k | v] rows of the Ni image positions,
        (layers, B, Ni, 2 * kv_heads * head_dim) f32.  Rows of different images are independent: slices along B can be kept and
        re-assembled per frame."""
        B, Ni, _ = img_tokens.shape
        l = self.model.llm
        self.ensure_workspace(B, 1, True)
        kv = torch.empty(l.layers, B, Ni, 2 * l.kv_heads * l.head_dim, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_llm_prefix(self.h, img_tokens.contiguous().data_ptr(), Ni, B, kv.data_ptr(), _stream()), "fv_llm_prefix", self.h)
        return kv

    def llm_pooled_prefixed(self, ids: torch.Tensor, lens: torch.Tensor, kv: torch.Tensor) -> torch.Tensor:
        """The text positions alone against a prefix cache from llm_prefix(): the pooled rows of llm_pooled(ids, lens, img_tokens)."""
        B, T = ids.shape
        if kv.ndim != 4 or kv.shape[1] != B:
            raise ValueError(f"prefix cache must be (layers, B={B}, Ni, 2*kv_dim), got {tuple(kv.shape)}")
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        lens = lens.to(device=self.device, dtype=torch.int32).contiguous()
        self.ensure_workspace(B, T, True)
        pooled = torch.empty(B, self.model.llm.hidden, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_llm_forward_pooled_prefixed(self.h, ids.data_ptr(), lens.data_ptr(), kv.contiguous().data_ptr(), kv.shape[2], B, T, 0,
                                                           pooled.data_ptr(), _stream()), "fv_llm_forward_pooled_prefixed", self.h)
        return pooled

    def backbone(self, images: Optional[torch.Tensor], ids: torch.Tensor, lens: torch.Tensor, *, splice: bool = False,
                 run_tower: bool = True, pad_value: float = 0.0, resize_with_padding: bool = True,
                 pool_mode: int = 0, pix: Optional[torch.Tensor] = None) -> torch.Tensor:
        """letterbox -> tower -> projector -> decoder -> pooled (B,H).  splice=False is the literal reference
        behaviour: the image tokens are computed and not consumed.  `pix`: pixels already letterboxed by
        preprocess() ((B,S,S,4) bf16) -- then `images` is not read."""
        B, T = ids.shape
        self.ensure_workspace(B, T, splice)
        if splice or not run_tower or not self.overlap_streams:
            tok = None
            if run_tower or splice:
                if pix is None and self.fused_letterbox:
                    tok = self.vision_forward_images(images, pad_value, resize_with_padding)
                else:
                    if pix is None:
                        pix = self.preprocess(images, pad_value, resize_with_padding)
                    tok = self.vision_forward(pix)
            return self.llm_pooled(ids, lens, tok if splice else None, pool_mode)
        # literal mode: the decoder does not consume the tower's output, so the two run on separate HIP streams (their
        # workspace regions are disjoint); the small-grid decoder kernels fill the tower kernels' tails.
        cur = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            pooled = self.llm_pooled(ids, lens, None, pool_mode)
        if pix is None and self.fused_letterbox:
            self._tok_keepalive = self.vision_forward_images(images, pad_value, resize_with_padding)
        else:
            if pix is None:
                pix = self.preprocess(images, pad_value, resize_with_padding)
            self._tok_keepalive = self.vision_forward(pix)
        cur.wait_stream(self._side)
        pooled.record_stream(cur)
        return pooled

    # ---------------------------------------------------------------- hipGraph capture of the inference step
    def capture_policy_step(self, images: torch.Tensor, ids: torch.Tensor, lens: torch.Tensor, flat_params: torch.Tensor,
                            states: torch.Tensor, *, splice: bool = False, pool_mode: int = 0):
        """Capture letterbox -> tower -> projector -> decoder -> pool -> head as ONE hipGraph (every entry point of the library is
        asynchronous on the caller's stream, allocates nothing and never synchronises: include/fastvla_hip.h).  The given
        tensors become the graph's static inputs: copy new data INTO them (same shapes) and call replay().
        -> (replay, actions): `replay()` launches the graph on the current stream, `actions` (B, A) is its static output.
        At B = 1 the eager step is launch-bound (~350 launches); the graph replays it in one submission."""
        B, T = ids.shape
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        lens = lens.to(device=self.device, dtype=torch.int32).contiguous()
        images, states = images.to(self.device).contiguous(), states.to(self.device, torch.float32).contiguous()
        self.ensure_workspace(B, T, splice)
        saved = self.head_saved(B)

        def step():
            pooled = self.backbone(images, ids, lens, splice=splice, pool_mode=pool_mode)
            act, _ = self.head_forward(flat_params, pooled, states, saved=saved)
            return act

        side = torch.cuda.Stream(device=self.device)   # warm-up off the default stream: one-time attribute calls, workspace, side stream
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            actions = step()

        def replay(_keep=(saved, images, ids, lens, states, flat_params)):
            # the graph writes `saved` and reads the static inputs on every replay: they live as long as the replay handle does (handing out graph.replay
            # alone let `saved` return to the allocator, and a later tensor of the caller's -- a clone of `actions` -- was overwritten by the next replay)
            graph.replay()

        return replay, actions

    # ---------------------------------------------------------------- action expert
    def head_numel(self) -> int:
        return self.head_offsets[12]

    def head_views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """name -> view into the flat buffer (state-dict order, each tensor 16-byte aligned)."""
        hd = self.head_dims
        shapes = [(hd["ds"],), (hd["ds"],), (hd["hid"], hd["ds"]), (hd["hid"],), (hd["fus"], self.head_cat_width()),
                  (hd["fus"],), (hd["fus"],), (hd["fus"],), (hd["fus"], hd["fus"]), (hd["fus"],), (self.head_out_width(), hd["fus"]),
                  (self.head_out_width(),)]
        out = {}
        for k, shp, off in zip(HEAD_KEYS, shapes, self.head_offsets):
            n = 1
            for s in shp:
                n *= s
            out[k] = flat[off:off + n].view(*shp)
        return out

    def head_cat_width(self) -> int:
        """columns of fusion.0.weight: feat + hid, in flow mode da + time_dim more (x_t and phi(t)), in prefix mode `chunk` mask columns behind them"""
        hd = self.head_dims
        pk = self.head_flow_prefix["chunk"] if self.head_flow_prefix else 0
        return hd["feat"] + hd["hid"] + (hd["da"] + self.head_flow["time_dim"] + pk if self.head_flow else 0)

    def head_out_width(self) -> int:
        """rows of action_head.weight: da, in bins mode da * bins logits"""
        return self.head_dims["da"] * (self.head_bins["bins"] if self.head_bins else 1)

    # ---------------------------------------------------------------- binned action head
    def set_head_bins(self, bins: Optional[int] = 256, range=(-3.0, 3.0), sigma: float = 0.0, decode: str = "argmax") -> None:
        """Bins mode of the action expert (fv_head_set_bins): action_head is Linear(fusion_dim, da * bins), head_forward hands out the DECODED (B, da) chunk
        ("argmax": the centre of the most likely bin, "mean": the mean of the centres under the softmax) and keeps the logits in `saved`; head_backward
        evaluates the cross-entropy of the logits against the binned targets (sigma == 0: one-hot, sigma > 0: HL-Gauss with sigma bin widths).  range: one
        (lo, hi) for every element, or n pairs with n dividing da (element e reads pair e % n), in normalised action space.  bins None switches the mode off.
        Only before the first workspace is bound and before any train_*begin, and never together with flow mode (the library answers FV_ERR_STATE)."""
        if bins is None:
            _lib.check(self.lib.fv_head_set_bins(self.h, None, None, None), "fv_head_set_bins", self.h)
            self.head_bins = None
        else:
            rec = check_head_bins(bins, range, sigma, decode)
            n = len(rec["range"])
            if self.head_dims["da"] % n:
                raise ValueError(f"action_bins_range holds {n} pairs, which does not divide the head's action width {self.head_dims['da']}")
            spec = _lib.HeadBinsSpec(rec["bins"], _lib.BINS_DECODES[rec["decode"]], rec["sigma"], n)
            lo, hi = (C.c_float * n)(*[p[0] for p in rec["range"]]), (C.c_float * n)(*[p[1] for p in rec["range"]])
            with torch.cuda.device(self.device):
                _lib.check(self.lib.fv_head_set_bins(self.h, C.byref(spec), lo, hi), "fv_head_set_bins", self.h)
            self.head_bins = rec
        self._refresh_head_layout()

    def _bins_saved(self, saved: torch.Tensor, B: int) -> None:
        if self.head_bins is None:
            raise ValueError("the head is not in bins mode (set_head_bins)")
        if saved.numel() != self.head_saved_numel(B):
            raise ValueError(f"saved holds {saved.numel()} floats, a head_forward of {B} rows writes {self.head_saved_numel(B)}")

    def head_bins_logits(self, saved: torch.Tensor, B: int) -> torch.Tensor:
        """-> (B, da, bins) view of the logits a bins-mode head_forward of B rows wrote into `saved` (fv_head_bins_logits)"""
        self._bins_saved(saved, B)
        ptr = C.c_void_p()
        _lib.check(self.lib.fv_head_bins_logits(self.h, saved.data_ptr(), B, C.byref(ptr)), "fv_head_bins_logits", self.h)
        off = (ptr.value - saved.data_ptr()) // 4
        return saved[off:off + B * self.head_out_width()].view(B, self.head_dims["da"], self.head_bins["bins"])

    def head_bins_probs(self, saved: torch.Tensor, B: int) -> torch.Tensor:
        """-> (B, da, bins) f32: the softmax of every group of those logits, by the decode kernel (fv_head_bins_probs)"""
        self._bins_saved(saved, B)
        out = torch.empty(B, self.head_dims["da"], self.head_bins["bins"], dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_head_bins_probs(self.h, saved.data_ptr(), B, out.data_ptr(), _stream()), "fv_head_bins_probs", self.h)
        return out

    # ---------------------------------------------------------------- flow-matching head
    def set_head_flow(self, time_dim: Optional[int] = 64, min_period: float = 4e-3, max_period: float = 4.0, time_dist: str = "uniform",
                      dist_a: float = 0.0, dist_b: float = 1.0) -> None:
        """Flow mode of the action expert (fv_head_set_flow): fusion.0 reads [pooled | state | x_t | phi(t)], head_numel / head_views / head_saved follow.
        time_dim None switches it off.  Only before the first workspace is bound and before any train_*begin (the library answers FV_ERR_STATE afterwards)."""
        if time_dim is None:
            _lib.check(self.lib.fv_head_set_flow(self.h, None), "fv_head_set_flow", self.h)
            self.head_flow = None
            self.head_flow_time = None
            self.head_flow_draws = 1
            self.head_flow_prefix = None
            self.head_flow_solver = "euler"
            self.head_flow_samples = None
        else:
            if time_dist not in _lib.FLOW_TIME_DISTS:
                raise ValueError(f"flow time_dist must be one of {sorted(_lib.FLOW_TIME_DISTS)}, got {time_dist!r}")
            spec = _lib.HeadFlowSpec(int(time_dim), float(min_period), float(max_period), _lib.FLOW_TIME_DISTS[time_dist], float(dist_a), float(dist_b))
            with torch.cuda.device(self.device):
                _lib.check(self.lib.fv_head_set_flow(self.h, C.byref(spec)), "fv_head_set_flow", self.h)
            self.head_flow = dict(time_dim=int(time_dim), min_period=float(min_period), max_period=float(max_period), time_dist=time_dist,
                                  dist_a=float(dist_a), dist_b=float(dist_b))
            self.head_flow_time = None           # (a fresh fv_head_set_flow resets fv_head_set_flow_time)
        self._refresh_head_layout()

    def _refresh_head_layout(self) -> None:
        offs = (C.c_int64 * 13)()
        _lib.check(self.lib.fv_head_layout(self.h, C.byref(offs)), "fv_head_layout")
        self.head_offsets = list(offs)

    def set_head_flow_prefix(self, chunk: Optional[int] = None, max_delay: int = 0, thresholds=None, dist: str = "uniform", rate: float = 0.0) -> None:
        """Action-prefix conditioning of the flow head (fv_head_set_flow_prefix): fusion.0 reads `chunk` mask columns behind phi(t); training gives the first
        d <= max_delay steps of a chunk to the network clean and keeps them out of the loss, head_flow_sample_prefix pins them at inference.  thresholds:
        max_delay + 1 integers (fastvla_hip.prefix.delay_thresholds; None builds them from dist / rate).  chunk None switches the mode off.  Flow mode only,
        before the first workspace is bound and before any train_*begin (the library answers FV_ERR_STATE otherwise)."""
        if chunk is None:
            _lib.check(self.lib.fv_head_set_flow_prefix(self.h, 0, 0, None), "fv_head_set_flow_prefix", self.h)
            self.head_flow_prefix = None
        else:
            from . import prefix as _prefix
            if thresholds is None:
                thresholds = _prefix.delay_thresholds(int(max_delay), dist, rate)
            thr = [int(x) for x in thresholds]
            if len(thr) != int(max_delay) + 1:
                raise ValueError(f"flow prefix thresholds must hold max_delay + 1 = {int(max_delay) + 1} integers, got {len(thr)}")
            if any(x < 0 or x > 1 << 24 for x in thr):
                raise ValueError("flow prefix thresholds must lie in 0 .. 2^24")
            arr = (C.c_uint32 * len(thr))(*thr)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.fv_head_set_flow_prefix(self.h, int(chunk), int(max_delay), arr), "fv_head_set_flow_prefix", self.h)
            self.head_flow_prefix = dict(chunk=int(chunk), max_delay=int(max_delay), thresholds=thr, dist=dist, rate=float(rate))
        self._refresh_head_layout()

    def set_head_flow_draws(self, draws: int = 1) -> None:
        """S = draws noise draws per observation in one training step (fv_head_set_flow_draws; 1 .. 16, 1 = off): the mean loss and gradient of S single-draw
        steps at offsets o + (s << 56) for one backbone pass.  Head rows are draw-major (row s B + b): head_flow_prepare returns u (S B, da), head_forward in
        a training form the predicted velocity (S B, da); targets, pad, pooled and states keep B rows.  Flow mode only, before the first workspace is bound
        and before any train_*begin (the library answers FV_ERR_STATE otherwise)."""
        draws = check_flow_draws(draws)
        _lib.check(self.lib.fv_head_set_flow_draws(self.h, draws), "fv_head_set_flow_draws", self.h)
        self.head_flow_draws = draws

    def set_head_flow_time(self, dist: Optional[str] = "uniform", a: float = 0.0, b: float = 1.0, t_lo: float = 0.0, t_hi: float = 1.0,
                           stratify: bool = False) -> None:
        """The distribution of the drawn training time (fv_head_set_flow_time): t = t_lo + (t_hi - t_lo) F^-1(u) from the row's one uniform.  dist "uniform" |
        "logit_normal" (a + b n) | "beta" (Beta(a, b), both in [0.25, 32]; pi0: "beta", 1.5, 1.0, 0.001, 1.0); stratify: draw s of the S of set_head_flow_draws
        takes the s-th of S equal-probability strata (nothing with S = 1).  dist None returns the handle to set_head_flow's own time_dist.  Flow mode only, at any
        time: no size depends on it.  Explicit t buffers still replace every draw."""
        if dist is None:
            _lib.check(self.lib.fv_head_set_flow_time(self.h, None), "fv_head_set_flow_time", self.h)
            self.head_flow_time = None
            return
        tm = check_flow_time(dist, a, b, t_lo, t_hi, stratify)
        spec = _lib.HeadFlowTimeSpec(_lib.FLOW_TIME_SPEC_DISTS[tm["dist"]], tm["a"], tm["b"], tm["t_lo"], tm["t_hi"], int(tm["stratify"]))
        _lib.check(self.lib.fv_head_set_flow_time(self.h, C.byref(spec)), "fv_head_set_flow_time", self.h)
        self.head_flow_time = tm

    def head_flow_prepare(self, targets: torch.Tensor, saved: torch.Tensor, *, seed: int = 0, offset: int = 0, noise: Optional[torch.Tensor] = None,
                          t: Optional[torch.Tensor] = None, delays: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> u = eps - targets (B, da); x_t and phi(t) land in `saved` (head_saved(B)), which the following head_forward(saved=saved) reads
        (fv_head_flow_prepare).  noise (B, da) / t (B) replace the draws of (seed, offset).  With set_head_flow_draws(S): targets stay (B, da); noise, t and
        the returned u have S B rows, draw-major.  Prefix mode (set_head_flow_prefix): delays (draws * B) int32 replace the drawn delays
        (fv_head_flow_prepare_prefix; the kernel clamps them to 0 .. max_delay)."""
        B, da = targets.shape[0], self.head_dims["da"]
        R = B * self.head_flow_draws
        targets = targets.to(device=self.device, dtype=torch.float32).contiguous()
        if targets.numel() != B * da:
            raise ValueError(f"targets must hold (B, {da}) elements, got {tuple(targets.shape)}")
        if noise is not None:
            noise = noise.to(device=self.device, dtype=torch.float32).contiguous()
            if noise.numel() != R * da:
                raise ValueError(f"noise must hold (draws * B, {da}) = ({R}, {da}) elements, got {tuple(noise.shape)}")
        if t is not None:
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
            if t.numel() != R:
                raise ValueError(f"t must hold draws * B = {R} elements, got {tuple(t.shape)}")
        u = torch.empty(R, da, dtype=torch.float32, device=self.device)
        if delays is not None:
            delays = torch.as_tensor(delays).to(device=self.device, dtype=torch.int32).contiguous()
            if delays.numel() != R:
                raise ValueError(f"delays must hold draws * B = {R} elements, got {tuple(delays.shape)}")
            _lib.check(self.lib.fv_head_flow_prepare_prefix(self.h, targets.data_ptr(), B, seed, offset, _ptr(noise), _ptr(t), delays.data_ptr(), saved.data_ptr(),
                                                            u.data_ptr(), _stream()), "fv_head_flow_prepare_prefix", self.h)
            return u
        _lib.check(self.lib.fv_head_flow_prepare(self.h, targets.data_ptr(), B, seed, offset, _ptr(noise), _ptr(t), saved.data_ptr(), u.data_ptr(), _stream()),
                   "fv_head_flow_prepare", self.h)
        return u

    def _states(self, states: torch.Tensor, B: int) -> torch.Tensor:
        """states as the head kernels read them: fp32 (B, ds), contiguous, on the device (every head call passes here: a tensor that is already both
        skips .to(), which would hand it back unchanged, and that pays for the call)"""
        if states.dtype is not torch.float32 or states.device != self.device:
            states = states.to(device=self.device, dtype=torch.float32)
        states = states.contiguous()
        if states.shape != (B, self.head_dims["ds"]):
            raise ValueError(f"states must be (B,{self.head_dims['ds']}), got {tuple(states.shape)}")
        return states

    def _f32(self, t: torch.Tensor, rows: int, da: int, name: str, what: str = "(B, {da})") -> torch.Tensor:
        """a sampler's float operand: fp32, contiguous, on the device, rows * da elements"""
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if t.numel() != rows * da:
            raise ValueError(f"{name} must hold {what.format(rows=rows, da=da)} elements, got {tuple(t.shape)}")
        return t

    def _i32(self, t: torch.Tensor, B: int, name: str) -> torch.Tensor:
        """a sampler's per-row integer operand: int32, contiguous, on the device, B elements"""
        t = t.to(device=self.device, dtype=torch.int32).contiguous()
        if t.numel() != B:
            raise ValueError(f"{name} must hold B = {B} elements, got {tuple(t.shape)}")
        return t

    def _chunk_out(self, chunk_out: Optional[torch.Tensor], B: int, da: int, like: torch.Tensor) -> torch.Tensor:
        """where a sampler writes its normalised chunk: the caller's tensor, checked (it lives where `like` does), or a new one"""
        if chunk_out is None:
            return torch.empty(B, da, dtype=torch.float32, device=self.device)
        if chunk_out.dtype != torch.float32 or not chunk_out.is_contiguous() or chunk_out.numel() != B * da or chunk_out.device != like.device:
            raise ValueError(f"chunk_out must be a contiguous float32 (B, {da}) tensor on {self.device}")
        return chunk_out

    def head_flow_sample(self, flat_params: torch.Tensor, pooled: torch.Tensor, states: torch.Tensor, *, steps: int = 10,
                         noise: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0) -> torch.Tensor:
        """-> actions (B, da): `steps` steps of the chosen solver (set_head_flow_solver; Euler by default) along the velocity field from x_1 = noise (None: drawn from (seed, offset)) to t = 0 (fv_head_flow_sample),
        un-normalised when set_io_norm is on.  Not differentiated."""
        B, da = pooled.shape[0], self.head_dims["da"]
        states, pooled = self._states(states, B), pooled.contiguous()
        if noise is not None:
            noise = self._f32(noise, B, da, "noise")
        self.ensure_workspace(B, 1, False)
        actions = torch.empty(B, da, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_head_flow_sample(self.h, flat_params.data_ptr(), pooled.data_ptr(), states.data_ptr(), B, int(steps), _ptr(noise), seed, offset,
                                                actions.data_ptr(), _stream()), "fv_head_flow_sample", self.h)
        return actions

    def set_head_flow_solver(self, name: str = "euler") -> None:
        """The integrator of head_flow_sample, head_flow_sample_prefix and head_flow_sample_guided (fv_head_set_flow_solver): "euler" | "midpoint" | "heun" |
        "rk4".  `steps` keeps meaning steps: a call makes steps x stages (1, 2, 2, 4) network evaluations.  The first call that names a higher-order solver
        must come before the first workspace is bound (the library answers FV_ERR_STATE afterwards: the plan grows by two rows); later calls switch freely
        among all four.  ValueError for an unknown name, before any library call."""
        name = check_flow_solver(name)
        _lib.check(self.lib.fv_head_set_flow_solver(self.h, _lib.FLOW_SOLVERS[name]), "fv_head_set_flow_solver", self.h)
        self.head_flow_solver = name
        self.head_flow_solver_rows = self.head_flow_solver_rows or name != "euler"

    def set_head_flow_guidance(self, step_weights=None, max_guidance_weight: float = 5.0) -> None:
        """Guidance of the flow sampler (fv_head_set_flow_guidance; real-time chunking): step_weights = K host floats >= 0 (fastvla_hip.rtc.prefix_weights),
        K a divisor of action_dim; None switches it off.  The first call must come before the first workspace is bound (the library answers FV_ERR_STATE
        afterwards); later calls with the same K may change the weights and the largest guidance weight at any time."""
        if step_weights is None:
            _lib.check(self.lib.fv_head_set_flow_guidance(self.h, 0, None, 0.0), "fv_head_set_flow_guidance", self.h)
            self.head_flow_guidance = None
            return
        w = [float(x) for x in step_weights]
        arr = (C.c_float * len(w))(*w)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fv_head_set_flow_guidance(self.h, len(w), arr, float(max_guidance_weight)), "fv_head_set_flow_guidance", self.h)
        self.head_flow_guidance = dict(chunk=len(w), weights=w, max_guidance_weight=float(max_guidance_weight))

    def head_flow_sample_guided(self, flat_params: torch.Tensor, pooled: torch.Tensor, states: torch.Tensor, prev: torch.Tensor, *, shift: int = 0,
                                row_mask: Optional[torch.Tensor] = None, steps: int = 10, noise: Optional[torch.Tensor] = None, seed: int = 0,
                                offset: int = 0, chunk_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (actions (B, da), chunk (B, da)): head_flow_sample guided by `prev` (B, da), the previous chunk in normalised space, read `shift` steps ahead
        (fv_head_flow_sample_guided).  row_mask (B) int32: rows with 0 are sampled unguided.  chunk: the final normalised x_0, the next call's `prev`
        (written into chunk_out when one is handed in)."""
        B, da = pooled.shape[0], self.head_dims["da"]
        states, pooled = self._states(states, B), pooled.contiguous()
        prev = self._f32(prev, B, da, "prev")
        if noise is not None:
            noise = self._f32(noise, B, da, "noise")
        if row_mask is not None:
            row_mask = self._i32(row_mask, B, "row_mask")
        chunk_out = self._chunk_out(chunk_out, B, da, prev)
        self.ensure_workspace(B, 1, False)
        actions = torch.empty(B, da, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_head_flow_sample_guided(self.h, flat_params.data_ptr(), pooled.data_ptr(), states.data_ptr(), B, int(steps), _ptr(noise), seed,
                                                       offset, prev.data_ptr(), int(shift), _ptr(row_mask), actions.data_ptr(), chunk_out.data_ptr(), _stream()),
                   "fv_head_flow_sample_guided", self.h)
        return actions, chunk_out

    def head_flow_sample_prefix(self, flat_params: torch.Tensor, pooled: torch.Tensor, states: torch.Tensor, prev: torch.Tensor, delays: torch.Tensor, *,
                                shift: int = 0, steps: int = 10, noise: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0,
                                chunk_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (actions (B, da), chunk (B, da)): head_flow_sample with row b's first min(delays[b], max_delay, chunk - shift) steps pinned to `prev` (B, da), the
        previous chunk in normalised space, read `shift` steps ahead (fv_head_flow_sample_prefix).  delays (B) int32, 0 pins nothing.  chunk: the final
        normalised x_0, the next call's `prev` (written into chunk_out when one is handed in)."""
        B, da = pooled.shape[0], self.head_dims["da"]
        states, pooled = self._states(states, B), pooled.contiguous()
        prev = self._f32(prev, B, da, "prev")
        delays = self._i32(torch.as_tensor(delays), B, "delays")
        if noise is not None:
            noise = self._f32(noise, B, da, "noise")
        chunk_out = self._chunk_out(chunk_out, B, da, prev)
        self.ensure_workspace(B, 1, False)
        actions = torch.empty(B, da, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_head_flow_sample_prefix(self.h, flat_params.data_ptr(), pooled.data_ptr(), states.data_ptr(), B, int(steps), _ptr(noise), seed,
                                                       offset, prev.data_ptr(), int(shift), delays.data_ptr(), actions.data_ptr(), chunk_out.data_ptr(), _stream()),
                   "fv_head_flow_sample_prefix", self.h)
        return actions, chunk_out

    def set_head_flow_samples(self, max_samples: int = 1, step_weights=None) -> None:
        """Several samples per observation (fv_head_set_flow_samples): head_flow_sample_multi may then draw up to max_samples (1 .. 16; 1 = off) candidates
        in one call.  step_weights: K host floats >= 0, K a divisor of action_dim, the per-step weights of the coherence score
        (fastvla_hip.select.coherence_weights); None: "coherent" is refused.  The first call that names more than one sample must come before the first
        workspace is bound (the library answers FV_ERR_STATE afterwards: the sampler's rows grow); later calls with the same count may change the weights."""
        max_samples = check_flow_samples(max_samples)
        w = None if step_weights is None else [float(x) for x in step_weights]
        arr = None if w is None else (C.c_float * len(w))(*w)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fv_head_set_flow_samples(self.h, max_samples, len(w) if w else 0, arr), "fv_head_set_flow_samples", self.h)
        self.head_flow_samples = dict(max_samples=max_samples, weights=w)

    def head_flow_sample_multi(self, flat_params: torch.Tensor, pooled: torch.Tensor, states: torch.Tensor, *, samples: int = 1, select: str = "first",
                               prev: Optional[torch.Tensor] = None, shift: int = 0, row_mask: Optional[torch.Tensor] = None,
                               delays: Optional[torch.Tensor] = None, steps: int = 10, noise: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0,
                               chunk_out: Optional[torch.Tensor] = None, extras: bool = True) -> Dict[str, torch.Tensor]:
        """`samples` candidates per observation in one call, one of them chosen on the device (fv_head_flow_sample_multi).  Candidate s is head_flow_sample
        (with delays: head_flow_sample_prefix) at offset + (s << 56); noise is (samples * B, da), sample-major.  select: "first" | "medoid" | "coherent"
        (prev (B, da) normalised, read `shift` steps ahead; row_mask (B) int32, rows with 0 take the medoid).
        -> dict: actions (B, da), chunk (B, da) normalised (written into chunk_out when one is handed in) and, with extras, candidates (samples * B, da)
        normalised and sample-major, choice (B) int32, scores (B, samples), spread (B, da).  Everything stays on the device."""
        if select not in _lib.FLOW_SELECTS:
            raise ValueError(f"select must be one of {list(_lib.FLOW_SELECTS)}, got {select!r}")
        S = check_flow_samples(samples)
        B, da = pooled.shape[0], self.head_dims["da"]
        states, pooled = self._states(states, B), pooled.contiguous()
        if prev is not None:
            prev = self._f32(prev, B, da, "prev")
        if delays is not None:
            delays = self._i32(torch.as_tensor(delays), B, "delays")
        if row_mask is not None:
            row_mask = self._i32(row_mask, B, "row_mask")
        if noise is not None:
            noise = self._f32(noise, S * B, da, "noise", "(samples * B, {da}) = ({rows}, {da})")
        chunk_out = self._chunk_out(chunk_out, B, da, pooled)
        self.ensure_workspace(B, 1, False)
        out = dict(actions=torch.empty(B, da, dtype=torch.float32, device=self.device), chunk=chunk_out)
        if extras:
            out.update(candidates=torch.empty(S * B, da, dtype=torch.float32, device=self.device), choice=torch.empty(B, dtype=torch.int32, device=self.device),
                       scores=torch.empty(B, S, dtype=torch.float32, device=self.device), spread=torch.empty(B, da, dtype=torch.float32, device=self.device))
        _lib.check(self.lib.fv_head_flow_sample_multi(self.h, flat_params.data_ptr(), pooled.data_ptr(), states.data_ptr(), B, int(steps), _ptr(noise), seed, offset, S,
                                                      _lib.FLOW_SELECTS[select], _ptr(prev), int(shift), _ptr(row_mask), _ptr(delays), out["actions"].data_ptr(),
                                                      chunk_out.data_ptr(), _ptr(out.get("candidates")), _ptr(out.get("choice")), _ptr(out.get("scores")),
                                                      _ptr(out.get("spread")), _stream()), "fv_head_flow_sample_multi", self.h)
        return out

    def head_saved_numel(self, B: int) -> int:
        n = C.c_size_t()
        _lib.check(self.lib.fv_head_saved_bytes(self.h, B, C.byref(n)), "fv_head_saved_bytes")
        return n.value // 4

    def head_saved(self, B: int) -> torch.Tensor:
        return torch.empty(self.head_saved_numel(B), dtype=torch.float32, device=self.device)

    def head_forward(self, flat_params: torch.Tensor, pooled: torch.Tensor, states: torch.Tensor, *, training: bool = False,
                     dropout_p: float = 0.0, seed: int = 0, offset: int = 0, saved: Optional[torch.Tensor] = None,
                     normalized_actions: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """normalized_actions: keep the output in normalised action space even without dropout (loss / training paths when
        set_io_norm folded the dataset statistics in)."""
        B = pooled.shape[0]
        states, pooled = self._states(states, B), pooled.contiguous()
        saved = saved if saved is not None else self.head_saved(B)
        # 1 = dropout active, 2 = training-mode arithmetic without dropout (folded action statistics are NOT applied), 0 = inference
        mode = 0 if not (training or normalized_actions) else (1 if training and dropout_p > 0.0 else 2)
        # (set_head_flow_draws: the training forms predict every draw's velocity, draws * B rows; inference ignores the setting)
        actions = torch.empty(B * (self.head_flow_draws if mode else 1), self.head_dims["da"], dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_head_forward(self.h, flat_params.data_ptr(), pooled.data_ptr(), states.data_ptr(), B,
                                            mode, float(dropout_p), seed, offset, actions.data_ptr(),
                                            saved.data_ptr(), _stream()), "fv_head_forward")
        return actions, saved

    def set_io_norm(self, state_mean=None, state_std=None, action_mean=None, action_std=None, eps: float = 1e-8) -> None:
        """Fold the dataset's MEAN_STD statistics into the head kernels (fv_head_set_io_norm); all None switches it off."""
        vecs = [state_mean, state_std, action_mean, action_std]
        if all(v is None for v in vecs):
            _lib.check(self.lib.fv_head_set_io_norm(self.h, None, None, None, None, float(eps)), "fv_head_set_io_norm", self.h)
            return
        dims = [self.head_dims["ds"], self.head_dims["ds"], self.head_dims["da"], self.head_dims["da"]]
        keep = []
        for v, n in zip(vecs, dims):
            t = torch.as_tensor(v, dtype=torch.float32).detach().cpu().contiguous().reshape(-1)
            if t.numel() != n:
                raise ValueError(f"normalisation vector has {t.numel()} elements, expected {n}")
            keep.append(t)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fv_head_set_io_norm(self.h, *[t.data_ptr() for t in keep], float(eps)), "fv_head_set_io_norm", self.h)

    # ---------------------------------------------------------------- action chunks: the loss of the fused backward
    def set_head_loss(self, kind: str = "mse", beta: float = 1.0, chunk: int = 1) -> None:
        """The loss every later head_backward / train_*forward_backward evaluates (fv_head_set_loss): kind "mse" | "l1" | "smooth_l1" over chunks of `chunk`
        steps (the head's action_dim = chunk * A).  The defaults are the library's own: the plain MSE kernel."""
        kind, beta, chunk = check_head_loss(kind, beta, chunk, self.head_dims["da"])
        if (kind, beta, chunk) == ("mse", 1.0, 1):
            _lib.check(self.lib.fv_head_set_loss(self.h, None), "fv_head_set_loss", self.h)
        else:
            spec = _lib.HeadLossSpec(_lib.LOSS_KINDS[kind], beta, chunk)
            _lib.check(self.lib.fv_head_set_loss(self.h, C.byref(spec)), "fv_head_set_loss", self.h)
        if chunk != self.head_loss["chunk"]:
            self.head_loss_weights = None      # (the library drops them: their sizes no longer fit)
        self.head_loss = dict(kind=kind, beta=beta, chunk=chunk)

    def loss_is_chunked(self, pad) -> bool:
        """whether a loss evaluation with this mask runs the chunked kernel (and writes head_loss_metrics) or the plain MSE kernel"""
        return pad is not None or self.head_loss["kind"] != "mse" or self.head_loss_weights is not None or self.head_flow_prefix is not None or self.head_bins is not None

    def set_head_loss_weights(self, dim_w=None, step_w=None) -> None:
        """Per-dimension (A = action_dim / chunk) and per-step (K = chunk) weights of the loss (fv_head_set_loss_weights): either may be None = ones, both
        None switches weighting off.  With weights on every loss kind runs the chunked kernel's weighted instance; an element whose weight is 0 is selected
        away like a padded one.  ValueError for a wrong length or a negative / non-finite value, before any library call.  set_head_loss with another chunk
        drops them."""
        K = self.head_loss["chunk"]
        w = check_loss_weights(dim_w, step_w, self.head_dims["da"] // K, K)
        if w is None:
            _lib.check(self.lib.fv_head_set_loss_weights(self.h, None, None), "fv_head_set_loss_weights", self.h)
        else:
            arrs = [None if v is None else (C.c_float * len(v))(*v) for v in (w["dim"], w["step"])]
            with torch.cuda.device(self.device):
                _lib.check(self.lib.fv_head_set_loss_weights(self.h, *[None if a is None else C.cast(a, C.c_void_p) for a in arrs]), "fv_head_set_loss_weights", self.h)
        self.head_loss_weights = w

    def head_loss_per_dim(self, actions: torch.Tensor, targets: torch.Tensor, pad=None) -> torch.Tensor:
        """-> (A,) f32: mean |actions - targets| over the non-padded steps of each action dimension (fv_head_loss_per_dim), in the space the loss lives in;
        0 for a dimension without a valid step.  actions, targets: (B, K, A) or (B, K * A); pad: optional (B, chunk) bool.  Never weighted.
        (set_head_flow_draws(S): actions and targets have S B rows, pad keeps B.)"""
        S, K = self.head_flow_draws, self.head_loss["chunk"]
        B = self._draw_rows(actions.shape[0])
        actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        targets = targets.to(device=self.device, dtype=torch.float32).contiguous()
        if actions.numel() != S * B * self.head_dims["da"] or targets.numel() != actions.numel():
            raise ValueError(f"actions and targets must hold (B, {self.head_dims['da']}) elements, got {tuple(actions.shape)} and {tuple(targets.shape)}")
        pad = self._pad_arg(pad, B)
        out = torch.empty(self.head_dims["da"] // K, dtype=torch.float32, device=self.device)
        with self._Mask(self, pad):
            _lib.check(self.lib.fv_head_loss_per_dim(self.h, actions.data_ptr(), targets.data_ptr(), B, out.data_ptr(), _stream()), "fv_head_loss_per_dim", self.h)
        return out

    def head_loss_per_time(self, actions: torch.Tensor, targets: torch.Tensor, t: torch.Tensor, buckets: int = 10, pad=None) -> torch.Tensor:
        """-> (buckets, 2) f32: per time bucket the sum of (actions - targets)^2 over the non-padded elements of the rows whose t falls into it, and the number
        of those elements (fv_head_loss_per_time); row r's bucket is min(buckets - 1, int(t buckets)).  actions = v, targets = u: (R, da), t: (R,); pad:
        optional (B, chunk) bool.  Never weighted, whatever the loss kind.  (set_head_flow_draws(S): R = S B rows, pad keeps B.)"""
        S, da = self.head_flow_draws, self.head_dims["da"]
        B = self._draw_rows(actions.shape[0])
        if isinstance(buckets, bool) or not isinstance(buckets, int) or not 1 <= buckets <= _lib.LOSS_TIME_BUCKETS_MAX:
            raise ValueError(f"buckets must be an integer 1 .. {_lib.LOSS_TIME_BUCKETS_MAX}, got {buckets!r}")
        actions = actions.to(device=self.device, dtype=torch.float32).contiguous()
        targets = targets.to(device=self.device, dtype=torch.float32).contiguous()
        t = t.to(device=self.device, dtype=torch.float32).contiguous()
        if actions.numel() != S * B * da or targets.numel() != actions.numel() or t.numel() != S * B:
            raise ValueError(f"actions and targets must hold (R, {da}) elements and t R, got {tuple(actions.shape)}, {tuple(targets.shape)} and {tuple(t.shape)}")
        pad = self._pad_arg(pad, B)
        out = torch.empty(buckets, 2, dtype=torch.float32, device=self.device)
        with self._Mask(self, pad):
            _lib.check(self.lib.fv_head_loss_per_time(self.h, actions.data_ptr(), targets.data_ptr(), t.data_ptr(), B, buckets, out.data_ptr(), _stream()),
                       "fv_head_loss_per_time", self.h)
        return out

    def _draw_rows(self, rows: int) -> int:
        """head rows -> observations: rows / draws (set_head_flow_draws; the head's rows are draw-major)"""
        S = self.head_flow_draws
        if rows % S:
            raise ValueError(f"{rows} head rows are not a multiple of the {S} noise draws per observation (set_head_flow_draws)")
        return rows // S

    def _pad_arg(self, pad, B: int) -> Optional[torch.Tensor]:
        if pad is None:
            return None
        K = self.head_loss["chunk"]
        pad = torch.as_tensor(pad)
        if tuple(pad.shape) != (B, K):
            raise ValueError(f"action_is_pad must be (B, chunk) = ({B}, {K}), got {tuple(pad.shape)}")
        return (pad != 0).to(device=self.device, dtype=torch.uint8).contiguous()

    class _Mask:
        """the padding mask on the handle for exactly one loss call: set immediately before, cleared after (a look-ahead prepare never touches it)"""

        def __init__(self, eng: "FastVLAEngine", pad: Optional[torch.Tensor]):
            self.eng, self.pad = eng, pad

        def __enter__(self):
            if self.pad is not None:
                self.eng._pad_keep = self.pad
                _lib.check(self.eng.lib.fv_head_set_loss_mask(self.eng.h, self.pad.data_ptr()), "fv_head_set_loss_mask", self.eng.h)

        def __exit__(self, *exc):
            if self.pad is not None:
                _lib.check(self.eng.lib.fv_head_set_loss_mask(self.eng.h, None), "fv_head_set_loss_mask", self.eng.h)
            return False

    def head_loss_metrics(self) -> torch.Tensor:
        """-> (2,) f32 copy of what the last chunked loss evaluation on the current stream wrote: [masked MSE, valid steps / (B * chunk)].  In bins mode (3,):
        [masked squared error of the decoded chunk, valid steps / (B * chunk), the fraction of valid elements whose most likely bin is the target's]."""
        ptr = C.c_void_p()
        _lib.check(self.lib.fv_head_loss_metrics(self.h, C.byref(ptr)), "fv_head_loss_metrics", self.h)
        # a stream-ordered device copy with the library's own y += x over the metrics' 16-byte slot (0 + m == m exactly; include/fastvla_hip.h: 4 floats, two reserved zeros)
        out = torch.zeros(4, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_grad_accumulate(self.h, out.data_ptr(), ptr.value, 4, _stream()), "fv_grad_accumulate", self.h)
        return out[:3] if self.head_bins is not None else out[:2]

    def head_backward(self, flat_params: torch.Tensor, actions: torch.Tensor, targets: torch.Tensor, saved: torch.Tensor,
                      dropout_p: float = 0.0, flat_grads: Optional[torch.Tensor] = None, pad=None):
        """pad: optional (B, chunk) bool, True = the step lies past the episode end and must not train.  (set_head_flow_draws(S): actions and targets have
        S B rows, pad keeps B rows and applies to every draw of its observation.)"""
        B = self._draw_rows(actions.shape[0])
        self.ensure_workspace(B, 1, False)
        targets = targets.to(device=self.device, dtype=torch.float32).contiguous()
        if targets.numel() != actions.numel():
            raise ValueError(f"targets must hold {tuple(actions.shape)} elements, got {tuple(targets.shape)}")
        pad = self._pad_arg(pad, B)
        if flat_grads is None:
            flat_grads = torch.zeros(self.head_numel(), dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        with self._Mask(self, pad):
            _lib.check(self.lib.fv_head_mse_backward(self.h, flat_params.data_ptr(), actions.data_ptr(), targets.data_ptr(), B,
                                                     float(dropout_p), saved.data_ptr(), loss.data_ptr(),
                                                     flat_grads.data_ptr(), _stream()), "fv_head_mse_backward")
        return loss, flat_grads

    def head_backward_from_grad(self, flat_params: torch.Tensor, grad_actions: torch.Tensor, saved: torch.Tensor,
                                dropout_p: float = 0.0, flat_grads: Optional[torch.Tensor] = None) -> torch.Tensor:
        """generic backward: dL/dactions (B,A) -> all 12 head grads in one flat buffer (overwritten)."""
        B = self._draw_rows(grad_actions.shape[0])
        self.ensure_workspace(B, 1, False)
        grad_actions = grad_actions.to(device=self.device, dtype=torch.float32).contiguous()
        if flat_grads is None:
            flat_grads = torch.zeros(self.head_numel(), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.fv_head_backward(self.h, flat_params.data_ptr(), grad_actions.data_ptr(), B, float(dropout_p),
                                             saved.data_ptr(), flat_grads.data_ptr(), _stream()), "fv_head_backward")
        return flat_grads

    def grad_accumulate(self, acc: torch.Tensor, grads: torch.Tensor) -> None:
        """acc += grads (flat head buffers) on the current stream."""
        _lib.check(self.lib.fv_grad_accumulate(self.h, acc.data_ptr(), grads.data_ptr(), acc.numel(), _stream()),
                   "fv_grad_accumulate", self.h)

    def grad_scale(self, grads: torch.Tensor, scale_dev: torch.Tensor) -> None:
        """grads *= scale_dev[0] (a device scalar) on the current stream."""
        _lib.check(self.lib.fv_grad_scale(self.h, grads.data_ptr(), grads.numel(), scale_dev.data_ptr(), _stream()),
                   "fv_grad_scale", self.h)

    # ---------------------------------------------------------------- unfrozen-backbone training (fv_train_*)
    def train_begin(self) -> None:
        """One-time set-up of the unfrozen decoder + projector training slice (library-owned transposed weight copies)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fv_train_begin(self.h), "fv_train_begin", self.h)

    _TRAIN_OPTION_DEFAULTS = {"grad_split": 2, "wgrad_f16": True, "loss_scale_log2": 12}

    def train_set_options(self, grad_split: Optional[int] = None, wgrad_f16: Optional[bool] = None, loss_scale_log2: Optional[int] = None,
                          keep: bool = False) -> None:
        """Arithmetic of the backward's contractions (fv_train_set_options).  grad_split: dgrad's gradient operand -- 2 (default) ONE fp16 pass against
        fp16 transposed weights, 1 split bf16 (two passes, the most exact);
        wgrad_f16=False: weight gradients as split-bf16 gradient x bf16 activation (two passes) instead of ONE fp16 pass;
        loss_scale_log2: every gradient of train_forward_backward carries 2^k (train_loss_scale()): divide it out in the optimiser's grad_scale.
        An argument left None takes its default -- or, with keep=True, the value of the previous call (to change one knob only)."""
        base = getattr(self, "_train_options", None) if keep else None
        opts = dict(base or self._TRAIN_OPTION_DEFAULTS)
        for k, v in (("grad_split", grad_split), ("wgrad_f16", wgrad_f16), ("loss_scale_log2", loss_scale_log2)):
            if v is not None:
                opts[k] = v
        _lib.check(self.lib.fv_train_set_options(self.h, int(opts["grad_split"]), int(opts["wgrad_f16"]), int(opts["loss_scale_log2"])),   # wgrad_f16: False / True
                   "fv_train_set_options", self.h)
        self._train_options = opts

    def train_set_forward_f16(self, on: bool = True) -> None:
        """The TRAINING forward's projections in ONE fp16 pass instead of the split-bf16 form's two (fv_train_set_forward_f16); inference is untouched."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fv_train_set_forward_f16(self.h, int(on)), "fv_train_set_forward_f16", self.h)

    def train_loss_scale(self) -> float:
        v = C.c_float()
        _lib.check(self.lib.fv_train_loss_scale(self.h, C.byref(v)), "fv_train_loss_scale", self.h)
        return float(v.value)

    def train_layout(self):
        """-> (tensors, total_numel, n_buckets): every trainable tensor of the ONE flat fp32 buffer, in order: dicts with name, offset,
        numel, rows, cols, bucket (0 head, 1 projector, 2 embedding, 3 + l layer l, 3 + L final norm) and packing (0 plain, 1 q|k|v rows
        concatenated, 2 gate/up rows interleaved by 8)."""
        n, total, nb = C.c_int(), C.c_int64(), C.c_int()
        _lib.check(self.lib.fv_train_layout(self.h, None, 0, C.byref(n), C.byref(total), C.byref(nb)), "fv_train_layout", self.h)
        arr = (_lib.TrainTensor * n.value)()
        _lib.check(self.lib.fv_train_layout(self.h, arr, n.value, C.byref(n), C.byref(total), C.byref(nb)), "fv_train_layout", self.h)
        return _train_tensors(arr), int(total.value), int(nb.value)

    def train_export_params(self, flat: torch.Tensor) -> None:
        """backbone part of the flat master buffer <- the library's current weights (fv_train_export_params)"""
        _lib.check(self.lib.fv_train_export_params(self.h, flat.data_ptr(), _stream()), "fv_train_export_params", self.h)

    def train_commit(self, flat: torch.Tensor) -> None:
        """the library's bf16 operand copies (and their transposes) <- the master, after an optimiser step (fv_train_commit)"""
        _lib.check(self.lib.fv_train_commit(self.h, flat.data_ptr(), _stream()), "fv_train_commit", self.h)

    def train_workspace(self, B: int, T: int) -> torch.Tensor:
        n = C.c_size_t()
        _lib.check(self.lib.fv_train_workspace_bytes(self.h, B, T, C.byref(n)), "fv_train_workspace_bytes", self.h)
        ws = torch.empty(n.value + 256, dtype=torch.uint8, device=self.device)
        return ws

    def train_named_tensors(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """canonical checkpoint key -> a COPY of that tensor taken out of a flat buffer in the library's packed layout (parameters,
        gradients or Adam moments alike): q / k / v split back out of qkv_proj, gate / up de-interleaved, head tensors under "head.<key>"."""
        tensors, _, _ = self.train_layout()
        l = self.model.llm
        qd, kd = l.heads * l.head_dim, l.kv_heads * l.head_dim
        out = {}
        for t in tensors:
            v = flat[t["offset"]: t["offset"] + t["rows"] * t["cols"]]
            v = v.view(t["rows"], t["cols"]) if t["rows"] > 1 else v
            name = t["name"]
            if t["bucket"] == 0:
                out["head." + name] = v.clone()
            elif t["packing"] == 1:
                base, kind = name.rsplit(".qkv_proj.", 1)
                for nm, r0, r1 in (("q", 0, qd), ("k", qd, qd + kd), ("v", qd + kd, qd + 2 * kd)):
                    out[f"{base}.{nm}_proj.{kind}"] = v[r0:r1].clone()
            elif t["packing"] == 2:
                base = name.rsplit(".gate_up_proj.weight", 1)[0]
                g = v.view(l.inter // 8, 2, 8, l.hidden)
                out[base + ".gate_proj.weight"] = g[:, 0].reshape(l.inter, l.hidden).clone()
                out[base + ".up_proj.weight"] = g[:, 1].reshape(l.inter, l.hidden).clone()
            elif t["packing"] == 3:      # depthwise weight, tap-major [k*k][C] -> [C, 1, k, k]
                k = int(round(t["rows"] ** 0.5))
                out[name] = v.t().reshape(t["cols"], 1, k, k).clone()
            elif t["packing"] == 4:      # the stem's dense 3x3, [27][C0] with row (ky*3+kx)*3+ci -> [C0, 3, 3, 3]
                out[name] = v.view(3, 3, 3, t["cols"]).permute(3, 2, 0, 1).contiguous()
            else:
                out[name] = v.clone()
        return out

    def _train_step_inputs(self, tower_out, ids, lens, states, targets, ws):
        """what train_forward_backward and train_lora_forward_backward share: the inputs on the device in the library's types, the outputs, the aligned workspace"""
        B, T = ids.shape
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        lens = lens.to(device=self.device, dtype=torch.int32).contiguous()
        states = states.to(device=self.device, dtype=torch.float32).contiguous()
        targets = targets.to(device=self.device, dtype=torch.float32).contiguous()
        if targets.numel() != B * self.head_dims["da"]:
            raise ValueError(f"targets must hold (B, {self.head_dims['da']}) elements, got {tuple(targets.shape)}")
        tower_out = tower_out.contiguous()
        if tower_out.dtype != torch.bfloat16 or tower_out.shape != (B, self.model.tower.num_tokens, self.model.tower.out_dim):
            raise ValueError(f"tower_out must be (B, {self.model.tower.num_tokens}, {self.model.tower.out_dim}) bf16, got {tuple(tower_out.shape)} {tower_out.dtype}")
        actions = torch.empty(B, self.head_dims["da"], dtype=torch.float32, device=self.device)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        return (B, T, tower_out, ids, lens, states, targets, actions, loss, *self._aligned(ws))

    def train_forward_backward(self, flat_params: torch.Tensor, tower_out: torch.Tensor, ids: torch.Tensor, lens: torch.Tensor, states: torch.Tensor,
                               targets: torch.Tensor, ws: torch.Tensor, *, training: bool = True, dropout_p: float = 0.0, seed: int = 0, offset: int = 0,
                               flat_grads: Optional[torch.Tensor] = None, bucket_cb=None, pad=None):
        """One step's forward + MSE + backward over every trainable tensor (fv_train_forward_backward).  tower_out: (B, Ni, tower_out_dim)
        bf16 from vision_forward(..., return_tower_out=True).  bucket_cb(bucket, offset, numel) is called when a bucket's gradient has
        been enqueued completely.  -> (actions (B, A) in normalised space, loss (1,), flat_grads TIMES train_loss_scale())."""
        B, T, tower_out, ids, lens, states, targets, actions, loss, ws_ptr, ws_bytes = self._train_step_inputs(tower_out, ids, lens, states, targets, ws)
        if flat_grads is None:
            flat_grads = torch.empty_like(flat_params)
        fn, err = _bucket_trampoline(bucket_cb)
        with self._Mask(self, self._pad_arg(pad, B)):
            rc = self.lib.fv_train_forward_backward(self.h, flat_params.data_ptr(), tower_out.data_ptr(), ids.data_ptr(), lens.data_ptr(), states.data_ptr(),
                                                    targets.data_ptr(), B, T, int(training), float(dropout_p), seed, offset, ws_ptr, ws_bytes,
                                                    actions.data_ptr(), loss.data_ptr(), flat_grads.data_ptr(), fn, None, _stream())
        if "exc" in err:
            raise err["exc"]
        _lib.check(rc, "fv_train_forward_backward", self.h)
        return actions, loss, flat_grads

    # ---------------------------------------------------------------- LoRA mode of the slice (fv_train_lora_*; csrc/lora_path.inc)
    def train_lora_begin(self, rank: int, alpha: Optional[float] = None, targets=None, dora: bool = False, rslora: bool = False) -> None:
        """After train_begin(): adapters W0 + (alpha / rank) B A on the target matrices of every decoder layer (default: alpha = rank, all seven targets);
        the master stays frozen.  Not together with train_tower_begin().  rslora: s = alpha / sqrt(rank).  dora: a trained magnitude per output row over the
        direction W0 + s B A (fv_train_lora_begin_ex; initialise it with train_lora_init_magnitude)."""
        from . import lora
        cfg = lora.check_config(rank, alpha, targets, dora=dora, rslora=rslora)
        flags = lora.flags_of(cfg)
        with torch.cuda.device(self.device):
            if flags:
                _lib.check(self.lib.fv_train_lora_begin_ex(self.h, cfg["rank"], cfg["alpha"], lora.target_mask(cfg["targets"]), flags), "fv_train_lora_begin_ex", self.h)
            else:
                _lib.check(self.lib.fv_train_lora_begin(self.h, cfg["rank"], cfg["alpha"], lora.target_mask(cfg["targets"])), "fv_train_lora_begin", self.h)
        self.lora_config = cfg

    def train_lora_init_magnitude(self, flat_master: torch.Tensor, lora_params: torch.Tensor) -> None:
        """DoRA: every lora_magnitude_vector in lora_params <- the row norms of W0 + s B A for the A, B it holds (fv_train_lora_init_magnitude), so that
        m / n == 1 exactly and the next train_lora_commit builds what a commit without the magnitude would."""
        _lib.check(self.lib.fv_train_lora_init_magnitude(self.h, flat_master.data_ptr(), lora_params.data_ptr(), _stream()), "fv_train_lora_init_magnitude", self.h)

    def train_lora_layout(self):
        """-> (tensors, total_numel) of the TRAINABLE flat buffer [head | projector | layer adapters] (fv_train_lora_layout), dicts as train_layout()'s."""
        n, total = C.c_int(), C.c_int64()
        _lib.check(self.lib.fv_train_lora_layout(self.h, None, 0, C.byref(n), C.byref(total)), "fv_train_lora_layout", self.h)
        arr = (_lib.TrainTensor * n.value)()
        _lib.check(self.lib.fv_train_lora_layout(self.h, arr, n.value, C.byref(n), C.byref(total)), "fv_train_lora_layout", self.h)
        return _train_tensors(arr), int(total.value)

    def train_lora_project(self, flat_grads_full: torch.Tensor, lora_params: torch.Tensor, lora_grads: torch.Tensor) -> None:
        """lora_grads <- head / projector gradients copied, dA = s B^T dW', dB = s dW' A^T of every adapted matrix (fv_train_lora_project)"""
        _lib.check(self.lib.fv_train_lora_project(self.h, flat_grads_full.data_ptr(), lora_params.data_ptr(), lora_grads.data_ptr(), _stream()),
                   "fv_train_lora_project", self.h)

    def train_lora_forward_backward(self, flat_params: torch.Tensor, lora_params: torch.Tensor, tower_out: torch.Tensor, ids: torch.Tensor, lens: torch.Tensor,
                                    states: torch.Tensor, targets: torch.Tensor, ws: torch.Tensor, *, training: bool = True, dropout_p: float = 0.0, seed: int = 0,
                                    offset: int = 0, lora_grads: Optional[torch.Tensor] = None, pad=None):
        """The DIRECT LoRA step (fv_train_lora_forward_backward): train_forward_backward's forward and input-gradient chain, dA / dB of every adapter straight from
        the gradient rows and the kept activations -- no full-size gradient buffer, no train_lora_project.  flat_params: the master; lora_params: the trainable
        buffer.  -> (actions, loss (1,), lora_grads in the trainable layout TIMES train_loss_scale()).  Needs train_lora_begin() and the default backward options."""
        B, T, tower_out, ids, lens, states, targets, actions, loss, ws_ptr, ws_bytes = self._train_step_inputs(tower_out, ids, lens, states, targets, ws)
        if lora_grads is None:
            lora_grads = torch.empty_like(lora_params)
        with torch.cuda.device(self.device), self._Mask(self, self._pad_arg(pad, B)):     # (the first call allocates the kernels' scratch)
            rc = self.lib.fv_train_lora_forward_backward(self.h, flat_params.data_ptr(), lora_params.data_ptr(), tower_out.data_ptr(), ids.data_ptr(), lens.data_ptr(),
                                                         states.data_ptr(), targets.data_ptr(), B, T, int(training), float(dropout_p), seed, offset, ws_ptr,
                                                         ws_bytes, actions.data_ptr(), loss.data_ptr(), lora_grads.data_ptr(), _stream())
        _lib.check(rc, "fv_train_lora_forward_backward", self.h)
        return actions, loss, lora_grads

    def train_lora_commit(self, flat_master: torch.Tensor, lora_params: torch.Tensor) -> None:
        """operand images <- W0 + s B A (adapted matrices; DoRA: diag(m / n) (W0 + s B A), the row norms n refreshed) / the master (the rest); the master's
        head | projector front <- lora_params' (fv_train_lora_commit).  DoRA: flat_master must stay alive and in place until train_lora_project has run."""
        _lib.check(self.lib.fv_train_lora_commit(self.h, flat_master.data_ptr(), lora_params.data_ptr(), _stream()), "fv_train_lora_commit", self.h)

    def train_lora_merge(self, flat_master: torch.Tensor, lora_params: torch.Tensor) -> None:
        """flat_master's adapted matrices += s B A, the very fp32 values train_lora_commit rounds (fv_train_lora_merge)"""
        _lib.check(self.lib.fv_train_lora_merge(self.h, flat_master.data_ptr(), lora_params.data_ptr(), _stream()), "fv_train_lora_merge", self.h)

    # ---------------------------------------------------------------- the tower half of the slice (fv_train_tower_*; csrc/tower_train.inc)
    def train_tower_begin(self) -> None:
        """After train_begin(): the FastViT-HD tower's tensors (inference form) join the flat master -- train_layout() then lists them behind
        "model.norm.weight" (packing 3 = depthwise weights tap-major [k*k][C], 4 = the stem's [27][C0]) with their own gradient buckets."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fv_train_tower_begin(self.h), "fv_train_tower_begin", self.h)
        self._tower_training = True

    def train_tower_workspace(self, B: int) -> torch.Tensor:
        n = C.c_size_t()
        _lib.check(self.lib.fv_train_tower_workspace_bytes(self.h, B, C.byref(n)), "fv_train_tower_workspace_bytes", self.h)
        return torch.empty(n.value + 256, dtype=torch.uint8, device=self.device)

    @staticmethod
    def _aligned(ws: torch.Tensor):
        """-> (pointer, bytes) of a workspace from its first 256-byte boundary on (every workspace is allocated 256 bytes larger than the library asks for)"""
        base = ws.data_ptr()
        pad = (-base) % 256
        return base + pad, ws.numel() - pad

    def train_tower_forward(self, pix: torch.Tensor, tws: torch.Tensor) -> torch.Tensor:
        """pixels (B, S, S, 4) bf16 (preprocess()) -> tower_out (B, tokens, tower_out_dim) bf16; every unit's tensors stay in tws for train_tower_backward."""
        B = pix.shape[0]
        t = self.model.tower
        tower_out = torch.empty(B, t.num_tokens, t.out_dim, dtype=torch.bfloat16, device=self.device)
        p, n = self._aligned(tws)
        _lib.check(self.lib.fv_train_tower_forward(self.h, pix.data_ptr(), B, p, n, tower_out.data_ptr(), _stream()), "fv_train_tower_forward", self.h)
        return tower_out

    def train_tower_unit_outputs(self, B: int, tws: torch.Tensor):
        """-> [output of unit 0, 1, ...] (bf16 NHWC) as the last train_tower_forward left them in tws"""
        p, n = self._aligned(tws)
        outs = []
        for u, (_, _, sd, ch) in enumerate(self.tower_units()):
            t = torch.empty(B, sd, sd, ch, dtype=torch.bfloat16, device=self.device)
            _lib.check(self.lib.fv_train_tower_read_unit(self.h, u, B, p, n, t.data_ptr(), _stream()), "fv_train_tower_read_unit", self.h)
            outs.append(t)
        return outs

    def train_set_tower_grad(self, buf: Optional[torch.Tensor]) -> None:
        """bind (or, with None, unbind) the fp16 (B, tokens, tower_out_dim) buffer train_forward_backward leaves dL/d(tower_out) in"""
        _lib.check(self.lib.fv_train_set_tower_grad(self.h, _ptr(buf)), "fv_train_set_tower_grad", self.h)

    def train_set_step_guard(self, guard) -> None:
        """bind (or, with None, unbind) a fastvla_hip.guard.StepGuard to train_forward_backward / train_lora_forward_backward: dL/dactions is multiplied by the
        guard's device delta, so every gradient carries train_loss_scale() * delta; the guarded adamw_step divides delta out again"""
        _lib.check(self.lib.fv_train_set_step_guard(self.h, guard.handle() if guard is not None else None), "fv_train_set_step_guard", self.h)

    def train_tower_backward(self, pix: torch.Tensor, d_tower_out: torch.Tensor, tws: torch.Tensor, flat_grads: torch.Tensor, bucket_cb=None) -> None:
        """the tower's backward from dL/d(tower_out) (fp16, loss-scaled): its gradients into flat_grads at their train_layout() offsets"""
        B = pix.shape[0]
        fn, err = _bucket_trampoline(bucket_cb)
        p, n = self._aligned(tws)
        rc = self.lib.fv_train_tower_backward(self.h, pix.data_ptr(), d_tower_out.data_ptr(), B, p, n, flat_grads.data_ptr(), fn, None, _stream())
        if "exc" in err:
            raise err["exc"]
        _lib.check(rc, "fv_train_tower_backward", self.h)

    def train_tower_unit(self, unit: int, x_in: torch.Tensor, g_out: torch.Tensor, tws: torch.Tensor, flat_grads: torch.Tensor, gscale: float = 1.0):
        """ONE tower unit, teacher-forced (parity tests): x_in bf16 NHWC (stem: pixels), g_out fp32 NHWC = dL/d(output).
        -> (y bf16 NHWC, g_in fp32 NHWC or None for the stem); the unit's weight gradients x gscale land in flat_grads."""
        B = x_in.shape[0]
        units = self.tower_units()
        t = self.model.tower
        if unit == len(units):
            side, ch = t.tokens_side, t.out_dim
        else:
            side, ch = units[unit][2], units[unit][3]
        y = torch.empty(B, side, side, ch, dtype=torch.bfloat16, device=self.device)
        g_in = None if unit == 0 else torch.empty(tuple(x_in.shape), dtype=torch.float32, device=self.device)
        g_out = g_out.to(device=self.device, dtype=torch.float32).contiguous()
        assert g_out.numel() == y.numel(), (tuple(g_out.shape), tuple(y.shape))
        p, n = self._aligned(tws)
        _lib.check(self.lib.fv_train_tower_unit(self.h, unit, x_in.contiguous().data_ptr(), g_out.data_ptr(), float(gscale), B, p, n, y.data_ptr(), _ptr(g_in),
                                                flat_grads.data_ptr(), _stream()), "fv_train_tower_unit", self.h)
        return y, g_in

    # ---------------------------------------------------------------- RCCL without torch in between (fv_comm_*)
    def comm_unique_id(self) -> bytes:
        rid = _lib.RcclId()
        _lib.check(self.lib.fv_comm_unique_id(self.h, C.byref(rid)), "fv_comm_unique_id", self.h)
        return C.string_at(C.addressof(rid), 128)

    def comm_init(self, uid: bytes, rank: int, world: int) -> int:
        rid = _lib.RcclId()
        C.memmove(C.addressof(rid), uid, 128)
        comm = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fv_comm_init(self.h, C.byref(rid), rank, world, C.byref(comm)), "fv_comm_init", self.h)
        return comm.value

    def comm_destroy(self, comm: int) -> None:
        _lib.check(self.lib.fv_comm_destroy(self.h, comm), "fv_comm_destroy", self.h)

    def allreduce_grads(self, comm: int, flat_grads: torch.Tensor) -> None:
        """one in-place sum all-reduce of the flat head gradient on the CURRENT torch stream (ncclAllReduce over xGMI)."""
        _lib.check(self.lib.fv_allreduce_grads(self.h, comm, flat_grads.data_ptr(), flat_grads.numel(), _stream()),
                   "fv_allreduce_grads", self.h)

    # ---------------------------------------------------------------- profiling (bench.py)
    def profile(self, enable: bool) -> None:
        _lib.check(self.lib.fv_profile(self.h, int(enable)), "fv_profile")

    def profile_read(self):
        """-> (families: name -> dict(ms, flops, bytes, launches), gemm shapes: list of dicts).  Synchronises."""
        fam = (_lib.ProfileEntry * len(_lib.FAMILIES))()
        gem = (_lib.GemmProfile * 128)()
        n = C.c_int()
        _lib.check(self.lib.fv_profile_read(self.h, fam, gem, 128, C.byref(n)), "fv_profile_read")
        fams = {name: dict(ms=fam[i].ms, flops=fam[i].flops, bytes=fam[i].bytes, launches=fam[i].launches)
                for i, name in enumerate(_lib.FAMILIES)}
        shapes = [dict(m=gem[i].m, n=gem[i].n, k=gem[i].k, epi=gem[i].epi, ms=gem[i].ms, launches=gem[i].launches)
                  for i in range(n.value)]
        return fams, shapes

    def adamw_groups(self, groups, n: int) -> "AdamWGroups":
        """The device table of a parameter-group list (fv_adamw_groups_create): groups = dicts (or tuples) of begin, end, lr_scale, weight_decay, frozen that
        tile [0, n) on multiples of 4 floats -- fastvla_hip.optim.build_param_groups makes them from a layout.  The returned object destroys its table
        (close(), or when it is collected); pass it as adamw_step(..., groups=)."""
        t = AdamWGroups(self, groups, n)
        self.__dict__.setdefault("_group_tables", weakref.WeakSet()).add(t)
        return t

    def adamw_step(self, flat_params, flat_grads, m, v, step: int, *, lr: float, betas=(0.9, 0.95), eps: float = 1e-8,
                   weight_decay: float = 1e-4, max_grad_norm: float = 1.0, grad_scale: float = 1.0,
                   grad_norm_out: Optional[torch.Tensor] = None, groups: Optional["AdamWGroups"] = None,
                   group_norms_out: Optional[torch.Tensor] = None, ema: Optional[torch.Tensor] = None, ema_weight: Optional[float] = None,
                   guard=None) -> None:
        """fused clip + AdamW on the flat buffers.  groups=None: fv_adamw_clip_step, one learning rate and one decay for the whole buffer.  With a table from
        adamw_groups(): fv_adamw_clip_step_groups -- lr and decay per group (`weight_decay` here is then ignored: the table carries the decays), frozen groups
        untouched, group_norms_out (n_groups f32, device) <- every group's gradient norm.  With ema= (a float32 buffer shaped like flat_params) and
        ema_weight = 1 - decay (fastvla_hip.ema.ema_weight): fv_adamw_clip_step_ema, the same step on either path and ema <- ema + ema_weight (p_new - ema) in
        the same pass.  With guard= (a fastvla_hip.guard.StepGuard): fv_adamw_clip_step_guarded on whichever of the four paths the other arguments name -- the
        step is skipped on the device when the gradient is non-finite or the guard's saturation flag is set, and the guard's delta is divided out of an
        applied one.  `step` stays the caller's count and advances on a skipped step too."""
        hp = _lib.AdamWHParams(lr, betas[0], betas[1], eps, weight_decay, max_grad_norm if max_grad_norm else 0.0,
                               grad_scale)
        if ema is not None or guard is not None:
            if ema is not None and ema_weight is None:
                raise ValueError("ema= needs ema_weight=")
            if ema is None and ema_weight is not None:
                raise ValueError("ema_weight= needs ema=")
            if ema is not None and (ema.dtype != torch.float32 or ema.numel() != flat_params.numel() or ema.device != flat_params.device or not ema.is_contiguous()):
                raise ValueError("ema must be a contiguous float32 buffer of flat_params' size on its device")
            if groups is None and group_norms_out is not None:
                raise ValueError("group_norms_out needs groups=")
            if groups is not None and group_norms_out is not None and (group_norms_out.dtype != torch.float32 or group_norms_out.numel() < groups.n_groups):
                raise ValueError(f"group_norms_out must hold {groups.n_groups} float32 values")
        if guard is not None:
            _lib.check(self.lib.fv_adamw_clip_step_guarded(self.h, flat_params.data_ptr(), flat_grads.data_ptr(), m.data_ptr(), v.data_ptr(), _ptr(ema),
                                                           float(ema_weight) if ema is not None else 0.0, flat_params.numel(), C.byref(hp),
                                                           groups.handle() if groups is not None else None, step, guard.handle(), _ptr(grad_norm_out),
                                                           _ptr(group_norms_out), _stream()), "fv_adamw_clip_step_guarded", self.h)
            return
        if ema is not None:
            _lib.check(self.lib.fv_adamw_clip_step_ema(self.h, flat_params.data_ptr(), flat_grads.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr(),
                                                       float(ema_weight), flat_params.numel(), C.byref(hp), groups.handle() if groups is not None else None,
                                                       step, _ptr(grad_norm_out), _ptr(group_norms_out), _stream()), "fv_adamw_clip_step_ema", self.h)
            return
        if ema_weight is not None:
            raise ValueError("ema_weight= needs ema=")
        if groups is not None:
            if group_norms_out is not None and (group_norms_out.dtype != torch.float32 or group_norms_out.numel() < groups.n_groups):
                raise ValueError(f"group_norms_out must hold {groups.n_groups} float32 values")
            _lib.check(self.lib.fv_adamw_clip_step_groups(self.h, flat_params.data_ptr(), flat_grads.data_ptr(), m.data_ptr(), v.data_ptr(), flat_params.numel(),
                                                          C.byref(hp), groups.handle(), step, _ptr(grad_norm_out), _ptr(group_norms_out), _stream()),
                       "fv_adamw_clip_step_groups", self.h)
            return
        if group_norms_out is not None:
            raise ValueError("group_norms_out needs groups=")
        _lib.check(self.lib.fv_adamw_clip_step(self.h, flat_params.data_ptr(), flat_grads.data_ptr(), m.data_ptr(),
                                               v.data_ptr(), flat_params.numel(), C.byref(hp), step,
                                               _ptr(grad_norm_out), _stream()), "fv_adamw_clip_step")
