"""The bits the flow head's noising step and its three samplers put out, as one sha256 per leg -- for comparing two builds of the library:
    python tools/flow_digest.py [--parent-checkout DIR] [--timeout 300] [--out FILE.json]
Every checkout (this one, then --parent-checkout: the root of a BUILT checkout of the parent commit) runs in a fresh process of its own, one after the
other, each under --timeout seconds; the inputs are this checkout's tests/ cases in both, the package and the library are the checkout's own.  Only
entry points that the parent has are called.  Legs (each digest runs over the raw bytes of every output of the leg, in the order below):
prepare    = head_flow_prepare on head `awkward` and `larger`, B = 9: plain and prefix mode x S = 1, 2 draws x uniform and logit-normal t; within a leg
             drawn noise / t / delays, then explicit ones (u and the whole zero-initialised `saved`: x_t, phi(t), the mask columns and bytes)
samplers   = plain (on a plain and on a prefix-width handle), prefix, guided x euler, midpoint, heun, rk4 x heads `awkward`, `larger` x B = 1, 9; within
             a leg steps 1 and 4 x folded statistics off and on x drawn and explicit noise x (prefix, guided) shift 0 and 2, the prefix sampler with
             flow_solver_util.mixed_delays (actions, then chunk_out)
`identical` says whether every leg of the two builds agrees; written to profiles/flow_digest.json unless --out names another file."""
import argparse
import hashlib
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADS, BATCHES, STEPS, SHIFTS = ("awkward", "larger"), (1, 9), (1, 4), (0, 2)
SOLVERS = ("euler", "midpoint", "heun", "rk4")
SEED, OFFSET = 1234, (3 << 40) + 17


def worker(checkout: Path) -> dict:
    for p in (str(ROOT / "tests"), str(checkout), str(checkout / "vla-from-fastvlm_amd")):
        sys.path.insert(0, p)
    import torch
    import fastvla_hip
    import flow_prefix_util as pu
    import flow_solver_util as su
    import flow_util as fu
    import rtc_util as ru
    from fastvla_hip import FastVLAEngine, arch
    from fastvla_hip.rtc import prefix_weights
    dev = torch.device("cuda", 0)
    legs = {}

    def engine(name, B, *, D=None, weights=None, draws=1, time_dist="uniform", rows=False):
        feat, ds, hid, fus, K, A, E = fu.DIMS[name]
        m = arch.ModelConfig("h", arch.LLMConfig(hidden=feat, layers=1, heads=1, kv_heads=1, head_dim=32, inter=8, vocab=8),
                             arch.TowerConfig(layers=(1, 1, 1, 1, 1), dims=(32, 64, 128, 256, 512), image_size=64))
        eng = FastVLAEngine(m, state_dim=ds, action_dim=K * A, hidden_dim=hid, fusion_dim=fus, max_batch=B)
        eng.set_head_flow(E, time_dist=time_dist, dist_a=-0.3, dist_b=1.2)
        if D is not None:
            eng.set_head_flow_prefix(K, D)
        if draws > 1:
            eng.set_head_flow_draws(draws)
        if weights is not None:
            eng.set_head_flow_guidance(weights, ru.BETA)
        if rows:
            eng.set_head_flow_solver("rk4")      # reserves the two rows; every leg names its own solver
        return eng

    def flat_of(eng, p):
        flat = torch.zeros(eng.head_numel(), device=dev)
        for k, v in eng.head_views(flat).items():
            v.copy_(p[k])
        return flat

    def add(h, *outs):
        torch.cuda.synchronize()
        for o in outs:
            h.update(o.detach().cpu().contiguous().numpy().tobytes())

    # ---- the noising step
    B = 9
    for name in HEADS:
        c = pu.prefix_case(name, B)
        K, A = c["dims"][4], c["dims"][5]
        for mode in ("plain", "prefix"):
            for S in (1, 2):
                for dist in ("uniform", "logit_normal"):
                    eng = engine(name, B, D=c["D"] if mode == "prefix" else None, draws=S, time_dist=dist)
                    g = torch.Generator().manual_seed(99)
                    noise, t = torch.randn(S * B, K * A, generator=g), torch.rand(S * B, generator=g)
                    delays = torch.from_numpy(su.mixed_delays(S * B, c["D"] + 1))      # (one value above max_delay: clamped)
                    h = hashlib.sha256()
                    for kw in (dict(seed=SEED, offset=OFFSET), dict(noise=noise, t=t, **(dict(delays=delays) if mode == "prefix" else {}))):
                        saved = eng.head_saved(B).zero_()
                        add(h, eng.head_flow_prepare(c["prev"], saved, **kw), saved)
                    legs[f"prepare {mode} {name} S={S} {dist}"] = h.hexdigest()
                    eng.close()

    # ---- the samplers
    for name in HEADS:
        for B in BATCHES:
            c, pc = ru.rtc_case(name, B), su.prefix_case(name, B)
            K = c["dims"][4]
            w = prefix_weights(K, max(1, K // 3), max(1, K // 3) + 1, "exp")
            plain_eng, prefix_eng = engine(name, B, weights=w, rows=True), engine(name, B, D=pc["D"], rows=True)
            flats = {id(plain_eng): flat_of(plain_eng, c["p"]), id(prefix_eng): flat_of(prefix_eng, pc["p"])}
            pooled, states, prev = c["pooled"].to(dev), c["states"].to(dev), c["prev"].to(dev)
            delays = torch.from_numpy(pc["delays"]).to(dev)
            st = c["stats"]
            calls = {
                "plain": (plain_eng, lambda e, f, kw: [(e.head_flow_sample(f, pooled, states, **kw),)]),
                "plain on a prefix-width head": (prefix_eng, lambda e, f, kw: [(e.head_flow_sample(f, pooled, states, **kw),)]),
                "prefix": (prefix_eng, lambda e, f, kw: [e.head_flow_sample_prefix(f, pooled, states, prev, delays, shift=sh, **kw) for sh in SHIFTS]),
                "guided": (plain_eng, lambda e, f, kw: [e.head_flow_sample_guided(f, pooled, states, prev, shift=sh, **kw) for sh in SHIFTS]),
            }
            for sampler, (eng, fn) in calls.items():
                for solver in SOLVERS:
                    eng.set_head_flow_solver(solver)
                    h = hashlib.sha256()
                    for N in STEPS:
                        for io in (False, True):
                            eng.set_io_norm(*((st["state_mean"], st["state_std"], st["action_mean"], st["action_std"]) if io else ()))
                            for kw in (dict(seed=SEED, offset=OFFSET), dict(noise=c["noise"])):
                                for outs in fn(eng, flats[id(eng)], dict(steps=N, **kw)):
                                    add(h, *outs)
                    legs[f"{sampler} {solver} {name} B={B}"] = h.hexdigest()
            plain_eng.close(), prefix_eng.close()
    return {"library": str(Path(fastvla_hip.library_path()).resolve().relative_to(checkout.resolve())), "legs": legs}


def run(checkout: Path, timeout: int) -> dict:
    out = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--worker", str(checkout)], check=True, capture_output=True, text=True, timeout=timeout)
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-checkout", default=None, help="root of a built checkout of the parent commit")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each checkout's process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print(json.dumps(worker(Path(args.worker).resolve())))
        return
    res = {"this_build": run(ROOT, args.timeout)}
    if args.parent_checkout:
        res["parent_build"] = run(Path(args.parent_checkout).resolve(), args.timeout)
        a, b = res["this_build"]["legs"], res["parent_build"]["legs"]
        res["differing_legs"] = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        res["identical"] = not res["differing_legs"]
    print(json.dumps(res))
    out = Path(args.out) if args.out else ROOT / "profiles" / "flow_digest.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    if args.parent_checkout and not res["identical"]:
        raise SystemExit(f"{len(res['differing_legs'])} legs differ between the two builds")


if __name__ == "__main__":
    main()
