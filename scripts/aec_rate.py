"""Decision rate of external-action mode with the policy on the host and on the device: c3 (64 switches / 32 trains)
at 4,096 and 65,536 envs, a policy that draws a uniformly random allowed action per env, timed through

  host    AECBatch.step(): numpy arrays out, the policy in numpy, the actions uploaded (sfl_env_step)
  device  AECBatch.step_torch(): tensors on the GPU, torch.multinomial(mask.float(), 1), nothing through the host
          (sfl_env_step_dev)

The two paths alternate in one process, on one batch (ROUNDS windows each per size); a window is warmed up, lasts at least
SECONDS, and ends in sync() (device) or with the last call's own synchronisation (host).  Decisions are the actions
applied, counted as (step_now >= 0).sum() -- on the device for the device path.  Prints one JSON line and writes
profiles/[<tag>_]aec_device_io.json.  Needs a GPU: there is no CPU fallback.  Not part of bench.py: reported, not
gated.

--kernel lane|wave|both selects the env step's kernel (AECBatch(kernel=...): the lane-per-env body or the wave kernel of
the handle's shape, sfl_env_begin_wave; default: SFL_ENV_KERNEL or lane).  With both, a lane batch and a wave batch of the
same seeds alternate in the same windows (lane host, lane device, wave host, wave device, ...), the result holds the two
kernels side by side with wave / lane ratios, and the file is profiles/[<tag>_]aec_wave_rate.json.

Usage: python scripts/aec_rate.py [--tag TAG] [--config c3] [--envs 4096,65536] [--seconds S] [--rounds N] [--out FILE]
       [--only host|device] (one path alone, e.g. under a kernel trace) [--kernel lane|wave|both]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "network-distributed-q-learning_amd"
WARMUP = 20


def host_window(b, out, rng, seconds, calls=None):
    """Calls of step() for `seconds` (or exactly `calls`); returns (decisions, calls, wall seconds, last outputs)."""
    na = np.asarray(b.cm.n_actions, np.int64)
    bits = np.arange(int(na.max()))
    dec = n = 0
    t0 = time.perf_counter()
    while (n < calls) if calls else (time.perf_counter() - t0 < seconds):
        ag = out["agent"]
        m = ((out["mask"].astype(np.int64)[:, None] >> bits) & 1).astype(np.float64)
        m[ag < 0, 0] = 1.0  # (an ended env: any column, its action is -1 below)
        # a uniformly random allowed action: the first column whose cumulative count passes u * (allowed count)
        c = m.cumsum(axis=1)
        a = (c > rng.random(len(ag))[:, None] * c[:, -1:]).argmax(axis=1)
        out = b.step(np.where(ag < 0, -1, a))
        dec += int((out["step_now"] >= 0).sum())
        n += 1
    return dec, n, time.perf_counter() - t0, out


def device_window(b, out, torch, seconds, calls=None):
    dec = torch.zeros((), dtype=torch.int64, device=out["obs"].device)
    n = 0
    t0 = time.perf_counter()
    while (n < calls) if calls else (time.perf_counter() - t0 < seconds):
        m = out["action_mask"].float()
        m[:, 0] += out["done"].float()  # (an ended env: a row multinomial accepts, its action is -1 below)
        a = torch.multinomial(m, 1).squeeze(1).to(torch.int32)
        out = b.step_torch(torch.where(out["done"] != 0, torch.full_like(a, -1), a))
        dec += (out["step_now"] >= 0).sum()
        n += 1
    b.sync()
    return int(dec), n, time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["host", "device"], default=None)
    ap.add_argument("--kernel", choices=["lane", "wave", "both"], default=None)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    mapgen = importlib.import_module(PKG + ".mapgen")
    comp = importlib.import_module(PKG + ".compiler")
    aec = importlib.import_module(PKG + ".aec")
    lib = importlib.import_module(PKG + "._lib").load_product()  # (raises without a GPU: no fallback)
    cm = comp.compile_scenario(mapgen.make_config(a.config))
    kernels = ["lane", "wave"] if a.kernel == "both" else [a.kernel]  # (None: AECBatch's default)
    sizes = {}
    for E in [int(x) for x in a.envs.split(",")]:
        seeds = [1000 + e for e in range(E)]
        rng = np.random.default_rng(E)
        torch.manual_seed(E)
        # one batch per kernel serves both paths (the two calls mix on one handle), window by window: a c3 env
        # carries its 1.5 MB Q-table allocation, so 65,536 envs are 103 GB of HBM per batch.  Each window starts
        # from a call without actions, which re-emits the pending observations on its side (host arrays / device
        # tensors).
        bs = {k: aec.AECBatch(cm, seeds, lib=lib, kernel=k) for k in kernels}
        for b in bs.values():
            if a.only != "device":
                host_window(b, b.step(None), rng, 0, calls=WARMUP)
            if a.only != "host":
                device_window(b, b.step_torch(None), torch, 0, calls=WARMUP)
        runs = {k: {"host": [], "device": []} for k in kernels}
        calls = {k: {"host": [], "device": []} for k in kernels}
        for _ in range(a.rounds):
            for k, b in bs.items():
                if a.only != "device":
                    d, n, t, _o = host_window(b, b.step(None), rng, a.seconds)
                    runs[k]["host"].append(d / t)
                    calls[k]["host"].append(n / t)
                if a.only != "host":
                    d, n, t, _o = device_window(b, b.step_torch(None), torch, a.seconds)
                    runs[k]["device"].append(d / t)
                    calls[k]["device"].append(n / t)
        per = {}
        for k, b in bs.items():
            res = {p: dict(median=statistics.median(runs[k][p]), min=min(runs[k][p]), max=max(runs[k][p]), runs=runs[k][p],
                           calls_per_s=statistics.median(calls[k][p])) for p in runs[k] if runs[k][p]}
            if "host" in res and "device" in res:
                res["device_over_host"] = res["device"]["median"] / res["host"]["median"]
            cn = b.batch.counters()
            res["kernel"] = dict(selected=b.kernel, kernel_variant=cn["kernel_variant"], group_lanes=cn["group_lanes"])
            per[k] = res
            b.close()
        if a.kernel == "both":
            per["wave_over_lane"] = {p: per["wave"][p]["median"] / per["lane"][p]["median"] for p in ("host", "device")
                                     if p in per["wave"]}
            sizes[str(E)] = per
        else:
            sizes[str(E)] = per[kernels[0]]
    out = dict(config=a.config, policy="uniformly random allowed action", window_seconds=a.seconds, rounds=a.rounds,
               warmup_calls=WARMUP, unit="decisions/s (actions applied, all envs)", build_id=lib.build_id,
               device=torch.cuda.get_device_name(0), envs=sizes)
    name = "aec_wave_rate.json" if a.kernel == "both" else "aec_device_io.json"
    path = a.out or os.path.join(REPO, "profiles", (a.tag + "_" if a.tag else "") + name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
