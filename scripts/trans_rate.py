"""Cost of the transition assembler (AECBatch.transitions_begin) on the device path of external-action
mode: c3 on the wave step kernel at 4,096 and 65,536 envs, the policy of scripts/aec_rate.py (a uniformly random allowed
action per env, torch.multinomial on the device), one batch per size, windows with the assembler off and on alternating
in one process (off, on, off, on, ...).  A window is warmed up, lasts at least SECONDS and ends in sync(); decisions are
the actions applied, counted on the device.  Reports decisions/s (median, min, max), the on / off ratio, rows emitted per
call and pending entries dropped.  On a tree without the assembler (the parent commit) only the off windows run: the
same script gives the baseline.

Kernel times come from a run of their own under the profiler, which this script only summarises:

    rocprofv3 --kernel-trace --stats -d DIR -o ktrace --output-format csv -- \\
        python scripts/trans_rate.py --only on --rounds 1 --envs 65536 --out DIR/rate.json
    python scripts/trans_rate.py --fold DIR/.../ktrace_kernel_stats.csv --into profiles/trans_rate.json

--fold adds each library kernel's calls and average time, the assembler's share of the library's kernel time per call
and of the process's, to the JSON.  Needs a GPU: there is no CPU fallback.  Not part of bench.py: reported, not gated.

Usage: python scripts/trans_rate.py [--tag TAG] [--envs 4096,65536] [--seconds S] [--rounds N] [--only off|on]
       [--capacity N] [--out FILE]"""
import argparse
import csv
import importlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "network-distributed-q-learning_amd"
WARMUP = 20
LIB_KERNELS = ("k_wave", "k_run_ext", "k_env_encode", "k_trans_count", "k_trans_write")


def window(b, out, torch, seconds, calls=None):
    """scripts/aec_rate.py's device_window."""
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


def fold(stats_csv, into):
    """rocprofv3's kernel stats (Name, Calls, TotalDurationNs, AverageNs, Percentage) into the result file."""
    rows = list(csv.DictReader(open(stats_csv)))
    res = json.load(open(into))
    tot_col = next(c for c in rows[0] if c.startswith("TotalDuration"))  # (nanoseconds; the name varies with the version)
    avg_col = next(c for c in rows[0] if c.startswith("Average"))
    for r in rows:
        r["TotalDurationNs"], r["AverageNs"] = r[tot_col], r[avg_col]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    ks = {}
    for r in rows:
        for k in LIB_KERNELS:
            if k in r["Name"] and "at::native" not in r["Name"]:
                key = "step kernel (" + r["Name"].split("(")[0].replace("void ", "") + ")" if k in ("k_wave", "k_run_ext") else k
                ks[key] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, total_ms=float(r["TotalDurationNs"]) / 1e6,
                               share_of_process_kernel_time=float(r["TotalDurationNs"]) / total)
    asm = sum(v["avg_us"] for k, v in ks.items() if k.startswith("k_trans"))
    step = sum(v["avg_us"] for k, v in ks.items() if k.startswith("step kernel"))
    enc = sum(v["avg_us"] for k, v in ks.items() if k == "k_env_encode")
    res["kernel_trace"] = dict(source=os.path.basename(stats_csv), kernels=ks, assembler_us_per_call=asm,
                               step_kernel_us_per_call=step, encode_us_per_call=enc,
                               assembler_over_step_kernel=asm / step if step else None,
                               assembler_share_of_library_kernel_time=asm / (asm + step + enc) if step else None,
                               assembler_share_of_process_kernel_time=sum(v["share_of_process_kernel_time"] for k, v in ks.items()
                                                                          if k.startswith("k_trans")))
    with open(into, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--envs", default="4096,65536")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["off", "on"], default=None)
    ap.add_argument("--capacity", type=int, default=None)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fold", default=None)
    ap.add_argument("--into", default=None)
    a = ap.parse_args()
    if a.fold:
        return fold(a.fold, a.into or os.path.join(REPO, "profiles", "trans_rate.json"))
    import torch
    mapgen = importlib.import_module(PKG + ".mapgen")
    comp = importlib.import_module(PKG + ".compiler")
    aec = importlib.import_module(PKG + ".aec")
    lib = importlib.import_module(PKG + "._lib").load_product()  # (raises without a GPU: no fallback)
    has = hasattr(aec.AECBatch, "transitions_begin")
    modes = [m for m in ("off", "on") if (a.only in (None, m)) and (m == "off" or has)]
    cm = comp.compile_scenario(mapgen.make_config(a.config))
    sizes = {}
    for E in [int(x) for x in a.envs.split(",")]:
        torch.manual_seed(E)
        b = aec.AECBatch(cm, [1000 + e for e in range(E)], lib=lib, kernel="wave")
        runs = {m: [] for m in modes}
        calls = {m: [] for m in modes}
        rows = dropped = ncalls = 0

        def one(m, seconds, n=None):
            nonlocal rows, dropped, ncalls
            ring = b.transitions_begin(capacity=a.capacity) if m == "on" else None
            r = window(b, b.step_torch(None), torch, seconds, calls=n)
            if ring is not None:
                if n is None:
                    rows += int(ring["total"].cpu()[0])
                    dropped += int(ring["dropped"].sum().cpu())
                    ncalls += r[1] + 1
                b.transitions_end()
            return r

        for m in modes:
            one(m, 0, n=WARMUP)
        for _ in range(a.rounds):
            for m in modes:
                d, n, t, _o = one(m, a.seconds)
                runs[m].append(d / t)
                calls[m].append(n / t)
        res = {m: dict(median=statistics.median(runs[m]), min=min(runs[m]), max=max(runs[m]), runs=runs[m],
                       calls_per_s=statistics.median(calls[m])) for m in modes}
        if "off" in res and "on" in res:
            res["on_over_off"] = res["on"]["median"] / res["off"]["median"]
            res["added_us_per_call"] = 1e6 / res["on"]["calls_per_s"] - 1e6 / res["off"]["calls_per_s"]
        if "on" in res:
            res["ring"] = dict(capacity=a.capacity or 2 * E, rows_per_call=rows / max(ncalls, 1), dropped=dropped)
        cn = b.batch.counters()
        res["kernel"] = dict(selected=b.kernel, kernel_variant=cn["kernel_variant"], group_lanes=cn["group_lanes"])
        sizes[str(E)] = res
        b.close()
    out = dict(config=a.config, policy="uniformly random allowed action", window_seconds=a.seconds, rounds=a.rounds,
               warmup_calls=WARMUP, unit="decisions/s (actions applied, all envs), device path (step_torch)",
               assembler="transitions_begin / transitions_end around each 'on' window" if has else "absent in this tree",
               build_id=lib.build_id, device=torch.cuda.get_device_name(0), envs=sizes)
    path = a.out or os.path.join(REPO, "profiles", (a.tag + "_" if a.tag else "") + "trans_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
