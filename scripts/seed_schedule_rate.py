"""Step rate of a batch with a seed schedule (runtime.Batch seed_pool): c3 (64 switches / 32 trains), 65,536 envs,
step(1024), an unscheduled handle against pool 64 and pool 0 (a new scenario every episode) in one process; the
unscheduled batch runs again at the end, so that drift over the run shows.  c3 as bench.py builds it has no
malfunctions, so the draw's cost is the same in every configuration: what differs is the scheduled kernels' held seed
and its derivation at every reset.  --mf RATE,MIN,MAX gives the map malfunctions (then the scenarios differ too).
Not part of bench.py: reported, not gated.

Per configuration: WARMUP steps of DECISIONS decisions per env, then STEPS timed ones, ROUNDS times; the rate is the
timed steps' decisions over their wall time, the kernel rate over the HIP events' kernel time.  Writes
profiles/[<tag>_]seed_schedule_rate.json with the rates and the library's build id.

Usage: python scripts/seed_schedule_rate.py [--tag TAG] [--envs N] [--mf 0.01,5,15] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "network-distributed-q-learning_amd"
HP = dict(gamma=1.0, epsilon=0.5, epsilon_decay_rate=0.9997, lr=0.1, lr_decay_rate=1.0, default_q=0.0)
DECISIONS, WARMUP, STEPS, ROUNDS, NTAB = 1024, 2, 4, 3, 1 << 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="", help="prefix of the output file's name")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--mf", default=None, help="malfunction rate,min,max of the map (default: c3's own, none)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mapgen = importlib.import_module(PKG + ".mapgen")
    comp = importlib.import_module(PKG + ".compiler")
    runtime = importlib.import_module(PKG + ".runtime")
    lib = importlib.import_module(PKG + "._lib").load_product()  # (raises without a GPU: no fallback)
    mf = None
    if a.mf:
        r, lo, hi = a.mf.split(",")
        mf = (float(r), int(lo), int(hi))
    cm = comp.compile_scenario(mapgen.make_config("c3", malfunction=mf) if mf else mapgen.make_config("c3"))
    seeds = [1000 + e for e in range(a.envs)]
    wall, kern, variant = {}, {}, None
    for name, pool in (("unscheduled", None), ("pool_64", 64), ("pool_0", 0), ("unscheduled_again", None)):
        b = runtime.Batch(cm, HP, seeds, lib=lib, ntab=NTAB, **({} if pool is None else dict(seed_pool=pool)))
        b.learn_begin()
        b.apply_qinit()
        for _ in range(WARMUP):
            b.step(DECISIONS)
        variant = b.counters()["kernel_variant"]
        wall[name], kern[name] = [], []
        for _ in range(ROUNDS):
            dec, ms, t0 = 0, 0.0, time.perf_counter()
            for _ in range(STEPS):
                d, k = b.step(DECISIONS)
                dec += d
                ms += k
            wall[name].append(dec / (time.perf_counter() - t0))
            kern[name].append(dec / (ms * 1e-3) if ms > 0 else 0.0)
        b.close()
    res = dict(config="c3", malfunction=mf, envs=a.envs, decisions_per_step=DECISIONS, warmup_steps=WARMUP, timed_steps=STEPS,
               rounds=ROUNDS, ntab=NTAB, kernel_variant=variant, build_id=lib.build_id, unit="agent-env-steps/s",
               rates={n: dict(median=statistics.median(wall[n]), runs=wall[n], kernel_median=statistics.median(kern[n]),
                              kernel_runs=kern[n]) for n in wall})
    base = res["rates"]["unscheduled"]["kernel_median"]
    res["kernel_ratio_to_unscheduled"] = {n: (r["kernel_median"] / base if base else None) for n, r in res["rates"].items()}
    out = a.out or os.path.join(REPO, "profiles", (a.tag + "_" if a.tag else "") + "seed_schedule_rate.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(out=out, medians={n: r["median"] for n, r in res["rates"].items()},
                          kernel_ratio=res["kernel_ratio_to_unscheduled"])))


if __name__ == "__main__":
    main()
