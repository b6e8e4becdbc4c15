"""Step rate of a batch with hyperparameter groups (runtime.Batch hparam_groups): c3 (64 switches / 32 trains),
65,536 envs, ungrouped, with 16 groups and with 256 groups (env e in group e % n: the envs of a wavefront are in
different groups), and with 16 groups that all hold the ungrouped schedule -- the grouped kernel on the ungrouped
workload, which separates the kernel's cost from the other schedules' other mix of decisions.  Not part of bench.py:
reported, not gated.

Per configuration: WARMUP steps of DECISIONS decisions per env, then STEPS timed ones; the rate is the timed steps'
decisions over their wall time (sfl_step returns after the device finished), the kernel rate over the HIP events'
kernel time, ROUNDS times per configuration.  Writes
profiles/[<tag>_]hpg_rate.json with the rates and the library's build id.

Usage: python scripts/hpg_rate.py [--tag TAG] [--envs N] [--out FILE]"""
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


def groups(n):
    """n schedules around HP (lr_decay stays 1.0: a decaying lr past the table stops the launch)."""
    return [dict(HP, epsilon=0.2 + 0.6 * g / n, epsilon_decay_rate=0.999 + 0.0009 * (g % 7) / 7, lr=0.05 + 0.4 * (g % 16) / 16)
            for g in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="", help="prefix of the output file's name")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mapgen = importlib.import_module(PKG + ".mapgen")
    comp = importlib.import_module(PKG + ".compiler")
    runtime = importlib.import_module(PKG + ".runtime")
    lib = importlib.import_module(PKG + "._lib").load_product()  # (raises without a GPU: no fallback)
    cm = comp.compile_scenario(mapgen.make_config("c3"))
    seeds = [1000 + e for e in range(a.envs)]
    # one batch at a time (a c3 env's Q-table is 1.5 MB: 65,536 envs are 103 GB of the 288 GB HBM); the ungrouped
    # batch runs again at the end, so that drift of the box over the run shows
    wall, kern, variant = {}, {}, None
    for name, n, same in (("ungrouped", 0, False), ("groups_16", 16, False), ("groups_256", 256, False),
                          ("groups_16_same_schedule", 16, True), ("ungrouped_again", 0, False)):
        kw = dict(hparam_groups=[dict(HP)] * n if same else groups(n), env_group=[e % n for e in range(a.envs)]) if n else {}
        b = runtime.Batch(cm, HP, seeds, lib=lib, ntab=NTAB, **kw)
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
    res = dict(config="c3", envs=a.envs, decisions_per_step=DECISIONS, warmup_steps=WARMUP, timed_steps=STEPS, rounds=ROUNDS,
               ntab=NTAB, kernel_variant=variant, build_id=lib.build_id, unit="agent-env-steps/s",
               rates={n: dict(median=statistics.median(wall[n]), runs=wall[n], kernel_median=statistics.median(kern[n]),
                              kernel_runs=kern[n]) for n in wall})
    out = a.out or os.path.join(REPO, "profiles", (a.tag + "_" if a.tag else "") + "hpg_rate.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
