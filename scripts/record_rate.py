"""What recording episodes of a policy-bank evaluation (runtime.EvalBatch.record, sfl_bank_record) costs.
Needs a GPU; not a test, not part of bench.py.  Writes profiles/[<tag>_]record_rate.json (or --out) and prints it as one
JSON line.

The setting is scripts/diag_rate.py's: --config (c3), bench.py's hyperparameters, one learner's table (a one-env
learn(--episodes), seed 450565), one policy, env e on seed 450565 + e.  Per size of --envs (16,384 and 65,536), after a
warm-up of every handle:
  (i)   unarmed    the episode launch's kernel ms (the launch's HIP events) with no recording armed, --repeats times, on
                   this build and -- with --parent-lib, a libsfl.so built from the parent commit -- on the parent's,
                   alternated launch by launch in one process; both means, both spreads (max / min of the repeats) and
                   whether this build's mean lies within the parent's measured range.  The two builds' outputs are
                   compared bit for bit first.
  (ii)  recorded   the same launch with the first 1, 64 and 4,096 envs (--record) recorded, the caps the largest tick and
                   decision counts of the batch (nothing is cut)
  (iii) traffic    sfl_bank_record_ms of a traffic fold behind each of those launches
(ii) and (iii) are reported, not gated.

Usage: python scripts/record_rate.py [--tag TAG] [--config c3] [--envs 16384,65536] [--record 1,64,4096] [--repeats 7]
                                     [--episodes 30] [--parent-lib PATH] [--out PATH] [--host]
--host rehearses the script's logic on the host build at whatever sizes are given (its times are not measurements)."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "network-distributed-q-learning_amd"
HP = dict(gamma=1.0, epsilon=0.5, epsilon_decay_rate=0.9997, lr=0.1, lr_decay_rate=1.0, default_q=0.0)  # bench.py's
OUT_KEYS = ("cum_reward", "arrived", "num_malfunctions", "decisions", "ticks", "delays", "truncated", "at_dest")


def spread(xs):
    return dict(all=xs, mean=statistics.fmean(xs), median=statistics.median(xs), min=min(xs), max=max(xs),
                max_over_min=max(xs) / min(xs) if min(xs) > 0 else None)


def load_older(_lib, path):
    """A library of an older commit of the same ABI version: bound without the entry points it does not have."""
    dll = ctypes.CDLL(path)
    full = _lib.EXPORTS
    _lib.EXPORTS = {k: v for k, v in full.items() if hasattr(dll, k)}
    try:
        return _lib.Lib(path), sorted(set(full) - set(_lib.EXPORTS))
    finally:
        _lib.EXPORTS = full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--config", default="c3")
    ap.add_argument("--envs", default="16384,65536")
    ap.add_argument("--record", default="1,64,4096")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--episodes", type=int, default=30)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    build = importlib.import_module(PKG + ".build")
    mapgen = importlib.import_module(PKG + ".mapgen")
    comp = importlib.import_module(PKG + ".compiler")
    runtime = importlib.import_module(PKG + ".runtime")
    _lib = importlib.import_module(PKG + "._lib")
    if args.host:
        lib = _lib.Lib(build.build_hostsim())
        device = "host build (rehearsal: no time below is a measurement)"
    else:
        import torch
        lib = _lib.load_product()
        device = torch.cuda.get_device_name(0)
    parent, missing = load_older(_lib, args.parent_lib) if args.parent_lib else (None, [])
    cm = comp.compile_scenario(mapgen.make_config(args.config))
    one = runtime.Batch(cm, HP, [450565], lib=lib)
    one.learn(args.episodes)
    q, touched = one.q_raw(0)
    one.close()
    res = dict(build_id=build.product_build_id(), parent_build_id=parent.build_id if parent else None,
               parent_lacks=missing, device=device, hp=HP, config=args.config, trains=cm.T, cells=cm.H * cm.W,
               table="one env, learn(%d), seed 450565" % args.episodes, repeats=args.repeats, by_envs={})
    for E in [int(x) for x in args.envs.split(",")]:
        seeds = [450565 + e for e in range(E)]
        pol = np.zeros(E, np.int64)
        evs = {}
        try:
            for name, L in (("this", lib), ("parent", parent)):
                if L is not None:
                    evs[name] = runtime.EvalBatch(cm, HP, seeds, 1, lib=L)
                    evs[name].set_policy_raw(0, q, touched)
            outs = {name: ev.evaluate(pol) for name, ev in evs.items()}  # warm-up, and the outputs to compare
            same = None
            if parent is not None:
                same = all(np.array_equal(outs["this"][k].view(np.uint8), outs["parent"][k].view(np.uint8)) for k in OUT_KEYS)
            ms = {name: [] for name in evs}
            for _ in range(args.repeats):  # (i): alternated launch by launch
                for name in sorted(evs):
                    evs[name].evaluate(pol, per_env=False)
                    ms[name].append(evs[name].counters()["last_kernel_ms"])
            ev = evs["this"]
            c = ev.counters()
            r = dict(kernel_variant=int(c["kernel_variant"]), group_lanes=int(c["group_lanes"]),
                     decisions_per_launch=int(c["last_launch_decisions"]), ticks_per_launch=int(c["last_launch_ticks"]),
                     outputs_equal_parent=same, unarmed_ms={name: spread(v) for name, v in ms.items()})
            if parent is not None:
                a, b = r["unarmed_ms"]["this"], r["unarmed_ms"]["parent"]
                r["this_over_parent_mean"] = a["mean"] / b["mean"] if b["mean"] > 0 else None
                r["this_mean_within_parent_range"] = bool(a["mean"] <= b["max"])
            ticks, decs = int(outs["this"]["ticks"].max()), int(outs["this"]["decisions"].max())
            r["caps"] = dict(max_ticks=ticks, max_decisions=decs)
            r["recorded"] = {}
            for n in [int(x) for x in args.record.split(",")]:
                if n > E:
                    continue
                ev.record(list(range(n)), max_ticks=ticks, max_decisions=decs)
                ev.evaluate(pol, per_env=False)  # warm-up
                ev.traffic(0)
                ep, tr = [], []
                for _ in range(args.repeats):
                    ev.evaluate(pol, per_env=False)
                    ep.append(ev.counters()["last_kernel_ms"])
                    t = ev.traffic(0)
                    tr.append(ev.record_ms()[0])
                bytes_ = n * (ticks * cm.T * 8 + decs * 4 * len(_lib.REC_DEC_FIELDS))
                r["recorded"][str(n)] = dict(buffer_bytes=bytes_, episode_kernel_ms=spread(ep), traffic_ms=spread(tr),
                                             over_unarmed_mean=statistics.fmean(ep) / r["unarmed_ms"]["this"]["mean"]
                                             if r["unarmed_ms"]["this"]["mean"] > 0 else None,
                                             occupancy=int(t["occupancy"].sum()), standing=int(t["standing"].sum()),
                                             decisions=int(t["decisions"].sum()))
            ev.record(None)
            res["by_envs"][str(E)] = r
        finally:
            for x in evs.values():
                x.close()
    res["headline"] = "README's and DESIGN's headline rates stay bench.py's; (i) is the bar, (ii) and (iii) are reported"
    path = args.out or os.path.join(REPO, "profiles", (args.tag + "_" if args.tag else "") + "record_rate.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
