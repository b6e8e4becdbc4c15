"""What a step-mode learning curve (sfl_curve_*, csrc/sfl_curve.hip) costs: the step kernel with and without the
episode-end rows going to the handle's ring, and the fold kernel's share of a step.  Needs a GPU; not a test, not part
of bench.py: reported, not gated -- the headline rates stay those with the curve off.  Writes
profiles/[<tag>_]curve_rate.json (or --out) and prints it as one JSON line.

setup    two batches A and B of the same config, envs and seeds in one process: learn_begin, apply_qinit, a warm-up
         step(--decisions) each.  They stay in lock step: every window runs on both, so both hold the same state.
windows  a window is --launches launches of step(--decisions).  Each of --rounds rounds runs four windows: A with the
         curve off, B with a curve of one series (ring --ring), A off again, B with a curve of 256 series (e % 256).
output   per arm: the step kernel ms of every launch and their median, the fold kernel ms of every launch, the
         episodes folded and lost per launch; on / off of the step kernel's medians (each on window against the off
         window before it), and the fold's share of a step (fold ms / step ms).

Usage: python scripts/curve_rate.py [--tag TAG] [--config c3] [--envs 65536] [--decisions 1024] [--ring 16]
                                    [--launches 2] [--rounds 3] [--out PATH]"""
import argparse
import importlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "network-distributed-q-learning_amd"
HP = dict(gamma=1.0, epsilon=0.5, epsilon_decay_rate=0.9997, lr=0.1, lr_decay_rate=1.0, default_q=0.0)  # bench.py's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--config", default="c3")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--decisions", type=int, default=1024)
    ap.add_argument("--ring", type=int, default=16)
    ap.add_argument("--launches", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    build = importlib.import_module(PKG + ".build")
    mapgen = importlib.import_module(PKG + ".mapgen")
    comp = importlib.import_module(PKG + ".compiler")
    runtime = importlib.import_module(PKG + ".runtime")
    _lib = importlib.import_module(PKG + "._lib")
    lib = _lib.load_product()
    E, D = args.envs, args.decisions
    cm = comp.compile_scenario(mapgen.make_config(args.config))
    seeds = [450565 + e for e in range(E)]
    batches = []
    for _ in range(2):
        b = runtime.Batch(cm, HP, seeds, lib=lib)
        b.learn_begin()
        b.apply_qinit()
        b.step(D)
        batches.append(b)
    A, B = batches
    res = dict(build_id=build.product_build_id(), device=torch.cuda.get_device_name(0), hp=HP, config=args.config, envs=E,
               trains=cm.T, decisions_per_launch=D, ring=args.ring, launches_per_window=args.launches, rounds=args.rounds,
               kernel_variant=A.counters()["kernel_variant"], ring_bytes=args.ring * E * (24 + 4 * cm.T))
    arms = {k: dict(step_ms=[], fold_ms=[], folded=[], lost=[], window_step_ms=[]) for k in ("off", "one_series", "series_256")}
    ratios = dict(one_series=[], series_256=[])

    def window(b, arm):
        acc, ms_all = arms[arm], []
        for _ in range(args.launches):
            before = b.curve() if arm != "off" else None
            ms = b.step(D)[1]
            ms_all.append(ms)
            acc["step_ms"].append(ms)
            if before is not None:
                after = b.curve()
                acc["fold_ms"].append(b.curve_fold_ms()[0])
                acc["folded"].append(int(after["count"].sum() - before["count"].sum()))
                acc["lost"].append(int(after["lost"].sum() - before["lost"].sum()))
        acc["window_step_ms"].append(statistics.median(ms_all))
        return acc["window_step_ms"][-1]

    import warnings
    warnings.simplefilter("ignore", RuntimeWarning)  # (a ring below decisions + 1: lost episodes are reported)
    for _ in range(args.rounds):
        for arm, series, ns in (("one_series", None, 1), ("series_256", [e % 256 for e in range(E)], 256)):
            off = window(A, "off")
            B.curve_begin(1 << 20, 1, series, ns, args.ring)
            on = window(B, arm)
            ratios[arm].append(on / off if off > 0 else float("nan"))
            B.curve_end()
    for k, acc in arms.items():
        acc["step_ms_median"] = statistics.median(acc["step_ms"])
        if acc["fold_ms"]:
            acc["fold_ms_median"] = statistics.median(acc["fold_ms"])
            acc["fold_share_of_step"] = acc["fold_ms_median"] / acc["step_ms_median"]
            acc["step_on_over_off"] = statistics.median(ratios[k])
            acc["step_on_over_off_all"] = ratios[k]
    res["arms"] = arms
    res["headline"] = "rates are reported with the curve off; this file is the curve's cost, not gated"
    A.close()
    B.close()
    path = args.out or os.path.join(REPO, "profiles", (args.tag + "_" if args.tag else "") + "curve_rate.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
