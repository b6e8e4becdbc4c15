"""What a policy-bank evaluation (runtime.EvalBatch, sfl_bank_eval) costs beside the path it replaces.
Needs a GPU; not a test, not part of bench.py: reported, not gated.  Writes profiles/[<tag>_]eval_bank_rate.json (or --out)
and prints it as one JSON line.

table    one learner's table: a one-env learn(--episodes) on --config with bench.py's hyperparameters.
same     --envs-same envs (16,384), one table, the same seeds on both sides, alternating, --repeats times after a warm-up:
         (i) the parent's path, Batch.test(1) with a private copy of the table in every env (sfl_set_q per env, timed):
             kernel ms per greedy decision (last_kernel_ms / last_launch_decisions) of every repeat;
         (ii) EvalBatch.evaluate on the same table: the same figure; and the ratio (ii) / (i) of the medians, beside
             (i)'s own spread (max / min of its repeats).  test() launches the phase-timed instantiation of the learn
             kernel (TIMED), evaluate() the BANK instantiation: the two are not the same instantiation, and the
             comparison is of the two paths a user has, not of two builds of one kernel.  The outputs of the two sides
             (cum_reward, arrived, decisions, ticks, delays) are compared bit for bit in the same run.
large    --envs-large envs (65,536), which the parent's path cannot hold (103 GB of tables): P = 1, 16 and 1,024 tables
         with env_policy = e % P.  Per P: free device memory before and after the create, seconds to upload P tables
         from the host and to copy_policy them from a training Batch, then --repeats evaluations after a warm-up:
         greedy decisions per second (from the launch's HIP events) and the fold's ms.
kres     the Bank kernels' VGPRs / SGPRs / LDS beside their Plain twins are in profiles/eval_bank_kres.txt
         (scripts/kres_diff.py; no GPU needed).

Usage: python scripts/eval_rate.py [--tag TAG] [--config c3] [--envs-same 16384] [--envs-large 65536]
                                   [--policies 1,16,1024] [--repeats 5] [--episodes 30] [--out PATH] [--host]
--host rehearses the script's logic on the host build at whatever sizes are given (its times are not measurements)."""
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
HP = dict(gamma=1.0, epsilon=0.5, epsilon_decay_rate=0.9997, lr=0.1, lr_decay_rate=1.0, default_q=0.0)  # bench.py's
KEYS = ("cum_reward", "arrived", "num_malfunctions", "decisions", "ticks", "delays")


def spread(xs):
    return dict(all=xs, median=statistics.median(xs), min=min(xs), max=max(xs), max_over_min=max(xs) / min(xs) if min(xs) > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--config", default="c3")
    ap.add_argument("--envs-same", type=int, default=16384)
    ap.add_argument("--envs-large", type=int, default=65536)
    ap.add_argument("--policies", default="1,16,1024")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--episodes", type=int, default=30)
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
        device, free = "host build (rehearsal: no time below is a measurement)", lambda: 0
    else:
        import torch
        lib = _lib.load_product()
        device = torch.cuda.get_device_name(0)

        def free():
            torch.cuda.synchronize()
            return int(torch.cuda.mem_get_info()[0])
    cm = comp.compile_scenario(mapgen.make_config(args.config))
    one = runtime.Batch(cm, HP, [450565], lib=lib)
    one.learn(args.episodes)
    q, touched = one.q_raw(0)
    res = dict(build_id=build.product_build_id(), device=device, hp=HP, config=args.config, trains=cm.T,
               q_bytes_per_table=int(cm.q_per_env * 8), table="one env, learn(%d), seed 450565" % args.episodes,
               repeats=args.repeats)

    # ---- the same work on both paths ----
    E = args.envs_same
    seeds = [450565 + e for e in range(E)]
    m0 = free()
    par = runtime.Batch(cm, HP, seeds, lib=lib)
    m1 = free()
    t0 = time.time()
    for e in range(E):
        par.set_q_raw(e, q, touched)
    t_load = time.time() - t0
    ev = runtime.EvalBatch(cm, HP, seeds, 1, lib=lib)
    m2 = free()
    ev.set_policy_raw(0, q, touched)
    ref, got = par.test(1), ev.evaluate()  # the warm-up of both, and the comparison of their outputs
    same = {k: bool(np.array_equal(np.ascontiguousarray(ref[k][0]).view(np.uint8), np.ascontiguousarray(got[k]).view(np.uint8)))
            for k in KEYS}
    a, b = [], []
    for _ in range(args.repeats):  # alternating
        par.test(1)
        c = par.counters()
        a.append(c["last_kernel_ms"] / c["last_launch_decisions"])
        ev.evaluate(per_env=False)
        c = ev.counters()
        b.append(c["last_kernel_ms"] / c["last_launch_decisions"])
        dec_ev, var_ev, ms_ev = int(c["last_launch_decisions"]), int(c["kernel_variant"]), c["last_kernel_ms"]
    res["same"] = dict(
        envs=E, decisions_per_launch=dec_ev, kernel_variant=var_ev, outputs_bit_equal=same,
        parent_test=dict(kernel_ms_per_decision=spread(a), instantiation="TIMED (learn kernel, run-time greedy mode)",
                         device_bytes_at_create=m0 - m1, seconds_to_load_tables=t_load),
        bank_eval=dict(kernel_ms_per_decision=spread(b), instantiation="BANK", device_bytes_at_create=m1 - m2,
                       last_kernel_ms=ms_ev, fold_ms=ev.fold_ms()[0]),
        ratio_bank_over_parent=statistics.median(b) / statistics.median(a) if not args.host else None,
        note="test() launches the TIMED instantiation, evaluate() the BANK one: not the same instantiation")
    par.close()
    ev.close()

    # ---- what the parent's path cannot hold ----
    E = args.envs_large
    seeds = [450565 + e for e in range(E)]
    res["large"] = dict(envs=E, parent_table_bytes=int(E * cm.q_per_env * 8), by_policies={})
    for P in [int(x) for x in args.policies.split(",")]:
        m0 = free()
        ev = runtime.EvalBatch(cm, HP, seeds, P, lib=lib)
        m1 = free()
        t0 = time.time()
        for p in range(P):
            ev.set_policy_raw(p, q, touched)
        t_up = time.time() - t0
        t0 = time.time()
        for p in range(P):
            ev.copy_policy(p, one, env=0)
        t_cp = time.time() - t0
        pol = np.arange(E) % P
        ev.evaluate(pol, per_env=False)  # warm-up
        rate, fold, ms = [], [], []
        for _ in range(args.repeats):
            out = ev.evaluate(pol, per_env=False)
            c = ev.counters()
            ms.append(c["last_kernel_ms"])
            rate.append(c["last_launch_decisions"] / (c["last_kernel_ms"] * 1e-3) if c["last_kernel_ms"] > 0 else 0.0)
            fold.append(ev.fold_ms()[0])
        t = out["table"]
        res["large"]["by_policies"][str(P)] = dict(
            free_before_create=m0, free_after_create=m1, device_bytes_at_create=m0 - m1, bank_bytes=int(P * cm.q_per_env * 8),
            seconds_to_upload_tables=t_up, seconds_to_copy_policy=t_cp, decisions_per_launch=int(c["last_launch_decisions"]),
            kernel_ms=spread(ms), greedy_decisions_per_second=spread(rate), fold_ms=spread(fold),
            episodes_min_max=[int(t["episodes"].min()), int(t["episodes"].max())],
            early_late_not_arrived_mean_policy0=[float(t["early_mean"][0]), float(t["late_mean"][0]), float(t["not_arrived_mean"][0])],
            truncated=int(t["truncated"].sum()))
        ev.close()
    one.close()
    res["headline"] = "README's and DESIGN's headline rates stay bench.py's; this file is the evaluation path's, not gated"
    path = args.out or os.path.join(REPO, "profiles", (args.tag + "_" if args.tag else "") + "eval_bank_rate.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
