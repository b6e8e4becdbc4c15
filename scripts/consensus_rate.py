"""Rate of the consensus kernels (sfl_consensus, csrc/sfl_consensus.hip) against a device-to-device copy of the same
bytes, its cost against a training step, and what sharing does to learning.  Needs a GPU; not a test, not part of
bench.py: reported, not gated.  Writes profiles/[<tag>_]consensus_rate.json and prints it as one JSON line.

rate     c3 at 16,384 envs (26 GB of Q), learn_begin + apply_qinit + step(25) so that the tables hold learned rows, then
         MEAN with SHARE for one cohort, 64 cohorts of 256 and 1,024 cohorts of 16, members interleaved (e % n_cohorts):
         kernel ms (median of ROUNDS calls after a warm-up call), bytes moved = 2 * E * q_per_env * 8, GB/s.
copy     in the same process, torch copy_ of a buffer the size of the Q block onto another (the same bytes: one
         read, one write); ratio = consensus ms / copy ms.  The issue's expectation is a ratio of at most 1.5.
step     the kernel ms of one step(25) of the same handle: what a sync costs relative to the training between syncs.
learning c2 at 4,096 envs, DECISIONS decisions per env: independent learners (step) against step_shared with one
         cohort and a sync every SYNC_EVERY decisions; the mean over the envs of test(1)'s arrived trains for each.
         Recorded only.

Usage: python scripts/consensus_rate.py [--tag TAG] [--envs 16384] [--config c3] [--rounds 3] [--skip-learning]"""
import argparse
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
DECISIONS, SYNC_EVERY = 2000, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--config", default="c3")
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-learning", action="store_true")
    args = ap.parse_args()
    import torch
    build = importlib.import_module(PKG + ".build")
    mapgen = importlib.import_module(PKG + ".mapgen")
    comp = importlib.import_module(PKG + ".compiler")
    runtime = importlib.import_module(PKG + ".runtime")
    _lib = importlib.import_module(PKG + "._lib")
    lib = _lib.load_product()
    res = dict(build_id=build.product_build_id(), device=torch.cuda.get_device_name(0), hp=HP, rounds=args.rounds)

    E = args.envs
    cm = comp.compile_scenario(mapgen.make_config(args.config))
    b = runtime.Batch(cm, HP, [450565 + e for e in range(E)], lib=lib)
    b.learn_begin()
    b.apply_qinit()
    b.step(25)
    step_ms = statistics.median(b.step(25)[1] for _ in range(args.rounds))
    nbytes = 2 * E * cm.q_per_env * 8
    src = torch.empty(E * cm.q_per_env, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    dst.copy_(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    copy = []
    for _ in range(args.rounds):
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        copy.append(ev[0].elapsed_time(ev[1]))
    copy_ms = statistics.median(copy)
    del src, dst
    torch.cuda.empty_cache()
    rate = dict(config=args.config, envs=E, q_per_env=cm.q_per_env, q_block_gb=E * cm.q_per_env * 8 / 1e9,
                bytes_moved=nbytes, copy_ms=copy_ms, copy_gbs=nbytes / copy_ms / 1e6, step25_ms=step_ms,
                kernel_variant=b.counters()["kernel_variant"], cohorts=[])
    for n in (1, 64, 1024):
        ids = None if n == 1 else [e % n for e in range(E)]
        b.consensus("mean", ids, share=True)  # (warm-up; it also shares, so the timed calls merge shared tables)
        b.step(25)                            # ... which the step between them makes differ again
        ms = []
        for _ in range(args.rounds):
            ms.append(b.consensus("mean", ids, share=True))
            b.step(25)
        m = statistics.median(ms)
        rate["cohorts"].append(dict(n_cohorts=n, members=E // n, kernel_ms=m, all_ms=ms, gbs=nbytes / m / 1e6,
                                    ratio_to_copy=m / copy_ms, ratio_to_step25=m / step_ms))
    # the shared tables are the consensus tables (a spot check at this size)
    b.consensus("mean", None, share=True)
    cq, ct = b.consensus_raw(0)
    held = np.unpackbits(ct.view(np.uint8), bitorder="little").astype(bool)
    for e in (0, E // 2 + 1, E - 1):
        q, t = b.q_raw(e)
        assert np.array_equal(t, ct), e
        rows = importlib.import_module("tests._consensus").cell_rows(cm)
        sel = held[rows]
        assert np.array_equal(q[sel].view(np.uint64), cq[sel].view(np.uint64)), e
    rate["spot_check"] = "envs 0, E/2+1, E-1 equal the consensus table on its held rows after SHARE"
    b.close()
    res["rate"] = rate

    if not args.skip_learning:
        cm2 = comp.compile_scenario(mapgen.make_config("c2"))
        seeds = [450565 + e for e in range(4096)]
        out = {}
        for how in ("independent", "shared"):
            b = runtime.Batch(cm2, HP, seeds, lib=lib)
            b.learn_begin()
            b.apply_qinit()
            if how == "shared":
                n, sms, cms = b.step_shared(DECISIONS, SYNC_EVERY, "mean")
            else:
                n, sms, cms = 0, 0.0, 0.0
                for _ in range(DECISIONS // SYNC_EVERY):
                    d, ms = b.step(SYNC_EVERY)
                    n, sms = n + d, sms + ms
            arrived = b.test(1)["arrived"][0]
            out[how] = dict(decisions=n, step_ms=sms, consensus_ms=cms, mean_arrived=float(np.mean(arrived)),
                            trains=cm2.T)
            b.close()
        res["learning"] = dict(config="c2", envs=4096, decisions_per_env=DECISIONS, sync_every=SYNC_EVERY, mode="mean",
                               **out)
    path = os.path.join(REPO, "profiles", (args.tag + "_" if args.tag else "") + "consensus_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
