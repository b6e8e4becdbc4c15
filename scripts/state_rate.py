"""Cost of suspend and resume (sfl_state_*, csrc/sfl_snap.hip) against a device-to-device copy of the Q block, how much
of the Q block is live, and the Q-dict extraction through one capture against the per-env dense copies.  Needs a GPU;
not a test, not part of bench.py: reported, not gated.  Writes profiles/[<tag>_]state_rate.json and prints it as one
JSON line.

state    c3 at 16,384 envs (26 GB of Q) after learn_begin, apply_qinit and LAUNCHES x step(1024), by which every env
         has ended episodes (min_ep_t is recorded).  count_ms: the device time of sfl_state_capture over every env (the
         pass that reads the whole Q block); the live-row fraction and the capture's bytes against the dense bytes.
         capture_ms / restore_ms (sfl_state_ms): a capture with its gather, and a restore into the same slots, of every
         env -- or, when the packed cells exceed --max-gb of host memory, of the first --subset envs (recorded).
copy     in the same process, torch copy_ of a buffer the size of the Q block onto another (one read, one write).
dicts    the Q dicts of 625 envs (a sweep checkpoint): [q_dict(e)] through sfl_get_q against q_dicts, wall seconds.

Usage: python scripts/state_rate.py [--tag TAG] [--envs 16384] [--config c3] [--rounds 3] [--launches 4]"""
import argparse
import ctypes as C
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="")
    ap.add_argument("--config", default="c3")
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--max-gb", type=float, default=6.0)
    ap.add_argument("--subset", type=int, default=2048)
    ap.add_argument("--dict-envs", type=int, default=625)
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
    step_ms = [b.step(1024)[1] for _ in range(args.launches)]
    info = b.state_info()
    dense = E * cm.q_per_env * 8

    # the Q block's device-to-device copy: the yardstick
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

    # the count pass over every env: the one read of the Q block
    P = C.POINTER
    ids = np.arange(E, dtype=np.uint32)
    row_off, cell_off = np.zeros(E + 1, np.uint64), np.zeros(E + 1, np.uint64)
    count = []
    for _ in range(args.rounds + 1):   # (the first call also builds the row table)
        lib.check(lib.dll.sfl_state_capture(b.h, E, ids.ctypes.data_as(P(C.c_uint32)), row_off.ctypes.data_as(P(C.c_uint64)),
                                            cell_off.ctypes.data_as(P(C.c_uint64))), "sfl_state_capture")
        count.append(b.state_ms()[0])
    lib.check(lib.dll.sfl_state_read(b.h, None, None, None, None), "sfl_state_read")   # (releases the buffers)
    count_ms = statistics.median(count[1:])
    rows, cells = int(row_off[E]), int(cell_off[E])
    per_env = np.diff(row_off.astype(np.int64))
    packed = cells * 8 + rows * 4 + E * (info["state_bytes"] + info["touched_words"] * 4) + 2 * (E + 1) * 8
    state = dict(config=args.config, envs=E, q_per_env=cm.q_per_env, rows_per_env=cm.rows_per_env,
                 kernel_variant=b.counters()["kernel_variant"], layout=info["layout"], state_bytes=info["state_bytes"],
                 launches=args.launches, step1024_ms=step_ms, dense_bytes=dense, copy_ms=copy_ms,
                 copy_gbs=2 * dense / copy_ms / 1e6, count_ms=count_ms, count_all_ms=count,
                 count_read_gbs=dense / count_ms / 1e6, count_ratio_to_copy=count_ms / copy_ms,
                 live_rows=rows, live_row_fraction=rows / (E * cm.rows_per_env), live_cells=cells,
                 live_cell_fraction=cells / (E * cm.q_per_env), live_rows_per_env_min=int(per_env.min()),
                 live_rows_per_env_max=int(per_env.max()), capture_bytes=packed, capture_to_dense=packed / dense)

    # a whole capture and a restore into the same slots
    n = E if cells * 8 <= args.max_gb * 1e9 else min(args.subset, E)
    envs = None if n == E else list(range(n))
    cap, rst = [], []
    for _ in range(args.rounds):
        t0 = time.time()
        s = b.capture(envs)
        t1 = time.time()
        b.restore(s, into=envs)
        t2 = time.time()
        c_ms, r_ms = b.state_ms()
        cap.append(dict(device_ms=c_ms, wall_s=t1 - t0))
        rst.append(dict(device_ms=r_ms, wall_s=t2 - t1))
    ep_t = np.ascontiguousarray(s.state[:, 12:16]).view(np.int32)
    again = b.capture(envs)   # a restore into the same slots changes nothing
    same = all(np.array_equal(getattr(s, k), getattr(again, k)) for k, _ in runtime.BatchState.ARRAYS)
    sub_dense = n * cm.q_per_env * 8
    state.update(round_trip_envs=n, round_trip_dense_bytes=sub_dense, min_ep_t=int(ep_t.min()), max_ep_t=int(ep_t.max()),
                 capture_ms=statistics.median(c["device_ms"] for c in cap), capture_all=cap,
                 restore_ms=statistics.median(r["device_ms"] for r in rst), restore_all=rst,
                 capture_ratio_to_copy=statistics.median(c["device_ms"] for c in cap) / (copy_ms * n / E),
                 restore_ratio_to_copy=statistics.median(r["device_ms"] for r in rst) / (copy_ms * n / E),
                 restored_capture_identical=bool(same))
    del s, again
    res["state"] = state

    # the Q dicts of a sweep checkpoint
    k = min(args.dict_envs, E)
    t0 = time.time()
    old = [b.q_dict(e) for e in range(k)]
    t1 = time.time()
    new = b.q_dicts(range(k))
    t2 = time.time()
    res["dicts"] = dict(envs=k, per_env_s=t1 - t0, q_dicts_s=t2 - t1, speedup=(t1 - t0) / (t2 - t1),
                        dense_bytes_moved=k * cm.q_per_env * 8, identical=bool(old == new),
                        rows_per_dict_mean=float(np.mean([len(d) for d in new])))
    b.close()
    path = os.path.join(REPO, "profiles", (args.tag + "_" if args.tag else "") + "state_rate.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
