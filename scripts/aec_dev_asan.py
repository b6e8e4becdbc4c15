"""Sanitizer run of the host side of the device-resident external-action calls (sfl_env_step_dev, sfl_env_sync, the
coordinate tables of sfl_create, env_encode_item): builds scripts/debug/aec_dev_asan.cpp -- the host build's sources
with a main() of their own -- with -fsanitize=address,undefined and runs it on c1.  CPU only; nothing is loaded into
Python.  Usage: python scripts/aec_dev_asan.py"""
import importlib
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = "network-distributed-q-learning_amd"
ARRAYS = [("grid", np.uint16), ("cell_sw", np.int16), ("sw_np", np.uint8), ("sw_na", np.uint8), ("act_src", np.uint8),
          ("act_dst", np.uint8), ("act_turn", np.uint8), ("act_j", np.uint8), ("first_other", np.uint8),
          ("port_side", np.uint8), ("slot_nroutes", np.uint8), ("slot_route_act", np.uint8), ("q_w", np.uint8),
          ("port_nb", np.int16), ("port_len", np.int16), ("port_unique", np.int16), ("q_off", np.uint64),
          ("row_base", np.uint32), ("dist", np.int32), ("tr_ed", np.int32), ("tr_la", np.int32), ("tr_k", np.int32),
          ("tr_target", np.int32), ("tr_init_cell", np.int32), ("tr_init_dist", np.int32), ("tr_init_delay", np.int32),
          ("tr_init_dir", np.uint8), ("tr_init_port", np.int16)]  # sfl_map_desc's order (runtime.Batch)


def main():
    mapgen = importlib.import_module(PKG + ".mapgen")
    comp = importlib.import_module(PKG + ".compiler")
    aec = importlib.import_module(PKG + ".aec")
    build = importlib.import_module(PKG + ".build")
    _lib = importlib.import_module(PKG + "._lib")
    cm = comp.compile_scenario(mapgen.make_config("c1"))
    sc = cm.scenario
    # the expected first observation of env 0, from the ordinary host build's host call
    b = aec.AECBatch(cm, [450565, 7], lib=_lib.Lib(build.build_hostsim()))
    out = b.step(None)
    s, slot = int(out["agent"][0]), int(out["slot"][0])
    o, P = cm.obs_of_row(s, slot, int(out["state"][0])), len(cm.ports[s])
    b.close()
    row = [-1] * _lib.OBS_WIDTH
    row[0:2], row[2:2 + P], row[6:6 + 2 * P], row[14:14 + P] = o[0:2], o[2:2 + P], o[2 + P:2 + 3 * P], o[2 + 3 * P:]
    with tempfile.TemporaryDirectory() as d:
        path, exe = os.path.join(d, "c1.map"), os.path.join(d, "aec_dev_asan")
        with open(path, "wb") as f:
            f.write(struct.pack("<10i", cm.H, cm.W, cm.S, cm.T, cm.K, sc.max_episode_steps, sc.malfunction_min,
                                sc.malfunction_max, cm.rows_per_env, 20))
            f.write(struct.pack("<dQ", sc.malfunction_rate, cm.q_per_env))
            for name, dt in ARRAYS:
                a = np.ascontiguousarray(cm.arrays[name], dtype=dt).tobytes()
                f.write(struct.pack("<Q", len(a)) + a)
            a = np.array(row, np.int32).tobytes()
            f.write(struct.pack("<Q", len(a)) + a)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(REPO, "scripts", "debug", "aec_dev_asan.cpp")],
                       check=True)
        r = subprocess.run([exe, path])
    print("sanitizer run:", "clean" if r.returncode == 0 else f"FAILED (exit {r.returncode})")
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
