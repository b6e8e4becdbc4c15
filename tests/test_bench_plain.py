"""bench.py's plain run and its options --dump-outputs and --full, on one rank of the host build of the kernel
body (``--rehearse-on-host``): a plain run times exactly --steps steps and carries nothing beyond the headline
figure; --dump-outputs writes the same float64 arrays run after run, and they are what the last timed step left
(equal to a host run of the sampled envs' seeds over the same schedule); --full brings the parity check back."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "network-distributed-q-learning_amd"
ARGS = ["--gpus", "1", "--rehearse-on-host", "--config", "c2", "--envs", "40", "--decisions", "32", "--steps", "3",
        "--warmup", "1"]


def _bench(args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_dumps_the_same_outputs_every_time(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    res = _bench(ARGS + ["--dump-outputs", str(a)])
    _bench(ARGS + ["--dump-outputs", str(b)])
    # the headline figure and nothing that takes a run of its own
    assert res["steps"] == 3 and res["warmup"] == 1 and res["full"] is False
    assert res["unit"] == "agent-env-steps/sec" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert abs(res["value"] * res["ms_per_step"] * 1e-3 * 3 - 40 * 32 * 3) < 1e-6 * res["value"] + 1
    assert res["parity"] == "not verified" and res["parity_envs_checked"] == 0 and res["sustained"] is None
    assert not {"cpu_baseline", "cpu_oracle_baseline", "partition_leg"} & set(res)
    names = sorted(f[:-4] for f in os.listdir(a))
    assert names == res["dumped_outputs"] == sorted(f[:-4] for f in os.listdir(b))
    out = {n: np.load(a / (n + ".npy")) for n in names}
    assert sum(x.nbytes for x in out.values()) <= 64 << 20
    for n, x in out.items():
        assert x.dtype == np.float64, n
        assert np.array_equal(x, np.load(b / (n + ".npy"))), n
    # the sample is the state after warm-up + timed steps: a host run of its seeds over the same schedule
    from tests import hostsim
    mapgen, comp, parity = (importlib.import_module(PKG + "." + m) for m in ("mapgen", "compiler", "parity"))
    bench = importlib.import_module("bench")
    cm = comp.compile_scenario(mapgen.make_config("c2"))
    pick = [int(e) for e in out["envs"]]
    assert pick == parity.spread(40, bench.DUMP_ENVS) and len(pick) > 8
    ref = parity.host_run(cm, bench.HP, [450565 + e for e in pick], [32] * 4, hostsim.lib())
    try:
        for i in range(len(pick)):
            q, t = ref.q_raw(i)
            el, ph, sem, pos, bits = parity.env_state(ref, i)
            assert np.array_equal(out["q"][i], q) and np.array_equal(out["key_set"][i], t), pick[i]
            assert out["env_clock"][i].tolist() == [el, ph]
            lo, hi = out["semaphores"][i][:, 0].astype(np.uint64), out["semaphores"][i][:, 1].astype(np.uint64)
            assert np.array_equal(lo | (hi << np.uint64(32)), sem)
            assert np.array_equal(out["train_cells"][i], pos) and np.array_equal(out["train_bits"][i], bits)
    finally:
        ref.close()
    assert out["last_step"].tolist()[0] == 40 * 32 and out["last_step"].tolist()[3] == 40 * 32 * 4


def test_full_run_verifies_itself():
    res = _bench(ARGS + ["--full", "--verify-envs", "4"])
    assert res["full"] is True and res["steps"] == 3
    # (parity.spread(40, 4): envs 0, 21 and 39)
    assert res["parity"] == "ok" and res["parity_envs_checked"] == 3, res
