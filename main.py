"""Launch a training run from an ini file (the reference's main.py -c config.ini).

Sections/keys as in the reference (main.py:21-60; writer hyperparam_tuning.py:49-82):
  [MISC]  random_seed, out_dir, checkpoint_freq, exploit_freq   (+ optional n_envs, device; optional seed_pool
          and heldout_exploit, the seed schedule of runtime.Batch.set_seed_schedule: learning episode t runs on
          runtime.episode_seed(random_seed, t % seed_pool) -- 0: a new scenario every episode -- and with
          heldout_exploit = true the exploit rounds run on a held-out seed.  Absent: every episode replays the
          malfunctions of random_seed, as in the reference)
  [ENV]   width, height, max_num_cities, max_rails_between_cities, max_rail_pairs_in_city,
          number_of_agents, malfunction_rate, min_duration, max_duration   (+ optional scenario:
          a mapgen config name or a scenario JSON path, used instead of the size keys; optional
          malfunction_stream = counter | flatland: the frozen spec's counter-based draw, or
          ParamMalfunctionGen's np_random draw order, mfstream.py)

The size keys give mapgen's stand-in layout (mapgen.from_flatland_params), not Flatland's
sparse_rail_generator output, which is absent: max_num_cities is honoured as a cap inside
width x height, max_rails_between_cities / max_rail_pairs_in_city have no counterpart (warned).
  [MODEL] gamma, epsilon, epsilon_decay_rate, lr, lr_decay_rate, default_q, num_episodes
"""
import argparse
import configparser
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = "network-distributed-q-learning_amd"
mapgen = importlib.import_module(PKG + ".mapgen")
ASyncSwitchEnv = importlib.import_module(PKG + ".env").ASyncSwitchEnv
DistrQLearning = importlib.import_module(PKG + ".distr_q").DistrQLearning


def build_scenario(config):
    env = config["ENV"]
    seed = int(config["MISC"]["random_seed"])
    mf = (float(env.get("malfunction_rate", 0)), int(env.get("min_duration", 0)), int(env.get("max_duration", 0)))
    if "scenario" in env:
        s = env["scenario"]
        sc = mapgen.make_config(s, seed=seed, malfunction=mf) if s in mapgen.CONFIGS else mapgen.Scenario.load(s)
        return sc
    opt = {k: int(env[k]) for k in ("max_rails_between_cities", "max_rail_pairs_in_city") if k in env}
    return mapgen.from_flatland_params(int(env["width"]), int(env["height"]), int(env["max_num_cities"]),
                                       int(env["number_of_agents"]), seed, malfunction=mf, **opt)


def seed_schedule(config):
    """(seed_pool, heldout_exploit) of a config's [MISC] section; (1, False) where the keys are absent."""
    misc = config["MISC"]
    return int(misc.get("seed_pool", 1)), misc.getboolean("heldout_exploit", fallback=False)


def launch_experiment(config_path, lib=None):
    """``lib``: the library handle to run on (default: the HIP product library; tests pass the host build)."""
    start_time = time.time()
    config = configparser.ConfigParser()
    config.read(config_path)
    out_dir = config["MISC"]["out_dir"]
    os.makedirs(out_dir, exist_ok=True)
    checkpoint_freq = int(config["MISC"]["checkpoint_freq"])
    exploit_freq = int(config["MISC"]["exploit_freq"])
    n_envs = int(config["MISC"].get("n_envs", 1))
    device = int(config["MISC"].get("device", 0))
    env = ASyncSwitchEnv(build_scenario(config), render_mode="human", max_steps=100_000, n_envs=n_envs, device=device,
                         malfunction_stream=config["ENV"].get("malfunction_stream", "counter"))
    m = config["MODEL"]
    seed_pool, heldout_exploit = seed_schedule(config)
    model = DistrQLearning(env=env, gamma=float(m["gamma"]), epsilon=float(m["epsilon"]),
                           epsilon_decay_rate=float(m["epsilon_decay_rate"]), lr=float(m["lr"]),
                           lr_decay_rate=float(m["lr_decay_rate"]), default_q=float(m["default_q"]),
                           seed=int(config["MISC"]["random_seed"]), lib=lib, seed_pool=seed_pool,
                           heldout_exploit=heldout_exploit)
    n_ep = int(m["num_episodes"])
    model.learn(num_episodes=n_ep, out_dir=out_dir, checkpoint_freq=checkpoint_freq, exploit_freq=exploit_freq)
    model.save(os.path.join(out_dir, "distr_q_model.pkl"))
    elapsed_time = time.time() - start_time
    print("DONE!")
    print(f"TOTAL TIME: {elapsed_time:.1f} seconds")
    print(f"Seconds per episode: {elapsed_time / n_ep:.1f}")
    print(f"Device (kernel) time: {env.flatland_step_time:.3f} seconds")


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("-c", "--config", type=str, help="Config file path", required=True)
    args = parser.parse_args()
    launch_experiment(args.config)
