"""Load the committed golden fixtures (tests/golden/*.json.gz; a case too big for gzip to keep under 1 MiB
is stored as *.json.xz)."""
import gzip
import importlib
import json
import lzma
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden")
mapgen = importlib.import_module("network-distributed-q-learning_amd.mapgen")


def cases():
    return sorted(f[:-8] for f in os.listdir(GOLDEN_DIR) if f.endswith((".json.gz", ".json.xz")))


def load(name):
    path = os.path.join(GOLDEN_DIR, name + ".json.gz")
    opener = gzip.open
    if not os.path.exists(path):
        path, opener = os.path.join(GOLDEN_DIR, name + ".json.xz"), lzma.open
    with opener(path, "rt") as f:
        d = json.load(f)
    d["scenario_obj"] = mapgen.Scenario.from_json(json.dumps(d["scenario"]))
    return d
