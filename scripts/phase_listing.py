"""Static instruction counts of a kernel per loop phase, from the compiler's own listing.

Compiles one translation unit of libsfl.so with build.py's flags plus `-gline-tables-only --cuda-device-only -S`
into a temporary directory and attributes every instruction of each kernel to the phase of the flat loop it was
inlined from, through the inlined-at chain of its `.loc` comment (`; file:line:col @[ caller @[ ... ] ]`): the
phases are the call sites of load / reset / tick / post / decide / store in the kernel drivers of sfl_wave.h (run,
run_groups, ext_run), and the staging is decide()'s call of prefetch().  The tick's instructions are also broken
down in ten-line bands of tick().

Counts are static (an instruction in a loop counts once) and by class only, from the first letters of the mnemonic:
v_ VALU, s_ SALU (every scalar instruction: waits, branches and scalar loads included), ds_ LDS, global_ / buffer_ /
flat_ VMEM, scratch_ SCR (spills).

Usage: python scripts/phase_listing.py [--tu sfl_kwave_v7.hip] [--kernel SUBSTR] [--csrc DIR] [--listing FILE.s]
  --kernel   only the kernels whose mangled name contains SUBSTR (default: every kernel of the unit)
  --csrc     another tree's csrc directory (e.g. a checkout of the parent commit), compiled with this tree's flags
  --listing  read an existing listing instead of compiling
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKGDIR = os.path.join(ROOT, "network-distributed-q-learning_amd")
sys.path.insert(0, PKGDIR)
import build  # noqa: E402

CLASSES = (("v_", "VALU"), ("s_", "SALU"), ("ds_", "LDS"), ("global_", "VMEM"), ("buffer_", "VMEM"), ("flat_", "VMEM"),
           ("scratch_", "SCR"))
COLS = ("VALU", "SALU", "LDS", "VMEM", "SCR")
PHASES = ("load", "reset", "tick", "post", "decide", "staging", "store", "loop")
# the drivers' calls that start a phase (the staging: decide()'s own call of prefetch())
CALLS = (("load", r"\bv\.load\("), ("reset", r"\bv\.reset\("), ("tick", r"\bv\.tick\("), ("post", r"\bv\.post\w*\("),
         ("decide", r"\bv\.(template )?decide\b"), ("store", r"\bv\.store\w*\("), ("staging", r"^\s*prefetch\(greedy\);"))
BAND = 10


def classify(op):
    for prefix, c in CLASSES:
        if op.startswith(prefix):
            return c
    return None


def call_sites(wave_h):
    """line -> phase for the phase calls of sfl_wave.h, and the first line of tick()."""
    sites, tick_def = {}, None
    for n, line in enumerate(open(wave_h), 1):
        if tick_def is None and re.search(r"\bvoid tick\(\)", line):
            tick_def = n
        for ph, pat in CALLS:
            if re.search(pat, line):
                sites[n] = ph
    return sites, tick_def


def compile_listing(tu, csrc, out):
    cmd = [build.HIPCC, f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-Wno-unused-result", "-Wno-unused-value", '-DSFL_BUILD_ID="listing"', '-DSFL_BUILD_DEFS=""',
           '-DSFL_BUILD_FLAGS=""'] + build.TUS[tu] + ["-gline-tables-only", "--cuda-device-only", "-S", "-o", out,
                                                      os.path.join(csrc, tu)]
    subprocess.run(cmd, check=True, cwd=csrc, stderr=subprocess.DEVNULL)


def frames_of(comment):
    """[(file, line)] of a .loc comment, innermost first."""
    return [(os.path.basename(f), int(n)) for f, n in re.findall(r"([^\s\[\]@;]+):(\d+):\d+", comment)]


def attribute(listing, sites, tick_def, kernel):
    """{kernel name: (phase -> Counter, tick band -> Counter)}"""
    res, name, cur = {}, None, None
    for line in open(listing):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            name = m.group(1) if ("k_wave" in m.group(1) or "k_run" in m.group(1)) and (not kernel or kernel in m.group(1)) else None
            if name:
                res[name] = (collections.defaultdict(collections.Counter), collections.defaultdict(collections.Counter))
            cur = None
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        s = line.strip()
        if s.startswith(".loc"):
            cur = frames_of(s.split(";", 1)[1]) if ";" in s else None
            continue
        if not s or s[0] in ".;" or s.split(";")[0].strip().endswith(":"):
            continue
        c = classify(s.split()[0])
        if c is None:
            continue
        phase, band = "loop", None
        if cur:
            # from the kernel inwards: the first phase call on the chain; decide()'s staging call inside it takes over
            hits = [(i, sites[n]) for i, (f, n) in reversed(list(enumerate(cur))) if f == "sfl_wave.h" and n in sites]
            calls = [(i, ph) for i, ph in hits if ph != "staging"]
            if calls:
                i, phase = calls[0]
                if phase == "decide" and any(ph == "staging" and j < i for j, ph in hits):
                    phase = "staging"
                if phase == "tick" and i > 0 and cur[i - 1][0] == "sfl_wave.h":
                    band = (cur[i - 1][1] - tick_def) // BAND
        res[name][0][phase][c] += 1
        if band is not None:
            res[name][1][band][c] += 1
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tu", default="sfl_kwave_v7.hip", choices=sorted(build.TUS))
    ap.add_argument("--kernel", default="")
    ap.add_argument("--csrc", default=build.CSRC)
    ap.add_argument("--listing")
    a = ap.parse_args()
    csrc = os.path.abspath(a.csrc)
    sites, tick_def = call_sites(os.path.join(csrc, "sfl_wave.h"))
    with tempfile.TemporaryDirectory() as tmp:
        listing = a.listing
        if not listing:
            listing = os.path.join(tmp, os.path.splitext(a.tu)[0] + ".s")
            compile_listing(a.tu, csrc, listing)
        res = attribute(listing, sites, tick_def, a.kernel)
    row = lambda label, c: f"  {label:24s}" + "".join(f"{c.get(k, 0):8d}" for k in COLS)  # noqa: E731
    head = f"  {'':24s}" + "".join(f"{k:>8s}" for k in COLS)
    print(f"# {a.tu}: static instruction counts per loop phase (tick() starts at sfl_wave.h:{tick_def})")
    for name, (ph, bands) in res.items():
        print(f"\n{name}")
        print(head)
        tot = collections.Counter()
        for p in PHASES:
            tot.update(ph[p])
            print(row(p, ph[p]))
        print(row("total", tot))
        print(f"  tick() in {BAND}-line bands")
        for b in sorted(bands):
            lo = tick_def + b * BAND
            print(row(f"sfl_wave.h:{lo}-{lo + BAND - 1}", bands[b]))
    if not res:
        raise SystemExit("no kernel matched")


if __name__ == "__main__":
    main()
