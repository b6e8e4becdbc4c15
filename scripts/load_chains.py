"""Static count of exposed vector-memory round trips per kernel and loop phase, from the compiler's own listing.

Sits on phase_listing.py's compile line and attribution (the inlined-at chain of each instruction's `.loc` comment).
An *exposed round trip* is an `s_waitcnt` with a `vmcnt(N)` operand that has at least one `global_` / `flat_` load
between it and the previous such wait: the wave stops there for (at least part of) a memory round trip.  Two
dependent loads cost two of them, two loads issued together and waited for once cost one.  The count is static and
linear (listing order: an instruction in a loop counts once, a branch is not followed) and by mnemonic prefix only,
as in phase_listing.py; `vmcnt(N)` with N > 0 counts like `vmcnt(0)` (it waits for the oldest loads).

A wait is attributed to its own phase; the loads it retires are listed with the source line they were inlined from
into the phase's function (tick(), prefetch_slot(), ...), so the chains of a block can be read off:

  staging      exposed round trips    4   loads   14   per wait  3.50
      wait @1766  <- 5 loads @1739 1777 1739 1739 1739

Usage: python scripts/load_chains.py [--tu sfl_kwave_v7.hip] [--kernel SUBSTR] [--csrc DIR] [--listing FILE.s] [--lines]
  --lines    list every exposed wait with its loads (default: the per-phase table only)
"""
import argparse
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phase_listing as pl  # noqa: E402

LOADS = ("global_load", "flat_load")
WAIT = "s_waitcnt"
# calls of sfl_wave.h that only pass on to the function doing the work: the source line reported is the callee's
PASS_THROUGH = r"\bprefetch_slot\("


def is_load(op):
    return op.startswith(LOADS)


def is_vm_wait(op, args):
    return op == WAIT and "vmcnt(" in args


def pass_lines(wave_h):
    return {n for n, line in enumerate(open(wave_h), 1) if re.search(PASS_THROUGH, line) and "void prefetch_slot" not in line}


def place(cur, sites, passthru):
    """(phase, line inside the phase's function or None) of an instruction's frame chain (innermost first)."""
    phase, where = "loop", None
    if not cur:
        return phase, where
    hits = [(i, sites[n]) for i, (f, n) in reversed(list(enumerate(cur))) if f == "sfl_wave.h" and n in sites]
    calls = [(i, ph) for i, ph in hits if ph != "staging"]
    if not calls:
        return phase, where
    i, phase = calls[0]
    if phase == "decide":
        st = [j for j, ph in hits if ph == "staging" and j < i]
        if st:
            phase, i = "staging", st[0]
    i -= 1
    while i > 0 and cur[i][0] == "sfl_wave.h" and cur[i][1] in passthru:
        i -= 1
    if i >= 0 and cur[i][0] == "sfl_wave.h":
        where = cur[i][1]
    return phase, where


def chains(lines, sites=None, passthru=(), kernel=""):
    """{kernel: [(phase, wait line, [load lines])]}: the exposed waits of each kernel in listing order."""
    sites = sites or {}
    res, name, cur, pending = {}, None, None, []
    for line in lines:
        m = re.match(r"^(_Z\S+):", line)
        if m:
            name = m.group(1) if ("k_wave" in m.group(1) or "k_run" in m.group(1)) and (not kernel or kernel in m.group(1)) else None
            if name:
                res[name] = []
            cur, pending = None, []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        s = line.strip()
        if s.startswith(".loc"):
            cur = pl.frames_of(s.split(";", 1)[1]) if ";" in s else None
            continue
        if not s or s[0] in ".;" or s.split(";")[0].strip().endswith(":"):
            continue
        parts = s.split(";")[0].split(None, 1)
        op, args = parts[0], parts[1] if len(parts) > 1 else ""
        if is_load(op):
            pending.append(place(cur, sites, passthru)[1])
        elif is_vm_wait(op, args) and pending:
            phase, where = place(cur, sites, passthru)
            res[name].append((phase, where, pending))
            pending = []
    return res


def summary(waits):
    """{phase: (exposed round trips, loads)}"""
    out = {}
    for phase, _, loads in waits:
        n, k = out.get(phase, (0, 0))
        out[phase] = (n + 1, k + len(loads))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tu", default="sfl_kwave_v7.hip", choices=sorted(pl.build.TUS))
    ap.add_argument("--kernel", default="")
    ap.add_argument("--csrc", default=pl.build.CSRC)
    ap.add_argument("--listing")
    ap.add_argument("--lines", action="store_true")
    a = ap.parse_args()
    csrc = os.path.abspath(a.csrc)
    wave_h = os.path.join(csrc, "sfl_wave.h")
    sites, tick_def = pl.call_sites(wave_h)
    with tempfile.TemporaryDirectory() as tmp:
        listing = a.listing
        if not listing:
            listing = os.path.join(tmp, os.path.splitext(a.tu)[0] + ".s")
            pl.compile_listing(a.tu, csrc, listing)
        res = chains(open(listing), sites, pass_lines(wave_h), a.kernel)
    if not res:
        raise SystemExit("no kernel matched")
    # (a listing read against another tree's sfl_wave.h, or one built without -gline-tables-only, attributes next to
    # nothing; in a listing of this tree more than half of the wave kernels' waits lie in a phase)
    wave = [ph for name, waits in res.items() if "k_wave" in name for ph, _, _ in waits]
    if wave and 10 * sum(ph != "loop" for ph in wave) < len(wave):
        raise SystemExit("fewer than a tenth of the wave kernels' waits could be attributed to a loop phase -- "
                         "does --csrc match the listing?")
    print(f"# {a.tu}: exposed vector-memory round trips per loop phase (static; source lines of sfl_wave.h, tick() at {tick_def})")
    fmt = lambda xs: " ".join("?" if x is None else str(x) for x in xs)  # noqa: E731
    for name, waits in res.items():
        print(f"\n{name}")
        sm = summary(waits)
        tot_n = tot_k = 0
        for p in pl.PHASES:
            n, k = sm.get(p, (0, 0))
            tot_n, tot_k = tot_n + n, tot_k + k
            print(f"  {p:12s} exposed round trips {n:4d}   loads {k:4d}   per wait {k / n if n else 0.0:5.2f}")
            if a.lines:
                for ph, where, loads in waits:
                    if ph == p:
                        print(f"      wait @{fmt([where])}  <- {len(loads)} load{'s' if len(loads) != 1 else ''} @{fmt(loads)}")
        print(f"  {'total':12s} exposed round trips {tot_n:4d}   loads {tot_k:4d}   per wait {tot_k / tot_n if tot_n else 0.0:5.2f}")


if __name__ == "__main__":
    main()
