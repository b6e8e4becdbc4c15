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

`--counter lgkm` counts the other counter the same way: the operations are the LDS instructions (`ds_*`, reads, writes
and `ds_bpermute` alike -- all of them count on lgkmcnt) and the scalar loads (`s_load*`, `s_buffer_load*`), the waits
every `s_waitcnt` with an `lgkmcnt(N)` operand; a wait with `vmcnt` alone retires none of them.  A wait is listed under
each kind it retires an operation of, with the waits that retire a single operation of the kind counted apart (those
are the serial ones: a field loaded where it is used, a record read behind the value that indexes it), and `--lines`
marks every operation `s:` (scalar load) or `d:` (LDS):

  post         exposed waits   30   ops   52   per wait  1.73   scalar   25 (single  23)   LDS    5 (single   5)
      wait @2263  <- 1 op @s:2263

Usage: python scripts/load_chains.py [--tu sfl_kwave_v7.hip] [--kernel SUBSTR] [--csrc DIR] [--listing FILE.s] [--lines]
                                     [--counter vm|lgkm]
  --lines    list every exposed wait with its loads (default: the per-phase table only)
  --counter  vm (default): vector-memory loads against vmcnt; lgkm: LDS instructions and scalar loads against lgkmcnt
"""
import argparse
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phase_listing as pl  # noqa: E402

LOADS = ("global_load", "flat_load")
SCALAR_LOADS = ("s_load", "s_buffer_load")
WAIT = "s_waitcnt"
KINDS = (("s", "scalar"), ("d", "LDS"))
# calls of sfl_wave.h that only pass on to the function doing the work: the source line reported is the callee's
PASS_THROUGH = r"\bprefetch_slot\("


def is_load(op):
    return op.startswith(LOADS)


def is_vm_wait(op, args):
    return op == WAIT and "vmcnt(" in args


def lgkm_kind(op):
    """'d' for an LDS instruction, 's' for a scalar load, None for anything else."""
    if op.startswith("ds_"):
        return "d"
    if op.startswith(SCALAR_LOADS):
        return "s"
    return None


def is_lgkm_wait(op, args):
    return op == WAIT and "lgkmcnt(" in args


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


def chains(lines, sites=None, passthru=(), kernel="", counter="vm"):
    """{kernel: [(phase, wait line, [load lines])]}: the exposed waits of each kernel in listing order.
    counter "lgkm": the LDS instructions and scalar loads against lgkmcnt, each as (kind, line)."""
    lgkm = counter == "lgkm"
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
        if lgkm and lgkm_kind(op):
            pending.append((lgkm_kind(op), place(cur, sites, passthru)[1]))
        elif not lgkm and is_load(op):
            pending.append(place(cur, sites, passthru)[1])
        elif (is_lgkm_wait(op, args) if lgkm else is_vm_wait(op, args)) and pending:
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


def kind_split(waits):
    """{phase: {kind: (waits that retire an operation of the kind, of them retiring just one of the kind)}} (lgkm)"""
    out = {}
    for phase, _, ops in waits:
        for k in sorted({k for k, _ in ops}):
            n, one = out.setdefault(phase, {}).get(k, (0, 0))
            out[phase][k] = (n + 1, one + (sum(kk == k for kk, _ in ops) == 1))
    return out


def print_lgkm(tu, tick_def, res, lines):
    print(f"# {tu}: exposed LDS / scalar-load waits (lgkmcnt) per loop phase (static; source lines of sfl_wave.h, tick() at {tick_def})")
    fmt = lambda ops: " ".join(f"{k}:{'?' if w is None else w}" for k, w in ops)  # noqa: E731
    for name, waits in res.items():
        print(f"\n{name}")
        sm, ks = summary(waits), kind_split(waits)
        tot, tot_k = [0, 0], {k: [0, 0] for k, _ in KINDS}
        row = lambda label, n, k, kk: (  # noqa: E731
            f"  {label:12s} exposed waits {n:4d}   ops {k:4d}   per wait {k / n if n else 0.0:5.2f}"
            + "".join(f"   {kn} {kk[kd][0]:4d} (single {kk[kd][1]:3d})" for kd, kn in KINDS))
        for p in pl.PHASES:
            n, k = sm.get(p, (0, 0))
            kk = {kd: ks.get(p, {}).get(kd, (0, 0)) for kd, _ in KINDS}
            tot[0], tot[1] = tot[0] + n, tot[1] + k
            for kd, _ in KINDS:
                tot_k[kd][0] += kk[kd][0]
                tot_k[kd][1] += kk[kd][1]
            print(row(p, n, k, kk))
            if lines:
                for ph, where, ops in waits:
                    if ph == p:
                        print(f"      wait @{'?' if where is None else where}  <- {len(ops)} op{'s' if len(ops) != 1 else ''} @{fmt(ops)}")
        print(row("total", tot[0], tot[1], tot_k))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tu", default="sfl_kwave_v7.hip", choices=sorted(pl.build.TUS))
    ap.add_argument("--kernel", default="")
    ap.add_argument("--csrc", default=pl.build.CSRC)
    ap.add_argument("--listing")
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("--counter", default="vm", choices=("vm", "lgkm"))
    a = ap.parse_args()
    csrc = os.path.abspath(a.csrc)
    wave_h = os.path.join(csrc, "sfl_wave.h")
    sites, tick_def = pl.call_sites(wave_h)
    with tempfile.TemporaryDirectory() as tmp:
        listing = a.listing
        if not listing:
            listing = os.path.join(tmp, os.path.splitext(a.tu)[0] + ".s")
            pl.compile_listing(a.tu, csrc, listing)
        res = chains(open(listing), sites, pass_lines(wave_h), a.kernel, a.counter)
    if not res:
        raise SystemExit("no kernel matched")
    # (a listing read against another tree's sfl_wave.h, or one built without -gline-tables-only, attributes next to
    # nothing; in a listing of this tree more than half of the wave kernels' waits lie in a phase)
    wave = [ph for name, waits in res.items() if "k_wave" in name for ph, _, _ in waits]
    if wave and 10 * sum(ph != "loop" for ph in wave) < len(wave):
        raise SystemExit("fewer than a tenth of the wave kernels' waits could be attributed to a loop phase -- "
                         "does --csrc match the listing?")
    if a.counter == "lgkm":
        return print_lgkm(a.tu, tick_def, res, a.lines)
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
