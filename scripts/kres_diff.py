"""Compare the wave kernels of two built libsfl.so files: VGPRs, SGPRs, spills, scratch, LDS and code size of every
k_wave / k_wave2 / k_wave_g / k_wave_part / k_wave2_part instantiation, matched by shape (template arguments).  A
trailing HPG = false argument (the hyperparameter-group switch, csrc/sfl_kwave_g.h) is dropped, so a library with it
compares against one from before it; HPG = true kernels are listed on their own.  Likewise the EXT argument behind it
(external-action mode's kernels, sfl_env_begin_wave).  The policy-bank evaluation's kernels (k_wave_bank, k_wave2_bank,
k_wave_g_bank: sfl_bank_eval) are listed as "BANK " + the key of their Plain twin (those of an evaluation with a
recording armed, k_wave*_bank_rec, as "BANKREC " + that key), and a second table puts each beside
that twin.  The kernels of handles with a seed schedule (k_wave_sched, k_wave2_sched, k_wave_g_sched) are listed as
"SCHED " + the key of their unscheduled twin (Plain, HPG or EXT), with a table of their own beside those twins.  The "code" column says whether the
kernel's machine code (the symbol's bytes in its code object's .text) is the same in both, or the same but for
pc-relative addresses (same_code).  Exit status 1 if a kernel
present in both differs in a resource field (registers, spills, scratch, LDS); code bytes alone do not fail.  The
transition assembler's kernels (k_trans_count, k_trans_write: sfl_trans.hip) are listed by name, and so are the cell
folds and their reset kernels (k_curve_*: sfl_curve.hip; k_eval_*: sfl_eval.hip) and the non-arrival diagnosis's
kernels (k_diag_*: sfl_diag.hip) and the recordings' traffic fold (k_rec_*: sfl_rec.hip).
Usage: python scripts/kres_diff.py OLD.so NEW.so [--md]"""
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")


def code_objects(path):
    """The gfx950 code object of every offload bundle in the library (one per translation unit)."""
    data, magic, i = open(path, "rb").read(), b"__CLANG_OFFLOAD_BUNDLE__", 0
    while (i := data.find(magic, i)) >= 0:
        n = struct.unpack_from("<Q", data, i + len(magic))[0]
        p = i + len(magic) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", data, p)
            if b"gfx950" in data[p + 24:p + 24 + idlen]:
                yield data[i + off:i + off + size]
            p += 24 + idlen
        i += len(magic)


def kernels(path):
    out = {}
    for co in code_objects(path):
        out.update(kernels_of(co))
    return out


def kernels_of(co):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        notes = subprocess.run([LLVM + "llvm-readelf", "--notes", f.name], capture_output=True, text=True).stdout
        syms = subprocess.run([LLVM + "llvm-readelf", "-sW", f.name], capture_output=True, text=True).stdout
        secs = subprocess.run([LLVM + "llvm-readelf", "-SW", f.name], capture_output=True, text=True).stdout
    # .text's address and file offset: a kernel's code is the symbol's bytes in it
    t = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", secs)
    t_addr, t_off, t_size = (int(x, 16) for x in t.groups())
    size, code = {}, {}
    for line in syms.splitlines():
        w = line.split()
        if len(w) >= 8 and w[3] == "FUNC":
            at, n = int(w[1], 16), int(w[2], 0)
            size[w[7]] = n
            if t_addr <= at and at + n <= t_addr + t_size:
                code[w[7]] = (co[t_off + at - t_addr:t_off + at - t_addr + n], at)
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        # (Itanium mangling: k_waveILi8ELi2ELb1E...E -- integer and bool template arguments only)
        m = re.search(r"\d+(k_wave_g_sched|k_wave2_sched|k_wave_sched|k_wave_g_bank_rec|k_wave2_bank_rec|k_wave_bank_rec|k_wave_g_bank|k_wave2_bank|k_wave_bank|k_wave_g|k_wave2_part|k_wave_part|k_wave2|k_wave)I((?:L[ib]\d+E)+)E", name)
        if not m:
            # the transition assembler's kernels (sfl_trans.hip) and the cell folds with their reset kernels
            # (sfl_curve.hip, sfl_eval.hip): no template arguments, listed by name
            t = re.search(r"\d+(k_(?:trans|curve|eval|diag|rec)_[a-z_]+)", name)
            if t:
                vals = [int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in FIELDS]
                out[t.group(1)] = vals + [size.get(name, -1), code.get(name)]
            continue
        args = [("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([ib])(\d+)E", m.group(2))]
        vals = [int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in FIELDS]
        if m.group(1).endswith(("_bank", "_bank_rec")):  # <PPL,SPL,TW[,G,OCC,LM]>: the key of the Plain twin (TRACE, TIMED false)
            twin = args[:3] + ["false"] + (args[3:5] + ["false", args[5]] if len(args) == 6 else ["false"])
            rec = m.group(1).endswith("_rec")  # (the kernels of an evaluation with a recording armed: listed on their own)
            out[("BANKREC " if rec else "BANK ") + m.group(1)[:-9 if rec else -5] + "<" + ",".join(twin) + ">"] = \
                vals + [size.get(name, -1), code.get(name)]
            continue
        if m.group(1).endswith("_sched"):  # <PPL,SPL,TW[,G,OCC,LM],HPG,EXT>: "SCHED " + the key of the unscheduled twin
            base, (hpg, ext) = m.group(1)[:-6], (v == "true" for v in args[-2:])
            twin = args[:3] + ["false"] + (args[3:5] + ["false", args[5]] if len(args) == 8 else ["false"])
            out["SCHED " + ("EXT " if ext else "") + ("HPG " if hpg else "") + base + "<" + ",".join(twin) + ">"] = \
                vals + [size.get(name, -1), code.get(name)]
            continue
        full = {"k_wave": 6, "k_wave2": 6, "k_wave_g": 9}.get(m.group(1))  # (the part kernels have no HPG argument)
        # (a trailing EXT argument behind HPG: external-action mode's kernels, listed on their own like HPG's)
        ext = full is not None and len(args) == full + 1 and args[-1] == "true"
        if full is not None and len(args) == full + 1:
            args = args[:-1]
        hpg = len(args) == full and args[-1] == "true"
        if len(args) == full:
            args = args[:-1]
        key = ("EXT " if ext else "") + ("HPG " if hpg else "") + m.group(1) + "<" + ",".join(args) + ">"
        out[key] = vals + [size.get(name, -1), code.get(name)]
    return out


def same_code(x, y):
    """x, y: a kernel's (bytes, address) in the two libraries.  'identical'; or 'pc-relative only (n)' if they differ
    in nothing but n literals of an s_add_u32 that follows an s_getpc_b64 -- the offset to an address elsewhere in the
    code object, which moves with the kernel's place in .text -- and both point at the same address; or 'differs'."""
    if x is None or y is None or len(x[0]) != len(y[0]):
        return "differs"
    if x[0] == y[0]:
        return "identical"
    a, b = struct.unpack(f"<{len(x[0]) // 4}I", x[0]), struct.unpack(f"<{len(y[0]) // 4}I", y[0])
    moved = [i for i in range(len(a)) if a[i] != b[i]]
    for i in moved:  # words i - 2, i - 1: s_getpc_b64 (SOP1 op 0x1c); SOP2 s_add_u32 (op 0) with src1 = literal (255)
        if i < 2 or a[i - 2:i] != b[i - 2:i] or (a[i - 2] & 0xFF80FFFF) != 0xBE801C00 or (a[i - 1] & 0xFF80FF00) != 0x8000FF00:
            return "differs"
        if (x[1] + 4 * (i - 1) + a[i]) & 0xFFFFFFFF != (y[1] + 4 * (i - 1) + b[i]) & 0xFFFFFFFF:
            return "differs"
    return f"pc-relative only ({len(moved)})"


def main(old, new, md=False):
    a, b = kernels(old), kernels(new)
    head = ["kernel", "vgpr", "sgpr", "vspill", "sspill", "scratch", "lds", "code bytes", "code", ""]
    rows, bad, recoded = [], 0, 0
    nf = len(FIELDS)
    for k in sorted(set(a) | set(b)):
        if k in a and k in b:
            same = a[k][:nf] == b[k][:nf]
            ident = same_code(a[k][-1], b[k][-1])
            bad += not same
            recoded += ident == "differs"
            rows.append([k] + [str(x) if x == y else f"{x} -> {y}" for x, y in zip(a[k][:-1], b[k][:-1])] +
                        [ident, "equal" if same else "DIFFERS"])
        else:
            rows.append([k] + [str(x) for x in (a.get(k) or b[k])[:-1]] + ["-", "old only" if k in a else "new only"])
    if md:
        print("| " + " | ".join(head) + " |\n|" + "---|" * len(head))
        for r in rows:
            print("| " + " | ".join(r) + " |")
    else:
        for r in [head] + rows:
            print(f"{r[0]:64s}" + "".join(f"{x:>24s}" for x in r[1:]))
    banks = [k for k in sorted(b) if k.startswith("BANK ") and k[5:] in b]
    if banks:
        print("\npolicy-bank kernels of the new library beside their Plain twins (twin -> bank)")
        bh = ["kernel"] + head[1:8]
        brows = [[k[5:]] + [f"{x} -> {y}" for x, y in zip(b[k[5:]][:-1], b[k][:-1])] for k in banks]
        if md:
            print("| " + " | ".join(bh) + " |\n|" + "---|" * len(bh))
            for r in brows:
                print("| " + " | ".join(r) + " |")
        else:
            for r in [bh] + brows:
                print(f"{r[0]:64s}" + "".join(f"{x:>24s}" for x in r[1:]))
    scheds = [k for k in sorted(b) if k.startswith("SCHED ") and k[6:] in b]
    if scheds:
        print("\nseed-schedule kernels of the new library beside their unscheduled twins (twin -> scheduled)")
        bh = ["kernel"] + head[1:8]
        brows = [[k[6:]] + [f"{x} -> {y}" for x, y in zip(b[k[6:]][:-1], b[k][:-1])] for k in scheds]
        if md:
            print("| " + " | ".join(bh) + " |\n|" + "---|" * len(bh))
            for r in brows:
                print("| " + " | ".join(r) + " |")
        else:
            for r in [bh] + brows:
                print(f"{r[0]:64s}" + "".join(f"{x:>24s}" for x in r[1:]))
    print(f"{sum(1 for k in a if k in b)} kernels in both, {len(set(a) ^ set(b))} in one only, {bad} differ in resources, "
          f"{recoded} in machine code")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], "--md" in sys.argv))
