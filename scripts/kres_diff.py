"""Compare the wave kernels of two built libsfl.so files: VGPRs, SGPRs, spills, scratch, LDS and code size of every
k_wave / k_wave2 / k_wave_g instantiation, matched by shape (template arguments).  A trailing HPG = false argument
(the hyperparameter-group switch, csrc/sfl_kwave_g.h) is dropped, so a library with it compares against one from
before it; HPG = true kernels are listed on their own.  Exit status 1 if a kernel present in both differs.
Usage: python scripts/kres_diff.py OLD.so NEW.so [--md]"""
import re
import subprocess
import sys
import tempfile

import struct

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
    size = {}
    for line in syms.splitlines():
        w = line.split()
        if len(w) >= 8 and w[3] == "FUNC":
            size[w[7]] = int(w[2], 0)
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        # (Itanium mangling: k_waveILi8ELi2ELb1E...E -- integer and bool template arguments only)
        m = re.search(r"\d+(k_wave_g|k_wave2|k_wave)I((?:L[ib]\d+E)+)E", name)
        if not m:
            continue
        args = [("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([ib])(\d+)E", m.group(2))]
        full = {"k_wave": 6, "k_wave2": 6, "k_wave_g": 9}[m.group(1)]
        hpg = len(args) == full and args[-1] == "true"
        if len(args) == full:
            args = args[:-1]
        key = ("HPG " if hpg else "") + m.group(1) + "<" + ",".join(args) + ">"
        vals = [int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in FIELDS]
        out[key] = vals + [size.get(name, -1)]
    return out


def main(old, new, md=False):
    a, b = kernels(old), kernels(new)
    head = ["kernel", "vgpr", "sgpr", "vspill", "sspill", "scratch", "lds", "code bytes", ""]
    rows, bad = [], 0
    for k in sorted(set(a) | set(b)):
        if k in a and k in b:
            same = a[k] == b[k]
            bad += not same
            rows.append([k] + [str(x) if x == y else f"{x} -> {y}" for x, y in zip(a[k], b[k])] + ["equal" if same else "DIFFERS"])
        else:
            rows.append([k] + [str(x) for x in (a.get(k) or b[k])] + ["old only" if k in a else "new only"])
    if md:
        print("| " + " | ".join(head) + " |\n|" + "---|" * len(head))
        for r in rows:
            print("| " + " | ".join(r) + " |")
    else:
        for r in [head] + rows:
            print(f"{r[0]:64s}" + "".join(f"{x:>12s}" for x in r[1:]))
    print(f"{sum(1 for k in a if k in b)} kernels in both, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], "--md" in sys.argv))
