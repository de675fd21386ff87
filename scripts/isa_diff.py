"""Compare the gfx950 machine code of two builds of libmmego_hip.so kernel by kernel (no GPU needed): the check behind a refactor
that must not change what any kernel computes.

    python scripts/isa_diff.py OLD.so NEW.so [--rename OLD_KERNEL=NEW_KERNEL ...]

--rename (repeatable) pairs a kernel that changed its symbol with its predecessor: both sides are matched on the demangled name without
its parameter list, e.g. --rename 'adam_kernel=adam_step_kernel<false, false, false>', and the pair gets one verdict like any other.

Per kernel symbol one verdict:
  identical  the instruction text is equal (addresses and encodings dropped).
  reordered  the same instructions in another order or in other registers: the multiset of mnemonics is equal (s_nop and s_waitcnt
             left out -- their counts follow the schedule, not the arithmetic), scratch size, spill counts and LDS size of the kernel
             metadata are equal, and the VGPR + AGPR count allows the same number of waves per SIMD (512 / count rounded up to 8).
             Changed raw register counts are printed.
  DIFFERENT  anything else: an expression was regrouped, a statement was lost or added.
Exit status 0 when both libraries hold the same kernel symbols and none is DIFFERENT."""
import collections
import re
import shutil
import subprocess
import sys
import tempfile

from isa_pk_scan import OBJDUMP, device_code_objects

READELF = OBJDUMP.replace("llvm-objdump", "llvm-readelf")
CXXFILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")       # (only --rename needs it)
SCHEDULE_ONLY = ("s_nop", "s_waitcnt")
META_EQUAL = ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size")
META_REGS = ("vgpr_count", "agpr_count", "sgpr_count")


def kernels(lib):
    """-> {kernel symbol: (instruction lines, metadata dict)} over every gfx950 code object of the library."""
    out = {}
    for co in device_code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as fh:
            fh.write(co)
            fh.flush()
            txt = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", fh.name], capture_output=True, text=True, check=True).stdout
            notes = subprocess.run([READELF, "--notes", fh.name], capture_output=True, text=True, check=True).stdout
        meta, cur = {}, None
        for line in notes.splitlines():
            m = re.match(r"^  - \.(\w+):\s*(.*)$", line)
            if m:
                cur = {}
            else:
                m = re.match(r"^    \.(\w+):\s*(.*)$", line)
            if m and cur is not None:
                cur[m.group(1)] = m.group(2)
                if m.group(1) == "name":
                    meta[m.group(2)] = cur
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                assert m.group(1) not in out, "kernel symbol twice: " + m.group(1)
                cur = out[m.group(1)] = ([], meta.get(m.group(1), {}))
            elif cur is not None and line.startswith("\t"):
                ins, _, enc = line.partition("//")
                cur[0].append((ins.strip(), enc.split(":")[-1].split("<")[0].split()))
    for ins, _ in out.values():
        # the fill between one kernel's last instruction and the next kernel's aligned start is not code: zero words (they decode
        # as v_cndmask_b32 v0, s0, v0, vcc), s_code_end, and behind the last kernel of a section a run of s_nop
        while ins and (ins[-1][0].startswith(("s_code_end", "s_nop")) or set(ins[-1][1]) <= {"00000000"}):
            ins.pop()
        ins[:] = [i for i, _ in ins]
    return out


def waves_per_simd(meta):
    regs = int(meta.get("vgpr_count", 0)) + int(meta.get("agpr_count", 0))
    return 512 // max(8, (regs + 7) // 8 * 8)


def mnemonics(ins):
    return collections.Counter(w for w in (i.split()[0] for i in ins if i) if w not in SCHEDULE_ONLY)


def verdict(old, new):
    """-> (verdict, note) of one kernel present in both libraries."""
    (oi, om), (ni, nm) = old, new
    regs = ", ".join("%s %s -> %s" % (k, om.get(k), nm.get(k)) for k in META_REGS if om.get(k) != nm.get(k))
    if oi == ni:
        return "identical", regs
    why = []
    if mnemonics(oi) != mnemonics(ni):
        d = mnemonics(ni)
        d.subtract(mnemonics(oi))
        why.append("mnemonics " + " ".join("%s%+d" % (k, v) for k, v in sorted(d.items()) if v))
    why += ["%s %s -> %s" % (k, om.get(k), nm.get(k)) for k in META_EQUAL if om.get(k) != nm.get(k)]
    if waves_per_simd(om) != waves_per_simd(nm):
        why.append("waves per SIMD %d -> %d" % (waves_per_simd(om), waves_per_simd(nm)))
    return ("DIFFERENT" if why else "reordered"), "; ".join(why + ([regs] if regs else []))


def short_names(symbols):
    """-> {demangled name without return type and parameter list: symbol}"""
    symbols = sorted(symbols)
    txt = subprocess.run([CXXFILT], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout
    return {re.sub(r"^void ", "", d).split("(")[0]: s for s, d in zip(symbols, txt.splitlines())}


def main(old_lib, new_lib, renames=()):
    old, new = kernels(old_lib), kernels(new_lib)
    old_short, new_short = (short_names(old), short_names(new)) if renames else ({}, {})
    for was, now in renames:
        if was not in old_short or now not in new_short:
            sys.exit("--rename %s=%s: no such kernel in %s" % (was, now, old_lib if was not in old_short else new_lib))
        label = "%s -> %s" % (was, now)
        old[label], new[label] = old.pop(old_short[was]), new.pop(new_short[now])
    counts = collections.Counter()
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            v, note = "DIFFERENT", "only in " + (new_lib if name in new else old_lib)
        else:
            v, note = verdict(old[name], new[name])
        counts[v] += 1
        print("%-9s %s%s" % (v, name, "   [" + note + "]" if note else ""))
    print("%d kernels: %d identical, %d reordered, %d DIFFERENT" % (sum(counts.values()), counts["identical"], counts["reordered"], counts["DIFFERENT"]))
    return 1 if counts["DIFFERENT"] else 0


if __name__ == "__main__":
    args, renames = sys.argv[1:], []
    while "--rename" in args:
        i = args.index("--rename")
        if i + 1 >= len(args) or "=" not in args[i + 1]:
            sys.exit(__doc__)
        renames.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1], renames))
