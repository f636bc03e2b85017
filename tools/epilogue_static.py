#!/usr/bin/env python3
"""Static counts per kernel of a device-only assembly listing (hipcc ... -S --cuda-device-only): instructions, and what
sits behind the kernel's last MFMA -- scalar loads, drained scalar waits, branches, global stores -- with the register,
scratch and occupancy lines the compiler prints.  tools/epilogue_static.py LISTING.s [substring of the demangled name]

(The table of profiles/conv2d_epilogue_args.txt: parent against change for conv2d_f16s_kernel.)"""
import re
import subprocess
import sys


def kernels(path):
    name, body = None, []
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        body.append(line)
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            pass
        if re.match(r"^; Occupancy:", line):
            yield name, body
            name = None


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "conv2d_f16s_kernel"
    rows = []
    for name, body in kernels(path):
        dem = subprocess.run(["c++filt", name], stdout=subprocess.PIPE, text=True).stdout.strip()
        if want not in dem:
            continue
        short = re.sub(r"\(.*", "", re.sub(r"^void ", "", dem))
        ins = [ln.split()[0] for ln in body if ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;")
               and ln.split()]
        text = [ln for ln in body if ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;") and ln.split()]
        last = max((i for i, op in enumerate(ins) if op.startswith("v_mfma")), default=-1)
        tail_ops, tail_txt = ins[last + 1:], text[last + 1:]
        meta = "".join(ln for ln in body if ln.startswith(";"))
        get = lambda k: (re.search(r"; %s: (\d+)" % k, meta) or [None, "?"])[1]
        rows.append((short, len(ins), len(tail_ops),
                     sum(op.startswith("s_load_dword") for op in ins),
                     sum(op.startswith("s_load_dword") for op in tail_ops),
                     sum(1 for t in tail_txt if t.split()[0] == "s_waitcnt" and "lgkmcnt(0)" in t),
                     sum(op.startswith("s_cbranch") for op in tail_ops),
                     sum(op.startswith("global_store") for op in tail_ops),
                     get("NumVgprs"), get("NumSgprs"), get("ScratchSize"), get("Occupancy")))
    print("%-46s %6s %6s %6s %6s %6s %6s %6s %5s %5s %7s %4s" % ("kernel", "instr", "tail", "sload", "t.sld", "t.lgkm0", "t.br",
                                                                "t.st", "vgpr", "sgpr", "scratch", "occ"))
    for r in sorted(rows):
        print("%-46s %6d %6d %6d %6d %6d %6d %6d %5s %5s %7s %4s" % r)


if __name__ == "__main__":
    main()
