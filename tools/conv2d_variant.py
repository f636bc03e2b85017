#!/usr/bin/env python3
"""Builds a variant of the library whose conv2d_f16s_kernel differs by a source substitution, under tools/_build (the way
tools/c8_variant.py does for conv_c8): the other objects are those of the last build, only conv2d.hip's seven units are recompiled.

    python tools/conv2d_variant.py --tag=noepi [--source=PATH/conv2d.hip]    ->  tools/_build/conv2d_noepi/libdktstereo.so

noepi: the tile's epilogue is compiled but never run (its call sits behind a test no launch satisfies), so full minus noepi
is the time the epilogues take.  Run a tool against the variant with DKT_LIB_PATH=tools/_build/conv2d_noepi/libdktstereo.so;
results are garbage by construction.  --source builds the variant of another revision's conv2d.hip (git show REV:... > file)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dkt_stereo_amd import build as B  # noqa: E402

SUBST = {"noepi": [("        epilogue();\n        if (!have_next) break;", "        if (a.nch16 < 0) epilogue();\n        if (!have_next) break;")]}


def main():
    opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
    tag = opts.get("tag", "noepi")
    src = opts.get("source", os.path.join(B.CSRC, "conv2d.hip"))
    out = os.path.join(ROOT, "tools", "_build", "conv2d_" + opts.get("name", tag))
    os.makedirs(out, exist_ok=True)
    text = open(src).read()
    for old, new in SUBST[tag]:
        assert text.count(old) == 1, "substitution target not found exactly once: %r" % old
        text = text.replace(old, new)
    var = os.path.join(out, "conv2d.hip")
    open(var, "w").write(text)
    jobs = [(tu, os.path.join(out, "conv2d_tu%d.o" % tu)) for tu in range(7)]

    def cc(job):
        tu, obj = job
        return subprocess.run([B.HIPCC] + B.CFLAGS + ["-I", B.CSRC, "-DCONV_TU_PASSES=%d" % tu, "-c", var, "-o", obj],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    with ThreadPoolExecutor(7) as pool:
        for res in pool.map(cc, jobs):
            if res.returncode != 0:
                sys.exit(res.stdout)
    others = sorted(os.path.join(B.OBJ_DIR, f) for f in os.listdir(B.OBJ_DIR) if f.endswith(".o") and not f.startswith("conv2d_tu"))
    lib = os.path.join(out, "libdktstereo.so")
    res = subprocess.run([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + others + [o for _, o in jobs] + ["-o", lib],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        sys.exit(res.stdout)
    print(lib)


if __name__ == "__main__":
    main()
