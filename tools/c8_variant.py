#!/usr/bin/env python3
"""Builds a tools-side variant of csrc/conv_c8.hip (text substitutions: `--sub=A=>B`, several allowed) into
tools/_build/libdktstereo_c8<tag>.so -- timing-only ablations; the product source carries no ablation branches.  Run the variant
with DKT_LIB_PATH=<that library> in front of any tool (tools/window_kernels.py, bench.py ...).  The (chunk, tap) step lives in
csrc/c8_pipe.h: a copy of the header is written beside the variant source and every substitution is applied to both texts (it
must match in at least one).
    python tools/c8_variant.py --tag=noepi '--sub=        epilogue();\n        if (!have_next) break;=>        if (a.H < 0) epilogue();\n        if (!have_next) break;'
`noepi` (what round 6 used for VERDICT r05 item 6): every tile's epilogue behind a condition that is never true (the accumulators stay live) -- no gates, no stores: the difference to the
product library is the most that ANY overlap of one work item's epilogue with the next item's MFMAs could hide."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "_build")


PIPE_H = "c8_pipe.h"


def write_variant(B, src, subs, name):
    """Applies the (from, to) substitutions to the kernel text `src` and to csrc/c8_pipe.h, writes both into tools/_build
    (<name>.hip and its own <name>_pipe.h) and returns the path of the .hip file."""
    hdr = open(os.path.join(B.CSRC, PIPE_H)).read()
    for a, b in subs:
        assert a in src or a in hdr, a
        src, hdr = src.replace(a, b), hdr.replace(a, b)
    assert '#include "%s"' % PIPE_H in src
    src = src.replace('#include "%s"' % PIPE_H, '#include "%s_pipe.h"' % name)
    src = src.replace('#include "dkt_common.h"', '#include "%s/dkt_common.h"' % B.CSRC)
    os.makedirs(OUT, exist_ok=True)
    open(os.path.join(OUT, "%s_pipe.h" % name), "w").write(hdr)
    path = os.path.join(OUT, "%s.hip" % name)
    open(path, "w").write(src)
    return path


def main():
    from dkt_stereo_amd import build as B
    B.build()
    tag = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--tag=")] or ["variant"])[0]
    subs = [a.split("=", 1)[1].encode().decode("unicode_escape").split("=>") for a in sys.argv[1:] if a.startswith("--sub=")]
    path = write_variant(B, open(os.path.join(B.CSRC, "conv_c8.hip")).read(), subs, "conv_c8_%s" % tag)
    obj = os.path.join(OUT, "conv_c8_%s.o" % tag)
    subprocess.check_call([B.HIPCC] + B.CFLAGS + B.EXTRA_FLAGS["conv_c8"] + ["-I", B.CSRC, "-c", path, "-o", obj])
    objs = [os.path.join(B.OBJ_DIR, f) for f in sorted(os.listdir(B.OBJ_DIR)) if f.endswith(".o") and not f.startswith("conv_c8")]
    lib = os.path.join(OUT, "libdktstereo_c8%s.so" % tag)
    subprocess.check_call([B.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", obj] + objs + ["-o", lib])
    print(lib)


if __name__ == "__main__":
    main()
