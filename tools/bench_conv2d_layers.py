#!/usr/bin/env python3
"""Stand-alone times of the encoder layers conv2d_f16s_kernel runs in the benchmark (HIP-event time over back-to-back launches,
us per launch): 96 -> 96 and 64 -> 96 stride 2 at 368 x 624, 128 -> 128 and 96 -> 128 stride 2 at 184 x 312; batches 1 and 2;
plain, in_norm + statistics, residual (what the stride allows).  One JSON line per row.

    [DKT_LIB_PATH=.../libdktstereo.so] python tools/bench_conv2d_layers.py [label]

Compare libraries in ONE job on one machine (the label is copied into every row)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dkt_stereo_amd import conv, extractor  # noqa: E402

DEV = "cuda:0"
LAYERS = [("96_96", 96, 96, 1, 368, 624), ("64_96_s2", 64, 96, 2, 368, 624), ("128_128", 128, 128, 1, 184, 312),
          ("96_128_s2", 96, 128, 2, 184, 312)]


def timeit(fn, n=40, warm=5, reps=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) * 1000.0 / n)
    best.sort()
    return best[len(best) // 2], best[0], best[-1]


@torch.no_grad()
def main():
    label = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DKT_LIB_PATH", "tree")
    torch.manual_seed(0)
    with conv.use_backend("f16x3"):
        for name, cin, cout, stride, H, W in LAYERS:
            layer = torch.nn.Conv2d(cin, cout, 3, stride=stride, padding=1).to(DEV)
            for B in (1, 2):
                x = torch.randn(B, cin, H, W, device=DEV)
                forms = [("plain", lambda: conv.conv2d(x, layer, relu=True))]
                if conv.stats_eligible(layer):
                    forms.append(("stats", lambda: conv.conv2d_stats(x, layer)))
                if stride == 1:
                    params = extractor.instance_norm_params(torch.nn.InstanceNorm2d(cin), x)
                    res = torch.randn(B, cout, H, W, device=DEV)
                    forms.append(("in_norm+stats", lambda: conv.conv2d_stats(x, layer, in_norm=params)))
                    forms.append(("residual", lambda: conv.conv2d_fused(x, layer, relu=True, residual=res)))
                for form, fn in forms:
                    med, lo, hi = timeit(fn)
                    print(json.dumps({"lib": label, "layer": name, "B": B, "form": form, "us": round(med, 1),
                                      "min": round(lo, 1), "max": round(hi, 1)}), flush=True)


if __name__ == "__main__":
    main()
