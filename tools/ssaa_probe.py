"""Measurement probe of the supersampling resolve (run from the repo root).
  trace: resolve_box<2>, resolve_box<4> and blit_kernel at a 3840x2160 output (for rocprofv3 --kernel-trace)
  cost:  frm_render(stats) kernel_ms, headline workload: 3840x2160 at S = 2 against plain 7680x4320, alternating
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fractal-ray-marching_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import frm  # noqa: E402

W, H = 3840, 2160
wl = frm.WORKLOADS["HEADLINE"]


def trace():
    torch.manual_seed(1)
    with frm.Renderer(max_steps=wl.max_steps) as r:
        dst = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
        for S in (2, 4):
            src = torch.randint(0, 256, (S * S * W * H * 4,), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            for _ in range(25):
                r.resolve(src.data_ptr(), src.numel(), W, H, S, dst.data_ptr(), dst.numel())
            r.synchronize()
            del src
        # blit_kernel at the same output size: a 4K frame presented at 4K (sRGB)
        r.resize(W, H)
        r.update_parameters_buffer(frm.make_parameters(wl, pose="P1"))
        r.render(stats=False)
        for _ in range(25):
            r.present(W, H, srgb=True)
    print("trace done")


def cost():
    p = frm.make_parameters(wl, pose="P1")  # aspect from 3840x2160 (= 7680x4320's)
    with frm.Renderer(max_steps=wl.max_steps, supersampling=2) as ss, frm.Renderer(max_steps=wl.max_steps) as plain:
        ss.resize(W, H)
        plain.resize(2 * W, 2 * H)
        for r in (ss, plain):
            r.update_parameters_buffer(p)
        ms = {"ssaa2_3840x2160": [], "plain_7680x4320": []}
        steps = {}
        for rep in range(10):
            for name, r in (("ssaa2_3840x2160", ss), ("plain_7680x4320", plain)):
                st = r.render(stats=True)
                steps[name] = st["march_steps"]
                if rep >= 2:  # two warm-up rounds (first launch, scheduled order)
                    ms[name].append(st["kernel_ms"])
        a = ss.read_frame()
        b = plain.read_frame()
    out = {k: {"kernel_ms": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
               "min": round(min(v), 3), "max": round(max(v), 3), "march_steps": steps[k]} for k, v in ms.items()}
    out["shapes"] = [list(a.shape), list(b.shape)]
    print(json.dumps(out))


if __name__ == "__main__":
    {"trace": trace, "cost": cost}[sys.argv[1]]()
