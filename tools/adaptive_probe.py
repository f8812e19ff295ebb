"""Measurement probe of adaptive supersampling (run from the repo root; needs a GPU).

  python tools/adaptive_probe.py [--frames N] [--warmup K] [--baseline-only] [--out FILE.json]

The headline workload at its own size (3840x2160, scene 18, N = 12, 256 steps, pose P1), kernel_ms of
frm_render(stats), the cases alternating frame by frame within this process: plain,
frm_set_supersampling(2), adaptive S = 2 at thresholds 8, 16, 32, 64 and adaptive S = 4 at 16. One
context per case, all alive at once. A library without frm_set_adaptive (FRM_LIB = a build of an
earlier commit), or --baseline-only, runs the first two cases only: the yardstick the others are
compared with, and the check that this build's existing paths match the earlier commit's. Prints
one JSON object: per case the times, their median, min and max, the refined share phi = R / (W H)
and, for the adaptive cases, the efficiency e = (t_A - t_plain) / (phi * t_SSAA) with this run's
medians (1 = a refined pixel costs what a pixel of the supersampled frame costs).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fractal-ray-marching_amd")):
    sys.path.insert(0, p)

import frm  # noqa: E402

W, H = 3840, 2160
wl = frm.WORKLOADS["HEADLINE"]
ADAPTIVE_CASES = [(2, 8), (2, 16), (2, 32), (2, 64), (4, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-only", action="store_true", help="plain and SSAA-2 only, as a library without the feature runs")
    ap.add_argument("--out")
    args = ap.parse_args()
    if frm.device_count() < 1:
        sys.exit("adaptive_probe: no HIP device visible")
    has_adaptive = hasattr(frm.load(), "frm_set_adaptive") and not args.baseline_only
    p = frm.make_parameters(wl, pose="P1", width=W, height=H)
    cases = [("plain", {}), ("ssaa2", {"supersampling": 2})]
    if has_adaptive:
        cases += [(f"adaptive{S}_t{T}", {"adaptive": (S, T)}) for S, T in ADAPTIVE_CASES]
    renderers = []
    try:
        for name, kw in cases:
            r = frm.Renderer(max_steps=wl.max_steps, **kw)
            r.resize(W, H)
            r.update_parameters_buffer(p)
            renderers.append((name, kw, r))
        ms = {name: [] for name, _ in cases}
        last = {}
        for rep in range(args.warmup + args.frames):
            for name, kw, r in renderers:
                st = r.render(stats=True)
                last[name] = st
                if rep >= args.warmup:  # the first launches allocate and fetch in row-major order
                    ms[name].append(st["kernel_ms"])
    finally:
        for _, _, r in renderers:
            r.close()
    out = {"width": W, "height": H, "frames": args.frames, "warmup": args.warmup, "library": os.path.relpath(frm.LIB_PATH, ROOT),
           "has_adaptive": has_adaptive, "cases": {}}
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, kw in cases:
        v, st = ms[name], last[name]
        c = {"median_ms": round(med[name], 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
             "kernel_ms": [round(x, 3) for x in v], "pixels": st["pixels"], "march_steps": st["march_steps"]}
        if "adaptive" in kw:
            S = kw["adaptive"][0]
            refined = (st["pixels"] - W * H) // (S * S)
            phi = refined / (W * H)
            c.update(factor=S, threshold=kw["adaptive"][1], refined_pixels=refined, phi=round(phi, 5))
            if S == 2 and phi > 0:
                c["efficiency"] = round((med[name] - med["plain"]) / (phi * med["ssaa2"]), 3)
            c["vs_ssaa2"] = round(med[name] / med["ssaa2"], 3)
        out["cases"][name] = c
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
