"""Measurement probe of the depth of field (run from the repo root; needs a GPU).

  python tools/dof_probe.py [--frames F] [--reps N] [--warmup K] [--radius R] [--aperture A] [--label NAME]
                            [--out FILE.json]

On the 4K headline frame (3840x2160, pose P1), with the focus at the pose's median hit distance:
1. frame: frm_render's kernel_ms on one context with the effect on (R, A, F) and off, alternating
   frame by frame (a change of the lens needs no drain), medians; before that the plain frame on its
   own (plain_alone). With FRM_LIB set to a library without the feature only plain_alone is timed
   (the baseline of the parent commit).
2. gather: dof_gather alone through frm_depth_of_field on the frame and the depth plane of part 1,
   each call between two device events.
Prints one JSON object with every time, its median, min and max, and the gather's VALU bound:
(2R+1)^2 window positions x 10 lane-operations per pixel over the device's f32 lanes
(CUs x 64 lanes x --clock-ghz, one operation per lane and clock).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fractal-ray-marching_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import frm  # noqa: E402

wl = frm.WORKLOADS["HEADLINE"]
W, H = wl.width, wl.height


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "ms": [round(x, 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10, help="timed frames per case")
    ap.add_argument("--reps", type=int, default=10, help="timed calls of the gather alone")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radius", type=int, default=16)
    ap.add_argument("--aperture", type=float, default=8.0)
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="engine clock of the VALU bound (MI355X peak: 2.4)")
    ap.add_argument("--label", help="recorded as the run's library instead of the library's path")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    if frm.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("dof_probe: no HIP device visible")
    has_dof = hasattr(frm.load(), "frm_set_depth_of_field") and hasattr(frm.Renderer, "set_depth_of_field")
    out = {"width": W, "height": H, "radius": args.radius, "aperture": args.aperture, "frames": args.frames,
           "warmup": args.warmup, "library": args.label or os.path.relpath(frm.LIB_PATH, ROOT), "has_depth_of_field": has_dof}
    p = frm.make_parameters(wl, pose="P1", width=W, height=H)
    ms = {"plain": [], "depth_of_field": []}
    with frm.Renderer(max_steps=wl.max_steps) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        st = r.render(stats=True)
        out["march_steps"], out["hit_pixels"] = st["march_steps"], st["hit_pixels"]
        focus = 1.0
        if has_dof:
            z = r.read_depth()
            focus = float(np.median(z[np.isfinite(z)]))
            out["focus"] = focus
        for rep in range(args.warmup + args.frames):  # the plain frame on its own first, as a library without the feature runs it
            st = r.render(stats=True)
            if rep >= args.warmup:
                ms.setdefault("plain_alone", []).append(st["kernel_ms"])
        out["plain_alone"] = summary(ms.pop("plain_alone"))
        for rep in range(args.warmup + args.frames if has_dof else 0):
            for name in ms:
                if name == "depth_of_field":
                    if not has_dof:
                        continue
                    r.set_depth_of_field(args.aperture, focus, args.radius)
                elif has_dof:
                    r.set_depth_of_field(0.0, 1.0, 0)
                st = r.render(stats=True)
                if rep >= args.warmup:
                    ms[name].append(st["kernel_ms"])
        if has_dof:
            out["plain"] = summary(ms["plain"])
            out["depth_of_field"] = summary(ms["depth_of_field"])
            out["added_ms"] = round(out["depth_of_field"]["median_ms"] - out["plain"]["median_ms"], 4)
            # the gather alone, on the plain frame and its depth plane
            r.set_depth_of_field(0.0, 1.0, 0)
            r.render(stats=False)
            frame, z = r.read_frame(), r.read_depth()
            c = frm.dof_coc(args.aperture, focus, args.radius, z)
            out["coc"] = {"mean": round(float(c.mean()), 3), "at_limit": round(float((c >= args.radius).mean()), 4),
                          "below_one": round(float((c < 1).mean()), 4)}
            src = torch.from_numpy(frame).cuda()
            dep = torch.from_numpy(z).cuda()
            dst = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
            stream = torch.cuda.Stream()
            torch.cuda.synchronize()
            gather = []
            for rep in range(args.warmup + args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                r.depth_of_field(src.data_ptr(), src.numel(), dep.data_ptr(), dep.numel() * 4, W, H, args.aperture, focus,
                                 args.radius, dst.data_ptr(), dst.numel(), stream=stream.cuda_stream)
                b.record(stream)
                b.synchronize()
                if rep >= args.warmup:
                    gather.append(a.elapsed_time(b))
            out["gather"] = summary(gather)
            props = torch.cuda.get_device_properties(0)
            lanes, ghz = props.multi_processor_count * 64, args.clock_ghz
            ops = (2 * args.radius + 1) ** 2 * 10 * W * H
            out["valu_bound"] = {"cus": props.multi_processor_count, "clock_ghz": round(ghz, 3), "lane_ops": ops,
                                 "ms": round(ops / (lanes * ghz * 1e9) * 1e3, 4)}
            out["gather_over_bound"] = round(out["gather"]["median_ms"] / out["valu_bound"]["ms"], 3)
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
