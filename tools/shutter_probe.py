"""Measurement probe of motion blur (run from the repo root; needs a GPU).

  python tools/shutter_probe.py [--reps N] [--warmup K] [--frames F] [--out FILE.json]

1. kernel: the accumulation at a 3840x2160 output for (T, S) = (8, 1) and (4, 2) through
   frm_accumulate, and resolve_box<2> through frm_resolve at the same output size, alternating call by
   call on one stream, each call between two device events. Achieved bytes/s counts what the
   algorithm must move per output pixel: T*S*S*4 + 4 bytes for the accumulation, S*S*4 + 4 for
   the resolve (random texels, so every pixel's table look-ups differ).
2. frame: the headline scene at 3840x2160, 8 sub-frames of a 0.5 rad/s yaw-locked orbit over half
   a 60 Hz frame: frm_render_shutter against the same 8 frames through frm_render_bands_batch alone
   (the same marching work without the accumulation), alternating, each between two device events.
Prints one JSON object with every time, its median, min and max.
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
KERNEL_CASES = [("accumulate_T8_S1", 8, 1), ("accumulate_T4_S2", 4, 2), ("resolve_box_S2", 1, 2)]


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "ms": [round(x, 4) for x in ms]}


def kernel_part(torch, r, reps, warmup):
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL, which libfrm reads as its own stream)
    dst = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    srcs = {}
    for name, T, S in KERNEL_CASES:
        g = torch.Generator(device="cuda").manual_seed(T * 10 + S)
        srcs[name] = torch.randint(0, 256, (T * S * S * W * H * 4,), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in KERNEL_CASES}
    for rep in range(warmup + reps):
        for name, T, S in KERNEL_CASES:
            src = srcs[name]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            if name.startswith("resolve"):
                r.resolve(src.data_ptr(), src.numel(), W, H, S, dst.data_ptr(), dst.numel(), stream=stream.cuda_stream)
            else:
                r.accumulate(src.data_ptr(), src.numel(), src.numel() // T, T, W, H, S, divisor=T * S * S,
                             dst_ptr=dst.data_ptr(), dst_bytes=dst.numel(), stream=stream.cuda_stream)
            b.record(stream)
            b.synchronize()
            if rep >= warmup:
                ms[name].append(a.elapsed_time(b))
    out = {}
    for name, T, S in KERNEL_CASES:
        c = summary(ms[name])
        c["bytes_per_pixel"] = T * S * S * 4 + 4
        c["bytes"] = c["bytes_per_pixel"] * W * H
        c["median_gbytes_per_s"] = round(c["bytes"] / (c["median_ms"] * 1e-3) / 1e9, 1)
        c["best_gbytes_per_s"] = round(c["bytes"] / (c["min_ms"] * 1e-3) / 1e9, 1)
        out[name] = c
    return out


def frame_part(torch, frames, warmup):
    T = 8
    p = frm.make_parameters(wl, pose="P1", width=W, height=H)
    cam = frm.Camera(*frm.POSES["P1"])
    cam.raw.orbit_angle_per_second = 0.5
    cam.raw.lock_yaw_mode = 1
    subs = frm.shutter_parameters(p, cam, frm.Timing(), 0, frm.FRAME_SECONDS, T, 0.5)
    stream = torch.cuda.Stream()
    buf = torch.zeros(T * W * H * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = {"render_shutter_T8": [], "bands_batch_8": []}
    with frm.Renderer(max_steps=wl.max_steps) as rs, frm.Renderer(max_steps=wl.max_steps) as rb:
        rs.resize(W, H)
        rb.resize(W, H)
        for rep in range(warmup + frames):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = rs.render_shutter(subs, stats=True)
            a.record(stream)
            rb.render_bands_batch(subs, buf.data_ptr(), dst_bytes=buf.numel(), frame_stride=W * H * 4, band_rows=H,
                                  first_band=0, band_stride=1, stream=stream.cuda_stream)
            b.record(stream)
            b.synchronize()
            if rep >= warmup:
                ms["render_shutter_T8"].append(st["kernel_ms"])
                ms["bands_batch_8"].append(a.elapsed_time(b))
        steps = st["march_steps"]
    out = {"render_shutter_T8": summary(ms["render_shutter_T8"]), "bands_batch_8": summary(ms["bands_batch_8"]),
           "march_steps": steps}
    out["overhead"] = round(out["render_shutter_T8"]["median_ms"] / out["bands_batch_8"]["median_ms"] - 1.0, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40, help="timed calls per kernel case")
    ap.add_argument("--frames", type=int, default=10, help="timed frames per frame case")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    if frm.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("shutter_probe: no HIP device visible")
    with frm.Renderer(max_steps=64) as r:
        kernel = kernel_part(torch, r, args.reps, args.warmup)
    out = {"width": W, "height": H, "reps": args.reps, "frames": args.frames, "warmup": args.warmup,
           "kernel": kernel, "frame": frame_part(torch, args.frames, args.warmup)}
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
