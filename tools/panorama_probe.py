"""Measurement probe of the panorama (run from the repo root; needs a GPU).

  python tools/panorama_probe.py [--part all|kernel|frame] [--reps N] [--warmup K] [--frames F] [--out FILE.json]

With --part all (the default) each part runs once in a child process of its own under its own time
limit, and the probe stops at the first part that fails.

1. kernel: project_equirect alone at a 4096x2048 panorama with the default face size (N = 1024,
   faces of 1026^2 random texels) through frm_project_equirect, and blit_kernel's linear path
   (2048x1024 -> 4096x2048) through frm_blit at the same output size as the bandwidth yardstick,
   alternating call by call on one stream, each call between two device events. Bytes moved counts
   what the algorithm must move once: the source texels plus the output (the projection also reads
   its 2W + 2H table floats); the four taps per pixel mostly hit the caches. Calls of tens of
   microseconds carry the events' own resolution.
2. frame: the headline scene as a 4096x2048 panorama: frm_render on a panorama context (kernel_ms)
   against the same six face parameter sets through frm_render_bands_batch alone on a plain
   1026x1026 context (the same marching work without the projection), alternating.
Prints one JSON object with every time, its median, min and max.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fractal-ray-marching_amd")):
    sys.path.insert(0, p)

import frm  # noqa: E402

W, H = 4096, 2048
wl = frm.WORKLOADS["HEADLINE"]
LIMITS = {"kernel": 240, "frame": 420}  # seconds per part


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "ms": [round(x, 4) for x in ms]}


def kernel_part(torch, reps, warmup):
    n = frm.panorama_face_size(W)
    m = n + 2
    bw, bh = W // 2, H // 2  # the blit's source: magnified, so its linear path runs
    stream = torch.cuda.Stream()  # (the default stream's handle is NULL, which libfrm reads as its own stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    faces = torch.randint(0, 256, (6 * m * m * 4,), dtype=torch.uint8, device="cuda", generator=g)
    src = torch.randint(0, 256, (bw * bh * 4,), dtype=torch.uint8, device="cuda", generator=g)
    dst = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = {"project_equirect": [], "blit_linear": []}
    with frm.Renderer(max_steps=64) as r:
        for rep in range(warmup + reps):
            for name in ms:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                if name == "blit_linear":
                    r.blit(src.data_ptr(), src.numel(), bw, bh, dst.data_ptr(), dst.numel(), W, H,
                           stream=stream.cuda_stream)
                else:
                    r.project_equirect(faces.data_ptr(), faces.numel(), m * m * 4, n, dst.data_ptr(), dst.numel(), W, H,
                                       stream=stream.cuda_stream)
                b.record(stream)
                b.synchronize()
                if rep >= warmup:
                    ms[name].append(a.elapsed_time(b))
    out = {"face_size": n}
    moved = {"project_equirect": 6 * m * m * 4 + W * H * 4 + (2 * W + 2 * H) * 4, "blit_linear": bw * bh * 4 + W * H * 4}
    for name in ms:
        c = summary(ms[name])
        c["bytes"] = moved[name]
        c["gathered_bytes"] = 16 * W * H  # four dword taps per output pixel, before the caches
        c["median_tbytes_per_s"] = round(c["bytes"] / (c["median_ms"] * 1e-3) / 1e12, 3)
        c["best_tbytes_per_s"] = round(c["bytes"] / (c["min_ms"] * 1e-3) / 1e12, 3)
        out[name] = c
    return out


def frame_part(torch, frames, warmup):
    n = frm.panorama_face_size(W)
    m = n + 2
    p = frm.make_parameters(wl, pose="P1", width=W, height=H)
    faces = frm.panorama_parameters(p, n)
    stream = torch.cuda.Stream()
    buf = torch.zeros(6 * m * m * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = {"render_panorama": [], "bands_batch_6": []}
    with frm.Renderer(max_steps=wl.max_steps, panorama=n) as rp, frm.Renderer(max_steps=wl.max_steps) as rb:
        rp.resize(W, H)
        rp.update_parameters_buffer(p)
        rb.resize(m, m)
        for rep in range(warmup + frames):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = rp.render(stats=True)
            a.record(stream)
            rb.render_bands_batch(faces, buf.data_ptr(), dst_bytes=buf.numel(), frame_stride=m * m * 4, band_rows=m,
                                  first_band=0, band_stride=1, stream=stream.cuda_stream)
            b.record(stream)
            b.synchronize()
            if rep >= warmup:
                ms["render_panorama"].append(st["kernel_ms"])
                ms["bands_batch_6"].append(a.elapsed_time(b))
        steps, pixels = st["march_steps"], st["pixels"]
    out = {"face_size": n, "render_panorama": summary(ms["render_panorama"]), "bands_batch_6": summary(ms["bands_batch_6"]),
           "march_steps": steps, "pixels": pixels}
    out["projection_ms"] = round(out["render_panorama"]["median_ms"] - out["bands_batch_6"]["median_ms"], 4)
    out["overhead"] = round(out["render_panorama"]["median_ms"] / out["bands_batch_6"]["median_ms"] - 1.0, 4)
    return out


def run_part(part, args):
    import torch
    if frm.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("panorama_probe: no HIP device visible")
    if part == "kernel":
        return kernel_part(torch, args.reps, args.warmup)
    return frame_part(torch, args.frames, args.warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["all", "kernel", "frame"], default="all")
    ap.add_argument("--reps", type=int, default=40, help="timed calls per kernel case")
    ap.add_argument("--frames", type=int, default=10, help="timed frames per frame case")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    out = {"width": W, "height": H, "reps": args.reps, "frames": args.frames, "warmup": args.warmup}
    if args.part != "all":
        out[args.part] = run_part(args.part, args)
    else:  # each part once, in a fresh process under its own time limit; a failure ends the probe
        for part in ("kernel", "frame"):
            cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(args.reps), "--frames",
                   str(args.frames), "--warmup", str(args.warmup)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[part])
            if res.returncode != 0:
                sys.stderr.write(res.stderr)
                sys.exit(f"panorama_probe: part {part} failed with status {res.returncode}")
            out[part] = json.loads(res.stdout.strip().splitlines()[-1])[part]
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
