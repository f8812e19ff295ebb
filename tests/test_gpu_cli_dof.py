"""bin/frm_render --dof-aperture A --dof-focus F [--dof-radius R] [--depth-out file.pfm] on the GPU:
the written PPM equals the context mode's frame (and the reference's gather of the oracle's frame),
the PFM equals Renderer.read_depth(), and the options --dof-* excludes exit with status 2."""
import json
import os
import subprocess

import numpy as np
import pytest

import dof_reference as ref
import frm

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fractal-ray-marching_amd",
                   "bin", "frm_render")

W, H = 48, 36
POS, YAW, PITCH, ITERS, TIME, STEPS = (0.1, 0.2, -2.5), 0.2, -0.1, 4, frm.POWER8_TIME, 64
A, F, R = 6.0, 1.8, 7


def read_ppm(path):
    with open(path, "rb") as fh:
        data = fh.read()
    header, rest = data.split(b"\n", 1)
    dims, rest = rest.split(b"\n", 1)
    maxv, pix = rest.split(b"\n", 1)
    w, h = (int(v) for v in dims.split())
    assert header == b"P6" and maxv == b"255"
    return np.frombuffer(pix, np.uint8).reshape(h, w, 3)


def read_pfm(path):
    """A single-channel PFM: "Pf", the size, a negative scale for little-endian floats, then the rows
    bottom first."""
    with open(path, "rb") as fh:
        data = fh.read()
    header, rest = data.split(b"\n", 1)
    dims, rest = rest.split(b"\n", 1)
    scale, pix = rest.split(b"\n", 1)
    w, h = (int(v) for v in dims.split())
    assert header == b"Pf" and float(scale) < 0 and len(pix) == 4 * w * h
    return np.frombuffer(pix, "<f4").reshape(h, w)[::-1]


def cli(out, *extra):
    cmd = [EXE, "--width", str(W), "--height", str(H), "--pos", *map(str, POS), "--yaw", str(YAW), "--pitch", str(PITCH),
           "--iters", str(ITERS), "--time", str(TIME), "--max-steps", str(STEPS), "--scene", "18", "--out", out, *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def start_parameters():
    p = frm.Parameters()
    p.update_aspect(W, H)
    p.time, p.num_iterations, p.scene_index = TIME, ITERS, 18
    p.update_camera(frm.Camera(POS, YAW, PITCH))
    return p


def test_cli_depth_of_field_matches_the_context_and_the_reference(tmp_path, frm_lib, oracle):
    out, pfm = str(tmp_path / "dof.ppm"), str(tmp_path / "depth.pfm")
    res = cli(out, "--dof-aperture", str(A), "--dof-focus", str(F), "--dof-radius", str(R), "--depth-out", pfm)
    assert res.returncode == 0, res.stderr
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert (line["dof_aperture"], line["dof_focus"], line["dof_radius"]) == (A, F, R)
    assert (line["ssaa"], line["adaptive"], line["shutter_samples"], line["panorama"]) == (1, 1, 1, 0)
    p = start_parameters()
    with frm.Renderer(max_steps=STEPS, depth_of_field=(A, F, R)) as r:
        r.resize(W, H)
        r.update_parameters_buffer(p)
        st = r.render(stats=True)
        frame, depth = r.read_frame(), r.read_depth()
    got = read_ppm(out)
    assert got.shape == (H, W, 3) and np.array_equal(got, frame[..., :3])
    z = read_pfm(pfm)
    assert z.shape == (H, W) and np.array_equal(z.view(np.uint32), depth.view(np.uint32))
    assert np.isinf(z).any() and np.isfinite(z).any()
    plain = oracle.render(p, W, H, STEPS)
    assert np.array_equal(frame, ref.gather(plain["rgba"], depth, A, F, R, oracle))
    assert line["march_steps"] == st["march_steps"] == int(plain["counters"][2]) + int(plain["counters"][3])
    assert line["hit_pixels"] == int(plain["counters"][1])
    assert np.any(got != plain["rgba"][..., :3])  # blurred


def test_cli_depth_out_of_a_plain_frame_and_the_default_radius(tmp_path, frm_lib, oracle):
    out, pfm = str(tmp_path / "plain.ppm"), str(tmp_path / "depth.pfm")
    # (48 x 36 would run on the simple kernel, which leaves no depth: --depth-out says so)
    res = cli(out, "--depth-out", pfm)
    assert res.returncode == 1 and "frm_read_depth" in res.stderr
    res = cli(out, "--dof-aperture", "0", "--dof-focus", str(F), "--depth-out", pfm)
    assert res.returncode == 0, res.stderr
    line = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][0])
    assert (line["dof_aperture"], line["dof_focus"], line["dof_radius"]) == (0.0, F, frm.FRM_MAX_DOF_RADIUS)
    plain = oracle.render(start_parameters(), W, H, STEPS, trace=True)
    assert np.array_equal(read_ppm(out), plain["rgba"][..., :3])  # no aperture: the plain frame
    assert np.array_equal(np.isfinite(read_pfm(pfm)), plain["trace"][..., 0] > 0)


def test_cli_plain_lines_report_no_depth_of_field(tmp_path, frm_lib):
    res = cli(str(tmp_path / "plain.ppm"))
    assert res.returncode == 0, res.stderr
    line = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][0])
    assert (line["dof_aperture"], line["dof_focus"], line["dof_radius"]) == (0.0, 0.0, 0)


def test_cli_refuses_the_excluded_combinations_and_bad_values(tmp_path):
    """Each refusal by its own words: an unknown flag exits with status 2 as well."""
    lens = ("--dof-aperture", "4", "--dof-focus", "2")
    out = str(tmp_path / "f.ppm")

    def refused(words, *args):
        res = cli(out, *args)
        assert res.returncode == 2 and words in res.stderr and "unknown argument" not in res.stderr, (args, res.stderr)

    for extra in (("--ssaa", "2"), ("--adaptive", "2"), ("--shutter-samples", "3"), ("--panorama",), ("--batch", "2"),
                  ("--gpus", "1")):
        refused("--dof-* excludes --ssaa, --adaptive, --shutter-samples, --panorama, --batch and --gpus", *lens, *extra)
    refused("--dof-* excludes --simple", *lens, "--simple")
    for args in (("--dof-aperture", "4"), ("--dof-focus", "2"), ("--dof-radius", "4")):
        refused("needs both --dof-aperture and --dof-focus", *args)
    for value in ("-1", "nan", "inf", "x", "4x"):
        refused(f"--dof-aperture {value}: not a finite non-negative number", "--dof-aperture", value, "--dof-focus", "2")
    for value in ("0", "-2", "nan", "inf", "x"):
        refused(f"--dof-focus {value}: not a finite positive number", "--dof-aperture", "4", "--dof-focus", value)
    for value in ("0", "17", "x"):
        refused(f"--dof-radius {value} outside [1, 16]", *lens, "--dof-radius", value)
    for extra in (("--batch", "2"), ("--gpus", "1"), ("--panorama",), ("--shutter-samples", "3")):
        refused("--depth-out excludes --batch, --gpus, --panorama and --shutter-samples", "--depth-out",
                str(tmp_path / "d.pfm"), *extra)
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "d.pfm"))
