"""The GPU held to tests/f64_reference.py, the float64 restatement of the shader that shares nothing
with the oracle or the product source, by the rules of tests/f64_cases.py (the same ones
tests/test_f64_reference.py applies to the CPU oracle): distances and colours of every scene on
point sets that reach the iterations, whole frames of both kernels through invariants that do not
depend on the path a march took, and one supersampled frame against the float64 mean of its
float64-shaded samples. DESIGN.md, "Independent reference", has the measured figures."""
import numpy as np
import pytest

import f64_cases as fc
import f64_reference as ref
import frm

pytestmark = pytest.mark.gpu


def _fmt(fig):
    return {k: float(f"{v:.3g}") for k, v in fig.items()}


@pytest.fixture(scope="module")
def renderers(gpu_renderer_factory):
    """One renderer per flag set, made on first use and shared by the module's cases."""
    made = {}

    def get(flags, max_steps=0):
        if (flags, max_steps) not in made:
            made[(flags, max_steps)] = gpu_renderer_factory(max_steps=max_steps, flags=flags)
        return made[(flags, max_steps)]

    yield get
    for r in made.values():
        r.close()


# ---- distances -------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", fc.SCENES)
def test_gpu_distances(renderers, scene):
    sphere = scene == "sphere"
    for n in fc.ITERATIONS:
        for time in fc.TIMES:
            p, P, flags, pts, R = fc.distance_case(scene, n, time)
            fc.assert_coverage(R)
            r = renderers(flags)
            r.update_parameters_buffer(p)
            d, col = r.eval_scene(pts)
            label = f"gpu scene {scene} N={n} t={time}"
            fig = fc.check_distances(d, R, label)
            worst = fc.check_colors(col, P, sphere, pts, label)
            print(label, _fmt(fig), "colour ulp", round(worst, 2))


def test_gpu_mandelbulb_hardware_math(renderers):
    """FRM_FLAG_HW_MATH: the hardware transcendentals are not correctly rounded, so the only rule is the
    median relative error of the kept points, within 16 times the float32 reference's own."""
    r = renderers(frm.FRM_FLAG_HW_MATH)
    for n in fc.ITERATIONS:
        for time in fc.TIMES:
            p, P, flags, pts, R = fc.distance_case(18, n, time)
            r.update_parameters_buffer(p)
            d, _ = r.eval_scene(pts)
            k = R["keep"]
            with np.errstate(all="ignore"):
                rel = np.abs(d.astype(np.float64) - R["ref64"])[k] / np.abs(R["ref64"][k])
            lost = ~np.isfinite(rel)  # a NaN distance (the structured points on an axis) counts as an infinite error
            median = float(np.median(np.where(lost, np.inf, rel)))
            ratio = median / R["ref32_median"]
            print(f"hw math N={n} t={time}: median rel {median:.3g}, {ratio:.2f} x the float32 reference, "
                  f"{int(lost.sum())} of {int(k.sum())} kept points not finite")
            assert ratio <= 16.0, (n, time, median, R["ref32_median"])


# ---- frames ----------------------------------------------------------------------------------------

def _frame(r, F, trace):
    r.resize(F["width"], F["height"])
    r.update_parameters_buffer(F["params"])
    r.render(stats=True)
    return r.read_frame(), (r.trace() if trace else None)


@pytest.mark.parametrize("pose", list(fc.POSES))
@pytest.mark.parametrize("name", list(fc.FRAME_SCENES))
def test_gpu_frames(renderers, name, pose):
    for w, h in fc.FRAME_SIZES:
        F = fc.frame_reference(name, pose, w, h)
        label = f"gpu {name} {pose} {w}x{h}"
        rgba, trace = _frame(renderers(F["flags"] | frm.FRM_FLAG_PERSISTENT_KERNEL, fc.FRAME_STEPS), F, True)
        assert trace.shape == (h, w, 10)
        print(label, "persistent", _fmt(fc.check_frame(F, rgba, trace, label + " persistent")))
        simple, _ = _frame(renderers(F["flags"] | frm.FRM_FLAG_SIMPLE_KERNEL, fc.FRAME_STEPS), F, False)
        print(label, "simple", _fmt(fc.check_frame(F, simple, trace, label + " simple", bytes_only=True)))


def test_gpu_supersampled_sphere(gpu_renderer_factory):
    """Factor 2, output 48 x 36: every output pixel is the float64 box mean of its four sub-pixel
    colours, each shaded in float64 from the 96 x 72 trace (clamped to [0, 1] as the store clamps them,
    NaN and misses black), encoded again; within one code."""
    S, w, h = 2, 48, 36
    p, P, flags = fc.make_params("sphere", 0, 0.0, w, h, "hand")
    with gpu_renderer_factory(max_steps=fc.FRAME_STEPS, flags=flags | frm.FRM_FLAG_PERSISTENT_KERNEL) as r:
        r.set_supersampling(S)
        r.resize(w, h)
        r.update_parameters_buffer(p)
        r.render(stats=True)
        got = r.read_frame()
        tr = r.trace().reshape(-1, 10).astype(np.float64)
    assert got.shape == (h, w, 4) and len(tr) == S * S * w * h
    _, dirs = ref.camera_rays(P, S * w, S * h)
    hit = tr[:, 0] != 0
    assert 0.02 < hit.mean() < 0.5
    linear = np.zeros((S * S * w * h, 3))
    c = ref.shade(tr[hit, 7:10], tr[hit, 1], tr[hit, 2:5], tr[hit, 5] != 0, tr[hit, 6], dirs[hit], fc.FRAME_STEPS)
    c[np.isnan(c).any(axis=1)] = 0.0
    linear[hit] = np.clip(c, 0.0, 1.0)
    mean = linear.reshape(h, S, w, S, 3).mean(axis=(1, 3))
    want = ref.encode(mean)
    off = np.abs(got[..., :3].astype(int) - want.astype(int))
    print("supersampled sphere: channels off by one", int((off == 1).sum()), "of", off.size, "worst", int(off.max()))
    assert off.max() <= 1 and (got[..., 3] == 255).all()
    edge = (mean.max(axis=2) > 0) & (linear.reshape(h, S, w, S, 3).max(axis=4).min(axis=(1, 3)) == 0)
    assert edge.sum() >= 10  # pixels that mix hit and miss samples: the resolve did average
