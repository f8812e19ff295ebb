"""The scene evaluators over all of float32 on the CPU (tests/scene_point_cases.py): the x86-64
build of frm_scene.h equals the oracle's distance and colour bit for bit on every scene, and a
census from the oracle alone shows that each family's distances there are finite, NaN and (where
the family can produce them) infinite, so the GPU test (test_gpu_scene_points.py) cannot silently
test nothing."""
import numpy as np
import pytest

import scene_point_cases as sp
from helpers import hr_scene_de


def test_points_cover_the_type():
    s, h = sp.points("sorted"), sp.points("shuffled")
    assert s.shape == h.shape == (sp.N_POINTS, 3) and s.dtype == np.float32
    order = lambda p: np.lexsort(p.view(np.uint32).T)  # noqa: E731
    assert np.array_equal(s.view(np.uint32)[order(s)], h.view(np.uint32)[order(h)])  # the same points
    key = (s.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=1)
    assert np.all(np.diff(key.astype(np.int64)) >= 0) and not np.array_equal(s.view(np.uint32), h.view(np.uint32))
    field = (s.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)
    assert len(np.unique(field)) == 256 and len(np.unique(s.view(np.uint32) >> np.uint32(23))) == 512
    tame = np.all(np.abs(s) <= 1.5, axis=1)  # the half with two ordinary coordinates, mostly
    assert tame.sum() >= 1000
    for what, n in (("NaN", np.isnan(s).any(axis=1).sum()), ("inf", np.isinf(s).any(axis=1).sum()),
                    ("subnormal", ((s != 0) & (np.abs(s) < np.float32(2.0 ** -126))).any(axis=1).sum()),
                    ("zero", (s == 0).any(axis=1).sum()), ("above 2^64", (np.abs(s) > 2.0 ** 64).any(axis=1).sum())):
        # an infinity or a zero needs one exponent field of 256 and the zero mantissa: of 65,536
        # stratified coordinates, 65,536 / 256 / 5 = 51 are expected of each
        assert n >= (25 if what in ("inf", "zero") else 100), what
    # a 64-lane wave of the shuffled order mixes magnitudes; one of the sorted order does not
    spread = lambda p: np.median(np.ptp(((p.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)).max(axis=1)  # noqa: E731
                                        .reshape(-1, 64).astype(np.int64), axis=1))
    assert spread(s) <= 2 and spread(h) >= 100


@pytest.mark.parametrize("scene", sp.SCENES)
def test_host_build_equals_oracle_and_census(host_replay, oracle, scene):
    fam = sp.family(scene)
    seen = {"finite": 0, "nan": 0, "inf": 0, "zero": 0}
    for iters, time in sp.SETTINGS:
        p = sp.params_of(scene, iters, time)
        for order in sp.ORDERS:
            pts = sp.points(order)
            d, col = sp.reference(oracle, scene, iters, time, order)
            hd, hcol = hr_scene_de(host_replay, p, pts, flags=sp.flags_of(scene))
            bad = sp.differing(hd, d)
            assert not bad.any(), (f"scene {scene} N={iters} {order}: {bad.sum()} distances differ, e.g. p={pts[bad][:2]} "
                                   f"host={hd[bad][:2]} oracle={d[bad][:2]}")
            bad = sp.differing(hcol, col)
            assert not bad.any(), f"scene {scene} N={iters} {order}: {bad.sum()} colours differ, e.g. p={pts[bad][:2]}"
        seen["finite"] += int(np.isfinite(d).sum())
        seen["nan"] += int(np.isnan(d).sum())
        seen["inf"] += int(np.isinf(d).sum())
        seen["zero"] += int((d == 0).sum())
    print(f"scene {scene} ({fam}): of {3 * sp.N_POINTS} distances {seen}")
    assert seen["finite"] >= 10000
    if fam == "menger":  # box() and the folds take maxNum: a NaN coordinate is dropped, never returned
        assert seen["nan"] == 0 and seen["inf"] >= 10000
    else:
        assert seen["nan"] >= 100
    if fam in ("mandelbulb", "sphere"):
        assert seen["inf"] >= 10000 and seen["zero"] >= 1
