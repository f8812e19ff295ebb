"""The scene evaluators on the device over all of float32: Renderer.eval_scene equals the CPU
oracle's distance and colour bit for bit on the points of tests/scene_point_cases.py (every
exponent field, subnormals, zeros, infinities and NaN in any coordinate), for all 19 scenes and the
extension sphere at N = 0, 3 and 12, in an order whose waves are uniform and in one whose waves are
mixed. tests/test_scene_points.py shows on the CPU what those distances are and that the x86-64
build of the same source agrees."""
import pytest

import scene_point_cases as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def renderers(gpu_renderer_factory):
    made = {}

    def get(flags):
        if flags not in made:
            made[flags] = gpu_renderer_factory(flags=flags)
        return made[flags]

    yield get
    for r in made.values():
        r.close()


@pytest.mark.parametrize("scene", sp.SCENES)
def test_scene_equals_oracle_on_the_whole_type(renderers, oracle, scene):
    r = renderers(sp.flags_of(scene))
    for iters, time in sp.SETTINGS:
        r.update_parameters_buffer(sp.params_of(scene, iters, time))
        for order in sp.ORDERS:
            pts = sp.points(order)
            rd, rcol = sp.reference(oracle, scene, iters, time, order)
            d, col = r.eval_scene(pts)
            bad = sp.differing(d, rd)
            assert not bad.any(), (f"scene {scene} N={iters} {order}: {bad.sum()} distances differ, e.g. p={pts[bad][:3]} "
                                   f"gpu={d[bad][:3]} oracle={rd[bad][:3]}")
            bad = sp.differing(col, rcol)
            assert not bad.any(), (f"scene {scene} N={iters} {order}: {bad.sum()} colours differ, e.g. p={pts[bad][:3]} "
                                   f"gpu={col[bad][:3]} oracle={rcol[bad][:3]}")
