"""The host layer's answers, pinned: which call is refused, accepted or not ready in which frame
mode (supersampling, adaptive, panorama, depth of field: they exclude each other), what the four
getters return afterwards and whether the readback sequence was reset; and which status every
faulty device buffer of the stage entry points gets, alone and in pairs (the pair pins the order of
the checks). tests/golden/mode_matrix.json was recorded (tests/golden/make_mode_matrix.py) from
the library before its frame modes, batched-frame step and span checks were each written once;
the walks (tests/mode_matrix.py) replayed here must give the same. Nothing larger than a 32x32
frame is launched."""
import json
import os

import pytest

import frm
import mode_matrix as mm
from helpers import params_for

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mode_matrix.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def mode_bufs(frm_lib):
    return mm.mode_buffers()


@pytest.mark.parametrize("state", mm.STATES)
@pytest.mark.parametrize("phase", mm.PHASES)
def test_mode_walk(frm_lib, golden, mode_bufs, phase, state):
    want = golden["mode"][f"{phase}/{state}"]
    got = mm.mode_walk(frm_lib, phase, state, mode_bufs)
    assert sorted(got) == sorted(want)
    for call in want:
        assert got[call] == want[call], (phase, state, call)


@pytest.mark.parametrize("entry", mm.ENTRY_POINTS)
def test_span_walk(frm_lib, golden, entry):
    import torch
    want = golden["span"][entry]
    arena = torch.zeros(len(mm.BUFS) * mm.SLOT, dtype=torch.uint8, device="cuda")
    with frm.Renderer(max_steps=32) as r:
        r.update_parameters_buffer(params_for(18, 2, frm.POWER8_TIME, mm.OUT, mm.OUT))
        got = mm.span_walk(frm_lib, r.ctx, arena, entry)
        r.synchronize()
    assert sorted(got) == sorted(want)
    differ = {case: (got[case], want[case]) for case in want if got[case] != want[case]}
    assert not differ
