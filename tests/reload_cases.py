"""Runtime-reloaded kernels (frm_reload) held to the tables the suite already has: the helper of
test_gpu_reload_parity.py and test_gpu_reload_modes.py.

One frm_reload compiles every instantiation of the render kernels and takes seconds, so reloaded
contexts are made rarely and shared. context() keeps one per (flags, max_steps, frames_in_flight,
devices, supersampling, source variant, environment); the cases that share one go through resize +
update_parameters_buffer: a case runs on any context whose kernel flag and max_steps fit, whatever
its frames in flight. The contexts live until the process ends (a later module may want the one an
earlier module made), and every frm_reload(dir) of the two modules goes through reload() here,
which counts it: each module's last test asserts reload_calls() <= MAX_RELOADS.

Source variants are copies of csrc/ made once each, with exact text replacements:
  plain     unmodified
  fallback  the three preprocessor branches the ahead-of-time build never compiles, forced: lane_in's
            shift-and-test, div_fixup_'s plain C++ and xor_sign_'s and / xor
  teeth     mb_tame without its r >= 2^-13 term: a wrong kernel, which the edge frames must expose
  probe     #error in each of the three fallback branches, and one at the end of frm_render_kernels.h
            that always fires: the copy never compiles, and the compiler's log names the fallback
            branches the runtime compiler takes (probe_answers)"""
import atexit
import os
import shutil
import time

import numpy as np

import frm
from test_gpu_edges import counters_of

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fractal-ray-marching_amd", "csrc")
PERSISTENT, SIMPLE = frm.FRM_FLAG_PERSISTENT_KERNEL, frm.FRM_FLAG_SIMPLE_KERNEL
MAX_RELOADS = 16  # frm_reload(dir) calls of the two modules together

# contexts that host cases of two kinds (extra context() arguments): the persistent 100-step edge
# frames run on the shutter frames' context, the 256-step all-lean frames on the plain loop's; the
# wrong-kernel copy is loaded on the context of the FRM_RING=1 loop, whose frames then show the edit
SHARED = {(PERSISTENT, 100): {"frames_in_flight": 2}, (PERSISTENT, 256): {"frames_in_flight": 3}}
RING_LOOP = {"frames_in_flight": 3, "variant": "teeth", "env": (("FRM_RING", "1"),)}

_LANE_IN = "#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_inverse_ballot_w64)"
_LANE_IN_FALLBACK = "  return (mask >> (threadIdx.x & 63u)) & 1u;"
_DIV_FIXUP = "#if __has_builtin(__builtin_amdgcn_div_fixupf)"
_DIV_FIXUP_FALLBACK = "  const float aa = fabsf(a), ab = fabsf(b);"
_XOR_SIGN = "#if defined(__gfx950__)"
_XOR_SIGN_FALLBACK = "  return v ^ (m & 0x80000000u);"
_MB_TAME = "  return (r >= 0x1p-13f) & (m >= 0x1p-60f);"
PROBES = ("lane_in", "div_fixup_", "xor_sign_")


def _probe(name, line):
    return f"#error FRM_PROBE {name} takes its fallback\n{line}"


VARIANTS = {  # name -> [(file, old, new)]; every old text occurs exactly once in its file
    "plain": [],
    "fallback": [("frm_scene.h", _LANE_IN, "#if defined(__HIP_DEVICE_COMPILE__) && 0"),
                 ("frm_fast.h", _DIV_FIXUP, "#if 0"),
                 ("frm_fast.h", _XOR_SIGN, "#if 0")],
    "teeth": [("frm_scene.h", _MB_TAME, "  return (m >= 0x1p-60f);")],
    "probe": [("frm_scene.h", _LANE_IN_FALLBACK, _probe("lane_in", _LANE_IN_FALLBACK)),
              ("frm_fast.h", _DIV_FIXUP_FALLBACK, _probe("div_fixup_", _DIV_FIXUP_FALLBACK)),
              ("frm_fast.h", _XOR_SIGN_FALLBACK, _probe("xor_sign_", _XOR_SIGN_FALLBACK))],
}
_PROBE_END = "\n#error FRM_PROBE end of frm_render_kernels.h\n"

_dirs = {}
_contexts = {}
_calls = 0
compile_seconds = []  # of every successful reload()


def source_copy(tmp_path_factory, variant):
    """The directory of a source variant, copied and edited once per session."""
    if variant not in _dirs:
        d = tmp_path_factory.mktemp("reload") / f"csrc_{variant}"
        shutil.copytree(CSRC, d)
        for name, old, new in VARIANTS[variant]:
            text = (d / name).read_text()
            assert text.count(old) == 1, f"{name}: {old!r} occurs {text.count(old)} times"
            (d / name).write_text(text.replace(old, new))
        if variant == "probe":
            with open(d / "frm_render_kernels.h", "a") as f:
                f.write(_PROBE_END)
        _dirs[variant] = d
    return _dirs[variant]


def reload(r, source_dir):
    """r.reload(source_dir), counted (a failing call counts too) and timed."""
    global _calls
    _calls += 1
    t0 = time.perf_counter()
    r.reload(str(source_dir))
    compile_seconds.append(time.perf_counter() - t0)


def reload_calls():
    return _calls


def context(tmp_path_factory, flags, max_steps, frames_in_flight=1, devices=None, supersampling=1, variant="plain",
            env=()):
    """The shared context of a key, created (with the `env` pairs set, as frm_create reads them) and
    reloaded from the variant's copy on first use. Callers leave it as they found it but for its
    size and parameters."""
    key = (flags, max_steps, frames_in_flight, tuple(devices) if devices else None, supersampling, variant, tuple(env))
    if key not in _contexts:
        src = source_copy(tmp_path_factory, variant)
        old = {k: os.environ.get(k) for k, _ in env}
        os.environ.update(dict(env))
        try:
            r = frm.Renderer(device=0, max_steps=max_steps, flags=flags, frames_in_flight=frames_in_flight,
                             devices=devices, supersampling=supersampling)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        try:
            reload(r, src)
        except Exception:
            r.close()
            raise
        _contexts[key] = r
    return _contexts[key]


def retire(r):
    """Takes r out of the shared contexts (the caller is about to change it for good, and closes it)."""
    for key in [k for k, v in _contexts.items() if v is r]:
        del _contexts[key]


@atexit.register
def close_contexts():
    for r in _contexts.values():
        r.close()
    _contexts.clear()


def probe_answers(log):
    """{fallback name: True (the runtime compiler takes it), False, or None (the log ends early)}."""
    whole = "FRM_PROBE end of" in log
    return {n: True if f"FRM_PROBE {n} takes" in log else (False if whole else None) for n in PROBES}


def want_counters(*refs):
    return [sum(int(ref["counters"][i]) for ref in refs) for i in range(7)]


def assert_frame(img, ref_rgba, what):
    diff = np.any(img != ref_rgba, axis=-1)
    assert not diff.any(), f"{what}: {diff.sum()} pixels differ, first at {tuple(np.argwhere(diff)[0])}"


def same_trace(tr, ref_trace):
    """frm_debug_trace equals the oracle's bit for bit on hit pixels (NaN equal to NaN)."""
    ref = ref_trace.reshape(tr.shape)
    hit = ref[..., 0] != 0
    if not np.array_equal(tr[..., 0] != 0, hit):
        return False
    a, b = tr[hit], ref[hit]
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def launches(r_flags):
    """The persistent kernel renders every frame twice: its second launch sorts by the first one's keys."""
    return 2 if r_flags & PERSISTENT else 1


def check_frame(r, p, w, h, ref, n_launches, what, trace=False):
    """Bytes and the seven work counters of n_launches renders of `p` equal ref's (and the trace).
    With frames in flight the renders rotate over the slots, so a second launch asked for becomes one
    more round: the last launch then sorts by the keys an earlier one left in its own slot."""
    r.resize(w, h)
    r.update_parameters_buffer(p)
    if n_launches > 1:
        n_launches += r.frames_in_flight - 1
    for launch in range(n_launches):
        st = r.render(stats=True)
        assert_frame(r.read_frame(), ref["rgba"], f"{what} launch {launch}")
        assert counters_of(st) == want_counters(ref), f"{what} launch {launch}"
    if trace:
        assert same_trace(r.trace(), ref["trace"]), f"{what}: trace"


def frame_differs(r, p, w, h, ref):
    r.resize(w, h)
    r.update_parameters_buffer(p)
    st = r.render(stats=True)
    return bool(np.any(r.read_frame() != ref["rgba"])) or counters_of(st) != want_counters(ref)


POISON = 0xA5


def check_batch(r, ps, refs, w, h, what, pad=208, n_launches=2):
    """frm_render_bands_batch of whole frames fb + pad bytes apart in a poisoned buffer: every frame
    and the summed counters equal the oracle's, and the padding keeps its poison."""
    import torch

    fb = w * h * 4
    stride = fb + pad
    r.resize(w, h)
    out = torch.empty(len(ps) * stride, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    for launch in range(n_launches):
        out.fill_(POISON)
        counters.zero_()
        r.render_bands_batch(ps, out.data_ptr(), dst_bytes=out.numel(), frame_stride=stride, band_rows=h, first_band=0,
                             band_stride=1, stream=0, dev_counters=counters.data_ptr())
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(len(ps), stride)
        for k, ref in enumerate(refs):
            assert_frame(got[k, :fb].reshape(h, w, 4), ref["rgba"], f"{what} launch {launch} frame {k}")
        assert (got[:, fb:] == POISON).all(), f"{what} launch {launch}: padding written"
        assert [int(v) for v in counters.cpu().tolist()][:7] == want_counters(*refs), f"{what} launch {launch}"


def render_by_bands(r, w, h, band_rows, ranks):
    """The frame of r's parameters through frm_render_bands per rank and frm_unshuffle_bands:
    (image, the seven counters, the largest launch's pixel count)."""
    import ctypes

    import torch

    def local_rows(k):
        out = ctypes.c_uint32(0)
        assert frm.load().frm_band_rows_for(h, band_rows, k, ranks, ctypes.byref(out)) == 0
        return out.value

    rows = [local_rows(k) for k in range(ranks)]
    assert h <= sum(rows) < h + band_rows
    rank_stride = max(rows) * w * 4
    gathered = torch.zeros(ranks * rank_stride, dtype=torch.uint8, device="cuda")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda")
    out = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    for k in range(ranks):
        r.render_bands(gathered.data_ptr() + k * rank_stride, rows[k] * w * 4, band_rows, k, ranks, 0,
                       counters.data_ptr())
    r.unshuffle_bands(gathered.data_ptr(), rank_stride, out.data_ptr(), out.numel(), band_rows, ranks)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(h, w, 4), [int(v) for v in counters.cpu().tolist()][:7], max(rows) * w
