"""The two walks of tests/test_gpu_mode_matrix.py, shared with their recorder
(tests/golden/make_mode_matrix.py): what the host layer answers, as status codes and getter values,
to every call from every frame mode, and to every faulty device buffer of the stage entry points.

Mode walk. States: a plain context, one in each of the four frame modes (supersampling 2, adaptive
2, panorama faces of 4, depth of field (1, 1, 2)), a plain one with FRM_FLAG_SIMPLE_KERNEL and a
group over device 0 alone; each once before the first frm_resize ("unsized") and once after
frm_resize(16, 16) and one frm_render ("sized"). Every call of CALLS runs on a context of its own.
After each of its steps: the status, the four getters' values, and whether frm_read_frame_async
answers FRM_ERR_NOT_READY (render_seq was reset, or there is no size yet).

Span walk. Per stage entry point, 8x8 outputs (factor 2, faces of 2) in one device arena: every
single fault of its pointers, sizes and strides, every pair of those faults (the pair's status pins
the order of the checks) and the zero and above-limit sizes. The status alone is recorded. The one
"fault" the library accepts (frm_depth_of_field's two inputs overlapping) runs inside the arena."""
import ctypes
import itertools

import frm
from frm import _lib
from helpers import params_for

W = H = 16
STATES = ("plain", "supersampled", "adaptive", "panorama", "dof", "simple", "group")
PHASES = ("unsized", "sized")
MAX_DIM = 32768  # FRM_MAX_DIMENSION


class _Env:
    """A prepared context and the buffers its calls use."""

    def __init__(self, lib, state, phase, bufs):
        self.lib = lib
        flags = _lib.FRM_FLAG_SIMPLE_KERNEL if state == "simple" else 0
        self.renderer = frm.Renderer(max_steps=32, flags=flags, devices=[0] if state == "group" else None)
        self.ctx = self.renderer.ctx
        self.dst, self.src, self.host = bufs
        ps = [params_for(18, 2, frm.POWER8_TIME, W, H, pose=pose) for pose in ("P0", "P1")]
        self.params = (_lib.FrmParameters * 2)()
        for k, p in enumerate(ps):
            ctypes.memmove(ctypes.addressof(self.params[k]), p.to_bytes(), ctypes.sizeof(_lib.FrmParameters))
        prepare = {"supersampled": "ss_on", "adaptive": "ad_on", "panorama": "pano_on", "dof": "dof_on"}.get(state)
        done = [self.step(prepare)] if prepare else []
        done.append(lib.frm_set_parameters(self.ctx, ctypes.byref(self.params[1])))
        if phase == "sized":
            done += [lib.frm_resize(self.ctx, W, H), lib.frm_render(self.ctx, None)]
        assert done == [_lib.FRM_OK] * len(done), (state, phase, done)

    def step(self, name):
        lib, ctx, n = self.lib, self.ctx, self.dst.numel()
        if name == "ss_on":
            return lib.frm_set_supersampling(ctx, 2)
        if name == "ss_off":
            return lib.frm_set_supersampling(ctx, 1)
        if name == "ad_on":
            return lib.frm_set_adaptive(ctx, 2, _lib.FRM_ADAPTIVE_DEFAULT_THRESHOLD)
        if name == "ad_off":  # the threshold is kept while the pass is off
            return lib.frm_set_adaptive(ctx, 1, 32)
        if name == "pano_on":
            return lib.frm_set_panorama(ctx, 4)
        if name == "pano_off":
            return lib.frm_set_panorama(ctx, 0)
        if name == "dof_on":
            return lib.frm_set_depth_of_field(ctx, 1.0, 1.0, 2)
        if name == "dof_off":  # the lens is kept while the gather is off
            return lib.frm_set_depth_of_field(ctx, 0.5, 2.0, 0)
        if name == "resize":
            return lib.frm_resize(ctx, 24, 16)
        if name == "render":
            return lib.frm_render(ctx, None)
        if name == "bands":
            return lib.frm_render_bands(ctx, self.dst.data_ptr(), n, 16, 0, 1, None, None)
        if name == "batch":
            return lib.frm_render_bands_batch(ctx, 2, ctypes.addressof(self.params), self.dst.data_ptr(), n, n // 2,
                                              16, 0, 1, None, None)
        if name == "unshuffle":
            return lib.frm_unshuffle_bands(ctx, self.src.data_ptr(), n, self.dst.data_ptr(), n, 16, 1, None)
        if name == "shutter":
            return lib.frm_render_shutter(ctx, 2, ctypes.addressof(self.params), None)
        if name == "trace":
            return lib.frm_debug_trace(ctx, self.host.ctypes.data, self.host.size)
        if name == "depth":
            return lib.frm_read_depth(ctx, self.host.ctypes.data, self.host.size)
        if name == "reload":  # refused before anything is compiled
            return lib.frm_reload(ctx, b"mode-matrix-no-such-directory")
        raise KeyError(name)

    def record(self, rc):
        lib, ctx = self.lib, self.ctx
        u = [ctypes.c_uint32() for _ in range(5)]
        f = [ctypes.c_float() for _ in range(2)]
        got = [lib.frm_get_supersampling(ctx, ctypes.byref(u[0])),
               lib.frm_get_adaptive(ctx, ctypes.byref(u[1]), ctypes.byref(u[2])),
               lib.frm_get_panorama(ctx, ctypes.byref(u[3])),
               lib.frm_get_depth_of_field(ctx, ctypes.byref(f[0]), ctypes.byref(f[1]), ctypes.byref(u[4]))]
        assert got == [_lib.FRM_OK] * 4, got
        ticket = ctypes.c_uint64()
        not_ready = lib.frm_read_frame_async(ctx, ctypes.byref(ticket)) == _lib.FRM_ERR_NOT_READY
        return [rc, u[0].value, u[1].value, u[2].value, u[3].value, f[0].value, f[1].value, u[4].value, int(not_ready)]


# a call: the steps made, in order, on one fresh context
CALLS = {name: [name] for name in ("ss_on", "ad_on", "pano_on", "dof_on", "ss_off", "ad_off", "pano_off", "dof_off",
                                   "resize", "bands", "batch", "unshuffle", "shutter")}
CALLS["after_plain"] = ["render", "trace", "depth"]
CALLS["after_shutter"] = ["shutter", "trace", "depth"]
CALLS["after_panorama"] = ["pano_on", "render", "trace", "depth"]
RELOAD_STATES = ("adaptive", "dof")  # the two that refuse frm_reload before compiling


def mode_buffers():
    import numpy as np
    import torch
    nbytes = 2 * (2 * W) * (2 * H) * 4  # two frames at the largest render size
    return (torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros(nbytes, dtype=torch.uint8, device="cuda"),
            np.zeros((2 * W) * (2 * H) * 10, np.float32))


def mode_walk(lib, phase, state, bufs):
    """{call: [the record after each of its steps]} of one state in one phase."""
    calls = dict(CALLS)
    if state in RELOAD_STATES:
        calls["reload"] = ["reload"]
    out = {}
    for call, steps in calls.items():
        env = _Env(lib, state, phase, bufs)
        try:
            out[call] = [env.record(env.step(s)) for s in steps]
        finally:
            env.renderer.close()
    return out


# ---- span walk ------------------------------------------------------------------------------------

OUT, FACTOR, FACE = 8, 2, 2
SLOT = 1 << 14  # arena bytes per buffer: every call, accepted or not, stays inside the arena
BUFS = ("src", "acc", "dst", "depth", "counters")
ENTRY_POINTS = ("frm_resolve", "frm_refine", "frm_blit", "frm_accumulate", "frm_project_equirect",
                "frm_depth_of_field")


def _spec(entry):
    """(needs of the entry point's buffers, the frame a stride steps over or None, its size arguments
    with their limits, the pairs that may not overlap)."""
    px = OUT * OUT * 4
    big = px * FACTOR * FACTOR
    if entry == "frm_resolve":
        return {"src": big, "dst": px}, None, {"w": MAX_DIM // FACTOR, "h": MAX_DIM // FACTOR}, [("src", "dst")]
    if entry == "frm_refine":
        return {"src": px, "dst": px}, None, {"w": MAX_DIM // FACTOR, "h": MAX_DIM // FACTOR}, [("src", "dst")]
    if entry == "frm_blit":
        return ({"src": big, "dst": px}, None, {"src_w": MAX_DIM, "src_h": MAX_DIM, "w": MAX_DIM, "h": MAX_DIM},
                [("src", "dst")])
    if entry == "frm_accumulate":  # two frames
        return ({"src": 2 * big, "acc": OUT * OUT * 16, "dst": px}, big, {"w": MAX_DIM // FACTOR, "h": MAX_DIM // FACTOR},
                [("src", "acc"), ("src", "dst"), ("acc", "dst")])
    if entry == "frm_project_equirect":  # six faces with their guard band
        face = (FACE + 2) * (FACE + 2) * 4
        return {"src": 6 * face, "dst": px}, face, {"w": MAX_DIM, "h": MAX_DIM, "face": MAX_DIM - 2}, [("src", "dst")]
    return ({"src": px, "depth": px, "dst": px}, None, {"w": MAX_DIM, "h": MAX_DIM},
            [("src", "dst"), ("depth", "dst"), ("src", "depth")])


def _call(lib, ctx, entry, a):
    if entry == "frm_resolve":
        return lib.frm_resolve(ctx, a["src"], a["src_bytes"], a["w"], a["h"], FACTOR, a["dst"], a["dst_bytes"], None)
    if entry == "frm_refine":
        return lib.frm_refine(ctx, None, a["src"], a["src_bytes"], a["w"], a["h"], FACTOR, 16, a["dst"], a["dst_bytes"],
                              a["counters"], None)
    if entry == "frm_blit":
        return lib.frm_blit(ctx, a["src"], a["src_bytes"], a["src_w"], a["src_h"], a["dst"], a["dst_bytes"], a["w"],
                            a["h"], 0, None)
    if entry == "frm_accumulate":
        return lib.frm_accumulate(ctx, a["src"], a["src_bytes"], a["stride"], 2, a["w"], a["h"], FACTOR, a["acc"],
                                  a["acc_bytes"], 8, a["dst"], a["dst_bytes"], None)
    if entry == "frm_project_equirect":
        return lib.frm_project_equirect(ctx, a["src"], a["src_bytes"], a["stride"], a["face"], a["dst"], a["dst_bytes"],
                                        a["w"], a["h"], None)
    return lib.frm_depth_of_field(ctx, a["src"], a["src_bytes"], a["depth"], a["depth_bytes"], a["w"], a["h"], 1.0, 1.0,
                                  2, a["dst"], a["dst_bytes"], None)


def span_cases(entry):
    """[(name, faults)]: a fault is (order, key, kind, value), applied to the good arguments in `order`."""
    needs, frame, sizes, pairs = _spec(entry)
    faults = []
    for b in list(needs) + (["counters"] if entry == "frm_refine" else []):
        faults.append((f"{b}+2", (1, b, "add", 2)))
    if "acc" in needs:
        faults.append(("acc+8", (1, "acc", "add", 8)))
    for b, n in needs.items():
        faults.append((f"{b} short", (1, f"{b}_bytes", "set", n - 1)))
    if frame:
        faults.append(("stride-4", (1, "stride", "set", frame - 4)))
        faults.append(("stride+2", (1, "stride", "set", frame + 2)))
    for x, y in pairs:  # y starts on x's last texel
        faults.append((f"{x}/{y} overlap", (0, y, "onto", (x, needs[x] - 4))))
    cases = [(name, [f]) for name, f in faults]
    cases += [(f"{n1} & {n2}", [f1, f2]) for (n1, f1), (n2, f2) in itertools.combinations(faults, 2)]
    for key, limit in sizes.items():
        cases += [(f"{key}=0", [(1, key, "set", 0)]), (f"{key}={limit + 1}", [(1, key, "set", limit + 1)])]
    return cases


def span_walk(lib, ctx, arena, entry):
    """{case: status} of one entry point; `arena`: len(BUFS) * SLOT device bytes."""
    needs, frame, sizes, _ = _spec(entry)
    base = arena.data_ptr()
    assert base % 16 == 0 and arena.numel() >= len(BUFS) * SLOT
    out = {}
    for name, faults in span_cases(entry):
        a = {b: base + i * SLOT for i, b in enumerate(BUFS)}
        a.update({f"{b}_bytes": n for b, n in needs.items()})
        a.update(stride=frame, w=OUT, h=OUT, src_w=OUT * FACTOR, src_h=OUT * FACTOR, face=FACE)
        for _, key, kind, value in sorted(faults, key=lambda f: f[0]):
            if kind == "add":
                a[key] += value
            elif kind == "set":
                a[key] = value
            else:
                a[key] = a[value[0]] + value[1]
        out[name] = _call(lib, ctx, entry, a)
    return out
