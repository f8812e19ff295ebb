"""Renderer: the Python host's view of libfrm, mirroring the reference's `Graphics`
API (src/graphics.rs): init -> resize -> update_parameters_buffer -> render ->
(read_frame replaces the blit+present). Errors raise FrmError; nothing falls back to
the CPU."""
import ctypes
import os

import numpy as np

from . import _lib


class Renderer:
    def __init__(self, device=0, max_steps=0, flags=0, frames_in_flight=1, devices=None, supersampling=1,
                 adaptive=None, panorama=0, depth_of_field=None):
        """supersampling: samples per pixel and axis (frm_set_supersampling; 1 = off).
        adaptive: (S, threshold) or S: S x S samples for the pixels on an edge only (frm_set_adaptive).
        panorama: cube face size N; every frame is a 360-degree equirectangular one (frm_set_panorama; 0 = off).
        depth_of_field: (aperture, focus, radius): every frame is blurred by a thin lens (frm_set_depth_of_field).
        devices: a list of HIP device ordinals for a GROUP context (frm_config.device_count):
        every frame is row-tiled over them and gathered on devices[0] (RCCL, or device copies
        when a device repeats); the rest of the API is the same."""
        lib = _lib.load()
        self._lib = lib
        self.ctx = ctypes.c_void_p()
        cfg = _lib.FrmConfig(device, max_steps, flags, frames_in_flight)
        if devices is not None:
            devices = list(devices)
            if not 1 <= len(devices) <= 16:
                raise ValueError("a group holds 1..16 devices")
            cfg.device_count = len(devices)
            for i, d in enumerate(devices):
                cfg.devices[i] = d
            device = devices[0]
        _lib.check(lib.frm_create(ctypes.byref(self.ctx), ctypes.byref(cfg)))
        self.devices = devices
        self.device = device
        self.frames_in_flight = max(1, frames_in_flight)
        self.width = self.height = 0
        self.supersampling = 1
        self._adaptive = (1, _lib.FRM_ADAPTIVE_DEFAULT_THRESHOLD)
        self.panorama = 0
        self._dof = (0.0, 1.0, 0)
        try:
            if supersampling != 1:
                self.set_supersampling(supersampling)
            if adaptive is not None:
                self.set_adaptive(*(adaptive if isinstance(adaptive, (tuple, list)) else (adaptive,)))
            if panorama:
                self.set_panorama(panorama)
            if depth_of_field is not None:
                self.set_depth_of_field(*depth_of_field)
        except Exception:
            self.close()
            raise

    def close(self):
        if self.ctx:
            self._lib.frm_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        return _lib.check(rc, self.ctx)

    # graphics.rs:54-57 (render texture size) — arbitrary W x H here
    def resize(self, width, height):
        self._check(self._lib.frm_resize(self.ctx, width, height))
        self.width, self.height = width, height

    def set_supersampling(self, factor):
        """frm_set_supersampling: every frame is rendered at factor x the resize() size and box-resolved
        in linear light; width/height, read_frame, present and tickets stay at the output size."""
        self._check(self._lib.frm_set_supersampling(self.ctx, factor))
        self.supersampling = int(factor)

    # the internal render size: what trace(), pixel_keys() and set_pixel_keys() work on
    @property
    def render_width(self):
        return self.panorama + 2 if self.panorama else self.width * self.supersampling

    @property
    def render_height(self):
        return self.panorama + 2 if self.panorama else self.height * self.supersampling

    def set_panorama(self, face_size):
        """frm_set_panorama: from the next render on, every frame is the equirectangular projection, at
        the resize() size, of six cube faces of (face_size + 2)^2 texels rendered around the camera;
        0 switches it off."""
        self._check(self._lib.frm_set_panorama(self.ctx, face_size))
        self.panorama = int(face_size)

    def project_equirect(self, faces_ptr, faces_bytes, face_stride, face_size, dst_ptr, dst_bytes, out_w, out_h,
                         stream=0):
        """frm_project_equirect: projects the six (face_size + 2)^2 RGBA8 sRGB cube faces face_stride
        bytes apart at device pointer faces_ptr into the out_h x out_w equirectangular frame at dst_ptr,
        asynchronously on `stream` (0: the context's)."""
        self._check(self._lib.frm_project_equirect(self.ctx, faces_ptr, faces_bytes, face_stride, face_size, dst_ptr,
                                                   dst_bytes, out_w, out_h, stream or None))

    def set_depth_of_field(self, aperture, focus, max_radius):
        """frm_set_depth_of_field: from the next render on, every frame is gathered in linear light by each
        pixel's circle of confusion: `aperture` is the blur radius, in pixels, of a point at infinity,
        `focus` the ray distance in focus, `max_radius` (0..FRM_MAX_DOF_RADIUS) the largest radius; 0
        switches it off."""
        self._check(self._lib.frm_set_depth_of_field(self.ctx, aperture, focus, max_radius))
        self._dof = (float(aperture), float(focus), int(max_radius))

    @property
    def dof(self):
        """(aperture, focus, max_radius) of frm_set_depth_of_field; max_radius 0 = off."""
        return self._dof

    def depth_of_field(self, src_ptr, src_bytes, depth_ptr, depth_bytes, width, height, aperture, focus, max_radius,
                       dst_ptr, dst_bytes, stream=0):
        """frm_depth_of_field: gathers the height x width RGBA8 sRGB frame at device pointer src_ptr by the
        float32 depth plane at depth_ptr into dst_ptr, asynchronously on `stream` (0: the context's)."""
        self._check(self._lib.frm_depth_of_field(self.ctx, src_ptr, src_bytes, depth_ptr, depth_bytes, width, height,
                                                 aperture, focus, max_radius, dst_ptr, dst_bytes, stream or None))

    def read_depth(self):
        """frm_read_depth: the depth plane of the last render, (H, W) float32: the primary hit distance of
        every hit pixel, +inf elsewhere."""
        out = np.zeros((self.render_height, self.render_width), np.float32)
        self._check(self._lib.frm_read_depth(self.ctx, out.ctypes.data, out.size))
        return out

    def resolve(self, src_ptr, src_bytes, out_w, out_h, factor, dst_ptr, dst_bytes, stream=0):
        """frm_resolve: box-resolve (factor*out_h) x (factor*out_w) RGBA8 sRGB texels at device pointer
        src_ptr into out_h x out_w at dst_ptr, asynchronously on `stream` (0: the context's)."""
        self._check(self._lib.frm_resolve(self.ctx, src_ptr, src_bytes, out_w, out_h, factor, dst_ptr, dst_bytes,
                                          stream or None))

    def set_adaptive(self, factor, threshold=_lib.FRM_ADAPTIVE_DEFAULT_THRESHOLD):
        """frm_set_adaptive: from the next render on, the pixels whose 3 x 3 neighbourhood in the plain
        frame has a contrast of `threshold` sRGB codes or more (0: all, 256: none) are replaced by the
        box resolve of their factor x factor samples; factor 1 switches it off."""
        self._check(self._lib.frm_set_adaptive(self.ctx, factor, threshold))
        self._adaptive = (int(factor), int(threshold))

    @property
    def adaptive(self):
        """(factor, threshold) of frm_set_adaptive; factor 1 = off."""
        return self._adaptive

    def refine(self, src_ptr, src_bytes, width, height, factor, threshold, dst_ptr, dst_bytes, params=None,
               dev_counters=0, stream=0):
        """frm_refine: the adaptive frame of the height x width RGBA8 sRGB frame at device pointer
        src_ptr into dst_ptr, its refined pixels sampled with `params` (None: the context's),
        asynchronously on `stream` (0: the context's); dev_counters: FRM_NUM_COUNTERS device words the
        refined samples' work is added to."""
        raw = None
        if params is not None:
            raw = ctypes.byref(params.raw if hasattr(params, "raw") else params)
        self._check(self._lib.frm_refine(self.ctx, raw, src_ptr, src_bytes, width, height, factor, threshold,
                                         dst_ptr, dst_bytes, dev_counters or None, stream or None))

    def refine_mask(self):
        """frm_debug_refine_mask: the edge mask of the last (adaptive) render, (height, width) uint8 0/1."""
        out = np.zeros((self.height, self.width), np.uint8)
        got = self._lib.frm_debug_refine_mask(self.ctx, out.ctypes.data, out.size)
        if got < 0:
            self._check(-got)
        assert got == out.size, (got, out.size)
        return out

    # graphics.rs:59-61
    def update_parameters_buffer(self, parameters):
        raw = parameters.raw if hasattr(parameters, "raw") else parameters
        self._check(self._lib.frm_set_parameters(self.ctx, ctypes.byref(raw)))

    # graphics.rs:91-110 (one frame); returns frm_stats as a dict when stats=True
    def render(self, stats=True):
        if not stats:
            self._check(self._lib.frm_render(self.ctx, None))
            return None
        st = _lib.FrmStats()
        self._check(self._lib.frm_render(self.ctx, ctypes.byref(st)))
        return st.as_dict()

    def render_shutter(self, params_list, stats=True):
        """frm_render_shutter: one motion-blurred frame, the mean in linear light of the sub-frames
        rendered with params_list (1..FRM_MAX_SHUTTER_SAMPLES Parameters of one scene, e.g. from
        frm.shutter_parameters); the context's parameters become the last. Returns frm_stats summed
        over the sub-frames as a dict when stats=True."""
        arr = _params_array(params_list)
        st = _lib.FrmStats() if stats else None
        self._check(self._lib.frm_render_shutter(self.ctx, len(params_list), ctypes.addressof(arr),
                                                 ctypes.byref(st) if stats else None))
        return st.as_dict() if stats else None

    def accumulate(self, src_ptr, src_bytes, frame_stride, count, out_w, out_h, factor, acc_ptr=0, acc_bytes=0,
                   divisor=1, dst_ptr=0, dst_bytes=0, stream=0):
        """frm_accumulate: adds, in linear light, the factor x factor texels under each of the out_h x
        out_w output pixels over `count` RGBA8 sRGB frames frame_stride bytes apart at device pointer
        src_ptr, asynchronously on `stream` (0: the context's). acc_ptr (0: none): 16 bytes of f32 sums
        per output pixel the sum starts from and is stored to; dst_ptr (0: none) receives the frame of
        sum / divisor."""
        self._check(self._lib.frm_accumulate(self.ctx, src_ptr, src_bytes, frame_stride, count, out_w, out_h, factor,
                                             acc_ptr or None, acc_bytes, divisor, dst_ptr or None, dst_bytes,
                                             stream or None))

    def read_frame(self):
        buf = np.empty((self.height, self.width, 4), dtype=np.uint8)
        self._check(self._lib.frm_read_frame(self.ctx, buf.ctypes.data, buf.nbytes))
        return buf

    # blit.wgsl + present (graphics.rs:91-110): the frame resampled to a window size
    def present(self, width, height, srgb=True, bgra=False):
        buf = np.empty((height, width, 4), dtype=np.uint8)
        flags = _blit_flags(srgb, bgra)
        self._check(self._lib.frm_present(self.ctx, width, height, flags, buf.ctypes.data, buf.nbytes))
        return buf

    def blit(self, src_ptr, src_bytes, src_w, src_h, dst_ptr, dst_bytes, out_w, out_h, srgb=True, bgra=False,
             stream=0):
        """frm_blit: present()'s resample of src_h x src_w RGBA8 sRGB texels at device pointer src_ptr
        into out_h x out_w at dst_ptr, asynchronously on `stream` (0: the context's)."""
        flags = _blit_flags(srgb, bgra)
        self._check(self._lib.frm_blit(self.ctx, src_ptr, src_bytes, src_w, src_h, dst_ptr, dst_bytes, out_w, out_h,
                                       flags, stream or None))

    # asynchronous readback (frm_read_frame_async / frm_present_async + frm_frame_pixels): the
    # reference's surface presents with a frame of latency (wgpu's desired_maximum_frame_latency
    # 2), so a loop renders frame k, starts its readback and then waits for frame k-1's pixels
    def read_frame_async(self):
        t = ctypes.c_uint64()
        self._check(self._lib.frm_read_frame_async(self.ctx, ctypes.byref(t)))
        return self._remember(t.value, (self.height, self.width, 4))

    def present_async(self, width, height, srgb=True, bgra=False):
        t = ctypes.c_uint64()
        flags = _blit_flags(srgb, bgra)
        self._check(self._lib.frm_present_async(self.ctx, width, height, flags, ctypes.byref(t)))
        return self._remember(t.value, (height, width, 4))

    def _remember(self, ticket, shape):
        # a ticket keeps the shape of its frame across a later resize (frm_resize does not drain)
        shapes = self.__dict__.setdefault("_ticket_shapes", {})
        shapes[ticket] = shape
        if len(shapes) > 64:
            del shapes[min(shapes)]
        return ticket

    def frame_pixels(self, ticket, shape=None, copy=True):
        """Waits for the readback `ticket` and returns its pixels as a uint8 array of `shape`
        (default: the frame's (height, width, 4)); copy=False returns a view of the library's
        pinned image, valid until frames_in_flight further renders."""
        ptr = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_size_t()
        self._check(self._lib.frm_frame_pixels(self.ctx, int(ticket), ctypes.byref(ptr), ctypes.byref(n)))
        view = np.ctypeslib.as_array(ptr, shape=(n.value,))
        shape = shape or self.__dict__.get("_ticket_shapes", {}).get(int(ticket), (self.height, self.width, 4))
        view = view.reshape(shape)
        return view.copy() if copy else view

    def synchronize(self):
        self._check(self._lib.frm_synchronize(self.ctx))

    def kernel_for(self, pixels):
        """'persistent' or 'simple': the kernel a launch of `pixels` pixels runs here."""
        k = ctypes.c_uint32()
        self._check(self._lib.frm_kernel_for_pixels(self.ctx, int(pixels), ctypes.byref(k)))
        return "simple" if k.value == _lib.FRM_KERNEL_SIMPLE else "persistent"

    # graphics.rs:44-48 (reload): recompile the render kernels from an edited copy of csrc/
    # (hiprtc); raises FrmError (FRM_ERR_COMPILE + compiler log) and keeps the previous
    # kernels on failure. source_dir=None returns to the built-in kernels.
    def reload(self, source_dir):
        arg = None if source_dir is None else os.fsencode(source_dir)
        self._check(self._lib.frm_reload(self.ctx, arg))

    # graphics.rs:39-43 (try_reload): print the error instead of raising
    def try_reload(self, source_dir):
        try:
            self.reload(source_dir)
            return True
        except _lib.FrmError as e:
            print(e)
            return False

    # multi-GPU row tiling (device pointers, e.g. torch tensors' data_ptr())
    def render_bands(self, dev_ptr, nbytes, band_rows, first_band, band_stride, stream=0,
                     dev_counters=0):
        self._check(self._lib.frm_render_bands(self.ctx, dev_ptr, nbytes, band_rows, first_band,
                                               band_stride, stream or None, dev_counters or None))

    def render_bands_batch(self, params_list, dev_ptr, *, dst_bytes, frame_stride, band_rows, first_band,
                           band_stride, stream=0, dev_counters=0):
        """frm_render_bands_batch: len(params_list) frames (same scene; the camera, and for the
        Mandelbulb the time, may differ) in
        one launch, frame k at dev_ptr + k * frame_stride; dst_bytes = the size of the buffer at
        dev_ptr (the library checks every frame against it: pass the real allocation, e.g.
        tensor.numel(), never a size derived from the stride)."""
        arr = _params_array(params_list)
        self._check(self._lib.frm_render_bands_batch(self.ctx, len(params_list), ctypes.addressof(arr), dev_ptr,
                                                     dst_bytes, frame_stride, band_rows, first_band, band_stride,
                                                     stream or None, dev_counters or None))

    def unshuffle_bands(self, src_ptr, rank_stride, dst_ptr, dst_bytes, band_rows, ranks, stream=0):
        self._check(self._lib.frm_unshuffle_bands(self.ctx, src_ptr, rank_stride, dst_ptr, dst_bytes,
                                                  band_rows, ranks, stream or None))

    # diagnostics: scene() and builtins evaluated on the GPU
    MATH_FN = {"sin": 0, "cos": 1, "acos": 2, "atan2": 3, "log": 4, "log2": 5, "exp2": 6,
               "pow": 7, "sqrt": 8, "div": 9,
               # device fast paths (frm_fast.h), each bit-identical to a builtin on its domain
               "sqrt_nosmall": 10, "div_tame": 11, "div_tame_nz": 12, "sin_small": 13,
               "cos_small": 14, "acos_dev": 15, "atan2_tame": 16, "log2_tame": 17,
               "exp2_tame": 18, "log_posnormal": 19,
               # the sRGB store's code (frm_scene.h encode_srgb), as a float
               "srgb_encode": 20,
               # the division ended by v_div_fixup (frm_fast.h div_fix) and the last tap's normalize
               # of (a, b, b), guarded (normalize_wave) and plain
               "div_fix": 21, "normalize_guarded_x": 22, "normalize_guarded_y": 23,
               "normalize_x": 24, "normalize_y": 25,
               # atan2_tame for two non-zero operands (frm_fast.h atan2_tame_nz)
               "atan2_tame_nz": 26}

    def eval_scene(self, points):
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        d = np.zeros(len(pts), np.float32)
        col = np.zeros((len(pts), 3), np.float32)
        self._check(self._lib.frm_eval_scene(self.ctx, pts.ctypes.data, len(pts), d.ctypes.data,
                                             col.ctypes.data))
        return d, col

    def eval_math(self, name, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float32)
        bb = None if b is None else np.ascontiguousarray(np.broadcast_to(b, a.shape), dtype=np.float32)
        out = np.zeros_like(a)
        self._check(self._lib.frm_eval_math(self.ctx, self.MATH_FN[name], a.ctypes.data,
                                            None if bb is None else bb.ctypes.data, a.size,
                                            out.ctypes.data))
        return out

    def pixel_keys(self):
        """The 8-bit cost keys (16 log2(bodies + 1)) the last persistent launch recorded per
        local pixel, row-major (scheduling diagnostics)."""
        n = self.render_width * self.render_height
        out = np.zeros(n, np.uint8)
        got = self._lib.frm_debug_pixel_keys(self.ctx, out.ctypes.data, n)
        if got < 0:
            self._check(-got)
        return out[:got]

    def set_pixel_keys(self, keys):
        """Replace the cost keys the next persistent launch sorts its pixels by."""
        k = np.ascontiguousarray(keys, dtype=np.uint8)
        self._check(self._lib.frm_debug_set_pixel_keys(self.ctx, k.ctypes.data, k.size))

    def pixel_order(self, n=None):
        """frm_debug_pixel_order: (order, ranked). The fetch order in the last persistent launch's
        slot (local pixel indices, most expensive first); ranked: that launch ranked it from its own
        keys for the slot's next launch, else it is the order the launch itself fetched by.
        n: the capacity offered (default: a whole frame at the render size)."""
        n = self.render_width * self.render_height if n is None else int(n)
        out = np.zeros(max(n, 1), np.uint32)
        ranked = ctypes.c_uint32()
        got = self._lib.frm_debug_pixel_order(self.ctx, out.ctypes.data, n, ctypes.byref(ranked))
        if got < 0:
            self._check(-got)
        return out[:got], int(ranked.value)

    def trace(self):
        """frm_debug_trace: the shading inputs of every pixel of the last render, (H, W, 10) float32
        in the oracle's trace layout (hit, steps, normal xyz, sun hit, sun closeness, colour xyz)."""
        out = np.zeros((self.render_height, self.render_width, 10), np.float32)
        self._check(self._lib.frm_debug_trace(self.ctx, out.ctypes.data, out.size))
        return out

    def stats_from_counters(self, counters):
        arr = (ctypes.c_uint64 * _lib.FRM_NUM_COUNTERS)(*[int(c) for c in counters])
        st = _lib.FrmStats()
        self._check(self._lib.frm_stats_from_counters(self.ctx, arr, ctypes.byref(st)))
        return st.as_dict()


def _params_array(params_list):
    """The Parameters of params_list as one C array (at least one element long)."""
    arr = (_lib.FrmParameters * max(1, len(params_list)))()
    for k, p in enumerate(params_list):
        ctypes.memmove(ctypes.addressof(arr[k]), p.to_bytes(), ctypes.sizeof(_lib.FrmParameters))
    return arr


def _blit_flags(srgb, bgra):
    return (_lib.FRM_BLIT_SRGB if srgb else 0) | (_lib.FRM_BLIT_BGRA if bgra else 0)


def device_count():
    n = ctypes.c_int32(0)
    rc = _lib.load().frm_device_count(ctypes.byref(n))
    return n.value if rc == _lib.FRM_OK else 0
