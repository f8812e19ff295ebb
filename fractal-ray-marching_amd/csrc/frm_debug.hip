// frm_debug.hip — the diagnostic entry points of include/frm.h: what the last frame left in its slot
// (frm_debug_*, frm_read_depth), scene() and the builtins evaluated on the device (frm_eval_*), and
// frm_stats_from_counters.
#include "frm_ctx.h"

// The last frm_render as frm_debug_trace and frm_read_depth need it, `what` being "to trace" or
// "'s depth": one frame, not composed of several, whose persistent launch of the current frame size
// (npix pixels) still has its records in slot sl.
static int single_frame_records(frm_ctx* ctx, const Slot& sl, size_t npix, const char* what) {
  if (ctx->render_seq && ctx->composed_seq == ctx->render_seq && !ctx->last_is_ring)
    return fail(ctx, FRM_ERR_NOT_READY, "the last frame was composed of %s: no single frame%s", ctx->composed_of, what);
  if (!ctx->render_seq || sl.seq != ctx->render_seq)
    return fail(ctx, FRM_ERR_NOT_READY, "no frm_render, or a later launch reused its slot's records");
  if (!sl.records.p || sl.records.cap < npix * kRecordBytes || !sl.sched_whole || sl.sched_w != ctx->width || sl.sched_h != ctx->height)
    return fail(ctx, FRM_ERR_NOT_READY, "the last frm_render was not a persistent launch of this frame size");
  return FRM_OK;
}

extern "C" {

int frm_debug_refine_mask(frm_ctx* ctx, uint8_t* out, size_t n) {
  if (!ctx || !out) return -fail(ctx, FRM_ERR_INVALID_ARGUMENT, "NULL argument");
  if (ctx->last_is_ring || !ctx->render_seq)
    return -fail(ctx, FRM_ERR_NOT_READY, "frm_debug_refine_mask: no adaptive frm_render under the current settings");
  const Slot& sl = ctx->slots[ctx->last_slot];
  if (sl.second[sl.fb_idx] != kAdaptive || sl.seq != ctx->render_seq || !sl.refine_list.p)
    return -fail(ctx, FRM_ERR_NOT_READY, "frm_debug_refine_mask: the last frm_render was not adaptive");
  const size_t npix = (size_t)sl.refine_w * sl.refine_h;
  if (n > npix) n = npix;
  if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(sl.stream) != hipSuccess)
    return -fail(ctx, FRM_ERR_HIP, "frm_debug_refine_mask: synchronisation failed");
  uint32_t count = 0;
  if (hipMemcpy(&count, sl.refine_ctl, sizeof(count), hipMemcpyDeviceToHost) != hipSuccess || count > npix)
    return -fail(ctx, FRM_ERR_HIP, "frm_debug_refine_mask: reading the list length failed");
  uint32_t* list = new (std::nothrow) uint32_t[count ? count : 1u];
  if (!list) return -fail(ctx, FRM_ERR_OUT_OF_MEMORY, "host allocation failed");
  if (count && hipMemcpy(list, sl.refine_list.p, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) {
    delete[] list;
    return -fail(ctx, FRM_ERR_HIP, "frm_debug_refine_mask: reading the list failed");
  }
  memset(out, 0, n);
  for (uint32_t k = 0; k < count; ++k)
    if (list[k] < n) out[list[k]] = 1;
  delete[] list;
  return (int)n;
}

#ifdef FRM_STAMPS
extern "C" int frm_debug_read(frm_ctx* ctx, uint64_t* out5) {
  const Slot& sl = ctx->slots[(ctx->next_slot + ctx->nslots - 1u) % ctx->nslots];  // last launch
  return hipMemcpy(out5, sl.queue + kQueueDebugWord, 40, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
#endif

// The scheduling state in the slot of the last persistent launch, copied out for
// frm_debug_pixel_keys (keys) and frm_debug_pixel_order (order, ranked): min(n, that launch's
// local pixels) entries, the count in *copied. Returns a frm_status.
static int debug_sched_read(frm_ctx* ctx, const char* what, uint8_t* keys, uint32_t* order, uint32_t* ranked, size_t n,
                            size_t* copied) {
  if (ctx->group) return not_on_group(ctx, what);
  if (int rc = ring_leave(ctx)) return rc;
  const Slot& sl = ctx->slots[(ctx->next_slot + ctx->nslots - 1u) % ctx->nslots];  // last launch
  if (!sl.sched_keys || !sl.sched_order || !sl.sched_npix)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "%s: no persistent launch yet", what);
  if (n > sl.sched_npix) n = sl.sched_npix;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  FRM_HIP(ctx, hipDeviceSynchronize());
  if (keys) FRM_HIP(ctx, hipMemcpy(keys, sl.sched_keys, n, hipMemcpyDeviceToHost));
  if (order) FRM_HIP(ctx, hipMemcpy(order, sl.sched_order, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (ranked) *ranked = sl.order_ready ? 1u : 0u;
  *copied = n;
  return FRM_OK;
}

// per-pixel cost keys recorded by the last persistent launch (local pixel order; before
// the next launch overwrites them); the count copied, or a negative frm_status
int frm_debug_pixel_keys(frm_ctx* ctx, uint8_t* out, size_t n) {
  if (!ctx || !out) return -fail(ctx, FRM_ERR_INVALID_ARGUMENT, "NULL argument");
  size_t copied = 0;
  const int rc = debug_sched_read(ctx, "frm_debug_pixel_keys", out, nullptr, nullptr, n, &copied);
  return rc ? -rc : (int)copied;
}

// the fetch order in the last persistent launch's slot: the one that launch ranked for the slot's
// next launch of the same geometry (*out_ranked = 1), else the one it fetched by itself (0)
int frm_debug_pixel_order(frm_ctx* ctx, uint32_t* out, size_t n, uint32_t* out_ranked) {
  if (!ctx || !out || !out_ranked) return -fail(ctx, FRM_ERR_INVALID_ARGUMENT, "NULL argument");
  size_t copied = 0;
  const int rc = debug_sched_read(ctx, "frm_debug_pixel_order", nullptr, out, out_ranked, n, &copied);
  return rc ? -rc : (int)copied;
}

// replaces the cost keys the next launch sorts its pixels by (scheduling experiments): the
// slot of the next launch must hold the history of a whole frame of the current size
int frm_debug_set_pixel_keys(frm_ctx* ctx, const uint8_t* keys, size_t n) {
  if (!ctx || !keys) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "NULL argument");
  if (ctx->group) return not_on_group(ctx, "frm_debug_set_pixel_keys");
  if (int rc = ring_leave(ctx)) return rc;
  Slot& sl = ctx->slots[ctx->next_slot];
  if (!sl.sched_history || !sl.sched_whole || sl.sched_w != ctx->width || sl.sched_h != ctx->height ||
      n != (size_t)ctx->width * ctx->height || n > sl.sched_cap)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "no whole-frame history of this size in the next slot");
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  int rc = wait_slot(ctx, sl);
  if (rc) return rc;
  if (sl.keys_reader) FRM_HIP(ctx, hipEventSynchronize(sl.keys_read));
  FRM_HIP(ctx, hipMemcpy(sl.sched_keys, keys, n, hipMemcpyHostToDevice));
  sl.order_ready = false;  // the next launch sorts by these keys
  return FRM_OK;
}

// per-pixel shading inputs of the last frm_render (a whole persistent frame of the current size
// and parameters): 10 floats per pixel, row-major, as the oracle's om_render_trace
int frm_debug_trace(frm_ctx* ctx, float* out, size_t n_floats) {
  int rc = ensure_ready(ctx);
  if (rc) return rc;
  if (ctx->group) return not_on_group(ctx, "frm_debug_trace");
  if ((rc = ring_leave(ctx))) return rc;
  if (!out) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "out is NULL");
  const size_t npix = (size_t)ctx->width * ctx->height;
  if (n_floats < npix * 10u)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "out holds %zu floats, the trace needs %zu", n_floats, npix * 10u);
  const Slot& sl = ctx->slots[ctx->last_slot];
  if ((rc = single_frame_records(ctx, sl, npix, " to trace"))) return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  // the rays and colours of that render: its own parameters, not those set since
  KernelArgs a = make_args(ctx, ctx->render_params, ctx->render_scene, sl.fb(), ctx->counters, ctx->height, 0, 1,
                           ctx->height);
  a.geom = reinterpret_cast<ShadeGeom*>(sl.records.p);
  a.tails = record_tails(sl.records);
  float* d = nullptr;
  FRM_HIP(ctx, hipMalloc(&d, npix * 10u * sizeof(float)));
  hipError_t e = launch_trace(a, d, sl.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, npix * 10u * sizeof(float), hipMemcpyDeviceToHost, sl.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(sl.stream);
  (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(ctx, e, "frm_debug_trace");
  return FRM_OK;
}

// the depth plane of the last frm_render (frm_debug_trace's conditions): the plane its gather used
// on a depth-of-field context, else depth_pass over the records now
int frm_read_depth(frm_ctx* ctx, float* dst, size_t n_floats) {
  int rc = ensure_ready(ctx);
  if (rc) return rc;
  if (ctx->group) return not_on_group(ctx, "frm_read_depth");
  if ((rc = ring_leave(ctx))) return rc;
  if (!dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "dst is NULL");
  const size_t npix = (size_t)ctx->width * ctx->height;
  if (n_floats < npix)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu floats, the depth plane needs %zu", n_floats, npix);
  const Slot& sl = ctx->slots[ctx->last_slot];
  if ((rc = single_frame_records(ctx, sl, npix, "'s depth"))) return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  hipError_t e = hipSuccess;
  if (sl.second[sl.fb_idx] == kDof && sl.depth.p && sl.depth_w == ctx->width && sl.depth_h == ctx->height) {
    e = hipMemcpyAsync(dst, sl.depth.p, npix * sizeof(float), hipMemcpyDeviceToHost, sl.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(sl.stream);
  } else {
    // the plane is scratch of the call, from the context's pool in the order of the slot's stream: no
    // device-wide synchronisation, frames in flight on other slots go on
    float* d = nullptr;
    if ((rc = dev_alloc(ctx, (void**)&d, npix * sizeof(float), sl.stream))) return rc;
    e = launch_depth(reinterpret_cast<const ShadeGeom*>(sl.records.p), record_tails(sl.records), d, (uint32_t)npix, sl.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst, d, npix * sizeof(float), hipMemcpyDeviceToHost, sl.stream);
    const int r1 = dev_release(ctx, d, sl.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(sl.stream);
    if (e == hipSuccess && r1) return r1;
  }
  if (e != hipSuccess) return hip_fail(ctx, e, "frm_read_depth");
  return FRM_OK;
}

int frm_stats_from_counters(const frm_ctx* ctx, const uint64_t* c, frm_stats* out) {
  if (!ctx || !c || !out) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "NULL argument");
  memset(out, 0, sizeof(*out));
  out->pixels = c[kCntPixels];
  out->hit_pixels = c[kCntHits];
  out->primary_steps = c[kCntPrimary];
  out->shadow_steps = c[kCntShadow];
  out->normal_evals = c[kCntNormal];
  out->fractal_bodies = c[kCntBodies];
  out->fractal_bailouts = c[kCntBailouts];
  out->march_steps = c[kCntPrimary] + c[kCntShadow];
  out->wom_ops = wom_ops(ctx->scene, c);
  return FRM_OK;
}

int frm_eval_scene(frm_ctx* ctx, const float* points, uint32_t n, float* out_distance, float* out_color) {
  if (!ctx || !points || !out_distance || !out_color)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "NULL argument");
  if (!ctx->has_params) return fail(ctx, FRM_ERR_NOT_READY, "frm_set_parameters has not been called");
  if (n == 0) return FRM_OK;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  float* d = nullptr;
  FRM_HIP(ctx, hipMalloc(&d, (size_t)n * 7 * sizeof(float)));
  float *pts = d, *dist = d + 3 * (size_t)n, *col = d + 4 * (size_t)n;
  hipError_t e = hipMemcpyAsync(pts, points, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = launch_eval_scene(ctx->scene, pts, n, dist, col, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_distance, dist, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_color, col, (size_t)n * 12, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(ctx, e, "frm_eval_scene");
  return FRM_OK;
}

int frm_eval_math(frm_ctx* ctx, int32_t fn, const float* a, const float* b, uint32_t n, float* out) {
  if (!ctx || !a || !out || fn < 0 || fn > FRM_MATH_LAST) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "bad argument");
  if (n == 0) return FRM_OK;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  float* d = nullptr;
  FRM_HIP(ctx, hipMalloc(&d, (size_t)n * 3 * sizeof(float)));
  float *da = d, *db = b ? d + n : nullptr, *dout = d + 2 * (size_t)n;
  hipError_t e = hipMemcpyAsync(da, a, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && b) e = hipMemcpyAsync(db, b, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = launch_eval_math(fn, da, db, n, dout, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return hip_fail(ctx, e, "frm_eval_math");
  return FRM_OK;
}

}  // extern "C"
