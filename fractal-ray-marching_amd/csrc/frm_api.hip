// frm_api.hip — the C ABI of include/frm.h: context lifetime, uniform upload, frame dispatch and
// readback. Replaces the reference's wgpu host layer
// (graphics.rs:25-164, persistent_graphics.rs:33-173, blit_graphics.rs:16-62).
// Errors never cross the ABI as exceptions/aborts: every HIP failure becomes a status
// code plus a message retrievable with frm_last_error().
#include "frm_ctx.h"

static thread_local std::string g_error;  // failures without a context

int fail(frm_ctx* ctx, int code, const char* fmt, ...) {
  char buf[8192];  // room for a compiler log (frm_reload)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->error = buf;
  g_error = buf;
  return code;
}

int hip_fail(frm_ctx* ctx, hipError_t e, const char* what) {
  int code = (e == hipErrorOutOfMemory) ? FRM_ERR_OUT_OF_MEMORY : FRM_ERR_HIP;
  return fail(ctx, code, "%s failed: %s (%d)", what, hipGetErrorString(e), (int)e);
}

namespace {

int not_on_group(frm_ctx* ctx, const char* what) {
  return fail(ctx, FRM_ERR_UNSUPPORTED, "%s: not available on a group context (frm_config.device_count)", what);
}

int not_supersampled(frm_ctx* ctx, const char* what) {
  return fail(ctx, FRM_ERR_UNSUPPORTED,
              "%s: not available on a supersampled context (frm_set_supersampling); render the bands at the "
              "internal size on a plain context and call frm_resolve",
              what);
}

int not_adaptive(frm_ctx* ctx, const char* what) {
  return fail(ctx, FRM_ERR_UNSUPPORTED,
              "%s: not available on an adaptive context (frm_set_adaptive); render the bands on a plain "
              "context and call frm_refine",
              what);
}

int not_panorama(frm_ctx* ctx, const char* what) {
  return fail(ctx, FRM_ERR_UNSUPPORTED,
              "%s: not available on a panorama context (frm_set_panorama); render the faces "
              "(frm_panorama_parameters) on a plain context and call frm_project_equirect",
              what);
}

int not_dof(frm_ctx* ctx, const char* what) {
  return fail(ctx, FRM_ERR_UNSUPPORTED,
              "%s: not available on a depth-of-field context (frm_set_depth_of_field); switch that off, or render "
              "on a plain context and call frm_depth_of_field",
              what);
}

// The lens of frm_dof_coc, frm_depth_of_field and frm_set_depth_of_field.
int check_lens(frm_ctx* ctx, float aperture, float focus, uint32_t max_radius) {
  if (max_radius > FRM_MAX_DOF_RADIUS)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "depth-of-field radius %u above %u", max_radius, FRM_MAX_DOF_RADIUS);
  if (!(aperture >= 0.0f) || aperture > 3.402823466e+38f)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "depth-of-field aperture %g: not finite or negative", (double)aperture);
  if (!(focus > 0.0f) || focus > 3.402823466e+38f)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "depth-of-field focus %g: not finite and positive", (double)focus);
  return FRM_OK;
}

// The fractal loop work a frame's parameters ask for (include/frm.h FRM_MAX_NUM_ITERATIONS):
// trips of the DE's loop per evaluation, after the reference's own loop semantics
// (Sierpinski's i32 loop runs none for N >= 2^31: compute_scene_uniforms sets n = 0).
int check_parameters(frm_ctx* ctx, const SceneUniforms& su, const frm_parameters& p) {
  if (is_mandelbulb(su.family) && su.n == 0xFFFFFFFFu)
    return fail(ctx, FRM_ERR_UNSUPPORTED,
                "num_iterations 0xffffffff: the Mandelbulb's `i <= num_iterations` loop (fragment.wgsl:245) "
                "never ends; parameters not changed");
  const uint32_t trips = su.family == kSphere ? 0u : su.n;
  if (trips > FRM_MAX_NUM_ITERATIONS && !(ctx->flags & FRM_FLAG_UNBOUNDED_ITERATIONS))
    return fail(ctx, FRM_ERR_UNSUPPORTED,
                "num_iterations %u (scene %u) above FRM_MAX_NUM_ITERATIONS = %u: every DE runs that many "
                "loop bodies; create the context with FRM_FLAG_UNBOUNDED_ITERATIONS to allow it; "
                "parameters not changed",
                p.num_iterations, p.scene_index, FRM_MAX_NUM_ITERATIONS);
  return FRM_OK;
}

int ensure_ready(frm_ctx* ctx) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!ctx->width) return fail(ctx, FRM_ERR_NOT_READY, "frm_resize has not been called");
  if (!ctx->has_params) return fail(ctx, FRM_ERR_NOT_READY, "frm_set_parameters has not been called");
  return FRM_OK;
}

// The device source (src_w x src_h texels) and destination (dst_need bytes: "the `noun`") of
// frm_resolve, frm_refine and frm_blit, after their NULL checks: 4-byte aligned (frm_refine's
// counters, when given, 8-byte), large enough, not overlapping, reported in this order.
int check_src_dst(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, uint32_t src_w, uint32_t src_h,
                  const uint8_t* dev_dst, size_t dst_bytes, size_t dst_need, const char* noun,
                  const uint64_t* dev_counters = nullptr) {
  const uintptr_t sa = reinterpret_cast<uintptr_t>(dev_src), da = reinterpret_cast<uintptr_t>(dev_dst);
  if (sa % 4u || da % 4u) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "dev_src / dev_dst not 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(dev_counters) % 8u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "dev_counters not 8-byte aligned");
  const size_t src_need = (size_t)src_w * src_h * 4u;
  if (src_bytes < src_need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "src holds %zu bytes, %ux%u texels need %zu", src_bytes, src_w, src_h,
                src_need);
  if (dst_bytes < dst_need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu bytes, the %s needs %zu", dst_bytes, noun, dst_need);
  if (sa < da + dst_need && da < sa + src_need)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "dev_src and dev_dst overlap");
  return FRM_OK;
}

// The output size and blit flags of frm_present, frm_present_async and frm_blit; size_fmt: the
// caller's message for a bad size (width, height, FRM_MAX_DIMENSION).
int check_output(frm_ctx* ctx, uint32_t out_width, uint32_t out_height, uint32_t flags, const char* size_fmt) {
  if (out_width == 0 || out_height == 0 || out_width > FRM_MAX_DIMENSION || out_height > FRM_MAX_DIMENSION)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, size_fmt, out_width, out_height, FRM_MAX_DIMENSION);
  if (flags & ~(FRM_BLIT_SRGB | FRM_BLIT_BGRA)) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
  return FRM_OK;
}

// A context that failed to build: its message for frm_last_error(NULL), then released.
int create_failed(frm_ctx* ctx, int rc) {
  g_error = ctx->error;
  frm_destroy(ctx);
  return rc;
}

// The device state of a fresh context. A failure leaves what was built so far to frm_destroy.
int init_one(frm_ctx* ctx) {
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  FRM_HIP(ctx, hipDeviceGetAttribute(&ctx->cu_count, hipDeviceAttributeMultiprocessorCount, ctx->device));
  FRM_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  hipMemPoolProps props;
  memset(&props, 0, sizeof(props));
  props.allocType = hipMemAllocationTypePinned;
  props.handleTypes = hipMemHandleTypeNone;
  props.location.type = hipMemLocationTypeDevice;
  props.location.id = ctx->device;
  FRM_HIP(ctx, hipMemPoolCreate(&ctx->pool, &props));
  uint64_t keep = UINT64_MAX;
  FRM_HIP(ctx, hipMemPoolSetAttribute(ctx->pool, hipMemPoolAttrReleaseThreshold, &keep));
  FRM_HIP(ctx, hipEventCreate(&ctx->ev_start));
  FRM_HIP(ctx, hipEventCreate(&ctx->ev_stop));
  FRM_HIP(ctx, hipMalloc(&ctx->counters, FRM_NUM_COUNTERS * sizeof(unsigned long long)));
  ctx->slots[0].stream = ctx->stream;
  for (uint32_t i = 0; i < ctx->nslots; ++i) {
    Slot& sl = ctx->slots[i];
    for (hipEvent_t* ev : {&sl.done, &sl.keys_read, &sl.copied, &sl.fb_read[0], &sl.fb_read[1]})
      FRM_HIP(ctx, hipEventCreateWithFlags(ev, hipEventDisableTiming));
    FRM_HIP(ctx, hipMalloc(&sl.queue, kQueueBytes));
    FRM_HIP(ctx, hipMalloc(&sl.rank_words, 2 * kRankWords * sizeof(uint32_t)));
  }
  return FRM_OK;
}

}  // namespace

// One single-device context on `device` (frm_create's checks done).
int create_one(const frm_config* config, int device, frm_ctx** out_ctx) {
  frm_ctx* ctx = new (std::nothrow) frm_ctx();
  if (!ctx) return fail(nullptr, FRM_ERR_OUT_OF_MEMORY, "host allocation failed");
  ctx->device = device;
  ctx->max_steps = config->max_steps ? config->max_steps : FRM_DEFAULT_MAX_STEPS;
  ctx->flags = config->flags;
  ctx->nslots = config->frames_in_flight ? config->frames_in_flight : 1u;
  if (const char* env = getenv("FRM_SCHED")) ctx->fused_sched = strcmp(env, "sort") != 0;
  if (const char* env = getenv("FRM_RING")) ctx->ring_enabled = strcmp(env, "0") != 0;  // opt-in ring
  if (const char* env = getenv("FRM_RING_SERVICE")) {  // service waves of a ring grid (tuning)
    long v = strtol(env, nullptr, 10);
    if (v >= 1 && v <= 1024) ctx->ring.service_waves = (uint32_t)v;
  }
  if (const char* env = getenv("FRM_SERVICE_MIN")) {
    long v = strtol(env, nullptr, 10);
    if (v >= 1 && v <= 64) ctx->service_min = (uint32_t)v;
  }
  if (const char* env = getenv("FRM_SHUTTER_CHUNK")) {  // sub-frames per chunk of frm_render_shutter (tuning, tests)
    long v = strtol(env, nullptr, 10);
    if (v >= 1 && v <= (long)FRM_MAX_SHUTTER_SAMPLES) ctx->shutter_chunk = (uint32_t)v;
  }
  if (int rc = init_one(ctx)) return create_failed(ctx, rc);
  *out_ctx = ctx;
  return FRM_OK;
}

// A group: the context on devices[0] made one (frm_group.hip group_init).
static int create_group(const frm_config* config, frm_ctx** out_ctx) {
  frm_ctx* ctx = nullptr;
  if (int rc = create_one(config, config->devices[0], &ctx)) return rc;
  if (int rc = group_init(ctx, config)) return create_failed(ctx, rc);
  *out_ctx = ctx;
  return FRM_OK;
}

extern "C" {

uint32_t frm_abi_version(void) { return FRM_ABI_VERSION; }

const char* frm_last_error(const frm_ctx* ctx) { return ctx ? ctx->error.c_str() : g_error.c_str(); }

int frm_device_count(int32_t* out_count) {
  if (!out_count) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "out_count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *out_count = 0;
    return hip_fail(nullptr, e, "hipGetDeviceCount");
  }
  *out_count = n;
  return FRM_OK;
}

int frm_create(frm_ctx** out_ctx, const frm_config* config) {
  if (!out_ctx || !config) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "out_ctx/config is NULL");
  *out_ctx = nullptr;
  if (config->frames_in_flight > FRM_MAX_FRAMES_IN_FLIGHT)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "config.frames_in_flight %u above %u", config->frames_in_flight,
                FRM_MAX_FRAMES_IN_FLIGHT);
  if (config->max_steps > FRM_MAX_STEPS_LIMIT)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "config.max_steps %u above %u", config->max_steps,
                FRM_MAX_STEPS_LIMIT);
  const uint32_t kernels = FRM_FLAG_SIMPLE_KERNEL | FRM_FLAG_PERSISTENT_KERNEL;
  if ((config->flags & ~(kernels | FRM_FLAG_SCENE_SPHERE | FRM_FLAG_UNBOUNDED_ITERATIONS | FRM_FLAG_HW_MATH)) ||
      (config->flags & kernels) == kernels)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "config.flags 0x%x: unknown flag or both kernel flags",
                config->flags);
  if (config->device_count > FRM_MAX_DEVICES)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "config.device_count %u above %u", config->device_count,
                FRM_MAX_DEVICES);
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return fail(nullptr, FRM_ERR_NO_DEVICE, "no HIP device available (%s)", hipGetErrorString(e));
  if (config->device_count == 0) {
    if (config->device < 0 || config->device >= n)
      return fail(nullptr, FRM_ERR_NO_DEVICE, "device %d out of range [0, %d)", config->device, n);
    return create_one(config, config->device, out_ctx);
  }
  for (uint32_t r = 0; r < config->device_count; ++r)
    if (config->devices[r] < 0 || config->devices[r] >= n)
      return fail(nullptr, FRM_ERR_NO_DEVICE, "devices[%u] = %d out of range [0, %d)", r, config->devices[r], n);
  return create_group(config, out_ctx);
}

int frm_destroy(frm_ctx* ctx) {
  if (!ctx) return FRM_OK;
  group_destroy(ctx);  // a group's members first
  // Teardown is best effort: statuses are ignored so every resource gets released.
  (void)hipSetDevice(ctx->device);
  ring_destroy(ctx);
  for (uint32_t i = 0; i < ctx->nslots; ++i) {
    Slot& sl = ctx->slots[i];
    if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    if (sl.copy_stream) (void)hipStreamSynchronize(sl.copy_stream);
    if (sl.pending) (void)hipEventSynchronize(sl.done);
  }
  for (uint32_t i = 0; i < ctx->nslots; ++i) {
    Slot& sl = ctx->slots[i];
    // pool blocks back to the pool (every stream is idle), then the pool itself below
    if (ctx->stream) {
      for (const PoolBuf* b : {&sl.fbs[0], &sl.fbs[1], &sl.res[0], &sl.res[1], &sl.refine_list, &sl.records, &sl.present_dev,
                               &sl.shutter_src, &sl.shutter_acc, &sl.pano_src, &sl.pano_tables, &sl.depth})
        if (b->p) (void)hipFreeAsync(b->p, ctx->stream);
      for (void* b : {(void*)sl.refine_ctl, (void*)sl.sched_iota, (void*)sl.sched_order, (void*)sl.sched_keys, sl.sched_temp})
        if (b) (void)hipFreeAsync(b, ctx->stream);
    }
    if (sl.queue) (void)hipFree(sl.queue);
    if (sl.rank_words) (void)hipFree(sl.rank_words);
    for (hipEvent_t ev : {sl.done, sl.keys_read, sl.copied, sl.fb_read[0], sl.fb_read[1]})
      if (ev) (void)hipEventDestroy(ev);
    if (sl.host_img) (void)hipHostFree(sl.host_img);
    if (i > 0 && sl.stream) (void)hipStreamDestroy(sl.stream);
    if (sl.copy_stream) (void)hipStreamDestroy(sl.copy_stream);
  }
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  release_host_blocks(ctx, true);
  if (ctx->pool) (void)hipMemPoolDestroy(ctx->pool);
  if (ctx->present_buf) (void)hipFree(ctx->present_buf);
  unload_reloaded(ctx->reloaded);
  if (ctx->counters) (void)hipFree(ctx->counters);
  if (ctx->ev_start) (void)hipEventDestroy(ctx->ev_start);
  if (ctx->ev_stop) (void)hipEventDestroy(ctx->ev_stop);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return FRM_OK;
}

// The internal render size (supersample x the output size): everything that renders follows it.
static int resize_render(frm_ctx* ctx, uint32_t width, uint32_t height) {
  if (Group* G = ctx->group) {  // every member follows; the band geometry of the new size
    for (uint32_t r = 1; r < G->n; ++r)
      if (int rc = resize_render(G->sub[r], width, height)) return relay(ctx, G->sub[r], rc);
    G->band_rows = group_band_rows(height, G->n);
    G->stride = (size_t)band_local_rows(height, G->band_rows, 0, G->n) * width * 4u;
  }
  if (ctx->bands_only) {  // a group member: its band buffers belong to the group's frame slots
    ctx->width = width;
    ctx->height = height;
    return FRM_OK;
  }
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  // ring frames in flight finish first (a ring serves one size); their tickets keep their images
  if (int rc = ring_quiesce(ctx)) return rc;
  if (width != ctx->width || height != ctx->height) ctx->last_is_ring = false;
  if (ctx->slots[0].fb() && width == ctx->width && height == ctx->height) return FRM_OK;
  if (!ctx->slots[0].stream) return fail(ctx, FRM_ERR_HIP, "context stream missing");
  // No drain: frames in flight finish at their own size. Every buffer that follows the size grows
  // in its stream's order when a launch of the new size needs it (ensure_fb, launch); slot 0's
  // framebuffer (what frm_read_frame sees before the next frm_render) grows here.
  Slot& s0 = ctx->slots[0];
  int rc = select_fb(ctx, s0, s0.fb_idx);
  if (rc || (rc = ensure_fb(ctx, s0, (size_t)width * height * 4u))) return rc;
  ctx->width = width;
  ctx->height = height;
  ctx->last_slot = 0;
  for (Slot& sl : ctx->slots) sl.adaptive[0] = sl.adaptive[1] = sl.dof[0] = sl.dof[1] = false;  // second images of the old size
  // no frame of the new size yet: frm_read_frame_async / frm_present_async refuse until the next
  // frm_render (tickets issued before keep their frames)
  ctx->render_seq = 0;
  return FRM_OK;
}

// An output size and a supersampling factor (checked by the callers): the render size is their
// product. The slot that frm_read_frame sees before the next frm_render gets its resolved image.
static int apply_size(frm_ctx* ctx, uint32_t width, uint32_t height, uint32_t factor) {
  int rc = resize_render(ctx, factor * width, factor * height);
  if (rc) return rc;
  ctx->supersample = factor;
  if (Group* G = ctx->group)
    for (uint32_t r = 1; r < G->n; ++r) G->sub[r]->supersample = factor;
  ctx->out_width = width;
  ctx->out_height = height;
  if (factor > 1u) {
    Slot& sl = ctx->slots[ctx->last_slot];
    if ((rc = select_fb(ctx, sl, sl.fb_idx)) || (rc = ensure_res(ctx, sl, (size_t)width * height * 4u))) return rc;
  }
  return FRM_OK;
}

// An output size and a panorama face size N >= 1 (checked by the callers): the render size is that
// of a face with its guard band, (N + 2)^2. The framebuffer that frm_read_frame sees before the
// next frm_render holds the larger of a face and the panorama (shown() hands it out at the output
// size; begin_frame and render_panorama grow the others).
static int apply_panorama(frm_ctx* ctx, uint32_t width, uint32_t height, uint32_t face_size) {
  const uint32_t m = face_size + 2u;
  int rc = resize_render(ctx, m, m);
  if (rc) return rc;
  ctx->panorama = face_size;
  ctx->out_width = width;
  ctx->out_height = height;
  Slot& sl = ctx->slots[ctx->last_slot];
  const size_t face = (size_t)m * m * 4u, out = (size_t)width * height * 4u;
  if ((rc = select_fb(ctx, sl, sl.fb_idx)) || (rc = ensure_fb(ctx, sl, face > out ? face : out))) return rc;
  ctx->render_seq = 0;  // no panorama of this shape yet
  return FRM_OK;
}

int frm_resize(frm_ctx* ctx, uint32_t width, uint32_t height) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (ctx->panorama) {  // the output size is free of the render size
    if (width == 0 || height == 0 || width > FRM_MAX_DIMENSION || height > FRM_MAX_DIMENSION)
      return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "panorama size %ux%u outside [1, %u]^2", width, height,
                  FRM_MAX_DIMENSION);
    return apply_panorama(ctx, width, height, ctx->panorama);
  }
  // an adaptive frame's refined pixels are those of its full supersampled counterpart: the same bound
  const uint32_t factor = ctx->adaptive > 1u ? ctx->adaptive : ctx->supersample;
  const uint32_t limit = FRM_MAX_DIMENSION / factor;
  if (width == 0 || height == 0 || width > limit || height > limit)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "frame size %ux%u outside [1, %u]^2 (supersampling %u)", width, height,
                limit, factor);
  return apply_size(ctx, width, height, ctx->supersample);
}

int frm_set_supersampling(frm_ctx* ctx, uint32_t factor) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (factor == 0 || factor > FRM_MAX_SUPERSAMPLE)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "supersampling factor %u outside [1, %u]; factor not changed", factor,
                FRM_MAX_SUPERSAMPLE);
  if (factor > 1u && ctx->dof_radius)
    return fail(ctx, FRM_ERR_UNSUPPORTED,
                "supersampling factor %u on a depth-of-field context (frm_set_depth_of_field): switch that off "
                "first; factor not changed",
                factor);
  if (factor > 1u && ctx->panorama)
    return fail(ctx, FRM_ERR_UNSUPPORTED,
                "supersampling factor %u on a panorama context (frm_set_panorama): switch that off first; "
                "factor not changed",
                factor);
  if (factor > 1u && ctx->adaptive > 1u)
    return fail(ctx, FRM_ERR_UNSUPPORTED,
                "supersampling factor %u on an adaptive context (frm_set_adaptive): switch that off first; "
                "factor not changed",
                factor);
  if (ctx->out_width) {
    const uint32_t limit = FRM_MAX_DIMENSION / factor;
    if (ctx->out_width > limit || ctx->out_height > limit)
      return fail(ctx, FRM_ERR_INVALID_ARGUMENT,
                  "supersampling factor %u: the %ux%u frame would render above %u texels a side; factor not changed",
                  factor, ctx->out_width, ctx->out_height, FRM_MAX_DIMENSION);
    if (factor == ctx->supersample) return FRM_OK;
    return apply_size(ctx, ctx->out_width, ctx->out_height, factor);
  }
  ctx->supersample = factor;
  if (Group* G = ctx->group)
    for (uint32_t r = 1; r < G->n; ++r) G->sub[r]->supersample = factor;
  return FRM_OK;
}

int frm_get_supersampling(const frm_ctx* ctx, uint32_t* out_factor) {
  if (!ctx || !out_factor) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx/out_factor is NULL");
  *out_factor = ctx->supersample;
  return FRM_OK;
}

int frm_resolve(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, uint32_t out_width, uint32_t out_height,
                uint32_t factor, uint8_t* dev_dst, size_t dst_bytes, void* stream) {
  if (!ctx || !dev_src || !dev_dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_src/dev_dst is NULL");
  if (factor == 0 || factor > FRM_MAX_SUPERSAMPLE)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "supersampling factor %u outside [1, %u]", factor, FRM_MAX_SUPERSAMPLE);
  const uint32_t limit = FRM_MAX_DIMENSION / factor;
  if (out_width == 0 || out_height == 0 || out_width > limit || out_height > limit)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "output size %ux%u outside [1, %u]^2 (factor %u)", out_width, out_height,
                limit, factor);
  if (int rc = check_src_dst(ctx, dev_src, src_bytes, factor * out_width, factor * out_height, dev_dst, dst_bytes,
                             (size_t)out_width * out_height * 4u, "frame"))
    return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  FRM_HIP(ctx, launch_resolve(dev_src, dev_dst, out_width, out_height, factor, s));
  return FRM_OK;
}

int frm_set_adaptive(frm_ctx* ctx, uint32_t factor, uint32_t threshold) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (factor == 0 || factor > FRM_MAX_SUPERSAMPLE || threshold > 256u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT,
                "adaptive factor %u outside [1, %u] or edge threshold %u above 256; values not changed", factor,
                FRM_MAX_SUPERSAMPLE, threshold);
  const uint32_t limit = FRM_MAX_DIMENSION / factor;
  if (ctx->out_width > limit || ctx->out_height > limit)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT,
                "adaptive factor %u: the %ux%u frame's samples would lie on a frame above %u texels a side; values "
                "not changed",
                factor, ctx->out_width, ctx->out_height, FRM_MAX_DIMENSION);
  if (factor > 1u && ctx->dof_radius)
    return fail(ctx, FRM_ERR_UNSUPPORTED,
                "adaptive factor %u on a depth-of-field context (frm_set_depth_of_field): switch that off first; "
                "values not changed",
                factor);
  if (factor > 1u && ctx->panorama)
    return fail(ctx, FRM_ERR_UNSUPPORTED,
                "adaptive factor %u on a panorama context (frm_set_panorama): switch that off first; values "
                "not changed",
                factor);
  if (factor > 1u && ctx->supersample > 1u)
    return fail(ctx, FRM_ERR_UNSUPPORTED,
                "adaptive factor %u on a supersampled context (frm_set_supersampling): switch that off first; values "
                "not changed",
                factor);
  if (factor > 1u && ctx->reloaded)
    return fail(ctx, FRM_ERR_UNSUPPORTED,
                "adaptive factor %u with runtime-reloaded kernels (frm_reload): the refine kernel is built in; values "
                "not changed",
                factor);
  if (factor == ctx->adaptive && threshold == ctx->edge_threshold) return FRM_OK;
  // No drain: frames in flight and their tickets keep their bytes; like a size change, there is no
  // frame under the new setting for the async readbacks until the next frm_render.
  if (ctx->width) {
    FRM_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ring_leave(ctx)) return rc;
  }
  ctx->adaptive = factor;
  ctx->edge_threshold = threshold;
  ctx->render_seq = 0;
  return FRM_OK;
}

int frm_get_adaptive(const frm_ctx* ctx, uint32_t* out_factor, uint32_t* out_threshold) {
  if (!ctx || !out_factor || !out_threshold)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx/out_factor/out_threshold is NULL");
  *out_factor = ctx->adaptive;
  *out_threshold = ctx->edge_threshold;
  return FRM_OK;
}

int frm_refine(frm_ctx* ctx, const frm_parameters* params, const uint8_t* dev_src, size_t src_bytes, uint32_t width,
               uint32_t height, uint32_t factor, uint32_t threshold, uint8_t* dev_dst, size_t dst_bytes,
               uint64_t* dev_counters, void* stream) {
  if (!ctx || !dev_src || !dev_dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_src/dev_dst is NULL");
  if (factor == 0 || factor > FRM_MAX_SUPERSAMPLE || threshold > 256u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "adaptive factor %u outside [1, %u] or edge threshold %u above 256", factor,
                FRM_MAX_SUPERSAMPLE, threshold);
  const uint32_t limit = FRM_MAX_DIMENSION / factor;
  if (width == 0 || height == 0 || width > limit || height > limit)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "frame size %ux%u outside [1, %u]^2 (factor %u)", width, height, limit,
                factor);
  const size_t need = (size_t)width * height * 4u;
  if (int rc = check_src_dst(ctx, dev_src, src_bytes, width, height, dev_dst, dst_bytes, need, "frame", dev_counters))
    return rc;
  frm_parameters p;
  SceneUniforms su;
  if (params) {
    p = *params;
    compute_scene_uniforms(p, ctx->flags, &su);
    if (int rc = check_parameters(ctx, su, p)) return rc;
  } else {
    if (!ctx->has_params) return fail(ctx, FRM_ERR_NOT_READY, "params is NULL and frm_set_parameters has not been called");
    p = ctx->params;
    su = ctx->scene;
  }
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // scratch per call, allocated and released in the order of the call's stream: calls in flight on
  // different streams never share it
  uint32_t *list = nullptr, *ctl = nullptr;
  int rc = dev_alloc(ctx, (void**)&list, need, s);
  if (rc) return rc;
  if ((rc = dev_alloc(ctx, (void**)&ctl, kRefineCtlBytes, s))) {
    (void)hipFreeAsync(list, s);
    return rc;
  }
  FrameUniforms f;
  compute_frame_uniforms(p, factor * width, factor * height, ctx->max_steps, &f);
  const hipError_t e = launch_adaptive(f, su, dev_src, dev_dst, width, height, factor, threshold, list, ctl,
                                       (unsigned long long*)dev_counters, ctx->cu_count, s);
  const int r1 = dev_release(ctx, list, s), r2 = dev_release(ctx, ctl, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "launch_adaptive");
  return r1 ? r1 : r2;
}

int frm_debug_refine_mask(frm_ctx* ctx, uint8_t* out, size_t n) {
  if (!ctx || !out) return -fail(ctx, FRM_ERR_INVALID_ARGUMENT, "NULL argument");
  if (ctx->last_is_ring || !ctx->render_seq)
    return -fail(ctx, FRM_ERR_NOT_READY, "frm_debug_refine_mask: no adaptive frm_render under the current settings");
  const Slot& sl = ctx->slots[ctx->last_slot];
  if (!sl.adaptive[sl.fb_idx] || sl.seq != ctx->render_seq || !sl.refine_list.p)
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

int frm_blit(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, uint32_t src_width, uint32_t src_height,
             uint8_t* dev_dst, size_t dst_bytes, uint32_t out_width, uint32_t out_height, uint32_t flags, void* stream) {
  if (!ctx || !dev_src || !dev_dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_src/dev_dst is NULL");
  if (src_width == 0 || src_height == 0 || src_width > FRM_MAX_DIMENSION || src_height > FRM_MAX_DIMENSION)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "source size %ux%u outside [1, %u]^2", src_width, src_height,
                FRM_MAX_DIMENSION);
  if (int rc = check_output(ctx, out_width, out_height, flags, "output size %ux%u outside [1, %u]^2")) return rc;
  if (int rc = check_src_dst(ctx, dev_src, src_bytes, src_width, src_height, dev_dst, dst_bytes,
                             (size_t)out_width * out_height * 4u, "output"))
    return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  FRM_HIP(ctx, launch_blit(dev_src, src_width, src_height, dev_dst, out_width, out_height, flags, s));
  return FRM_OK;
}

int frm_set_parameters(frm_ctx* ctx, const frm_parameters* parameters) {
  if (!ctx || !parameters) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/parameters is NULL");
  SceneUniforms su;
  compute_scene_uniforms(*parameters, ctx->flags, &su);
  int rc = check_parameters(ctx, su, *parameters);
  if (rc) return rc;
  ctx->params = *parameters;
  ctx->scene = su;
  ctx->has_params = true;
  if (Group* G = ctx->group)  // the members render the same frame (same flags, same uniforms)
    for (uint32_t r = 1; r < G->n; ++r) {
      G->sub[r]->params = *parameters;
      G->sub[r]->scene = su;
      G->sub[r]->has_params = true;
    }
  return FRM_OK;
}

static int render_panorama(frm_ctx* ctx, frm_stats* stats);

int frm_render(frm_ctx* ctx, frm_stats* stats) {
  int rc = ensure_ready(ctx);
  if (rc) return rc;
  if (ctx->group) return group_render(ctx, stats);
  if (ctx->panorama) return render_panorama(ctx, stats);
  if (!stats && ring_eligible(ctx)) return ring_render(ctx);
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = ring_quiesce(ctx))) return rc;  // a frame outside the ring: the ring's frames first
  ctx->last_is_ring = false;
  if (stats && (rc = synchronize_all(ctx))) return rc;  // the counters must hold this frame alone
  Slot* sl = nullptr;
  hipStream_t s;
  if ((rc = begin_frame(ctx, &sl, &s))) return rc;
  KernelArgs a = make_args(ctx, ctx->params, ctx->scene, sl->fb(), ctx->counters, ctx->height, 0, 1, ctx->height);
  if (stats && (rc = stats_begin(ctx, s))) return rc;
  rc = launch(ctx, a, s);
  if (rc || (rc = resolve_frame(ctx, *sl))) return rc;
  show_slot(ctx, *sl);
  keep_render_params(ctx);
  if (stats) {
    uint64_t host[FRM_NUM_COUNTERS];
    float ms = 0.0f;
    if ((rc = stats_end(ctx, s, host, &ms)) || (rc = frm_stats_from_counters(ctx, host, stats))) return rc;
    stats->kernel_ms = ms;
  }
  return FRM_OK;
}

int frm_read_frame(frm_ctx* ctx, uint8_t* dst, size_t dst_bytes) {
  if (!ctx || !dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dst is NULL");
  if (!ctx->width) return fail(ctx, FRM_ERR_NOT_READY, "frm_resize has not been called");
  size_t need = (size_t)ctx->out_width * ctx->out_height * 4u;
  if (dst_bytes < need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu bytes, frame needs %zu", dst_bytes, need);
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_materialize(ctx)) return rc;
  const Slot& sl = ctx->slots[ctx->last_slot];  // the frame of the last frm_render
  FRM_HIP(ctx, hipMemcpyAsync(dst, shown(ctx, sl), need, hipMemcpyDeviceToHost, sl.stream));
  FRM_HIP(ctx, hipStreamSynchronize(sl.stream));
  return FRM_OK;
}

int frm_present(frm_ctx* ctx, uint32_t out_width, uint32_t out_height, uint32_t flags, uint8_t* dst,
                size_t dst_bytes) {
  if (!ctx || !dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dst is NULL");
  if (!ctx->width) return fail(ctx, FRM_ERR_NOT_READY, "frm_resize has not been called");
  if (int rc = check_output(ctx, out_width, out_height, flags, "bad output size %ux%u")) return rc;
  const size_t need = (size_t)out_width * out_height * 4u;
  if (dst_bytes < need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu bytes, output needs %zu", dst_bytes, need);
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_materialize(ctx)) return rc;
  const Slot& sl = ctx->slots[ctx->last_slot];  // the frame of the last frm_render
  if (need > ctx->present_cap) {
    FRM_HIP(ctx, hipStreamSynchronize(sl.stream));
    if (ctx->present_buf) FRM_HIP(ctx, hipFree(ctx->present_buf));
    ctx->present_buf = nullptr;
    ctx->present_cap = 0;
    FRM_HIP(ctx, hipMalloc(&ctx->present_buf, need));
    ctx->present_cap = need;
  }
  FRM_HIP(ctx, launch_blit(shown(ctx, sl), ctx->out_width, ctx->out_height, ctx->present_buf, out_width, out_height, flags,
                           sl.stream));
  FRM_HIP(ctx, hipMemcpyAsync(dst, ctx->present_buf, need, hipMemcpyDeviceToHost, sl.stream));
  FRM_HIP(ctx, hipStreamSynchronize(sl.stream));
  return FRM_OK;
}

// The slot's copy stream, ordered after the slot's last launch (its render).
static int copy_stream_after_render(frm_ctx* ctx, Slot& sl) {
  if (ctx->nslots >= 2 && sl.last_stream) {  // stream order: after the render
    sl.rb_stream = sl.last_stream;
    return FRM_OK;
  }
  if (!sl.copy_stream) FRM_HIP(ctx, hipStreamCreateWithFlags(&sl.copy_stream, hipStreamNonBlocking));
  FRM_HIP(ctx, hipStreamWaitEvent(sl.copy_stream, sl.done, 0));
  sl.rb_stream = sl.copy_stream;
  return FRM_OK;
}

// Enqueues the copy of `bytes` device bytes of the last frm_render's slot into its pinned host
// image (on sl.rb_stream, after copy_stream_after_render) and hands out a ticket for it.
static int readback_async(frm_ctx* ctx, Slot& sl, const uint8_t* src, size_t bytes, uint64_t* out_ticket) {
  if (bytes > sl.host_cap) {
    // the image's previous contents belong to an expired ticket (an earlier frame of this slot);
    // only its copy may still be running
    if (sl.copy_ticket) FRM_HIP(ctx, hipEventSynchronize(sl.copied));
    if (sl.host_img) FRM_HIP(ctx, hipHostFree(sl.host_img));
    sl.host_img = nullptr;
    sl.host_cap = 0;
    sl.copy_ticket = 0;
    const size_t cap = with_headroom(bytes);
    FRM_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&sl.host_img), cap, hipHostMallocDefault));
    sl.host_cap = cap;
  }
  FRM_HIP(ctx, hipMemcpyAsync(sl.host_img, src, bytes, hipMemcpyDeviceToHost, sl.rb_stream));
  FRM_HIP(ctx, hipEventRecord(sl.copied, sl.rb_stream));
  // the framebuffer is read (by this copy, or by frm_present_async's blit before it) until here
  FRM_HIP(ctx, hipEventRecord(sl.fb_read[sl.fb_idx], sl.rb_stream));
  sl.fb_read_pending[sl.fb_idx] = true;
  sl.copy_ticket = ++ctx->ticket_seq;
  sl.copy_bytes = bytes;
  *out_ticket = sl.copy_ticket;
  return FRM_OK;
}

int frm_read_frame_async(frm_ctx* ctx, uint64_t* out_ticket) {
  if (!ctx || !out_ticket) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/out_ticket is NULL");
  if (!ctx->width) return fail(ctx, FRM_ERR_NOT_READY, "frm_resize has not been called");
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->last_is_ring) return ring_read_async(ctx, out_ticket);
  if (!ctx->render_seq) return fail(ctx, FRM_ERR_NOT_READY, "no frm_render since the context was created");
  Slot& sl = ctx->slots[ctx->last_slot];  // the frame of the last frm_render
  int rc = copy_stream_after_render(ctx, sl);
  if (rc) return rc;
  return readback_async(ctx, sl, shown(ctx, sl), (size_t)ctx->out_width * ctx->out_height * 4u, out_ticket);
}

int frm_present_async(frm_ctx* ctx, uint32_t out_width, uint32_t out_height, uint32_t flags, uint64_t* out_ticket) {
  if (!ctx || !out_ticket) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/out_ticket is NULL");
  if (!ctx->width) return fail(ctx, FRM_ERR_NOT_READY, "frm_resize has not been called");
  if (!ctx->render_seq) return fail(ctx, FRM_ERR_NOT_READY, "no frm_render since the context was created");
  if (int rc = check_output(ctx, out_width, out_height, flags, "bad output size %ux%u")) return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_materialize(ctx)) return rc;
  Slot& sl = ctx->slots[ctx->last_slot];
  const size_t need = (size_t)out_width * out_height * 4u;
  int rc = copy_stream_after_render(ctx, sl);
  if (rc) return rc;
  if (need > sl.present_dev.cap) {  // its last use (an earlier frame of this slot) is ordered before
    if (sl.copy_ticket && sl.rb_stream) FRM_HIP(ctx, hipEventSynchronize(sl.copied));  // maybe on another stream
    if ((rc = pool_grow(ctx, sl.present_dev, need, sl.rb_stream))) return rc;
  }
  FRM_HIP(ctx, launch_blit(shown(ctx, sl), ctx->out_width, ctx->out_height, sl.present_dev.p, out_width, out_height, flags,
                           sl.rb_stream));
  return readback_async(ctx, sl, sl.present_dev.p, need, out_ticket);
}

int frm_frame_pixels(frm_ctx* ctx, uint64_t ticket, const uint8_t** out_pixels, size_t* out_bytes) {
  if (!ctx || !out_pixels) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/out_pixels is NULL");
  if (ticket) {  // a ring frame's zero-copy image
    const int rc = ring_ticket_pixels(ctx, ticket, out_pixels, out_bytes);
    if (rc >= 0) return rc;
  }
  for (uint32_t i = 0; i < ctx->nslots && ticket; ++i) {
    Slot& sl = ctx->slots[i];
    if (sl.copy_ticket != ticket) continue;
    FRM_HIP(ctx, hipSetDevice(ctx->device));
    FRM_HIP(ctx, hipEventSynchronize(sl.copied));
    *out_pixels = sl.host_img;
    if (out_bytes) *out_bytes = sl.copy_bytes;
    return FRM_OK;
  }
  return fail(ctx, FRM_ERR_INVALID_ARGUMENT,
              "ticket %llu is not held (expired: its slot has been read back again since, or never issued)",
              (unsigned long long)ticket);
}

int frm_reload(frm_ctx* ctx, const char* source_dir) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  // a group reloads every member: all compile, or every member keeps its kernels
  const uint32_t n = ctx->group ? ctx->group->n : 1u;
  ReloadedKernels* rk[FRM_MAX_DEVICES] = {};
  if (source_dir && ctx->adaptive > 1u)  // the refine kernel is not part of the runtime-compiled source
    return fail(ctx, FRM_ERR_UNSUPPORTED, "frm_reload on an adaptive context (frm_set_adaptive); previous kernels kept");
  if (source_dir && ctx->dof_radius)  // the depth pass reads the built-in kernels' records
    return fail(ctx, FRM_ERR_UNSUPPORTED,
                "frm_reload on a depth-of-field context (frm_set_depth_of_field); previous kernels kept");
  if (source_dir)
    for (uint32_t r = 0; r < n; ++r) {
      std::string log;
      const int rc = compile_reloaded(source_dir, member(ctx, r)->device, &rk[r], &log);
      if (rc != FRM_OK) {
        for (uint32_t q = 0; q < r; ++q) unload_reloaded(rk[q]);
        return fail(ctx, rc, "reload failed, previous kernels kept: %s", log.c_str());
      }
    }
  if (int rc = ring_leave(ctx)) {
    for (uint32_t r = 0; r < n; ++r) unload_reloaded(rk[r]);
    return rc;
  }
  for (uint32_t r = 0; r < n; ++r) {
    frm_ctx* c = member(ctx, r);
    // the old module may still run, on this context's stream or a caller's (frm_render_bands)
    FRM_HIP(ctx, hipSetDevice(c->device));
    FRM_HIP(ctx, hipDeviceSynchronize());
    unload_reloaded(c->reloaded);
    c->reloaded = rk[r];
  }
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  return FRM_OK;
}

int frm_synchronize(frm_ctx* ctx) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (ctx->group) return group_synchronize(ctx);
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_quiesce(ctx)) return rc;
  return synchronize_all(ctx);
}

int frm_kernel_for_pixels(const frm_ctx* ctx, uint64_t pixels, uint32_t* out_kernel) {
  if (!ctx || !out_kernel) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx/out_kernel is NULL");
  *out_kernel = kernel_for(ctx, pixels) == kKernelSimple ? FRM_KERNEL_SIMPLE : FRM_KERNEL_PERSISTENT;
  return FRM_OK;
}

int frm_group_band_rows(uint32_t height, uint32_t devices, uint32_t* out_band_rows) {
  if (!out_band_rows || height == 0 || devices == 0 || devices > FRM_MAX_DEVICES)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "invalid height %u or device count %u", height, devices);
  *out_band_rows = group_band_rows(height, devices);
  return FRM_OK;
}

int frm_band_rows_for(uint32_t height, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
                      uint32_t* out_rows) {
  if (!out_rows || height == 0 || band_rows == 0 || band_stride == 0)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "invalid band geometry");
  *out_rows = band_local_rows(height, band_rows, first_band, band_stride);
  return FRM_OK;
}

int frm_render_bands(frm_ctx* ctx, uint8_t* dev_dst, size_t dst_bytes, uint32_t band_rows,
                     uint32_t first_band, uint32_t band_stride, void* stream, uint64_t* dev_counters) {
  int rc = ensure_ready(ctx);
  if (rc) return rc;
  if (ctx->group) return not_on_group(ctx, "frm_render_bands");
  if (ctx->supersample > 1u) return not_supersampled(ctx, "frm_render_bands");
  if (ctx->adaptive > 1u) return not_adaptive(ctx, "frm_render_bands");
  if (ctx->panorama) return not_panorama(ctx, "frm_render_bands");
  if (ctx->dof_radius) return not_dof(ctx, "frm_render_bands");
  if (!dev_dst || band_rows == 0 || band_stride == 0)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "invalid dst or band geometry");
  uint32_t rows = band_local_rows(ctx->height, band_rows, first_band, band_stride);
  size_t need = (size_t)rows * ctx->width * 4u;
  if (dst_bytes < need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu bytes, bands need %zu", dst_bytes, need);
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = ring_leave(ctx))) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  unsigned long long* counters = dev_counters ? (unsigned long long*)dev_counters : ctx->counters;
  KernelArgs a = make_args(ctx, ctx->params, ctx->scene, dev_dst, counters, band_rows, first_band, band_stride, rows);
  return launch(ctx, a, s);
}

// The frames of one multi-frame launch may differ in camera, and for the Mandelbulb in time (its
// power, fragment.wgsl:75, is the only time-derived constant): otherwise the same scene uniforms
// (scene, iterations, time-derived constants). Returns the first frame whose uniforms differ from
// frame 0's in more than that (0: none); *s0: frame 0's uniforms, powers[k]: frame k's power,
// *anim: the powers differ.
static uint32_t batch_uniforms(const frm_ctx* ctx, uint32_t count, const frm_parameters* params, SceneUniforms* s0,
                               float* powers, bool* anim) {
  compute_scene_uniforms(params[0], ctx->flags, s0);
  *anim = false;
  powers[0] = s0->mb_power;
  for (uint32_t k = 1; k < count; ++k) {
    SceneUniforms sk;
    compute_scene_uniforms(params[k], ctx->flags, &sk);
    powers[k] = sk.mb_power;
    if (is_mandelbulb(s0->family) && sk.family == s0->family && sk.mb_power != s0->mb_power) {
      *anim = true;
      sk.mb_power = s0->mb_power;
      sk.mb_power_m1 = s0->mb_power_m1;
    }
    if (memcmp(s0, &sk, sizeof(sk)) != 0) return k;
  }
  return 0;
}
// Whether `count` such frames of a.npix local pixels share one launch; else one launch per frame:
// the simple kernel has no queue to share; runtime-reloaded modules carry the single-frame kernels
// only; per-frame powers need the Mandelbulb's N >= 1 kernels.
static bool batch_shares_launch(const frm_ctx* ctx, const KernelArgs& a, uint32_t count, bool anim) {
  return !(count == 1 || kernel_for(ctx, a.npix) == kKernelSimple || ctx->reloaded || (anim && a.s.n == 0));
}
// Makes `a` (make_args of any of the frames) the shared launch of the `count` frames, frame k written
// frame_stride_bytes after frame k - 1.
static void set_batch(const frm_ctx* ctx, KernelArgs& a, uint32_t count, const frm_parameters* params,
                      const float* powers, bool anim, size_t frame_stride_bytes) {
  a.batch = count;
  a.out_stride = (uint32_t)(frame_stride_bytes / 4u);
  a.anim = anim ? 1u : 0u;
  memcpy(a.mb_powers, powers, sizeof(float) * count);
  FrameUniforms fk;
  for (uint32_t k = 0; k < count; ++k) {
    compute_frame_uniforms(params[k], ctx->width, ctx->height, ctx->max_steps, &fk);
    memcpy(a.cams[k].row, fk.row, sizeof(fk.row));
    a.cams[k].origin = fk.origin;
  }
}

int frm_render_bands_batch(frm_ctx* ctx, uint32_t count, const frm_parameters* params, uint8_t* dev_dst,
                           size_t dst_bytes, size_t frame_stride_bytes, uint32_t band_rows, uint32_t first_band,
                           uint32_t band_stride,
                           void* stream, uint64_t* dev_counters) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (ctx->group) return not_on_group(ctx, "frm_render_bands_batch");
  if (ctx->supersample > 1u) return not_supersampled(ctx, "frm_render_bands_batch");
  if (ctx->adaptive > 1u) return not_adaptive(ctx, "frm_render_bands_batch");
  if (ctx->panorama) return not_panorama(ctx, "frm_render_bands_batch");
  if (ctx->dof_radius) return not_dof(ctx, "frm_render_bands_batch");
  if (!ctx->width) return fail(ctx, FRM_ERR_NOT_READY, "frm_resize has not been called");
  if (!params || !dev_dst || count == 0 || count > FRM_MAX_BATCH || band_rows == 0 || band_stride == 0)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "invalid batch (count %u, at most %u) or band geometry", count,
                FRM_MAX_BATCH);
  const uint32_t rows = band_local_rows(ctx->height, band_rows, first_band, band_stride);
  const size_t need = (size_t)rows * ctx->width * 4u;
  if (frame_stride_bytes < need || frame_stride_bytes % 4u || frame_stride_bytes / 4u > 0xFFFFFFFFull)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT,
                "frame stride %zu: below a frame's %zu bytes, not a multiple of 4 or not below 16 GiB",
                frame_stride_bytes, need);
  // a stride of 0 passes the check above only for a rank without bands (need == 0): its frames
  // occupy no bytes
  if (dst_bytes < need || (frame_stride_bytes != 0 && (dst_bytes - need) / frame_stride_bytes < count - 1u))
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu bytes, %u frames %zu bytes apart need %zu", dst_bytes,
                count, frame_stride_bytes, (size_t)(count - 1u) * frame_stride_bytes + need);
  // fetch positions are u32 and every wave's last queue claims run up to two chunks past the
  // end (kQueueHeadroom covers any persistent grid): keep them from wrapping
  if ((uint64_t)rows * ctx->width * count >= 0xFFFFFFFFull - kQueueHeadroom)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "batch of %u frames of %u x %u local pixels too large", count,
                ctx->width, rows);
  // the frames share their scene uniforms (batch_uniforms) and their aspect
  SceneUniforms s0;
  bool anim = false;
  float powers[FRM_MAX_BATCH];
  uint32_t differs = batch_uniforms(ctx, count, params, &s0, powers, &anim);
  if (int rc = check_parameters(ctx, s0, params[0])) return rc;
  for (uint32_t k = 1; k < count && (!differs || k < differs); ++k)
    if (params[k].aspect_scale[0] != params[0].aspect_scale[0] || params[k].aspect_scale[1] != params[0].aspect_scale[1])
      differs = k;
  if (differs)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT,
                "batch frame %u differs from frame 0 in more than the camera and the Mandelbulb's time "
                "(scene, iterations, time-derived constants, aspect)",
                differs);
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  ctx->params = params[count - 1];  // the context's parameters: the batch's last frame
  compute_scene_uniforms(params[count - 1], ctx->flags, &ctx->scene);
  ctx->has_params = true;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  unsigned long long* counters = dev_counters ? (unsigned long long*)dev_counters : ctx->counters;
  KernelArgs a = make_args(ctx, ctx->params, ctx->scene, dev_dst, counters, band_rows, first_band, band_stride, rows);
  if (!batch_shares_launch(ctx, a, count, anim)) {  // one launch per frame
    for (uint32_t k = 0; k < count; ++k) {
      SceneUniforms sk;
      compute_scene_uniforms(params[k], ctx->flags, &sk);
      a = make_args(ctx, params[k], sk, dev_dst + (size_t)k * frame_stride_bytes, counters, band_rows, first_band,
                    band_stride, rows);
      if (int rc = launch(ctx, a, s)) return rc;
    }
    return FRM_OK;
  }
  set_batch(ctx, a, count, params, powers, anim, frame_stride_bytes);
  return launch(ctx, a, s);
}

// Sub-frames per chunk of a shutter frame of the context's size (include/frm.h frm_render_shutter):
// what the context allows (FRM_SHUTTER_CHUNK), 1 GiB of scratch and a shared launch's u32 fetch
// positions (frm_render_bands_batch), at least 1.
static uint32_t shutter_chunk(const frm_ctx* ctx, uint32_t count) {
  const uint64_t npix = (uint64_t)ctx->width * ctx->height;
  uint64_t n = count < ctx->shutter_chunk ? count : ctx->shutter_chunk;
  const uint64_t by_bytes = (1ull << 30) / (npix * 4u), by_queue = (0xFFFFFFFFull - kQueueHeadroom - 1u) / npix;
  if (n > by_bytes) n = by_bytes;
  if (n > by_queue) n = by_queue;
  return n ? (uint32_t)n : 1u;
}

int frm_render_shutter(frm_ctx* ctx, uint32_t count, const frm_parameters* params, frm_stats* stats) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (!params || count == 0 || count > FRM_MAX_SHUTTER_SAMPLES)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "params is NULL or count %u outside [1, %u]", count,
                FRM_MAX_SHUTTER_SAMPLES);
  if (ctx->group) return not_on_group(ctx, "frm_render_shutter");
  if (ctx->adaptive > 1u)
    return fail(ctx, FRM_ERR_UNSUPPORTED, "frm_render_shutter: not available on an adaptive context (frm_set_adaptive)");
  if (ctx->panorama) return not_panorama(ctx, "frm_render_shutter");
  if (ctx->dof_radius) return not_dof(ctx, "frm_render_shutter");
  if (!ctx->width) return fail(ctx, FRM_ERR_NOT_READY, "frm_resize has not been called");
  for (uint32_t k = 0; k < count; ++k) {
    SceneUniforms sk;
    compute_scene_uniforms(params[k], ctx->flags, &sk);
    if (int rc = check_parameters(ctx, sk, params[k])) return rc;
    if (params[k].scene_index != params[0].scene_index || params[k].num_iterations != params[0].num_iterations ||
        params[k].aspect_scale[0] != params[0].aspect_scale[0] || params[k].aspect_scale[1] != params[0].aspect_scale[1])
      return fail(ctx, FRM_ERR_INVALID_ARGUMENT,
                  "sub-frame %u differs from sub-frame 0 in scene_index, num_iterations or aspect_scale", k);
  }
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ring_quiesce(ctx);  // a frame outside the ring: the ring's frames first
  if (rc) return rc;
  ctx->last_is_ring = false;
  if (stats && (rc = synchronize_all(ctx))) return rc;  // the counters must hold this frame alone
  ctx->params = params[count - 1];
  compute_scene_uniforms(ctx->params, ctx->flags, &ctx->scene);
  ctx->has_params = true;
  const uint32_t si = ctx->next_slot;
  Slot* sl = nullptr;
  hipStream_t s;
  if ((rc = begin_frame(ctx, &sl, &s))) return rc;
  const uint32_t S = ctx->supersample, chunk = shutter_chunk(ctx, count);
  const size_t sub_bytes = (size_t)ctx->width * ctx->height * 4u, npix_out = (size_t)ctx->out_width * ctx->out_height;
  const bool carried = chunk < count;  // several chunks: their sums go through the slot's accumulator
  if ((rc = ensure_shutter(ctx, *sl, chunk * sub_bytes, carried ? npix_out * sizeof(float4) : 0))) return rc;
  sl->adaptive[sl->fb_idx] = sl->dof[sl->fb_idx] = false;
  uint8_t* frame = sl->fb();  // what shown() reads of the slot
  if (S > 1u) {
    if ((rc = ensure_res(ctx, *sl, npix_out * 4u))) return rc;
    frame = sl->res[sl->fb_idx].p;
  }
  float* acc = carried ? (float*)sl->shutter_acc.p : nullptr;
  if (acc) FRM_HIP(ctx, hipMemsetAsync(acc, 0, npix_out * sizeof(float4), s));
  if (stats && (rc = stats_begin(ctx, s))) return rc;
  for (uint32_t first = 0; first < count; first += chunk) {
    const uint32_t n = count - first < chunk ? count - first : chunk;
    const frm_parameters* ps = params + first;
    SceneUniforms s0;
    float powers[FRM_MAX_BATCH];
    bool anim = false;
    const bool same = batch_uniforms(ctx, n, ps, &s0, powers, &anim) == 0;
    KernelArgs a = make_args(ctx, ps[0], s0, sl->shutter_src.p, ctx->counters, ctx->height, 0, 1, ctx->height);
    // every launch of the frame runs on its slot (launch() takes the context's next one and moves on)
    if (same && batch_shares_launch(ctx, a, n, anim)) {
      set_batch(ctx, a, n, ps, powers, anim, sub_bytes);
      ctx->next_slot = si;
      if ((rc = launch(ctx, a, s))) return rc;
    } else {
      for (uint32_t k = 0; k < n; ++k) {
        SceneUniforms sk;
        compute_scene_uniforms(ps[k], ctx->flags, &sk);
        a = make_args(ctx, ps[k], sk, sl->shutter_src.p + k * sub_bytes, ctx->counters, ctx->height, 0, 1, ctx->height);
        ctx->next_slot = si;
        if ((rc = launch(ctx, a, s))) return rc;
      }
    }
    const bool last = first + n == count;
    FRM_HIP(ctx, launch_shutter(sl->shutter_src.p, sub_bytes, n, acc, last ? frame : nullptr, ctx->out_width,
                                ctx->out_height, S, count * S * S, s));
  }
  FRM_HIP(ctx, hipEventRecord(sl->done, s));  // covers the accumulation
  show_slot(ctx, *sl);
  ctx->shutter_seq = ctx->render_seq;
  keep_render_params(ctx);
  if (stats) {
    uint64_t host[FRM_NUM_COUNTERS];
    float ms = 0.0f;
    if ((rc = stats_end(ctx, s, host, &ms)) || (rc = frm_stats_from_counters(ctx, host, stats))) return rc;
    stats->kernel_ms = ms;
  }
  return FRM_OK;
}

int frm_accumulate(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, size_t frame_stride_bytes, uint32_t count,
                   uint32_t out_width, uint32_t out_height, uint32_t factor, float* dev_acc, size_t acc_bytes,
                   uint32_t divisor, uint8_t* dev_dst, size_t dst_bytes, void* stream) {
  if (!ctx || !dev_src || (!dev_acc && !dev_dst))
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_src is NULL, or both dev_acc and dev_dst are");
  if (factor == 0 || factor > FRM_MAX_SUPERSAMPLE || count == 0 || count > FRM_MAX_SHUTTER_SAMPLES)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "factor %u outside [1, %u] or count %u outside [1, %u]", factor,
                FRM_MAX_SUPERSAMPLE, count, FRM_MAX_SHUTTER_SAMPLES);
  const uint32_t limit = FRM_MAX_DIMENSION / factor;
  if (out_width == 0 || out_height == 0 || out_width > limit || out_height > limit)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "output size %ux%u outside [1, %u]^2 (factor %u)", out_width, out_height,
                limit, factor);
  if (dev_dst && divisor == 0) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "divisor is 0");
  const size_t npix = (size_t)out_width * out_height, frame_need = npix * factor * factor * 4u;
  const uintptr_t sa = reinterpret_cast<uintptr_t>(dev_src), aa = reinterpret_cast<uintptr_t>(dev_acc),
                  da = reinterpret_cast<uintptr_t>(dev_dst);
  if (sa % 4u || da % 4u || aa % 16u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "dev_src / dev_dst not 4-byte aligned or dev_acc not 16-byte aligned");
  if (frame_stride_bytes % 4u || frame_stride_bytes < frame_need)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "frame stride %zu: below a frame's %zu bytes or not a multiple of 4",
                frame_stride_bytes, frame_need);
  if (src_bytes < frame_need || (src_bytes - frame_need) / frame_stride_bytes < count - 1u)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "src holds %zu bytes, %u frames %zu bytes apart need %zu", src_bytes, count,
                frame_stride_bytes, (size_t)(count - 1u) * frame_stride_bytes + frame_need);
  const size_t src_need = (size_t)(count - 1u) * frame_stride_bytes + frame_need;
  const size_t acc_need = dev_acc ? npix * sizeof(float4) : 0, dst_need = dev_dst ? npix * 4u : 0;
  if (acc_bytes < acc_need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "acc holds %zu bytes, the sums need %zu", acc_bytes, acc_need);
  if (dst_bytes < dst_need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu bytes, the frame needs %zu", dst_bytes, dst_need);
  auto overlap = [](uintptr_t a, size_t an, uintptr_t b, size_t bn) { return an && bn && a < b + bn && b < a + an; };
  if (overlap(sa, src_need, aa, acc_need) || overlap(sa, src_need, da, dst_need) || overlap(aa, acc_need, da, dst_need))
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "dev_src, dev_acc and dev_dst overlap");
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  FRM_HIP(ctx, launch_shutter(dev_src, frame_stride_bytes, count, dev_acc, dev_dst, out_width, out_height, factor, divisor, s));
  return FRM_OK;
}

// frm_render of a panorama context: frm_render_shutter's steps with the six faces as the batch and
// the projection in the place of the accumulation.
static int render_panorama(frm_ctx* ctx, frm_stats* stats) {
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ring_quiesce(ctx);  // a frame outside the ring: the ring's frames first
  if (rc) return rc;
  ctx->last_is_ring = false;
  if (stats && (rc = synchronize_all(ctx))) return rc;  // the counters must hold this frame alone
  frm_parameters faces[6];
  frm_panorama_parameters(&ctx->params, ctx->panorama, faces);
  const uint32_t si = ctx->next_slot;
  Slot* sl = nullptr;
  hipStream_t s;
  if ((rc = begin_frame(ctx, &sl, &s))) return rc;
  const size_t face_bytes = (size_t)ctx->width * ctx->height * 4u;
  // the frame shown() hands out is the panorama: the slot's framebuffer holds it, the faces are scratch
  if ((rc = ensure_fb(ctx, *sl, (size_t)ctx->out_width * ctx->out_height * 4u)) ||
      (rc = ensure_panorama(ctx, *sl, 6u * face_bytes, ctx->out_width, ctx->out_height)))
    return rc;
  sl->adaptive[sl->fb_idx] = sl->dof[sl->fb_idx] = false;
  if (stats && (rc = stats_begin(ctx, s))) return rc;
  // the faces differ in their cameras alone (frm_panorama_parameters)
  SceneUniforms s0;
  float powers[FRM_MAX_BATCH];
  bool anim = false;
  (void)batch_uniforms(ctx, 6, faces, &s0, powers, &anim);
  KernelArgs a = make_args(ctx, faces[0], s0, sl->pano_src.p, ctx->counters, ctx->height, 0, 1, ctx->height);
  // every launch of the frame runs on its slot (launch() takes the context's next one and moves on)
  if (batch_shares_launch(ctx, a, 6, anim)) {
    set_batch(ctx, a, 6, faces, powers, anim, face_bytes);
    ctx->next_slot = si;
    if ((rc = launch(ctx, a, s))) return rc;
  } else {
    for (uint32_t k = 0; k < 6u; ++k) {
      a = make_args(ctx, faces[k], s0, sl->pano_src.p + k * face_bytes, ctx->counters, ctx->height, 0, 1, ctx->height);
      ctx->next_slot = si;
      if ((rc = launch(ctx, a, s))) return rc;
    }
  }
  FRM_HIP(ctx, launch_project_equirect(sl->pano_src.p, face_bytes, ctx->panorama, (const float*)sl->pano_tables.p,
                                       sl->fb(), ctx->out_width, ctx->out_height, s));
  FRM_HIP(ctx, hipEventRecord(sl->done, s));  // covers the projection
  show_slot(ctx, *sl);
  ctx->panorama_seq = ctx->render_seq;
  keep_render_params(ctx);
  if (stats) {
    uint64_t host[FRM_NUM_COUNTERS];
    float ms = 0.0f;
    if ((rc = stats_end(ctx, s, host, &ms)) || (rc = frm_stats_from_counters(ctx, host, stats))) return rc;
    stats->kernel_ms = ms;
  }
  return FRM_OK;
}

int frm_set_panorama(frm_ctx* ctx, uint32_t face_size) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (face_size) {
    if (ctx->group) return not_on_group(ctx, "frm_set_panorama");
    if (ctx->supersample > 1u) return not_supersampled(ctx, "frm_set_panorama");
    if (ctx->adaptive > 1u) return not_adaptive(ctx, "frm_set_panorama");
    if (ctx->dof_radius) return not_dof(ctx, "frm_set_panorama");
    // the six faces are one batch in one scratch: 1 GiB of it at most, and a shared launch's u32
    // fetch positions (frm_render_bands_batch)
    const uint64_t m = (uint64_t)face_size + 2u, npix = 6u * m * m;
    if (m > FRM_MAX_DIMENSION || npix * 4u > (1ull << 30) || npix >= 0xFFFFFFFFull - kQueueHeadroom)
      return fail(ctx, FRM_ERR_INVALID_ARGUMENT,
                  "panorama face size %u: six faces of %llu texels a side exceed %u a side or 1 GiB; face size not "
                  "changed",
                  face_size, (unsigned long long)m, FRM_MAX_DIMENSION);
  }
  if (face_size == ctx->panorama) return FRM_OK;
  // No drain: frames in flight and their tickets keep their bytes; like a size change, there is no
  // frame under the new setting for the async readbacks until the next frm_render.
  if (!ctx->out_width) {
    ctx->panorama = face_size;
    return FRM_OK;
  }
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  if (face_size) return apply_panorama(ctx, ctx->out_width, ctx->out_height, face_size);
  if (int rc = apply_size(ctx, ctx->out_width, ctx->out_height, ctx->supersample)) return rc;
  ctx->panorama = 0;
  ctx->render_seq = 0;
  return FRM_OK;
}

int frm_get_panorama(const frm_ctx* ctx, uint32_t* out_face_size) {
  if (!ctx || !out_face_size) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx/out_face_size is NULL");
  *out_face_size = ctx->panorama;
  return FRM_OK;
}

int frm_panorama_face_size(uint32_t width, uint32_t* out_face_size) {
  if (!out_face_size || width == 0 || width > FRM_MAX_DIMENSION)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "out_face_size is NULL or width %u outside [1, %u]", width,
                FRM_MAX_DIMENSION);
  *out_face_size = (width + 3u) / 4u;
  return FRM_OK;
}

int frm_equirect_tables(uint32_t width, uint32_t height, float* sin_lon, float* cos_lon, float* sin_lat,
                        float* cos_lat) {
  if (!sin_lon || !cos_lon || !sin_lat || !cos_lat || width == 0 || height == 0 || width > FRM_MAX_DIMENSION ||
      height > FRM_MAX_DIMENSION)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "a table is NULL or size %ux%u outside [1, %u]^2", width, height,
                FRM_MAX_DIMENSION);
  float* t = new (std::nothrow) float[2u * (size_t)width + 2u * (size_t)height];
  if (!t) return fail(nullptr, FRM_ERR_OUT_OF_MEMORY, "host allocation failed");
  equirect_tables(width, height, t);
  memcpy(sin_lon, t, width * sizeof(float));
  memcpy(cos_lon, t + width, width * sizeof(float));
  memcpy(sin_lat, t + 2u * (size_t)width, height * sizeof(float));
  memcpy(cos_lat, t + 2u * (size_t)width + height, height * sizeof(float));
  delete[] t;
  return FRM_OK;
}

int frm_project_equirect(frm_ctx* ctx, const uint8_t* dev_faces, size_t faces_bytes, size_t face_stride_bytes,
                         uint32_t face_size, uint8_t* dev_dst, size_t dst_bytes, uint32_t out_width,
                         uint32_t out_height, void* stream) {
  if (!ctx || !dev_faces || !dev_dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_faces/dev_dst is NULL");
  if (face_size == 0 || face_size > FRM_MAX_DIMENSION - 2u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "face size %u outside [1, %u]", face_size, FRM_MAX_DIMENSION - 2u);
  if (out_width == 0 || out_height == 0 || out_width > FRM_MAX_DIMENSION || out_height > FRM_MAX_DIMENSION)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "output size %ux%u outside [1, %u]^2", out_width, out_height,
                FRM_MAX_DIMENSION);
  const size_t m = (size_t)face_size + 2u, face_need = m * m * 4u;
  const uintptr_t fa = reinterpret_cast<uintptr_t>(dev_faces), da = reinterpret_cast<uintptr_t>(dev_dst);
  if (fa % 4u || da % 4u) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "dev_faces / dev_dst not 4-byte aligned");
  if (face_stride_bytes % 4u || face_stride_bytes < face_need)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "face stride %zu: below a face's %zu bytes or not a multiple of 4",
                face_stride_bytes, face_need);
  if (faces_bytes < face_need || (faces_bytes - face_need) / face_stride_bytes < 5u)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "faces hold %zu bytes, six faces %zu bytes apart need %zu", faces_bytes,
                face_stride_bytes, 5u * face_stride_bytes + face_need);
  const size_t src_need = 5u * face_stride_bytes + face_need, dst_need = (size_t)out_width * out_height * 4u;
  if (dst_bytes < dst_need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu bytes, the panorama needs %zu", dst_bytes, dst_need);
  if (fa < da + dst_need && da < fa + src_need)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "dev_faces and dev_dst overlap");
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // the tables are scratch per call, allocated and released in the order of the call's stream: calls
  // in flight on different streams never share them
  float* tables = nullptr;
  int rc = dev_alloc(ctx, (void**)&tables, (2u * (size_t)out_width + 2u * (size_t)out_height) * sizeof(float), s);
  if (rc) return rc;
  hipError_t e = hipSuccess;
  if (!(rc = upload_tables(ctx, tables, out_width, out_height, s)))
    e = launch_project_equirect(dev_faces, face_stride_bytes, face_size, tables, dev_dst, out_width, out_height, s);
  const int r1 = dev_release(ctx, tables, s);
  if (rc) return rc;
  if (e != hipSuccess) return hip_fail(ctx, e, "launch_project_equirect");
  return r1;
}

int frm_dof_coc(float aperture, float focus, uint32_t max_radius, const float* depth, size_t n, float* out_c) {
  if (!depth || !out_c) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "depth/out_c is NULL");
  if (int rc = check_lens(nullptr, aperture, focus, max_radius)) return rc;
  dof_coc_host(aperture, focus, max_radius, depth, n, out_c);
  return FRM_OK;
}

int frm_depth_of_field(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, const float* dev_depth,
                       size_t depth_bytes, uint32_t width, uint32_t height, float aperture, float focus,
                       uint32_t max_radius, uint8_t* dev_dst, size_t dst_bytes, void* stream) {
  if (!ctx || !dev_src || !dev_depth || !dev_dst)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_src/dev_depth/dev_dst is NULL");
  if (width == 0 || height == 0 || width > FRM_MAX_DIMENSION || height > FRM_MAX_DIMENSION)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "frame size %ux%u outside [1, %u]^2", width, height, FRM_MAX_DIMENSION);
  if (int rc = check_lens(ctx, aperture, focus, max_radius)) return rc;
  const size_t need = (size_t)width * height * 4u;  // of each of the three
  if (int rc = check_src_dst(ctx, dev_src, src_bytes, width, height, dev_dst, dst_bytes, need, "frame")) return rc;
  const uintptr_t za = reinterpret_cast<uintptr_t>(dev_depth), da = reinterpret_cast<uintptr_t>(dev_dst);
  if (za % 4u) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "dev_depth not 4-byte aligned");
  if (depth_bytes < need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "depth holds %zu bytes, %ux%u floats need %zu", depth_bytes, width, height,
                need);
  if (za < da + need && da < za + need) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "dev_depth and dev_dst overlap");
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  FRM_HIP(ctx, launch_dof(dev_src, dev_depth, dev_dst, width, height, aperture, focus, max_radius, s));
  return FRM_OK;
}

int frm_set_depth_of_field(frm_ctx* ctx, float aperture, float focus, uint32_t max_radius) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (max_radius) {
    if (int rc = check_lens(ctx, aperture, focus, max_radius)) return rc;
    if (ctx->group) return not_on_group(ctx, "frm_set_depth_of_field");
    if (ctx->supersample > 1u) return not_supersampled(ctx, "frm_set_depth_of_field");
    if (ctx->adaptive > 1u) return not_adaptive(ctx, "frm_set_depth_of_field");
    if (ctx->panorama) return not_panorama(ctx, "frm_set_depth_of_field");
    if (ctx->flags & FRM_FLAG_SIMPLE_KERNEL)
      return fail(ctx, FRM_ERR_UNSUPPORTED,
                  "frm_set_depth_of_field: the depth plane comes from the persistent kernel's records; not available "
                  "with FRM_FLAG_SIMPLE_KERNEL");
    if (ctx->reloaded)
      return fail(ctx, FRM_ERR_UNSUPPORTED,
                  "frm_set_depth_of_field with runtime-reloaded kernels (frm_reload): the depth pass reads the built-in "
                  "kernels' records");
  }
  const bool same_bits = memcmp(&aperture, &ctx->dof_aperture, sizeof(float)) == 0 &&
                         memcmp(&focus, &ctx->dof_focus, sizeof(float)) == 0;
  if (max_radius == ctx->dof_radius && (same_bits || max_radius == 0)) {
    ctx->dof_aperture = aperture;
    ctx->dof_focus = focus;
    return FRM_OK;
  }
  // No drain: frames in flight and their tickets keep their bytes; like a size change, there is no
  // frame under the new setting for the async readbacks until the next frm_render.
  if (ctx->width) {
    FRM_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ring_leave(ctx)) return rc;
  }
  ctx->dof_radius = max_radius;
  ctx->dof_aperture = aperture;
  ctx->dof_focus = focus;
  ctx->render_seq = 0;
  return FRM_OK;
}

int frm_get_depth_of_field(const frm_ctx* ctx, float* out_aperture, float* out_focus, uint32_t* out_max_radius) {
  if (!ctx || !out_aperture || !out_focus || !out_max_radius)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx/out_aperture/out_focus/out_max_radius is NULL");
  *out_aperture = ctx->dof_aperture;
  *out_focus = ctx->dof_focus;
  *out_max_radius = ctx->dof_radius;
  return FRM_OK;
}

int frm_unshuffle_bands(frm_ctx* ctx, const uint8_t* dev_src, size_t rank_stride_bytes, uint8_t* dev_dst,
                        size_t dst_bytes, uint32_t band_rows, uint32_t ranks, void* stream) {
  if (!ctx || !dev_src || !dev_dst || band_rows == 0 || ranks == 0)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "invalid unshuffle arguments");
  if (ctx->supersample > 1u) return not_supersampled(ctx, "frm_unshuffle_bands");
  if (ctx->adaptive > 1u) return not_adaptive(ctx, "frm_unshuffle_bands");
  if (ctx->panorama) return not_panorama(ctx, "frm_unshuffle_bands");
  if (ctx->dof_radius) return not_dof(ctx, "frm_unshuffle_bands");
  if (!ctx->width) return fail(ctx, FRM_ERR_NOT_READY, "frm_resize has not been called");
  size_t need = (size_t)ctx->width * ctx->height * 4u;
  if (dst_bytes < need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu bytes, frame needs %zu", dst_bytes, need);
  uint32_t rows = band_local_rows(ctx->height, band_rows, 0, ranks);
  if (rank_stride_bytes < (size_t)rows * ctx->width * 4u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "rank stride %zu below one rank's bands", rank_stride_bytes);
  if (rank_stride_bytes % 4u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "rank stride must be a multiple of 4");
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  FRM_HIP(ctx, launch_unshuffle(dev_src, rank_stride_bytes, dev_dst, ctx->width, ctx->height, band_rows,
                                ranks, s));
  return FRM_OK;
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
  if (ctx->render_seq && ctx->shutter_seq == ctx->render_seq && !ctx->last_is_ring)
    return fail(ctx, FRM_ERR_NOT_READY, "the last frame was a frm_render_shutter frame: no single frame to trace");
  if (ctx->render_seq && ctx->panorama_seq == ctx->render_seq && !ctx->last_is_ring)
    return fail(ctx, FRM_ERR_NOT_READY, "the last frame was a panorama (frm_set_panorama): no single frame to trace");
  if (!ctx->render_seq || sl.seq != ctx->render_seq)
    return fail(ctx, FRM_ERR_NOT_READY, "no frm_render, or a later launch reused its slot's records");
  if (!sl.records.p || sl.records.cap < npix * kRecordBytes || !sl.sched_whole || sl.sched_w != ctx->width || sl.sched_h != ctx->height)
    return fail(ctx, FRM_ERR_NOT_READY, "the last frm_render was not a persistent launch of this frame size");
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
  if (ctx->render_seq && ctx->shutter_seq == ctx->render_seq && !ctx->last_is_ring)
    return fail(ctx, FRM_ERR_NOT_READY, "the last frame was a frm_render_shutter frame: no single frame's depth");
  if (ctx->render_seq && ctx->panorama_seq == ctx->render_seq && !ctx->last_is_ring)
    return fail(ctx, FRM_ERR_NOT_READY, "the last frame was a panorama (frm_set_panorama): no single frame's depth");
  if (!ctx->render_seq || sl.seq != ctx->render_seq)
    return fail(ctx, FRM_ERR_NOT_READY, "no frm_render, or a later launch reused its slot's records");
  if (!sl.records.p || sl.records.cap < npix * kRecordBytes || !sl.sched_whole || sl.sched_w != ctx->width || sl.sched_h != ctx->height)
    return fail(ctx, FRM_ERR_NOT_READY, "the last frm_render was not a persistent launch of this frame size");
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  hipError_t e = hipSuccess;
  if (sl.dof[sl.fb_idx] && sl.depth.p && sl.depth_w == ctx->width && sl.depth_h == ctx->height) {
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
