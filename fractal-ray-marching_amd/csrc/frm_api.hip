// frm_api.hip — the C ABI of include/frm.h: context lifetime, size and frame mode, uniform upload,
// frm_render and its variants, readback and presentation (the stream-level stages: frm_stages.hip;
// diagnostics: frm_debug.hip). Replaces the reference's wgpu host layer
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

int not_on_group(frm_ctx* ctx, const char* what) {
  return fail(ctx, FRM_ERR_UNSUPPORTED, "%s: not available on a group context (frm_config.device_count)", what);
}

// `what` (an entry point) does not serve the context's frame mode.
int refuse_mode(frm_ctx* ctx, const char* what) {
  const ModeText& m = kModeText[frame_mode(ctx)];
  return fail(ctx, FRM_ERR_UNSUPPORTED, "%s: not available on a %s context (%s); %s; nothing changed", what, m.noun,
              m.setter, m.instead);
}
// Whether a frame mode other than `mine` is on (a setter's question).
static bool other_mode(const frm_ctx* ctx, FrameMode mine) {
  const FrameMode m = frame_mode(ctx);
  return m != kPlain && m != mine;
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

namespace {

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
  for (Slot& sl : ctx->slots) sl.no_second(true);  // second images of the old size
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
  const FrameMode mode = frame_mode(ctx);
  if (mode == kPanorama) {  // the output size is free of the render size
    if (int rc = check_size(ctx, width, height, 1, "panorama size")) return rc;
    return apply_panorama(ctx, width, height, ctx->panorama);
  }
  // an adaptive frame's refined pixels are those of its full supersampled counterpart: the same bound
  if (int rc = check_size(ctx, width, height, mode == kAdaptive ? ctx->adaptive : ctx->supersample, "frame size"))
    return rc;
  return apply_size(ctx, width, height, ctx->supersample);
}

int frm_set_supersampling(frm_ctx* ctx, uint32_t factor) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (factor == 0 || factor > FRM_MAX_SUPERSAMPLE)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "supersampling factor %u outside [1, %u]; factor not changed", factor,
                FRM_MAX_SUPERSAMPLE);
  if (factor > 1u && other_mode(ctx, kSupersampled)) return refuse_mode(ctx, "frm_set_supersampling");
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
  if (factor > 1u && other_mode(ctx, kAdaptive)) return refuse_mode(ctx, "frm_set_adaptive");
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
  if (frame_mode(ctx) == kPanorama) return render_panorama(ctx, stats);
  if (!stats && ring_eligible(ctx)) return ring_render(ctx);
  if ((rc = frame_prologue(ctx, stats))) return rc;
  Slot* sl = nullptr;
  hipStream_t s;
  if ((rc = begin_frame(ctx, &sl, &s))) return rc;
  KernelArgs a = make_args(ctx, ctx->params, ctx->scene, sl->fb(), ctx->counters, ctx->height, 0, 1, ctx->height);
  if (stats && (rc = stats_begin(ctx, s))) return rc;
  rc = launch(ctx, a, s);
  if (rc || (rc = resolve_frame(ctx, *sl))) return rc;
  show_slot(ctx, *sl);
  keep_render_params(ctx);
  return finish_stats(ctx, s, stats);
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
  if (int rc = check_output(ctx, out_width, out_height, flags)) return rc;
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
  if (int rc = check_output(ctx, out_width, out_height, flags)) return rc;
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
  // the refine kernel is not part of the runtime-compiled source; the depth pass reads the built-in kernels' records
  const FrameMode mode = frame_mode(ctx);
  if (source_dir && (mode == kAdaptive || mode == kDof)) return refuse_mode(ctx, "frm_reload");
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

int frm_render_bands(frm_ctx* ctx, uint8_t* dev_dst, size_t dst_bytes, uint32_t band_rows,
                     uint32_t first_band, uint32_t band_stride, void* stream, uint64_t* dev_counters) {
  int rc = ensure_ready(ctx);
  if (rc) return rc;
  if (ctx->group) return not_on_group(ctx, "frm_render_bands");
  if (frame_mode(ctx) != kPlain) return refuse_mode(ctx, "frm_render_bands");
  if (!dev_dst || band_rows == 0 || band_stride == 0)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "invalid dst or band geometry");
  uint32_t rows = 0;
  if ((rc = band_rows_u32(ctx, ctx->height, band_rows, first_band, band_stride, &rows))) return rc;
  size_t need = (size_t)rows * ctx->width * 4u;
  if (dst_bytes < need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu bytes, bands need %zu", dst_bytes, need);
  if ((rc = check_spans(ctx, {{"dev_dst", dev_dst, dst_bytes, need, 4, true},
                              {"dev_counters", dev_counters, 0, 0, 8, true}})))
    return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = ring_leave(ctx))) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  unsigned long long* counters = dev_counters ? (unsigned long long*)dev_counters : ctx->counters;
  KernelArgs a = make_args(ctx, ctx->params, ctx->scene, dev_dst, counters, band_rows, first_band, band_stride, rows);
  return launch(ctx, a, s);
}

int frm_render_bands_batch(frm_ctx* ctx, uint32_t count, const frm_parameters* params, uint8_t* dev_dst,
                           size_t dst_bytes, size_t frame_stride_bytes, uint32_t band_rows, uint32_t first_band,
                           uint32_t band_stride,
                           void* stream, uint64_t* dev_counters) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (ctx->group) return not_on_group(ctx, "frm_render_bands_batch");
  if (frame_mode(ctx) != kPlain) return refuse_mode(ctx, "frm_render_bands_batch");
  if (!ctx->width) return fail(ctx, FRM_ERR_NOT_READY, "frm_resize has not been called");
  if (!params || !dev_dst || count == 0 || count > FRM_MAX_BATCH || band_rows == 0 || band_stride == 0)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "invalid batch (count %u, at most %u) or band geometry", count,
                FRM_MAX_BATCH);
  uint32_t rows = 0;
  if (int rc = band_rows_u32(ctx, ctx->height, band_rows, first_band, band_stride, &rows)) return rc;
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
  BatchUniforms u;
  batch_uniforms(ctx, count, params, &u);
  if (int rc = check_parameters(ctx, u.s0, params[0])) return rc;
  uint32_t differs = u.differs;
  for (uint32_t k = 1; k < count && (!differs || k < differs); ++k)
    if (params[k].aspect_scale[0] != params[0].aspect_scale[0] || params[k].aspect_scale[1] != params[0].aspect_scale[1])
      differs = k;
  if (differs)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT,
                "batch frame %u differs from frame 0 in more than the camera and the Mandelbulb's time "
                "(scene, iterations, time-derived constants, aspect)",
                differs);
  // (the sizes were checked above: what is left of the one span check is the alignment)
  if (int rc = check_spans(ctx, {{"dev_dst", dev_dst, dst_bytes, need ? (count - 1u) * frame_stride_bytes + need : 0, 4, true},
                                 {"dev_counters", dev_counters, 0, 0, 8, true}}))
    return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  ctx->params = params[count - 1];  // the context's parameters: the batch's last frame
  compute_scene_uniforms(params[count - 1], ctx->flags, &ctx->scene);
  ctx->has_params = true;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  unsigned long long* counters = dev_counters ? (unsigned long long*)dev_counters : ctx->counters;
  return launch_frames(ctx, count, params, u, true, dev_dst, frame_stride_bytes,
                       BandGeometry{band_rows, first_band, band_stride, rows}, counters, s, -1);
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
  const FrameMode mode = frame_mode(ctx);  // the sub-frames of a supersampled context are resolved as they are summed
  if (mode != kPlain && mode != kSupersampled) return refuse_mode(ctx, "frm_render_shutter");
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
  int rc = frame_prologue(ctx, stats);
  if (rc) return rc;
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
  sl->no_second();
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
    BatchUniforms u;
    batch_uniforms(ctx, n, params + first, &u);
    if ((rc = launch_frames(ctx, n, params + first, u, true, sl->shutter_src.p, sub_bytes,
                            BandGeometry{ctx->height, 0, 1, ctx->height}, ctx->counters, s, (int)si)))
      return rc;
    const bool last = first + n == count;
    FRM_HIP(ctx, launch_shutter(sl->shutter_src.p, sub_bytes, n, acc, last ? frame : nullptr, ctx->out_width,
                                ctx->out_height, S, count * S * S, s));
  }
  FRM_HIP(ctx, hipEventRecord(sl->done, s));  // covers the accumulation
  show_slot(ctx, *sl);
  ctx->composed_seq = ctx->render_seq;
  ctx->composed_of = "frm_render_shutter sub-frames";
  keep_render_params(ctx);
  return finish_stats(ctx, s, stats);
}

// frm_render of a panorama context: the six faces rendered as one batch into the slot's scratch, then
// projected into its framebuffer.
static int render_panorama(frm_ctx* ctx, frm_stats* stats) {
  int rc = frame_prologue(ctx, stats);
  if (rc) return rc;
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
  sl->no_second();
  if (stats && (rc = stats_begin(ctx, s))) return rc;
  // the faces differ in their cameras alone (frm_panorama_parameters): frame 0's scene uniforms serve all
  BatchUniforms u;
  batch_uniforms(ctx, 6, faces, &u);
  if ((rc = launch_frames(ctx, 6, faces, u, false, sl->pano_src.p, face_bytes,
                          BandGeometry{ctx->height, 0, 1, ctx->height}, ctx->counters, s, (int)si)))
    return rc;
  FRM_HIP(ctx, launch_project_equirect(sl->pano_src.p, face_bytes, ctx->panorama, (const float*)sl->pano_tables.p,
                                       sl->fb(), ctx->out_width, ctx->out_height, s));
  FRM_HIP(ctx, hipEventRecord(sl->done, s));  // covers the projection
  show_slot(ctx, *sl);
  ctx->composed_seq = ctx->render_seq;
  ctx->composed_of = "a panorama's faces (frm_set_panorama)";
  keep_render_params(ctx);
  return finish_stats(ctx, s, stats);
}

int frm_set_panorama(frm_ctx* ctx, uint32_t face_size) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (face_size) {
    if (ctx->group) return not_on_group(ctx, "frm_set_panorama");
    if (other_mode(ctx, kPanorama)) return refuse_mode(ctx, "frm_set_panorama");
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

int frm_set_depth_of_field(frm_ctx* ctx, float aperture, float focus, uint32_t max_radius) {
  if (!ctx) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (max_radius) {
    if (int rc = check_lens(ctx, aperture, focus, max_radius)) return rc;
    if (ctx->group) return not_on_group(ctx, "frm_set_depth_of_field");
    if (other_mode(ctx, kDof)) return refuse_mode(ctx, "frm_set_depth_of_field");
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

}  // extern "C"
