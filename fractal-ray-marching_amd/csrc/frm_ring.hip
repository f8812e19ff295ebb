// frm_ring.hip — the resident frame ring of a context (opt-in, FRM_RING=1; frm_internal.h RingArgs).
// Single-frame frm_render calls without stats on a context with frames in flight post their frames
// to the context's ring instead of launching a grid each: one persistent
// grid marches the posted frames in order (a wave moves on to the next frame when one's queue
// drains, as a multi-frame launch interleaves its frames) and its service waves shade, rank and
// publish each frame as its last pixel finishes, so a frame's tail overlaps the next frame's bulk as
// it does inside frm_render_bands_batch. The grid lives as long as frames keep arriving: a march wave
// that finds nothing left closes it (the last frame it serves is then fixed), and the host launches
// the next grid when it sees the closed flag after posting (the post and the flag are ordered by
// sequentially consistent accesses on both sides, so a frame is either seen by the closing grid or
// served by the next one). frm_read_frame_async tickets of ring frames are zero-copy: the shading also
// writes the frame into a pinned host image. Anything else on the context first drains the ring
// (ring_quiesce).
#include "frm_ctx.h"

static uint32_t ring_size(const frm_ctx* ctx) { return ctx->nslots >= 3 ? 4u : 2u; }

// Whether frm_render(ctx, NULL) goes through the ring.
bool ring_eligible(const frm_ctx* ctx) {
  if (!ctx->ring_enabled || ctx->group || ctx->bands_only || ctx->reloaded || ctx->nslots < 2) return false;
  if (frame_mode(ctx) != kPlain) return false;  // ring frames are not resolved, refined, gathered or projected
  const uint64_t npix = (uint64_t)ctx->width * ctx->height;
  if (kernel_for(ctx, npix) != kKernelPersistent || npix > (1ull << 28)) return false;
  // a ring's service waves give up after kRingWatchdogTicks (2 s) without progress: keep the
  // costliest possible pixel (2 marches of max_steps DEs of N + 1 bodies) well inside that
  const uint64_t trips = (ctx->scene.family == kSphere ? 0u : (uint64_t)ctx->scene.n) + 2u;
  return 2ull * ctx->max_steps * trips <= (1ull << 21);
}

static bool ring_same_gen(const frm_ctx* ctx) {
  const Ring& R = ctx->ring;
  if (!R.gen_valid || R.w != ctx->width || R.h != ctx->height || R.max_steps != ctx->max_steps ||
      R.aspect[0] != ctx->params.aspect_scale[0] || R.aspect[1] != ctx->params.aspect_scale[1] ||
      R.slots != ring_size(ctx))
    return false;
  SceneUniforms a = R.su, b = ctx->scene;
  if (is_mandelbulb(a.family)) {  // ring frames carry their own power (march_persistent<..., ANIM, RES>)
    a.mb_power = b.mb_power = 0.f;
    a.mb_power_m1 = b.mb_power_m1 = 0.f;
  }
  return memcmp(&a, &b, sizeof(a)) == 0;
}

// Waits (host) until ring frame `seq` (slot s) is done. A grid that ended without it (a service
// wave's watchdog) is reported instead of waited for.
static int ring_wait(frm_ctx* ctx, uint32_t s, uint32_t seq) {
  Ring& R = ctx->ring;
  for (uint64_t spin = 1;; ++spin) {
    if (__atomic_load_n(&R.host->done[s][0], __ATOMIC_ACQUIRE) >= seq) return FRM_OK;
    if ((spin & 255u) == 0) {
      const hipError_t e = hipStreamQuery(ctx->stream);
      if (e == hipSuccess) {
        if (__atomic_load_n(&R.host->done[s][0], __ATOMIC_ACQUIRE) >= seq) return FRM_OK;
        return fail(ctx, FRM_ERR_HIP, "resident frame ring: frame %u never completed (its grid ended)", seq);
      }
      if (e != hipErrorNotReady) return hip_fail(ctx, e, "hipStreamQuery");
      sched_yield();
    }
  }
}

// Every posted ring frame done and the ring's grids ended (the last one closes once nothing is
// left to claim). The context stream is then idle.
int ring_quiesce(frm_ctx* ctx) {
  Ring& R = ctx->ring;
  if (!R.grid_id) return FRM_OK;
  const uint32_t first = R.last_seq >= R.slots ? R.last_seq - R.slots + 1u : 1u;
  for (uint32_t q = first; q <= R.last_seq && q >= 1u; ++q)
    if (int rc = ring_wait(ctx, (q - 1u) & (R.slots - 1u), q)) return rc;
  FRM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FRM_OK;
}

static void ring_free_buffers(Ring& R) {
  for (void* b : {(void*)R.records, (void*)R.out, (void*)R.order, (void*)R.keys, (void*)R.iota, (void*)R.keys_sorted,
                  R.sched_temp})
    if (b) (void)hipFree(b);
  R.records = nullptr;
  R.out = R.order = R.iota = nullptr;
  R.keys = R.keys_sorted = nullptr;
  R.sched_temp = nullptr;
  R.cap = 0;
  R.keys_valid = false;
}

static void ring_free_images(Ring& R) {
  for (uint32_t s = 0; s < kRingSlots; ++s)
    for (uint32_t par = 0; par < 2; ++par) {
      uint32_t*& p = R.img[s][par];
      if (p && R.img_ticket[s][par])  // a ticket still names it (frm_frame_pixels)
        R.retired.push_back({R.img_ticket[s][par], p, R.img_seq[s][par], s, R.img_bytes[s][par]});
      else if (p)
        (void)hipHostFree(p);
      p = nullptr;
    }
  memset(R.img_seq, 0, sizeof(R.img_seq));
  memset(R.img_ticket, 0, sizeof(R.img_ticket));
  R.img_cap = 0;
}

// A fresh ring for the context's current size, scene and step cap, after every earlier ring frame
// (synchronous: rare, between generations). Each slot's counters carry the epoch of the first new
// frame that will use it; each slot's first fetch order comes from the ring's cost keys of a frame
// of the same size (row-major without).
static int ring_setup(frm_ctx* ctx) {
  Ring& R = ctx->ring;
  int rc = ring_quiesce(ctx);
  if (rc) return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (!R.host) {
    FRM_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&R.host), sizeof(RingHost), hipHostMallocCoherent));
    memset(R.host, 0, sizeof(RingHost));
  }
  if (!R.dev) FRM_HIP(ctx, hipMalloc(&R.dev, sizeof(RingDev)));
  const uint32_t slots = ring_size(ctx);
  const size_t npix = (size_t)ctx->width * ctx->height;
  if (npix > R.cap || slots != R.slots) {
    ring_free_buffers(R);
    const size_t n = npix * slots;
    FRM_HIP(ctx, hipMalloc(&R.records, n * kRecordBytes));
    FRM_HIP(ctx, hipMalloc(&R.out, n * 4u));
    FRM_HIP(ctx, hipMalloc(&R.order, n * 4u));
    FRM_HIP(ctx, hipMalloc(&R.keys, n));
    FRM_HIP(ctx, hipMalloc(&R.iota, npix * 4u));
    FRM_HIP(ctx, hipMalloc(&R.keys_sorted, npix));
    R.sched_temp_bytes = schedule_temp_bytes((uint32_t)npix);
    FRM_HIP(ctx, hipMalloc(&R.sched_temp, R.sched_temp_bytes ? R.sched_temp_bytes : 16));
    R.cap = npix;
  }
  if (slots != R.slots) ring_free_images(R);
  R.slots = slots;
  // slot s's next frame: the first seq >= next_seq with (seq - 1) % R == s
  const uint32_t k0 = R.next_seq;
  RingDev* img = new (std::nothrow) RingDev();
  if (!img) return fail(ctx, FRM_ERR_OUT_OF_MEMORY, "host allocation failed");
  img->base = k0;
  memset(img->trace, 0xff, sizeof(img->trace));
  memset(img->grid_trace, 0xff, sizeof(img->grid_trace));
  for (auto& t : img->trace) t[2] = 0;  // max field
  // the counter sets of the first `slots` frames (the later ones are set up by the frame that
  // completes `slots` frames before them, ring_finish)
  for (uint32_t seq = k0; seq < k0 + slots; ++seq) {
    const unsigned long long ep = (unsigned long long)seq << 32;
    RingFrameCtl& c = img->set[(seq - 1u) & (2u * slots - 1u)];
    for (uint32_t x = 0; x <= kQueueParts; ++x) c.queue[x * (kQueuePartWords / 2u)] = ep;
    c.pix_done[0] = c.shade_next[0] = c.shade_done[0] = c.rank_next[0] = c.rank_done[0] = ep;
    const uint32_t s = (seq - 1u) & (slots - 1u);
    const uint32_t prev = seq > slots ? seq - slots : 0u;  // the slot's last frame: done (quiesced)
    img->done_seq[s][0] = prev;
    __atomic_store_n(&R.host->done[s][0], prev, __ATOMIC_RELAXED);
  }
  const hipError_t e = hipMemcpy(R.dev, img, sizeof(RingDev), hipMemcpyHostToDevice);
  delete img;
  if (e != hipSuccess) return hip_fail(ctx, e, "hipMemcpy(ring state)");
  const bool history = R.keys_valid && R.keys_w == ctx->width && R.keys_h == ctx->height;
  FRM_HIP(ctx, fill_iota(R.iota, (uint32_t)npix, ctx->stream));
  for (uint32_t s = 0; s < slots; ++s)
    FRM_HIP(ctx, schedule_pixels((uint32_t)npix, history, R.keys + s * npix, R.keys_sorted, R.iota, R.order + s * npix,
                                 R.sched_temp, R.sched_temp_bytes, ctx->stream));
  FRM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  R.keys_valid = true;  // every ring frame's shading writes them
  R.keys_w = ctx->width;
  R.keys_h = ctx->height;
  R.gen_valid = true;
  R.su = ctx->scene;
  R.w = ctx->width;
  R.h = ctx->height;
  R.max_steps = ctx->max_steps;
  R.aspect[0] = ctx->params.aspect_scale[0];
  R.aspect[1] = ctx->params.aspect_scale[1];
  return FRM_OK;
}

// A new grid for the ring, serving frames from `first` on (or from where its predecessor stopped).
static int ring_launch(frm_ctx* ctx, uint32_t first) {
  Ring& R = ctx->ring;
  const uint32_t id = R.grid_id + 1u;
  __atomic_store_n(&R.host->grid_stop[id % kRingGridIds][0], 0xFFFFFFFFu, __ATOMIC_SEQ_CST);
  FRM_HIP(ctx, hipMemsetAsync(&R.dev->grid, 0, sizeof(RingGridCtl), ctx->stream));
  KernelArgs a = make_args(ctx, ctx->params, ctx->scene, nullptr, ctx->counters, ctx->height, 0, 1, ctx->height);
  const size_t n = R.cap * R.slots;
  a.geom = reinterpret_cast<ShadeGeom*>(R.records);
  a.tails = reinterpret_cast<ShadeTail*>(R.records + n * sizeof(ShadeGeom));
  a.ring.host = R.host;
  a.ring.dev = R.dev;
  a.ring.slots = R.slots;
  a.ring.grid_id = id;
  a.ring.first_seq = first;
  a.ring.service_waves = R.service_waves;
  a.ring.out = R.out;
  a.ring.order = R.order;
  a.ring.keys = R.keys;
  FRM_HIP(ctx, launch_ring(a, ctx->cu_count, ctx->stream, nullptr));
  R.grid_id = id;
  return FRM_OK;
}

// The ring's pinned host image (slot s, parity par) for a frame of `bytes`: R.img[s][par].
static int ring_image(frm_ctx* ctx, uint32_t s, uint32_t par, size_t bytes) {
  Ring& R = ctx->ring;
  if (bytes > R.img_cap) {  // images of another size: none of them is pending (ring_setup drained)
    ring_free_images(R);
    R.img_cap = with_headroom(bytes);
  }
  if (!R.img[s][par])
    FRM_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&R.img[s][par]), R.img_cap, hipHostMallocCoherent));
  return FRM_OK;
}

// frm_render(ctx, NULL) through the ring: post the frame, launching a grid if none will take it.
int ring_render(frm_ctx* ctx) {
  Ring& R = ctx->ring;
  int rc = FRM_OK;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (!ring_same_gen(ctx) && (rc = ring_setup(ctx))) return rc;
  const uint32_t k = R.next_seq;
  const uint32_t s = (k - 1u) & (R.slots - 1u);
  if ((rc = ring_wait(ctx, s, k > R.slots ? k - R.slots : 0u))) return rc;  // the slot's last frame
  FrameUniforms fu;
  compute_frame_uniforms(ctx->params, ctx->width, ctx->height, ctx->max_steps, &fu);
  RingFrame& F = R.host->frames[s];
  memcpy(F.row, fu.row, sizeof(F.row));
  F.ox = fu.origin.x;
  F.oy = fu.origin.y;
  F.oz = fu.origin.z;
  F.mb_power = ctx->scene.mb_power;
  F.seq = k;
  uint32_t* img = nullptr;
  if (R.zero_copy) {
    const size_t bytes = (size_t)ctx->width * ctx->height * 4u;
    const uint32_t par = ((k - 1u) / R.slots) & 1u;
    if ((rc = ring_image(ctx, s, par, bytes))) return rc;
    img = R.img[s][par];
    R.img_seq[s][par] = k;
    R.img_ticket[s][par] = 0;  // its earlier frame's ticket expires
    R.img_bytes[s][par] = bytes;
  }
  F.host_img = img;
  __atomic_store_n(&R.host->posted, k, __ATOMIC_SEQ_CST);  // after the frame's data
  // the running grid takes the frame unless it has closed (then it may or may not have seen it: a
  // new grid starts where the closed one stopped)
  if (R.grid_id == 0 || __atomic_load_n(&R.host->closed, __ATOMIC_SEQ_CST) == R.grid_id)
    if ((rc = ring_launch(ctx, k))) return rc;
  R.next_seq = k + 1u;
  R.last_seq = k;
  ctx->last_is_ring = true;
  keep_render_params(ctx);
  return FRM_OK;
}

// The last frm_render was a ring frame: drain the ring and copy that frame into slot 0's framebuffer,
// so the single-frame paths (frm_read_frame, frm_present, their async forms) see it as before.
int ring_materialize(frm_ctx* ctx) {
  if (!ctx->last_is_ring) return FRM_OK;
  Ring& R = ctx->ring;
  int rc = ring_quiesce(ctx);
  if (rc) return rc;
  Slot& sl = ctx->slots[0];
  const size_t bytes = (size_t)ctx->width * ctx->height * 4u;
  if ((rc = select_fb(ctx, sl, sl.fb_idx)) || (rc = ensure_fb(ctx, sl, bytes))) return rc;
  const uint32_t s = (R.last_seq - 1u) & (R.slots - 1u);
  sl.no_second();
  FRM_HIP(ctx, hipMemcpyAsync(sl.fb(), R.out + (size_t)s * R.w * R.h, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  FRM_HIP(ctx, hipEventRecord(sl.done, ctx->stream));
  sl.pending = true;
  sl.last_stream = ctx->stream;
  sl.seq = ++ctx->launch_seq;
  show_slot(ctx, sl);
  return FRM_OK;
}

// frm_read_frame_async of a ring frame: a ticket for its zero-copy image. The frame before the first
// such call was posted without an image: it is waited for and copied once, and from then on every
// ring frame carries one.
int ring_read_async(frm_ctx* ctx, uint64_t* out_ticket) {
  Ring& R = ctx->ring;
  R.zero_copy = true;
  const uint32_t k = R.last_seq, s = (k - 1u) & (R.slots - 1u), par = ((k - 1u) / R.slots) & 1u;
  const size_t bytes = (size_t)R.w * R.h * 4u;
  if (!(R.img[s][par] && R.img_seq[s][par] == k)) {
    int rc = ring_quiesce(ctx);
    if (rc || (rc = ring_image(ctx, s, par, bytes))) return rc;
    FRM_HIP(ctx, hipMemcpy(R.img[s][par], R.out + (size_t)s * R.w * R.h, bytes, hipMemcpyDeviceToHost));
    R.img_seq[s][par] = k;
    R.img_bytes[s][par] = bytes;
  }
  R.img_ticket[s][par] = *out_ticket = ++ctx->ticket_seq;
  return FRM_OK;
}

// Drains the ring before anything that is not a ring frame uses the context.
int ring_leave(frm_ctx* ctx) {
  if (ctx->last_is_ring) return ring_materialize(ctx);
  return ring_quiesce(ctx);
}

// frm_frame_pixels of a ring frame's ticket: its zero-copy image, after waiting for the frame (its
// shading wrote the image); -1 when no ring image has this ticket.
int ring_ticket_pixels(frm_ctx* ctx, uint64_t ticket, const uint8_t** out_pixels, size_t* out_bytes) {
  Ring& R = ctx->ring;
  for (uint32_t s = 0; s < kRingSlots; ++s)
    for (uint32_t par = 0; par < 2; ++par)
      if (R.img_ticket[s][par] == ticket) {
        if (int rc = ring_wait(ctx, s, R.img_seq[s][par])) return rc;
        *out_pixels = reinterpret_cast<const uint8_t*>(R.img[s][par]);
        if (out_bytes) *out_bytes = R.img_bytes[s][par];
        return FRM_OK;
      }
  for (const Ring::Retired& r : R.retired)
    if (r.ticket == ticket) {
      if (int rc = ring_wait(ctx, r.slot, r.seq)) return rc;
      *out_pixels = reinterpret_cast<const uint8_t*>(r.img);
      if (out_bytes) *out_bytes = r.bytes;
      return FRM_OK;
    }
  return -1;
}

// FRM_RING_DEBUG: the ring's totals; FRM_RING_TRACE builds: the device timeline of the last frames (us from the first event shown)
static void ring_dump(const Ring& R) {
  fprintf(stderr, "frm ring: %u frames posted, %u grids launched, %u service waves\n", R.last_seq, R.grid_id,
          R.service_waves);
  RingDev* d = R.dev ? new (std::nothrow) RingDev() : nullptr;
  if (d && hipMemcpy(d, R.dev, sizeof(RingDev), hipMemcpyDeviceToHost) == hipSuccess && d->trace[1][1] &&
      d->trace[1][1] != ~0ull) {
    const uint32_t first = R.last_seq > 40u ? R.last_seq - 40u : 1u;
    const unsigned long long t0 = d->trace[first & 63u][0];
    for (uint32_t q = first; q <= R.last_seq; ++q) {
      const unsigned long long* t = d->trace[q & 63u];
      fprintf(stderr, "frm ring trace: frame %u seen %.1f claims %.1f..%.1f marched %.1f shaded %.1f done %.1f\n", q,
              (double)(long long)(t[0] - t0) / 100.0, (double)(long long)(t[1] - t0) / 100.0,
              (double)(long long)(t[2] - t0) / 100.0, (double)(long long)(t[3] - t0) / 100.0,
              (double)(long long)(t[4] - t0) / 100.0, (double)(long long)(t[5] - t0) / 100.0);
    }
    for (uint32_t id = R.grid_id > 30u ? R.grid_id - 30u : 1u; id <= R.grid_id; ++id)
      fprintf(stderr, "frm ring trace: grid %u start %.1f close %.1f\n", id,
              (double)(long long)(d->grid_trace[id & 63u][0] - t0) / 100.0,
              (double)(long long)(d->grid_trace[id & 63u][1] - t0) / 100.0);
  }
  delete d;
}

// Teardown (best effort): the ring's last frames, then everything it holds.
void ring_destroy(frm_ctx* ctx) {
  Ring& R = ctx->ring;
  if (R.grid_id) (void)ring_quiesce(ctx);
  if (getenv("FRM_RING_DEBUG")) ring_dump(R);
  ring_free_buffers(R);
  ring_free_images(R);
  for (const Ring::Retired& r : R.retired) (void)hipHostFree(r.img);
  R.retired.clear();
  if (R.dev) (void)hipFree(R.dev);
  if (R.host) (void)hipHostFree(R.host);
}
