// frm_launch.hip — what every render path of a context shares: the pool buffers that follow the
// frame size, slot framebuffers and streams, a launch's arguments, launch(), several frames in one
// launch (launch_frames), the steps of a frame.
#include "frm_ctx.h"

// Device memory of the context pool, allocated / released in the order of stream s: a block
// released on s is reused only by work ordered after everything enqueued on s before the release.
int dev_alloc(frm_ctx* ctx, void** p, size_t bytes, hipStream_t s) {
  FRM_HIP(ctx, hipMallocFromPoolAsync(p, bytes, ctx->pool, s));
  return FRM_OK;
}
int dev_release(frm_ctx* ctx, void* p, hipStream_t s) {
  if (p) FRM_HIP(ctx, hipFreeAsync(p, s));
  return FRM_OK;
}
// Makes b hold at least `bytes`: nothing when it already does (outside the first frame of a size,
// the steady state), else the old block is released and the new one allocated from owner's pool,
// both in the order of stream s. The caller has ordered the old block's last use before s.
int pool_grow(frm_ctx* owner, PoolBuf& b, size_t bytes, hipStream_t s) {
  if (b.cap >= bytes) return FRM_OK;
  if (int rc = dev_release(owner, b.p, s)) return rc;
  b = PoolBuf{};
  if (int rc = dev_alloc(owner, (void**)&b.p, bytes, s)) return rc;
  b.cap = bytes;
  return FRM_OK;
}
// The ShadeTail records of a slot's persistent-kernel scratch: after the ShadeGeom records of the
// capacity the block was allocated for (not of the current launch's need).
ShadeTail* record_tails(const PoolBuf& records) {
  return reinterpret_cast<ShadeTail*>(records.p + records.cap / kRecordBytes * sizeof(ShadeGeom));
}

// Slot sl's framebuffer for a frame of `bytes`, grown on the slot stream (renders and synchronous
// readback use it there; an asynchronous readback on the copy stream is awaited first: frm_render /
// frm_resize wait, select_fb).
int ensure_fb(frm_ctx* ctx, Slot& sl, size_t bytes) {
  return pool_grow(ctx, sl.fbs[sl.fb_idx], with_headroom(bytes), sl.stream);
}
// Makes fbs[i] the slot's current framebuffer, its last asynchronous readback ordered before
// everything enqueued on the slot stream from here on.
int select_fb(frm_ctx* ctx, Slot& sl, uint32_t i) {
  sl.fb_idx = i;
  if (sl.fb_read_pending[i]) {
    FRM_HIP(ctx, hipStreamWaitEvent(sl.stream, sl.fb_read[i], 0));
    sl.fb_read_pending[i] = false;
  }
  return FRM_OK;
}

// The resolved image that goes with the slot's current framebuffer, for an output frame of `bytes`,
// grown on the slot stream like the framebuffer (ensure_fb; select_fb has ordered its readers).
int ensure_res(frm_ctx* ctx, Slot& sl, size_t bytes) {
  return pool_grow(ctx, sl.res[sl.fb_idx], with_headroom(bytes), sl.stream);
}
// The scratch of the slot's adaptive pass for a frame of npix pixels, grown on the slot stream (the
// slot's last pass ran there).
static int ensure_refine(frm_ctx* ctx, Slot& sl, size_t npix) {
  if (!sl.refine_ctl)
    if (int rc = dev_alloc(ctx, (void**)&sl.refine_ctl, kRefineCtlBytes, sl.stream)) return rc;
  return pool_grow(ctx, sl.refine_list, npix * sizeof(uint32_t), sl.stream);
}
// The slot's motion-blur scratch for chunks of src_bytes of sub-frames and, for a frame of several
// chunks, acc_bytes of sums (0: none), grown on the slot stream (the slot's last shutter frame ran there).
int ensure_shutter(frm_ctx* ctx, Slot& sl, size_t src_bytes, size_t acc_bytes) {
  if (int rc = pool_grow(ctx, sl.shutter_src, src_bytes, sl.stream)) return rc;
  return pool_grow(ctx, sl.shutter_acc, acc_bytes, sl.stream);
}
// Releases the host copies of uploaded tables whose copy has completed (wait: all of them, each
// waited for: frm_destroy).
void release_host_blocks(frm_ctx* ctx, bool wait) {
  size_t kept = 0;
  for (frm_ctx::HostBlock& b : ctx->host_blocks) {
    if (wait) (void)hipEventSynchronize(b.copied);
    if (wait || hipEventQuery(b.copied) == hipSuccess) {
      (void)hipEventDestroy(b.copied);
      free(b.p);
    } else {
      ctx->host_blocks[kept++] = b;
    }
  }
  ctx->host_blocks.resize(kept);
}
// The direction tables of a w x h panorama (equirect_tables: 2*w + 2*h floats) copied to dev in
// the order of stream s. The host copy lives until an event recorded after the transfer has
// completed, whether or not the runtime stages the transfer before it returns.
int upload_tables(frm_ctx* ctx, float* dev, uint32_t w, uint32_t h, hipStream_t s) {
  release_host_blocks(ctx, false);
  const size_t bytes = (2u * (size_t)w + 2u * (size_t)h) * sizeof(float);
  frm_ctx::HostBlock b{(float*)malloc(bytes), nullptr};
  if (!b.p) return fail(ctx, FRM_ERR_OUT_OF_MEMORY, "host allocation failed");
  equirect_tables(w, h, b.p);
  hipError_t e = hipEventCreateWithFlags(&b.copied, hipEventDisableTiming);
  if (e != hipSuccess) {
    free(b.p);
    return hip_fail(ctx, e, "hipEventCreateWithFlags");
  }
  ctx->host_blocks.push_back(b);  // released only after the event, also when a call below fails
  e = hipMemcpyAsync(dev, b.p, bytes, hipMemcpyHostToDevice, s);
  const hipError_t e2 = hipEventRecord(b.copied, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "hipMemcpyAsync");
  if (e2 != hipSuccess) return hip_fail(ctx, e2, "hipEventRecord");
  return FRM_OK;
}
// The slot's panorama scratch for six faces of src_bytes in all and the tables of a w x h output,
// grown (and the tables uploaded, when the output size is new to the slot) on the slot stream: the
// slot's last panorama ran there.
int ensure_panorama(frm_ctx* ctx, Slot& sl, size_t src_bytes, uint32_t w, uint32_t h) {
  if (int rc = pool_grow(ctx, sl.pano_src, src_bytes, sl.stream)) return rc;
  if (sl.pano_w == w && sl.pano_h == h) return FRM_OK;
  sl.pano_w = sl.pano_h = 0;
  if (int rc = pool_grow(ctx, sl.pano_tables, (2u * (size_t)w + 2u * (size_t)h) * sizeof(float), sl.stream)) return rc;
  if (int rc = upload_tables(ctx, (float*)sl.pano_tables.p, w, h, sl.stream)) return rc;
  sl.pano_w = w;
  sl.pano_h = h;
  return FRM_OK;
}
// The second image of the slot's current framebuffer, on the slot stream, after the frame is
// complete there: the box resolve of a supersampled context, the adaptive frame of an adaptive
// one (the edge pass over the frame, then the samples of its refined pixels; their work is added
// to the context's counters), or the gathered frame of a depth-of-field one (the depth plane of the
// slot's records, then the gather; kernel_for has put the frame on the persistent kernel, whose
// launch wrote the records of this slot). The slot's `done` event is recorded again, so that it
// covers it.
int resolve_frame(frm_ctx* ctx, Slot& sl) {
  sl.no_second();
  const FrameMode mode = frame_mode(ctx);
  if (mode == kPlain || mode == kPanorama) return FRM_OK;  // (a panorama is projected into the framebuffer)
  if (int rc = ensure_res(ctx, sl, (size_t)ctx->out_width * ctx->out_height * 4u)) return rc;
  uint8_t* res = sl.res[sl.fb_idx].p;
  if (mode == kDof) {  // (the render size is the output size)
    const size_t npix = (size_t)ctx->width * ctx->height;
    if (!sl.records.p || sl.records.cap < npix * kRecordBytes)
      return fail(ctx, FRM_ERR_HIP, "depth of field: the frame left no records in its slot");
    sl.depth_w = sl.depth_h = 0;
    if (int rc = pool_grow(ctx, sl.depth, npix * sizeof(float), sl.stream)) return rc;
    FRM_HIP(ctx, launch_depth(reinterpret_cast<const ShadeGeom*>(sl.records.p), record_tails(sl.records),
                              (float*)sl.depth.p, (uint32_t)npix, sl.stream));
    FRM_HIP(ctx, launch_dof(sl.fb(), (const float*)sl.depth.p, res, ctx->width, ctx->height, ctx->dof_aperture,
                            ctx->dof_focus, ctx->dof_radius, sl.stream));
    sl.depth_w = ctx->width;
    sl.depth_h = ctx->height;
  } else if (mode == kAdaptive) {  // (the render size is the output size)
    if (int rc = ensure_refine(ctx, sl, (size_t)ctx->width * ctx->height)) return rc;
    FrameUniforms f;
    compute_frame_uniforms(ctx->params, ctx->adaptive * ctx->width, ctx->adaptive * ctx->height, ctx->max_steps, &f);
    FRM_HIP(ctx, launch_adaptive(f, ctx->scene, sl.fb(), res, ctx->width, ctx->height, ctx->adaptive,
                                 ctx->edge_threshold, (uint32_t*)sl.refine_list.p, sl.refine_ctl, ctx->counters,
                                 ctx->cu_count, sl.stream));
    sl.refine_w = ctx->width;
    sl.refine_h = ctx->height;
  } else {
    FRM_HIP(ctx, launch_resolve(sl.fb(), res, ctx->out_width, ctx->out_height, ctx->supersample, sl.stream));
  }
  sl.second[sl.fb_idx] = mode;
  FRM_HIP(ctx, hipEventRecord(sl.done, sl.stream));
  return FRM_OK;
}
// What the presentation paths read of a slot: out_width x out_height texels. Supersampling is the
// context's, not the slot's: apply_size sizes the resolved image before the first render.
const uint8_t* shown(const frm_ctx* ctx, const Slot& sl) {
  return ctx->supersample > 1u || sl.second[sl.fb_idx] != kPlain ? sl.res[sl.fb_idx].p : sl.fb();
}

// Bands of a frame of height >= 1 rows: ceil(height / band_rows), without the sum height + band_rows
// - 1, which wraps for band_rows near 2^32 (one band would count as none).
uint32_t num_bands(uint32_t height, uint32_t band_rows) { return (height - 1u) / band_rows + 1u; }

// Rows produced by bands first, first+stride, ... below num_bands (the last band of the
// frame may be short, but a band buffer always reserves band_rows rows for it). In 64 bits: the
// count is below height + band_rows, which 32 bits need not hold.
uint64_t band_local_rows(uint32_t height, uint32_t band_rows, uint32_t first, uint32_t stride) {
  uint32_t nb = num_bands(height, band_rows);
  if (first >= nb) return 0;
  uint32_t count = (nb - 1 - first) / stride + 1;
  return (uint64_t)count * band_rows;
}
// band_local_rows as the 32 bits a launch and *out_rows hold: refused, *rows left alone, when it
// does not fit (only a height above FRM_MAX_DIMENSION can get there: a context's rows always fit).
int band_rows_u32(frm_ctx* ctx, uint32_t height, uint32_t band_rows, uint32_t first, uint32_t stride, uint32_t* rows) {
  const uint64_t r = band_local_rows(height, band_rows, first, stride);
  if (r > 0xFFFFFFFFull)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "bands of %u rows of a frame of %u rows: %llu rows do not fit 32 bits",
                band_rows, height, (unsigned long long)r);
  *rows = (uint32_t)r;
  return FRM_OK;
}

// Local rows that hold frame rows: all but the missing rows of a short last band, which
// can only be this launch's last band (its local rows are then a prefix).
static uint32_t band_valid_rows(uint32_t height, const BandGeometry& g) {
  if (g.local_rows == 0) return 0;
  const uint32_t last = g.first_band + (g.local_rows / g.band_rows - 1u) * g.band_stride;
  const uint32_t end = (last + 1u) * g.band_rows;  // one past its last global row
  return end > height ? g.local_rows - (end - height) : g.local_rows;
}

// Band height of a group's row split: the smallest height >= 16 that splits the frame into a
// multiple of n bands (else 16), so interleaved bands balance the devices (frm/tiling.py).
uint32_t group_band_rows(uint32_t height, uint32_t n) {
  for (uint32_t br = 16; br <= height; ++br)
    if (height % br == 0 && (height / br) % n == 0) return br;
  return 16;
}

// A launch of the context's frame size with the given parameters and their scene uniforms.
KernelArgs make_args(const frm_ctx* ctx, const frm_parameters& params, const SceneUniforms& scene, uint8_t* dst,
                     unsigned long long* counters, uint32_t band_rows, uint32_t first, uint32_t stride,
                     uint32_t local_rows) {
  KernelArgs a;
  memset(&a, 0, sizeof(a));
  compute_frame_uniforms(params, ctx->width, ctx->height, ctx->max_steps, &a.f);
  a.s = scene;
  a.g.band_rows = band_rows;
  a.g.first_band = first;
  a.g.band_stride = stride;
  a.g.local_rows = local_rows;
  a.out = (uint32_t*)dst;
  a.counters = counters;
  a.npix = band_valid_rows(ctx->height, a.g) * ctx->width;
  a.service_min = ctx->service_min;
  a.batch = 1;
  a.rec_stride = local_rows * ctx->width;
  a.out_stride = local_rows * ctx->width;
  memcpy(a.cams[0].row, a.f.row, sizeof(a.f.row));  // a single frame is a batch of one
  a.cams[0].origin = a.f.origin;
  return a;
}

KernelKind kernel_for(const frm_ctx* ctx, uint64_t pixels) {
  if (ctx->flags & FRM_FLAG_SIMPLE_KERNEL) return kKernelSimple;
  if (ctx->flags & FRM_FLAG_PERSISTENT_KERNEL) return kKernelPersistent;
  if (frame_mode(ctx) == kDof) return kKernelPersistent;  // the depth plane comes from its records (same bytes)
  return pixels < kSimplePixelsPerCu * (uint64_t)ctx->cu_count ? kKernelSimple : kKernelPersistent;
}

// Waits (host) until the slot's last launch has completed.
int wait_slot(frm_ctx* ctx, Slot& sl) {
  if (sl.pending) {
    FRM_HIP(ctx, hipEventSynchronize(sl.done));
    sl.pending = false;
  }
  return FRM_OK;
}

int synchronize_all(frm_ctx* ctx) {
  for (uint32_t i = 0; i < ctx->nslots; ++i) {
    Slot& sl = ctx->slots[i];
    if (sl.stream) FRM_HIP(ctx, hipStreamSynchronize(sl.stream));
    int rc = wait_slot(ctx, sl);
    if (rc) return rc;
  }
  return FRM_OK;
}

// The stream frm_render uses for slot i (created on first use: a context with one frame in
// flight never creates more than the context stream).
// Slots > 0 need a hardware queue of their own to overlap: HIP maps streams onto at most
// GPU_MAX_HW_QUEUES queues per process (4 by default) and hands the least-used one out again,
// and two frames whose streams share a queue never overlap. Plain
// non-blocking streams get distinct queues while the pool has room (bench.py raises the limit to
// 16); FRM_SLOT_STREAMS=cumask asks for CU-masked streams, which the runtime never pools.
static hipStream_t own_queue_stream(int device) {
  hipDeviceProp_t prop;
  // default: a pooled non-blocking stream. "cumask": a CU-masked stream, which gets a hardware queue
  // of its own but is a BLOCKING stream (hipExtStreamCreateWithCUMask takes no flags): it
  // synchronises with the legacy null stream (torch's default stream, synchronous hipMemcpy), so
  // it is opt-in for hosts that never use that stream
  const char* kind = getenv("FRM_SLOT_STREAMS");
  const bool cumask = kind && strcmp(kind, "cumask") == 0;
  if (cumask && hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) {
    const uint32_t words = (uint32_t)(prop.multiProcessorCount + 31) / 32u;
    uint32_t mask[64];
    if (words <= 64u) {
      for (uint32_t w = 0; w < words; ++w) mask[w] = 0xFFFFFFFFu;
      hipStream_t s = nullptr;
      if (hipExtStreamCreateWithCUMask(&s, words, mask) == hipSuccess) return s;
    }
  }
  hipStream_t s = nullptr;
  return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? s : nullptr;
}

int slot_stream(frm_ctx* ctx, uint32_t i, hipStream_t* out) {
  Slot& sl = ctx->slots[i];
  if (!sl.stream && !(sl.stream = own_queue_stream(ctx->device)))
    return fail(ctx, FRM_ERR_HIP, "stream creation failed for render slot %u", i);
  *out = sl.stream;
  return FRM_OK;
}

// The fetch order of persistent launch `a` (stream s, slot si's scratch) and its scheduling history.
static int schedule_launch(frm_ctx* ctx, uint32_t si, KernelArgs& a, hipStream_t s) {
  Slot& sl = ctx->slots[si];
  // pixel scheduling: fetch this launch's pixels by the cost the slot recorded last time
  // for the same geometry (most expensive first)
  const uint32_t npix = a.npix;
  const uint64_t key = ((uint64_t)a.f.width << 40) ^ ((uint64_t)a.g.local_rows << 20) ^
                       ((uint64_t)a.g.band_rows << 8) ^ ((uint64_t)a.g.first_band << 4) ^ a.g.band_stride ^
                       ((uint64_t)a.f.height << 52);
  // a whole frame (not a rank's bands): its keys can seed a resized whole frame's order
  const bool whole = a.g.first_band == 0 && a.g.band_stride == 1 && npix == a.f.width * a.f.height;
  const bool same = sl.sched_history && key == sl.sched_key;
  const bool rescale = !same && sl.sched_history && sl.sched_whole && whole;
  // a slot without history of this geometry takes another slot's keys: with frames in
  // flight, every slot's first launch would otherwise fetch in row-major order
  int donor = -1;
  if (!same && !rescale)
    for (uint32_t j = 0; j < ctx->nslots && donor < 0; ++j) {
      const Slot& o = ctx->slots[j];
      if (j != si && o.sched_history && o.sched_key == key && o.sched_cap >= npix) donor = (int)j;
    }
  if (npix > sl.sched_cap) {
    // stream-ordered like the records; a donor's copy of these keys was awaited above
    uint8_t* old_keys = sl.sched_keys;  // kept until a resize has resampled it
    int rc = FRM_OK;
    for (void* b : {(void*)sl.sched_iota, (void*)sl.sched_order, sl.sched_temp})
      if ((rc = dev_release(ctx, b, s))) return rc;
    if (!rescale && (rc = dev_release(ctx, old_keys, s))) return rc;
    sl.sched_iota = sl.sched_order = nullptr;
    sl.sched_keys = nullptr;
    sl.sched_temp = nullptr;
    sl.sched_cap = 0;
    sl.sched_temp_bytes = schedule_temp_bytes(npix);
    if ((rc = dev_alloc(ctx, (void**)&sl.sched_iota, (size_t)npix * sizeof(uint32_t), s)) ||
        (rc = dev_alloc(ctx, (void**)&sl.sched_order, (size_t)npix * sizeof(uint32_t), s)) ||
        (rc = dev_alloc(ctx, (void**)&sl.sched_keys, (size_t)npix * 2, s)) ||
        (rc = dev_alloc(ctx, &sl.sched_temp, sl.sched_temp_bytes ? sl.sched_temp_bytes : 16, s)))
      return rc;
    FRM_HIP(ctx, fill_iota(sl.sched_iota, npix, s));
    sl.sched_cap = npix;
    if (rescale) {
      FRM_HIP(ctx, rescale_keys(old_keys, sl.sched_w, sl.sched_h, sl.sched_keys, a.f.width, a.f.height, s));
      if ((rc = dev_release(ctx, old_keys, s))) return rc;  // after the resample reads it
    }
  } else if (rescale) {
    // resample into the sort's output half, then back (the map is read and written)
    uint8_t* tmp = sl.sched_keys + sl.sched_cap;
    FRM_HIP(ctx, rescale_keys(sl.sched_keys, sl.sched_w, sl.sched_h, tmp, a.f.width, a.f.height, s));
    FRM_HIP(ctx, hipMemcpyAsync(sl.sched_keys, tmp, npix, hipMemcpyDeviceToDevice, s));
  }
  if (donor >= 0) {  // keys order fetches only, never a pixel's bytes
    Slot& dn = ctx->slots[donor];
    if (dn.pending && dn.last_stream != s) FRM_HIP(ctx, hipStreamWaitEvent(s, dn.done, 0));
    // an earlier reader's copy on another stream: order this copy after it, so the one
    // keys_read event recorded below covers every copy the donor's next launch must await
    if (dn.keys_reader && dn.keys_reader != s) FRM_HIP(ctx, hipStreamWaitEvent(s, dn.keys_read, 0));
    FRM_HIP(ctx, hipMemcpyAsync(sl.sched_keys, dn.sched_keys, npix, hipMemcpyDeviceToDevice, s));
    FRM_HIP(ctx, hipEventRecord(dn.keys_read, s));  // the donor's next launch waits for this copy
    dn.keys_reader = s;
  }
  // the steady state: the slot's last launch (same geometry) has already ranked its pixels and
  // reset this launch's counters in its shading pass, so nothing runs between the two launches
  const bool fused = same && sl.order_ready && sl.order_key == key;
  uint32_t* half = sl.rank_words + sl.rank_half * kRankWords;
  if (!fused) {
    const bool history = same || rescale || donor >= 0;
    FRM_HIP(ctx, schedule_pixels(npix, history, sl.sched_keys, sl.sched_keys + sl.sched_cap,
                                 sl.sched_iota, sl.sched_order, sl.sched_temp, sl.sched_temp_bytes, s));
    FRM_HIP(ctx, hipMemsetAsync(sl.queue, 0, kQueueDebugWord * sizeof(unsigned int), s));
    FRM_HIP(ctx, hipMemsetAsync(half, 0, kRankWords * sizeof(uint32_t), s));
  }
  // runtime-reloaded kernels may not rank (edited sources): the next launch sorts again
  const bool rank = ctx->reloaded == nullptr && ctx->fused_sched;
  a.key_hist = rank ? half : nullptr;
  a.key_hist_next = sl.rank_words + (sl.rank_half ^ 1u) * kRankWords;
  a.order_out = sl.sched_order;
  sl.order_ready = false;  // set by launch() once the launch is enqueued
  sl.order_key = key;
  a.pixel_order = sl.sched_order;
  a.pixel_key = sl.sched_keys;
  sl.sched_key = key;
  sl.sched_history = true;
  sl.sched_whole = whole;
  sl.sched_w = a.f.width;
  sl.sched_h = a.f.height;
  sl.sched_npix = npix;
  return FRM_OK;
}

static int inflight_blocks_per_cu(uint32_t frames_in_flight) {
  return frames_in_flight <= 2u ? kInflightBlocksPerCu : (int)(2u * kInflightBlocksPerCu / frames_in_flight);
}

// Enqueues one render launch on stream s with the scratch of the context's next slot.
// Stream order covers a slot reused on the same stream; a slot last used on another
// stream is awaited on the device (hipStreamWaitEvent), so callers may rotate streams.
int launch(frm_ctx* ctx, KernelArgs a, hipStream_t s) {
  if (a.g.local_rows == 0) return FRM_OK;
  const uint32_t si = ctx->next_slot;
  Slot& sl = ctx->slots[si];
  if (sl.pending && sl.last_stream != s) FRM_HIP(ctx, hipStreamWaitEvent(s, sl.done, 0));
  if (sl.keys_reader) {  // another slot's launch read this slot's keys: they are rewritten below
    if (sl.keys_reader != s) FRM_HIP(ctx, hipStreamWaitEvent(s, sl.keys_read, 0));
    sl.keys_reader = nullptr;
  }
  const KernelKind kind = kernel_for(ctx, a.npix);
  a.queue = sl.queue;
  if (kind == kKernelPersistent) {
    // grows outside the steady state (first frame of a size); stream-ordered: s runs after the
    // slot's last launch (awaited above when on another stream)
    const size_t need = (size_t)a.g.local_rows * a.f.width * a.batch;
    if (int rc = pool_grow(ctx, sl.records, need * kRecordBytes, s)) return rc;
    a.geom = reinterpret_cast<ShadeGeom*>(sl.records.p);
    a.tails = record_tails(sl.records);
    if (int rc = schedule_launch(ctx, si, a, s)) return rc;
    unsigned int* dbg = sl.queue + kQueueDebugWord;
    a.debug = (unsigned long long*)dbg;  // the diagnostic words after the partition counters
#ifdef FRM_STAMPS
    FRM_HIP(ctx, hipMemsetAsync(dbg, 0, 16, s));
    FRM_HIP(ctx, hipMemsetAsync(dbg + 4, 0xff, 16, s));  // atomicMin slots
    FRM_HIP(ctx, hipMemsetAsync(dbg + 8, 0, 8, s));
#endif
  }
  if (kind != kKernelPersistent) sl.order_ready = false;
  // Single-frame persistent launches with frames in flight run a grid of 4 waves per SIMD (16
  // one-wave workgroups per CU) instead of the occupancy limit (8 for the Mandelbulb): two frames'
  // grids then share the GPU, each frame's shading and ranking find room beside the next frame's
  // grid, and one frame's tail runs beside the other's bulk. Measured (profiles/round5/dropin_bpc):
  // the drop-in loop 9.11-9.18 -> 8.57-8.60 ms (fixed pose), 10.08-10.13 -> 9.29-9.32 (HEADLINE_FLY);
  // multi-frame launches (one queue for all their frames) keep the full grid (8-way rank share
  // 1.098 ms/frame full, 1.117 at 12).
  int blocks_cap = 0;
  if (a.batch == 1) {
    if (ctx->nslots >= 2 && a.npix <= kInflightCapPixels)
      blocks_cap = inflight_blocks_per_cu(ctx->nslots);
    else if (ctx->nslots == 1)
      blocks_cap = kLoneFrameBlocksPerCu;
  }
  FRM_HIP(ctx, launch_render(a, kind, ctx->cu_count, s, ctx->reloaded, blocks_cap));
  if (a.key_hist) {
    sl.order_ready = true;
    sl.rank_half ^= 1u;
  }
  FRM_HIP(ctx, hipEventRecord(sl.done, s));
  sl.seq = ++ctx->launch_seq;
  sl.pending = true;
  sl.last_stream = s;
  ctx->next_slot = (si + 1u) % ctx->nslots;
  return FRM_OK;
}

// ---- several frames of the context's size, one launch if possible ------------------------------
// (frm_render_bands_batch's frames, a chunk of frm_render_shutter's sub-frames, a panorama's faces)

void batch_uniforms(const frm_ctx* ctx, uint32_t count, const frm_parameters* params, BatchUniforms* u) {
  compute_scene_uniforms(params[0], ctx->flags, &u->s0);
  u->anim = false;
  u->differs = 0;
  u->powers[0] = u->s0.mb_power;
  for (uint32_t k = 1; k < count && !u->differs; ++k) {
    SceneUniforms sk;
    compute_scene_uniforms(params[k], ctx->flags, &sk);
    u->powers[k] = sk.mb_power;
    if (is_mandelbulb(u->s0.family) && sk.family == u->s0.family && sk.mb_power != u->s0.mb_power) {
      u->anim = true;
      sk.mb_power = u->s0.mb_power;
      sk.mb_power_m1 = u->s0.mb_power_m1;
    }
    if (memcmp(&u->s0, &sk, sizeof(sk)) != 0) u->differs = k;
  }
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
// Renders the `count` frames of params (u: their batch_uniforms) on stream s, bands g of frame k at
// dst + k * frame_stride_bytes: in one launch when the frames differ in no more than a launch can
// carry and the kernel can share (batch_shares_launch), else one launch per frame, each with its own
// scene uniforms (scene_per_frame) or all with frame 0's (frames that differ in their cameras
// alone). pin_slot >= 0: every launch runs on that slot (launch() takes the context's next one and
// moves on: a frame of several launches stays on its slot).
int launch_frames(frm_ctx* ctx, uint32_t count, const frm_parameters* params, const BatchUniforms& u,
                  bool scene_per_frame, uint8_t* dst, size_t frame_stride_bytes, const BandGeometry& g,
                  unsigned long long* counters, hipStream_t s, int pin_slot) {
  KernelArgs a = make_args(ctx, params[0], u.s0, dst, counters, g.band_rows, g.first_band, g.band_stride, g.local_rows);
  const bool shared = !u.differs && batch_shares_launch(ctx, a, count, u.anim);
  if (shared) set_batch(ctx, a, count, params, u.powers, u.anim, frame_stride_bytes);
  for (uint32_t k = 0; k < (shared ? 1u : count); ++k) {
    if (!shared) {
      SceneUniforms sk = u.s0;
      if (scene_per_frame) compute_scene_uniforms(params[k], ctx->flags, &sk);
      a = make_args(ctx, params[k], sk, dst + (size_t)k * frame_stride_bytes, counters, g.band_rows, g.first_band,
                    g.band_stride, g.local_rows);
    }
    if (pin_slot >= 0) ctx->next_slot = (uint32_t)pin_slot;
    if (int rc = launch(ctx, a, s)) return rc;
  }
  return FRM_OK;
}

// ---- the steps of a frame (frm_render, group_render; the ring writes the last two) ----------

// Before a frame outside the ring, on the context's device: the ring's frames first, and for a frame
// with stats every slot drained (the counters must hold this frame alone).
int frame_prologue(frm_ctx* ctx, const frm_stats* stats) {
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_quiesce(ctx)) return rc;
  ctx->last_is_ring = false;
  return stats ? synchronize_all(ctx) : FRM_OK;
}

// Claims the context's next slot for a frame of the context's size: its stream, and the other
// framebuffer of the slot: the last one may still be read back (copy stream); this one's readback
// (two renders of the slot ago) is awaited on the slot stream, long done.
int begin_frame(frm_ctx* ctx, Slot** out_slot, hipStream_t* out_stream) {
  const uint32_t si = ctx->next_slot;
  Slot& sl = ctx->slots[si];
  *out_slot = &sl;
  if (int rc = slot_stream(ctx, si, out_stream)) return rc;
  if (int rc = select_fb(ctx, sl, sl.fb_idx ^ 1u)) return rc;
  return ensure_fb(ctx, sl, (size_t)ctx->width * ctx->height * 4u);
}

// A frame with stats, on stream s (the caller has drained the context: the counters must hold this
// frame alone). Before its launches: the counters zeroed and ev_start. After them: ev_stop, then
// (the host waits for s) the context's counters of the frame and its time on the device.
int stats_begin(frm_ctx* ctx, hipStream_t s) {
  FRM_HIP(ctx, hipMemsetAsync(ctx->counters, 0, FRM_NUM_COUNTERS * sizeof(unsigned long long), s));
  FRM_HIP(ctx, hipEventRecord(ctx->ev_start, s));
  return FRM_OK;
}
int stats_end(frm_ctx* ctx, hipStream_t s, uint64_t* out_counters, float* out_ms) {
  FRM_HIP(ctx, hipEventRecord(ctx->ev_stop, s));
  FRM_HIP(ctx, hipMemcpyAsync(out_counters, ctx->counters, FRM_NUM_COUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  FRM_HIP(ctx, hipStreamSynchronize(s));
  FRM_HIP(ctx, hipEventElapsedTime(out_ms, ctx->ev_start, ctx->ev_stop));
  return FRM_OK;
}
// The end of a single-device frame: nothing without stats, else stats_end into *stats.
int finish_stats(frm_ctx* ctx, hipStream_t s, frm_stats* stats) {
  if (!stats) return FRM_OK;
  uint64_t host[FRM_NUM_COUNTERS];
  float ms = 0.0f;
  int rc = stats_end(ctx, s, host, &ms);
  if (rc || (rc = frm_stats_from_counters(ctx, host, stats))) return rc;
  stats->kernel_ms = ms;
  return FRM_OK;
}

// The frame the presentation paths (frm_read_frame, frm_present, their async forms) see from here
// on: slot sl's last launch.
void show_slot(frm_ctx* ctx, const Slot& sl) {
  ctx->last_slot = (uint32_t)(&sl - ctx->slots);
  ctx->render_seq = sl.seq;
  ctx->last_is_ring = false;
}
// The parameters of the frame just rendered or posted, which frm_debug_trace replays.
void keep_render_params(frm_ctx* ctx) {
  ctx->render_params = ctx->params;
  ctx->render_scene = ctx->scene;
}
