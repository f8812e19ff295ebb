// frm_group.hip — group contexts (frm_config.device_count): one context row-tiles every frame over
// a device list and gathers the bands on devices[0]. Creation, the frame, synchronisation, teardown.
#include "frm_ctx.h"

// Makes the context on devices[0] a group: one band-rendering context per further device, the
// RCCL communicator over them (ncclCommInitAll: one process, one rank per device) when the
// devices are distinct, and the per-slot gather events (a failure leaves the rest to frm_destroy).
int group_init(frm_ctx* ctx, const frm_config* config) {
  const uint32_t n = config->device_count;
  Group* G = new (std::nothrow) Group();
  if (!G) return fail(ctx, FRM_ERR_OUT_OF_MEMORY, "host allocation failed");
  ctx->group = G;
  G->n = n;
  bool distinct = true;
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t q = 0; q < r; ++q) distinct = distinct && config->devices[q] != config->devices[r];
  const char* gather = getenv("FRM_GATHER");  // experiments: "copy" = device-to-device copies
  G->rccl = n > 1 && distinct && !(gather && strcmp(gather, "copy") == 0);
  for (uint32_t r = 1; r < n; ++r) {
    if (int rc = create_one(config, config->devices[r], &G->sub[r])) {
      // the member's message (create_one left it as the thread's last error) onto the group
      // context, whose error the caller reports
      const std::string why = frm_last_error(nullptr);
      return fail(ctx, rc, "devices[%u] = %d: %s", r, config->devices[r], why.c_str());
    }
    G->sub[r]->bands_only = true;
  }
  for (uint32_t r = 0; r < n; ++r) {
    FRM_HIP(ctx, hipSetDevice(config->devices[r]));
    FRM_HIP(ctx, hipEventCreateWithFlags(&G->comm_done[r], hipEventDisableTiming));
    for (uint32_t i = 0; i < ctx->nslots; ++i) {
      GroupSlot& gs = G->slots[i];
      if (r == 0) {
        FRM_HIP(ctx, hipEventCreateWithFlags(&gs.copied, hipEventDisableTiming));
      } else {
        FRM_HIP(ctx, hipEventCreateWithFlags(&gs.sent[r], hipEventDisableTiming));
        FRM_HIP(ctx, hipEventCreateWithFlags(&gs.rendered[r], hipEventDisableTiming));
      }
    }
  }
  if (G->rccl) {
    int devs[FRM_MAX_DEVICES];
    for (uint32_t r = 0; r < n; ++r) devs[r] = config->devices[r];
    const ncclResult_t nr = ncclCommInitAll(G->comm, (int)n, devs);
    if (nr != ncclSuccess) {
      for (uint32_t r = 0; r < n; ++r) G->comm[r] = nullptr;
      return fail(ctx, FRM_ERR_HIP, "ncclCommInitAll over %u devices failed: %s", n, ncclGetErrorString(nr));
    }
  }
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  return FRM_OK;
}

// Teardown of a group: the members first (best effort, statuses ignored).
void group_destroy(frm_ctx* ctx) {
  Group* G = ctx->group;
  if (!G) return;
  for (uint32_t r = 1; r < G->n; ++r) {
    frm_ctx* c = G->sub[r];
    if (!c) continue;
    (void)hipSetDevice(c->device);
    (void)synchronize_all(c);
    for (uint32_t i = 0; i < FRM_MAX_FRAMES_IN_FLIGHT; ++i) {
      GroupSlot& gs = G->slots[i];
      if (gs.bands[r].p && c->stream) (void)hipFreeAsync(gs.bands[r].p, c->stream);
      for (hipEvent_t ev : {gs.sent[r], gs.rendered[r]})
        if (ev) (void)hipEventDestroy(ev);
    }
    if (G->comm_done[r]) (void)hipEventDestroy(G->comm_done[r]);
    if (G->comm[r]) (void)ncclCommDestroy(G->comm[r]);
    frm_destroy(c);
  }
  (void)hipSetDevice(ctx->device);
  (void)synchronize_all(ctx);
  for (uint32_t i = 0; i < FRM_MAX_FRAMES_IN_FLIGHT; ++i) {
    GroupSlot& gs = G->slots[i];
    if (gs.gathered.p && ctx->stream) (void)hipFreeAsync(gs.gathered.p, ctx->stream);
    if (gs.copied) (void)hipEventDestroy(gs.copied);
  }
  if (G->comm_done[0]) (void)hipEventDestroy(G->comm_done[0]);
  if (G->comm[0]) (void)ncclCommDestroy(G->comm[0]);
  delete G;
  ctx->group = nullptr;
}

// One frame of a group context: every device renders its interleaved bands on the stream of its
// next frame slot (frames in flight overlap as on one device), the bands meet on device 0 (RCCL
// grouped send/receive over xGMI, or device-to-device copies for a repeated device), and device 0
// reassembles the frame into the slot's framebuffer on the same stream; the slot's `done` event
// then covers the whole frame for frm_read_frame / frm_present and their async forms.
int group_render(frm_ctx* ctx, frm_stats* stats) {
  Group& G = *ctx->group;
  const uint32_t n = G.n;
  int rc = FRM_OK;
  if (stats)  // the counters must hold this frame alone
    for (uint32_t r = 0; r < n; ++r) {
      frm_ctx* c = member(ctx, r);
      FRM_HIP(ctx, hipSetDevice(c->device));
      if ((rc = synchronize_all(c))) return relay(ctx, c, rc);
    }
  GroupSlot& gs = G.slots[ctx->next_slot];
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  Slot* slot = nullptr;
  hipStream_t st[FRM_MAX_DEVICES];
  if ((rc = begin_frame(ctx, &slot, &st[0]))) return rc;
  Slot& sl = *slot;
  const hipStream_t s0 = st[0];
  // the gather buffer's last use (this slot's last frame) is ordered before, on s0
  if ((rc = pool_grow(ctx, gs.gathered, (size_t)n * G.stride, s0))) return rc;
  if (stats && (rc = stats_begin(ctx, s0))) return rc;
  uint32_t rows[FRM_MAX_DEVICES];
  for (uint32_t r = 0; r < n; ++r) rows[r] = (uint32_t)band_local_rows(ctx->height, G.band_rows, r, n);  // below height + band_rows
  // ranks 1..n-1 on their devices
  for (uint32_t r = 1; r < n; ++r) {
    frm_ctx* c = G.sub[r];
    if (rows[r] == 0) continue;  // a frame of fewer bands than devices
    FRM_HIP(ctx, hipSetDevice(c->device));
    if ((rc = slot_stream(c, c->next_slot, &st[r]))) return relay(ctx, c, rc);
    // the band buffer's last gather (this slot's last frame) has read it
    if (gs.gather_pending)
      FRM_HIP(ctx, hipStreamWaitEvent(st[r], G.rccl ? gs.sent[r] : gs.copied, 0));
    if ((rc = pool_grow(c, gs.bands[r], G.stride, st[r]))) return relay(ctx, c, rc);
    if (stats) FRM_HIP(ctx, hipMemsetAsync(c->counters, 0, FRM_NUM_COUNTERS * sizeof(unsigned long long), st[r]));
    KernelArgs a = make_args(c, c->params, c->scene, gs.bands[r].p, c->counters, G.band_rows, r, n, rows[r]);
    if ((rc = launch(c, a, st[r]))) return relay(ctx, c, rc);
  }
  // rank 0, into the first part of the gather buffer
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  KernelArgs a0 = make_args(ctx, ctx->params, ctx->scene, gs.gathered.p, ctx->counters, G.band_rows, 0, n, rows[0]);
  if ((rc = launch(ctx, a0, s0))) return rc;
  // gather on device 0, rank-major
  if (G.rccl) {
    // one communicator, so its operations run in issue order on every device: each frame's
    // transfers wait for the previous frame's (frames in flight use other streams)
    if (G.comm_pending)
      for (uint32_t r = 0; r < n; ++r) {
        if (r > 0 && rows[r] == 0) continue;
        FRM_HIP(ctx, hipSetDevice(member(ctx, r)->device));
        FRM_HIP(ctx, hipStreamWaitEvent(st[r], G.comm_done[r], 0));
      }
    FRM_NCCL(ctx, ncclGroupStart());
    for (uint32_t r = 1; r < n; ++r) {
      const size_t bytes = (size_t)rows[r] * ctx->width * 4u;
      if (!bytes) continue;
      FRM_HIP(ctx, hipSetDevice(G.sub[r]->device));
      FRM_NCCL(ctx, ncclSend(gs.bands[r].p, bytes, ncclUint8, 0, G.comm[r], st[r]));
      FRM_HIP(ctx, hipSetDevice(ctx->device));
      FRM_NCCL(ctx, ncclRecv(gs.gathered.p + (size_t)r * G.stride, bytes, ncclUint8, (int)r, G.comm[0], s0));
    }
    FRM_NCCL(ctx, ncclGroupEnd());
    for (uint32_t r = 0; r < n; ++r) {
      if (r > 0 && rows[r] == 0) continue;
      FRM_HIP(ctx, hipSetDevice(member(ctx, r)->device));
      FRM_HIP(ctx, hipEventRecord(G.comm_done[r], st[r]));
      if (r > 0) FRM_HIP(ctx, hipEventRecord(gs.sent[r], st[r]));
    }
    G.comm_pending = true;
  } else {
    for (uint32_t r = 1; r < n; ++r) {
      const size_t bytes = (size_t)rows[r] * ctx->width * 4u;
      if (!bytes) continue;
      FRM_HIP(ctx, hipSetDevice(G.sub[r]->device));
      FRM_HIP(ctx, hipEventRecord(gs.rendered[r], st[r]));
      FRM_HIP(ctx, hipSetDevice(ctx->device));
      FRM_HIP(ctx, hipStreamWaitEvent(s0, gs.rendered[r], 0));
      FRM_HIP(ctx, hipMemcpyAsync(gs.gathered.p + (size_t)r * G.stride, gs.bands[r].p, bytes, hipMemcpyDeviceToDevice, s0));
    }
    FRM_HIP(ctx, hipSetDevice(ctx->device));
    FRM_HIP(ctx, hipEventRecord(gs.copied, s0));
  }
  gs.gather_pending = true;
  // reassemble; the slot's `done` now covers render, gather and reassembly
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  FRM_HIP(ctx, launch_unshuffle(gs.gathered.p, G.stride, sl.fb(), ctx->width, ctx->height, G.band_rows, n, s0));
  FRM_HIP(ctx, hipEventRecord(sl.done, s0));
  if ((rc = resolve_frame(ctx, sl))) return rc;
  show_slot(ctx, sl);
  keep_render_params(ctx);
  if (stats) {
    uint64_t sum[FRM_NUM_COUNTERS];
    float ms = 0.0f;
    if ((rc = stats_end(ctx, s0, sum, &ms))) return rc;
    for (uint32_t r = 1; r < n; ++r) {  // the members' counters onto the context's
      if (rows[r] == 0) continue;
      frm_ctx* c = G.sub[r];
      uint64_t host[FRM_NUM_COUNTERS];
      FRM_HIP(ctx, hipSetDevice(c->device));
      FRM_HIP(ctx, hipMemcpyAsync(host, c->counters, sizeof(host), hipMemcpyDeviceToHost, st[r]));
      FRM_HIP(ctx, hipStreamSynchronize(st[r]));
      for (uint32_t k = 0; k < FRM_NUM_COUNTERS; ++k) sum[k] += host[k];
    }
    FRM_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = frm_stats_from_counters(ctx, sum, stats))) return rc;
    stats->kernel_ms = ms;  // device 0's view: from its render's start to the reassembled frame
  }
  return FRM_OK;
}

int group_synchronize(frm_ctx* ctx) {
  for (uint32_t r = 1; r < ctx->group->n; ++r) {
    frm_ctx* c = ctx->group->sub[r];
    FRM_HIP(ctx, hipSetDevice(c->device));
    if (int rc = synchronize_all(c)) return relay(ctx, c, rc);
  }
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  return synchronize_all(ctx);
}
