// frm_ctx.h — the context behind include/frm.h's opaque frm_ctx, and what the host layer's files
// (frm_api.hip, frm_stages.hip, frm_debug.hip, frm_launch.hip, frm_group.hip, frm_ring.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sched.h>

#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "frm.h"
#include "frm_internal.h"

using namespace frm;

// Mandelbulb persistent kernel: lanes that must be waiting before a wave runs its service
// pass (tuning knob; FRM_SERVICE_MIN overrides it for experiments).
static constexpr uint32_t kDefaultServiceMin = 24;  // swept 16..36 on MI355X (round 1: 20); round-2 kernel: headline 16/20/24/28 = 11.43/11.36/11.18/11.24 ms, C2 flat
// Kernel choice without a FRM_FLAG_*_KERNEL flag: below one resident persistent grid
// (6 blocks of 256 lanes per CU for the Mandelbulb) a launch has fewer pixels than lanes,
// and the persistent kernel's fixed costs (pixel sort, grid, separate shading pass) outweigh
// its load balancing: 256x256 runs 23 G steps/s simple vs 10 persistent, 1920x1080 8 vs 20.
static constexpr uint64_t kSimplePixelsPerCu = 1536;
// Queue positions a launch may claim beyond its pixels (2 chunks per wave of a grid of up to
// 2^17 waves); launches are limited to 2^32 - 1 - this many fetch positions.
static constexpr uint64_t kQueueHeadroom = 1ull << 24;
// Persistent grid of a single-frame launch on a context with frames in flight (launch()), for
// launches of up to kInflightCapPixels pixels (four 4K frames: 8K): the capped grids of two frames
// fill the CUs side by side (8K drop-in loop 37.6 -> 36.2 ms/frame). A larger frame's boundary is
// a small part of its time and the cap costs more than it gains (C5, 16384^2: 3 in flight 533-547
// ms/frame capped against 489-491 at the occupancy limit, 2 in flight 578 against 511;
// profiles/round5/c5cap, c4cap, final/configs).
// 16 = half the 8-wave kernel's occupancy (sweep 12/14/16/32 on the drop-in loop: 8.22 / 8.03 /
// 7.90 / 8.55 ms fixed, 8.96 / 8.82 / 8.71 / 9.87 moving; profiles/round5/dropin_bpc8; with the
// round-5 7-wave kernel 12 was best, profiles/round5/dropin_bpc).
// With F frames in flight the cap is the kernel's occupancy (32 workgroups per CU) over F, so the F
// grids fit side by side (round 6, one rank's 8-way share of the headline, one frame per launch:
// 3 in flight 1.49 ms at 16 per CU, 1.21 at 10-11; 4 in flight 1.09 at 8; 2 in flight 16 stays best,
// 1.53-1.56 at 12-20; profiles/round6/share/). F = 2 gives the 16 above.
static constexpr int kInflightBlocksPerCu = 16;
static constexpr uint64_t kInflightCapPixels = 4ull * 3840u * 2160u;
// Single-frame launches with one frame in flight: 7 waves/SIMD (28 one-wave workgroups per CU)
// rather than the kernel's 8. A lone frame ends with its costliest pixels' marches, which an
// eighth wave per SIMD slows when they were not fetched first (render-and-wait loop, moving camera:
// 12.85-12.91 ms at 28 per CU, 13.11-13.29 at 32; fixed pose 9.55-9.60 against 9.38-9.46;
// profiles/round5/dropin_bpc8); multi-frame launches interleave their frames' tails and take 8.
static constexpr int kLoneFrameBlocksPerCu = 28;

// What a context's frm_render makes of a frame. The four modes beyond kPlain exclude each other: a
// setter refuses while another mode is on, and the per-rank and stage entry points serve plain
// contexts (frm_render_shutter: supersampled ones too). frame_mode() derives it from the setters'
// fields, which stay because the getters return them and their "off" values are kept state.
enum FrameMode : uint8_t { kPlain, kSupersampled, kAdaptive, kPanorama, kDof };
// A mode for refuse_mode(): "a <noun> context (<setter>); <instead>".
struct ModeText {
  const char *noun, *setter, *instead;
};
static constexpr ModeText kModeText[] = {
    {"plain", "", ""},
    {"supersampled", "frm_set_supersampling",
     "switch that off, or render the bands at the internal size on a plain context and call frm_resolve"},
    {"adaptive", "frm_set_adaptive", "switch that off, or render the bands on a plain context and call frm_refine"},
    {"panorama", "frm_set_panorama",
     "switch that off, or render the faces (frm_panorama_parameters) on a plain context and call frm_project_equirect"},
    {"depth-of-field", "frm_set_depth_of_field",
     "switch that off, or render on a plain context and call frm_depth_of_field"},
};

// A device buffer of a context's pool (frm_ctx::pool) that follows the frame size: grown on demand
// (pool_grow), a smaller need keeps the larger block. Pointer and capacity change together.
struct PoolBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;  // bytes
};

// One frame in flight: the device state a render launch owns until it completes. A context
// has config.frames_in_flight slots and launches round-robin over them, so frame k+1 can
// start (its own scratch, queue and framebuffer) while frame k's last pixels finish.
struct Slot {
  hipStream_t stream = nullptr;  // frm_render's stream for this slot (slot 0: the context stream)
  hipEvent_t done = nullptr;     // recorded after the slot's last launch (any stream)
  bool pending = false;          // `done` has been recorded since the slot was last waited for
  hipStream_t last_stream = nullptr;  // stream of the slot's last launch
  // frm_render's framebuffers for this slot (context pool), used alternately: a frame's
  // asynchronous readback (copy stream) overlaps the slot's next render, which writes the other
  // one; fb() is the current one. Capacity: a smaller frame size keeps the larger buffer.
  PoolBuf fbs[2];
  hipEvent_t fb_read[2] = {nullptr, nullptr};  // after the last asynchronous readback of fbs[i]
  bool fb_read_pending[2] = {false, false};
  uint32_t fb_idx = 0;
  uint8_t* fb() const { return fbs[fb_idx].p; }
  // supersampling (frm_set_supersampling, factor > 1): the resolved image of fbs[i], what the
  // presentation paths read; alternating with the framebuffers, so fb_read[i] covers its readers too
  PoolBuf res[2];
  // what res[i] holds of the slot's last frame into fbs[i]: its resolve, its adaptive or its gathered
  // frame (the FrameMode that frame was rendered in), kPlain: nothing, the frame is fbs[i] itself
  uint8_t second[2] = {kPlain, kPlain};
  void no_second(bool both = false) {
    second[fb_idx] = kPlain;
    if (both) second[fb_idx ^ 1u] = kPlain;
  }
  // adaptive supersampling (frm_set_adaptive, factor > 1): the slot's scratch of the pass: the list of
  // refined pixels (one u32 per pixel) and its control words
  PoolBuf refine_list;
  uint32_t* refine_ctl = nullptr;
  uint32_t refine_w = 0, refine_h = 0;  // the frame the list belongs to
  // motion blur (frm_render_shutter): the sub-frames of one chunk, back to back, and the f32 sums a
  // frame of several chunks carries between them (a float4 per output pixel)
  PoolBuf shutter_src, shutter_acc;
  // panoramas (frm_set_panorama): the six faces of a frame, back to back, and the direction tables
  // (equirect_tables) of a pano_w x pano_h output, uploaded when the output size changes
  PoolBuf pano_src, pano_tables;
  uint32_t pano_w = 0, pano_h = 0;
  // depth of field (frm_set_depth_of_field): the plane of the slot's last gathered frame, depth_w x
  // depth_h floats (frm_read_depth)
  PoolBuf depth;
  uint32_t depth_w = 0, depth_h = 0;
  unsigned int* queue = nullptr;
  PoolBuf records;  // persistent kernel scratch (ShadeGeom[n] then ShadeTail[n], record_tails), grown on demand
  // pixel scheduling state (frm_sched.hip), sched_cap entries each: 0..cap-1, the fetch
  // order, the cost keys the slot's last launch recorded per pixel and the sort's key output
  uint32_t* sched_iota = nullptr;
  uint32_t* sched_order = nullptr;
  uint8_t* sched_keys = nullptr;  // 2 x sched_cap: keys, sorted keys
  void* sched_temp = nullptr;
  size_t sched_cap = 0, sched_temp_bytes = 0;
  uint64_t sched_key = 0;  // geometry the recorded keys belong to
  bool sched_history = false;
  uint32_t sched_w = 0, sched_h = 0;  // frame size of the recorded keys when they cover a whole frame
  bool sched_whole = false;
  uint32_t sched_npix = 0;  // local pixels of the slot's last persistent launch (<= sched_cap)
  // another slot's launch copied this slot's keys as its scheduling history (on keys_reader):
  // this slot's next launch, which rewrites them, waits for that copy
  hipEvent_t keys_read = nullptr;
  hipStream_t keys_reader = nullptr;
  uint64_t seq = 0;  // launch sequence number of the slot's last launch (frm_ctx::launch_seq)
  // fused scheduling (KernelArgs::key_hist): two launches' histogram + cursor words, used
  // alternately; order_ready: the slot's last launch ranked its pixels into sched_order and zeroed
  // the queue and the other half of rank_words for geometry order_key
  uint32_t* rank_words = nullptr;
  uint32_t rank_half = 0;
  bool order_ready = false;
  uint64_t order_key = 0;
  // asynchronous readback (frm_read_frame_async / frm_present_async): the frame's bytes (or its
  // blit) copied into a pinned host image after the render, on `rb_stream`: the render's own stream
  // when frames are in flight (another slot's stream renders the next frame meanwhile), else the
  // slot's copy stream after `done`, so that a lone slot's stream goes straight on to the next frame.
  // One stream per slot keeps a context within HIP's default 4 hardware queues per process: with a
  // copy stream per slot as well, 2 frames in flight used 4 streams, queues were shared and a
  // frame's render queued behind the previous frame's copy (drop-in loop at
  // GPU_MAX_HW_QUEUES=4). `copied` is recorded after the copy; the slot's next frm_render waits for
  // it before its launch rewrites the framebuffer.
  hipStream_t copy_stream = nullptr;  // owned (one slot only)
  hipStream_t rb_stream = nullptr;    // the stream of the last readback's copy
  uint8_t* host_img = nullptr;
  size_t host_cap = 0;
  PoolBuf present_dev;  // frm_present_async's blit output (device, context pool), grown on demand
  hipEvent_t copied = nullptr;
  uint64_t copy_ticket = 0;  // 0: no readback held
  size_t copy_bytes = 0;
};

// A group context (frm_config.device_count): the context itself renders rank 0's bands on
// devices[0] and holds the frames; sub[r] (r >= 1) renders rank r's bands on devices[r]. Per frame
// slot: rank r's band buffer on its device, and on device 0 the rank-major gather buffer (rank 0's
// bands are rendered straight into its first part) that frm_unshuffle_bands' kernel reassembles
// into the slot's framebuffer.
struct GroupSlot {
  PoolBuf bands[FRM_MAX_DEVICES];         // r >= 1 (device r's pool)
  hipEvent_t sent[FRM_MAX_DEVICES] = {};  // r >= 1, device r: after the slot's last gather read bands[r]
  hipEvent_t rendered[FRM_MAX_DEVICES] = {};  // r >= 1, device r: the bands are written (copy transport)
  hipEvent_t copied = nullptr;            // device 0: after the copy transport's gather
  bool gather_pending = false;
  PoolBuf gathered;  // device 0 (context pool): ranks x stride bytes
};
struct Group {
  uint32_t n = 0;
  frm_ctx* sub[FRM_MAX_DEVICES] = {};  // sub[0] unused: rank 0 is the group context itself
  ncclComm_t comm[FRM_MAX_DEVICES] = {};
  bool rccl = false;  // RCCL point-to-point gather (distinct devices); else device-to-device copies
  hipEvent_t comm_done[FRM_MAX_DEVICES] = {};  // device r: after the last gather's RCCL operations
  bool comm_pending = false;
  uint32_t band_rows = 0;
  size_t stride = 0;  // bytes of rank 0's bands (the largest share): the gather buffer's rank stride
  GroupSlot slots[FRM_MAX_FRAMES_IN_FLIGHT];
};

// The resident frame ring of a context (frm_internal.h RingArgs; frm_ring.hip).
struct Ring {
  uint32_t slots = 0;         // R (2 or 4); 0: never set up
  RingHost* host = nullptr;   // pinned, coherent
  RingDev* dev = nullptr;
  // buffers of the ring's frame size (R frames each): records, framebuffers, fetch orders, cost keys,
  // and the scheduling scratch of its first orders
  uint8_t* records = nullptr;
  uint32_t* out = nullptr;
  uint32_t* order = nullptr;
  uint8_t* keys = nullptr;
  uint32_t* iota = nullptr;
  uint8_t* keys_sorted = nullptr;
  void* sched_temp = nullptr;
  size_t sched_temp_bytes = 0;
  size_t cap = 0;             // pixels per frame the buffers hold
  bool keys_valid = false;    // keys hold a frame of keys_w x keys_h
  uint32_t keys_w = 0, keys_h = 0;
  // zero-copy readback: two pinned host images per slot (frame g: image (g - 1) / R & 1 of its slot),
  // each the frame it holds (or will hold) and the ticket handed out for it
  uint32_t* img[kRingSlots][2] = {};
  size_t img_cap = 0;
  uint32_t img_seq[kRingSlots][2] = {};
  uint64_t img_ticket[kRingSlots][2] = {};
  size_t img_bytes[kRingSlots][2] = {};
  bool zero_copy = false;     // frm_read_frame_async has been called: frames carry a host image
  // images replaced by larger ones (a resize) while a ticket still named them: kept until destroy
  struct Retired {
    uint64_t ticket;
    uint32_t* img;
    uint32_t seq, slot;
    size_t bytes;
  };
  std::vector<Retired> retired;
  // the generation the ring is set up for (a frame with other scene uniforms, size, aspect or step
  // cap needs another grid and a fresh ring)
  bool gen_valid = false;
  SceneUniforms su{};
  uint32_t w = 0, h = 0, max_steps = 0;
  float aspect[2] = {0.f, 0.f};
  uint32_t next_seq = 1;      // seq of the next posted frame
  uint32_t last_seq = 0;      // the last posted frame
  uint32_t grid_id = 0;       // the last launched grid (0: none yet)
  uint32_t service_waves = 128;
};

struct frm_ctx {
  int device = 0;
  Group* group = nullptr;   // a group context (frm_config.device_count >= 1)
  bool bands_only = false;  // a group's rank r >= 1: renders bands, holds no frame
  uint32_t max_steps = FRM_DEFAULT_MAX_STEPS;
  uint32_t flags = 0;
  int cu_count = 0;
  hipStream_t stream = nullptr;  // the context stream (= slots[0].stream)
  // Stream-ordered pool of the buffers that follow the frame size (framebuffers, persistent-kernel
  // records, scheduling arrays, presentation output): they are released and re-allocated on the
  // stream that uses them, so frm_resize never drains the frames in flight. Freed blocks stay in
  // the pool (release threshold: never) for the next size change.
  hipMemPool_t pool = nullptr;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  uint32_t width = 0, height = 0;  // the internal render size: supersample x the output size
  uint32_t supersample = 1;        // frm_set_supersampling
  uint32_t out_width = 0, out_height = 0;  // frm_resize's size: what the presentation paths show
  uint32_t adaptive = 1;                   // frm_set_adaptive: samples per axis of a refined pixel (1: off)
  uint32_t edge_threshold = FRM_ADAPTIVE_DEFAULT_THRESHOLD;
  Slot slots[FRM_MAX_FRAMES_IN_FLIGHT];
  uint32_t nslots = 1;
  uint32_t next_slot = 0;  // slot of the next launch
  uint32_t last_slot = 0;  // slot of the last frm_render (the frame read_frame/present see)
  uint64_t launch_seq = 0;  // render launches so far (Slot::seq)
  uint64_t render_seq = 0;  // launch_seq of the last frm_render
  uint64_t ticket_seq = 0;  // asynchronous readbacks so far
  frm_parameters render_params{};  // the parameters of the last frm_render (frm_debug_trace)
  SceneUniforms render_scene{};
  ReloadedKernels* reloaded = nullptr;  // frm_reload: kernels compiled from edited sources
  uint8_t* present_buf = nullptr;  // frm_present output, grown on demand
  size_t present_cap = 0;
  unsigned long long* counters = nullptr;  // FRM_NUM_COUNTERS
  uint32_t service_min = kDefaultServiceMin;
  bool fused_sched = true;  // KernelArgs::key_hist; FRM_SCHED=sort: every launch sorts (experiments)
  frm_parameters params{};
  bool has_params = false;
  SceneUniforms scene{};
  uint32_t shutter_chunk = FRM_MAX_SHUTTER_SAMPLES;  // frm_render_shutter: sub-frames per chunk at most (FRM_SHUTTER_CHUNK)
  // the last frame composed of several (frm_render_shutter's sub-frames, a panorama's faces), which
  // leaves no single frame to trace: its render_seq (0: none) and what it was made of
  uint64_t composed_seq = 0;
  const char* composed_of = "";
  uint32_t panorama = 0;      // frm_set_panorama: the face size N (0: off); the render size is (N + 2)^2
  uint32_t dof_radius = 0;  // frm_set_depth_of_field: the largest radius R (0: off)
  float dof_aperture = 0.0f, dof_focus = 1.0f;
  // host copies of direction tables whose upload may still be running: each is released once the
  // event recorded after its copy has completed (upload_tables), the rest by frm_destroy
  struct HostBlock {
    float* p;
    hipEvent_t copied;
  };
  std::vector<HostBlock> host_blocks;
  Ring ring;
  bool ring_enabled = false;  // FRM_RING=1: the resident frame ring (opt-in: slower)
  bool last_is_ring = false; // the last frm_render posted a ring frame (ring.last_seq)
  std::string error;
};

#define FRM_HIP(ctx, call)                              \
  do {                                                  \
    hipError_t e_ = (call);                             \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, #call); \
  } while (0)

#define FRM_NCCL(ctx, call)                                                                         \
  do {                                                                                              \
    ncclResult_t r_ = (call);                                                                       \
    if (r_ != ncclSuccess) return fail(ctx, FRM_ERR_HIP, "%s failed: %s", #call, ncclGetErrorString(r_)); \
  } while (0)

// A framebuffer-sized allocation for a frame of `bytes`: headroom for the reference's +-1
// render-texture steps (4 % per axis), which then reuse the block.
static inline size_t with_headroom(size_t bytes) { return bytes + bytes / 4u; }

static inline FrameMode frame_mode(const frm_ctx* ctx) {
  if (ctx->dof_radius) return kDof;
  if (ctx->panorama) return kPanorama;
  if (ctx->adaptive > 1u) return kAdaptive;
  return ctx->supersample > 1u ? kSupersampled : kPlain;
}

// The frames of one multi-frame launch may differ in camera, and for the Mandelbulb in time (its
// power, fragment.wgsl:75, is the only time-derived constant): otherwise the same scene uniforms
// (scene, iterations, time-derived constants). s0: frame 0's uniforms, powers[k]: frame k's power,
// anim: the powers differ, differs: the first frame whose uniforms differ from frame 0's in more
// than that (0: none).
struct BatchUniforms {
  SceneUniforms s0;
  float powers[FRM_MAX_BATCH];
  bool anim;
  uint32_t differs;
};

// A device buffer of a stage or band entry point, for check_spans: the argument's name, the bytes the
// caller says it holds and the bytes the call touches (0: the buffer is not used, and may be NULL),
// its alignment, and whether the call writes it.
struct Span {
  const char* name;
  const void* p;
  size_t held, need;
  uint32_t align;
  bool written;
};

// The host layer's own functions stay out of libfrm.so's dynamic symbols.
#pragma GCC visibility push(hidden)
// frm_api.hip
int fail(frm_ctx* ctx, int code, const char* fmt, ...);
int hip_fail(frm_ctx* ctx, hipError_t e, const char* what);
int create_one(const frm_config* config, int device, frm_ctx** out_ctx);
int not_on_group(frm_ctx* ctx, const char* what);
int refuse_mode(frm_ctx* ctx, const char* what);
int ensure_ready(frm_ctx* ctx);
int check_parameters(frm_ctx* ctx, const SceneUniforms& su, const frm_parameters& p);
// frm_stages.hip
int check_size(frm_ctx* ctx, uint32_t width, uint32_t height, uint32_t factor, const char* noun);
int check_output(frm_ctx* ctx, uint32_t out_width, uint32_t out_height, uint32_t flags);
int check_lens(frm_ctx* ctx, float aperture, float focus, uint32_t max_radius);
int check_spans(frm_ctx* ctx, std::initializer_list<Span> spans);
// frm_launch.hip
int dev_alloc(frm_ctx* ctx, void** p, size_t bytes, hipStream_t s);
int dev_release(frm_ctx* ctx, void* p, hipStream_t s);
int pool_grow(frm_ctx* owner, PoolBuf& b, size_t bytes, hipStream_t s);
ShadeTail* record_tails(const PoolBuf& records);
int ensure_fb(frm_ctx* ctx, Slot& sl, size_t bytes);
int select_fb(frm_ctx* ctx, Slot& sl, uint32_t i);
int ensure_res(frm_ctx* ctx, Slot& sl, size_t bytes);
int resolve_frame(frm_ctx* ctx, Slot& sl);
int ensure_shutter(frm_ctx* ctx, Slot& sl, size_t src_bytes, size_t acc_bytes);
int upload_tables(frm_ctx* ctx, float* dev, uint32_t w, uint32_t h, hipStream_t s);
void release_host_blocks(frm_ctx* ctx, bool wait);
int ensure_panorama(frm_ctx* ctx, Slot& sl, size_t src_bytes, uint32_t w, uint32_t h);
const uint8_t* shown(const frm_ctx* ctx, const Slot& sl);
uint32_t num_bands(uint32_t height, uint32_t band_rows);
uint64_t band_local_rows(uint32_t height, uint32_t band_rows, uint32_t first, uint32_t stride);
int band_rows_u32(frm_ctx* ctx, uint32_t height, uint32_t band_rows, uint32_t first, uint32_t stride, uint32_t* rows);
uint32_t group_band_rows(uint32_t height, uint32_t n);
KernelArgs make_args(const frm_ctx* ctx, const frm_parameters& params, const SceneUniforms& scene, uint8_t* dst,
                     unsigned long long* counters, uint32_t band_rows, uint32_t first, uint32_t stride,
                     uint32_t local_rows);
KernelKind kernel_for(const frm_ctx* ctx, uint64_t pixels);
int wait_slot(frm_ctx* ctx, Slot& sl);
int synchronize_all(frm_ctx* ctx);
int slot_stream(frm_ctx* ctx, uint32_t i, hipStream_t* out);
int launch(frm_ctx* ctx, KernelArgs a, hipStream_t s);
void batch_uniforms(const frm_ctx* ctx, uint32_t count, const frm_parameters* params, BatchUniforms* u);
int launch_frames(frm_ctx* ctx, uint32_t count, const frm_parameters* params, const BatchUniforms& u,
                  bool scene_per_frame, uint8_t* dst, size_t frame_stride_bytes, const BandGeometry& g,
                  unsigned long long* counters, hipStream_t s, int pin_slot);
int frame_prologue(frm_ctx* ctx, const frm_stats* stats);
int begin_frame(frm_ctx* ctx, Slot** out_slot, hipStream_t* out_stream);
int stats_begin(frm_ctx* ctx, hipStream_t s);
int stats_end(frm_ctx* ctx, hipStream_t s, uint64_t* out_counters, float* out_ms);
int finish_stats(frm_ctx* ctx, hipStream_t s, frm_stats* stats);
void show_slot(frm_ctx* ctx, const Slot& sl);
void keep_render_params(frm_ctx* ctx);
// frm_group.hip
int group_init(frm_ctx* ctx, const frm_config* config);
void group_destroy(frm_ctx* ctx);
int group_render(frm_ctx* ctx, frm_stats* stats);
int group_synchronize(frm_ctx* ctx);
// frm_ring.hip
bool ring_eligible(const frm_ctx* ctx);
int ring_quiesce(frm_ctx* ctx);
int ring_render(frm_ctx* ctx);
int ring_materialize(frm_ctx* ctx);
int ring_read_async(frm_ctx* ctx, uint64_t* out_ticket);
int ring_leave(frm_ctx* ctx);
int ring_ticket_pixels(frm_ctx* ctx, uint64_t ticket, const uint8_t** out_pixels, size_t* out_bytes);
void ring_destroy(frm_ctx* ctx);
#pragma GCC visibility pop

// A group's rank r, and a failure of such a member context, reported on the group context.
static inline frm_ctx* member(frm_ctx* ctx, uint32_t r) { return r == 0 ? ctx : ctx->group->sub[r]; }
static inline int relay(frm_ctx* ctx, const frm_ctx* member, int rc) {
  return member == ctx ? rc : fail(ctx, rc, "device %d: %s", member->device, member->error.c_str());
}
