// frm_render_kernels.h — the render kernels of the fractal ray-marcher (gfx950):
// render_simple<FAM, ITERS>, march_persistent<FAM, ITERS>, shade_pass<FAM> and rank_pass, with
// their device helpers; the resident ring's device code, which march_persistent's ring grid runs,
// is in frm_ring_kernels.h. Included by frm_kernels.hip (compiled ahead of time by hipcc) and by
// the source frm_reload compiles at run time with hiprtc (frm_reload.hip), so an edited copy of
// these headers can replace the running kernels without rebuilding the library.
//
// render_simple<FAM>: one thread per pixel, one wave64 per 8x8 pixel tile (so the 64
//   lanes of a wave march spatially coherent rays), 256-thread blocks = 16x16 pixels.
//   Literal restatement of fragment_main (fragment.wgsl:327-349): primary march, on hit
//   the four normal taps, the shadow march toward the sun and the shading; sRGB encode
//   and a packed 32-bit RGBA8 store. Work counters are reduced per wave in registers and
//   added with one 64-bit atomic per wave and counter.
#pragma once
#include "frm_internal.h"
#include "frm_srgb_table.h"

// Build parameters of march_persistent's launch bounds (the Makefile sets both).
#ifndef FRM_MARCH_WAVES_PER_SIMD
#define FRM_MARCH_WAVES_PER_SIMD 1
#endif
#ifndef FRM_RING_WAVES_PER_SIMD
#define FRM_RING_WAVES_PER_SIMD FRM_MARCH_WAVES_PER_SIMD
#endif
// The two round-12 forms of the Mandelbulb launches' full service pass that are not settled
// (profiles/round12/pass). Both are bit-exact and
// take instructions out of the pass (-9 and -3 VALU), but neither measured faster alone (the masks
// +-0, the tap offsets +0.7 %, slower), so both are off until code placement is fixed. Neither
// touches the ring grid or the fixed-trip families. Every other A/B form of rounds 8-12 is settled:
// the shipped ones are the code below, the rejected ones are patches against it under
// profiles/round9/sgpr and profiles/round11/loop.
#ifndef FRM_PASS_MASKS
#define FRM_PASS_MASKS 0  // 1: "the DE has its result" as a wave-uniform mask instead of a per-lane flag (no gain alone)
#endif
#ifndef FRM_TAP_OFFSET
#define FRM_TAP_OFFSET 0  // 1: the start-DE block adds -0.0f for lanes that are no tap, no final selects (slower alone)
#endif

namespace frm {

// ---- wave helpers (also used by frm_ring_kernels.h, included below them) -------------------
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// Wave-wide inclusive prefix sum of one value per lane.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = __shfl_up(v, off, 64);
    if (lane >= (uint32_t)off) v += u;
  }
  return v;
}

__device__ __forceinline__ uint32_t band_row_to_global(const BandGeometry& g, uint32_t lr) {
  uint32_t b = lr / g.band_rows;
  return (g.first_band + b * g.band_stride) * g.band_rows + (lr - b * g.band_rows);
}

constexpr uint32_t kIdle = 0xFFFFFFFFu;  // a lane without a pixel; a claim that found nothing
constexpr uint32_t kChunk = 64u;  // pixels per queue fetch (one per lane of the fetching wave)

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// The work-queue partition a wave claims from first (frm_internal.h kQueueParts): one of the
// kQueueParts / 8 partitions of the XCD (XCC) it runs on (s_getreg HW_REG_XCC_ID, 0..7), picked by
// its workgroup index (workgroups b and b + 8 share an XCD). Placement only, never a pixel's bytes.
__device__ __forceinline__ uint32_t queue_part() {
  const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & (kXcds - 1u);
  constexpr uint32_t per = kQueueParts / kXcds;
  return xcc * per + (per > 1u ? (blockIdx.x / kXcds) % per : 0u);
}
__device__ __forceinline__ uint64_t count(bool c) { return (uint64_t)__popcll(ballot(c)); }

// Scheduling key of a finished pixel: 16 x log2(cost + 1), 0..255 (~4.4 % steps); cost =
// Mandelbulb bodies, or DE evaluations for the fixed-trip families. Only orders the next
// frame's fetches; never touches a pixel's bytes.
__device__ __forceinline__ uint8_t cost_key(uint32_t bodies) {
  return (uint8_t)min(255.0f, 16.0f * __log2f((float)bodies + 1.0f));
}

}  // namespace frm
#include "frm_ring_kernels.h"
namespace frm {

template <uint32_t FAM, bool ITERS>
__global__ __launch_bounds__(256) void render_simple(KernelArgs a) {
  __shared__ float table[256];
  table[threadIdx.x] = kSrgbThresholds[threadIdx.x];
  __syncthreads();

  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t x = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
  const uint32_t lr = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
  const uint32_t width = a.f.width;

  uint32_t n_pix = 0;
  PixelCount pc = {0u, 0u, 0u, 0u, {0u, 0u}};
  if (x < width && lr < a.g.local_rows) {
    const uint32_t y = band_row_to_global(a.g, lr);
    if (y < a.f.height) {
      n_pix = 1;
      v3 color = shade_pixel<FAM, ITERS>(a.f, a.s, x, y, pc);
      a.out[(size_t)lr * width + x] = pack_rgba(color, table);
    }
  }

  unsigned long long v[7] = {n_pix, pc.hit, pc.primary, pc.shadow, pc.normal, pc.de.bodies, pc.de.bailouts};
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    unsigned long long s = wave_sum(v[k]);
    if (lane == 0 && s) atomicAdd(&a.counters[k], s);
  }
}

// ---- persistent ray-regeneration kernel + deferred shading pass -------------------
// march_persistent<FAM>: one lane = one pixel at a time, driven by a per-lane state machine
// over the phases of fragment_main (primary march -> 4 normal taps -> shadow march).
// Every loop iteration advances every live lane by exactly one unit of DE work: one
// Mandelbulb loop body (the DE is resumable: z, dr, magnitude and body index live in
// registers), or one whole DE for the fixed-trip-count families. A lane whose pixel is
// done takes the next pixel of its wave's current chunk; a wave fetches chunks of 64
// pixels from a global queue (one atomic per chunk) in the order frm_sched.hip chose
// (most expensive pixels first), and computes the chunk's 64 camera rays in one coherent
// pass into LDS. Instead of shading at low lane occupancy, a finished
// pixel stores an 8-byte ShadeTail (+ a 16-byte ShadeGeom for a hit, at its last normal
// tap); shade_pass then shades and sRGB-packs all pixels
// coherently. Per-pixel arithmetic is the same operation sequence as shade_pixel<>, so
// the bytes are identical to render_simple and the oracle.
enum Phase : uint32_t { kPrimary = 0, kTap0 = 1, kTap3 = 4, kShadow = 5 };

#ifdef FRM_STAMPS
// diagnostic build: one 16 x u64 record per wave of the last persistent launch
constexpr uint32_t kWaveDebugSlots = 16384u;
__device__ unsigned long long g_wave_debug[16u * kWaveDebugSlots];
#endif

// The Mandelbulb body loop's counter: the bodies a lane's DE has left before its count exit, N
// where the DE starts (`left` in march_persistent). One
// subtract-with-borrow per iteration takes 1 from every lane of `pending` (the borrow-in is that wave-uniform mask: other lanes subtract 0) and returns the
// borrow-out, the pending lanes that went below 0: their body of this iteration is body N + 1,
// the count exit. It stands for the increment and the two compares of a count upwards, and the
// exit mask never passes through a VGPR. The DE's bodies so far are n_iter - left (mod 2^32:
// N + 1 after the count exit, where left is 0xffffffff).
__device__ __forceinline__ uint64_t count_down(uint32_t& left, uint64_t pending) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint64_t out;
  asm("v_subb_co_u32_e64 %0, %1, %0, 0, %2" : "+v"(left), "=s"(out) : "s"(pending));
  return out;
#else  // hipcc's host pass (never run: kernels are device code)
  const uint64_t bit = 1ull << (threadIdx.x & 63u);
  const bool in = (pending & bit) != 0, out = in && left == 0u;
  left -= in ? 1u : 0u;
  return out ? bit : 0ull;
#endif
}

// One work counter of a wave, exactly 64 bits wide. The loops add to its low word, one SGPR; the
// carry is a wave-uniform branch to a cold block that bumps the high word, which nothing else
// reads before the final flush, so the register allocator may park it in a spill lane. (As
// uint64_t the six counters held twelve SGPRs across both loops.) The loops pay s_add_u32,
// s_cmp, s_cbranch for the earlier s_add_u32, s_addc_u32. The empty asms keep the sum scalar (as
// one overflow-add it became a VALU add) and the cold block a block (folded into the add it is
// the add-with-carry pair again).
struct WaveCounter {
  uint32_t lo, hi;
  __device__ __forceinline__ explicit WaveCounter(uint32_t start) : lo(start), hi(0u) {}
  __device__ __forceinline__ void add(uint32_t n) {
    lo += n;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(lo));
#endif
    if (__builtin_expect(lo < n, 0)) {
      hi++;
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" : "+s"(hi));
#endif
    }
  }
  __device__ __forceinline__ uint64_t value() const { return ((uint64_t)hi << 32) | lo; }
};
// The drained-partitions mask: bits 0..kQueueParts-1 and the head's bit kQueueParts; 32 bits wide
// where they fit.
template <bool NARROW>
struct DrainMask {
  typedef uint64_t type;
};
template <>
struct DrainMask<true> {
  typedef uint32_t type;
};

// MULTI: a multi-frame launch (frm_render_bands_batch, a.batch > 1), a separate instantiation.
// Queue chunk c (64 fetch positions) is chunk c / batch of frame c % batch: the frames'
// pixels interleave chunk by chunk, each frame's longest first, and a chunk's frame (camera)
// is wave-uniform.
// ANIM (MULTI, Mandelbulb): the frames of the launch differ in time, so in the power; each lane
// carries its pixel's frame's power (a.mb_powers) instead of the uniform one.
// RES: a resident ring grid (frm_internal.h RingArgs): workgroups below a.ring.service_waves run
// ring_service; the others march the ring's frames in posting order, each frame's chunks as a
// single-frame launch's, moving on to the next frame when one's queue drains. A lane's record index
// is slot * rec_stride + its local pixel (as a multi-frame launch's frame * rec_stride + ...).
template <uint32_t FAM, bool ITERS, bool MULTI = false, bool ANIM = false, bool RES = false>
__global__ __launch_bounds__(kMarchBlock, RES ? FRM_RING_WAVES_PER_SIMD : FRM_MARCH_WAVES_PER_SIMD) void march_persistent(
    KernelArgs a) {
  __shared__ float4 chunk_rays[kMarchWaves][kChunk];  // per wave: camera ray xyz + record index bits
  static_assert(!RES || (!MULTI && kMarchWaves == 1u), "ring grids: one-wave workgroups, one frame per chunk");
  __shared__ float cam_lds[RES ? kRingSlots : 1][16];  // RES: per slot the camera of its frame (rows, origin, power)
  __shared__ uint32_t rw[RES ? (uint32_t)kRwWords : 1u];  // RES: the wave's claim state (RingWaveWord)
  __shared__ RingLds ring_lds[RES ? 1 : 0 + 1];           // RES: the ring arguments of the march (RingLds)
  if constexpr (RES) {
    // service waves: key counts / bucket bases in the LDS the march waves use for chunk rays (one
    // workgroup is one wave: either kind)
    if (blockIdx.x < a.ring.service_waves) {
      // a call (inlined, the service's registers pushed the march state into scratch), on the
      // kernel arguments where they lie (a reference to the parameter copies it to scratch)
      ring_service<FAM>(*(const KernelArgs*)__builtin_amdgcn_kernarg_segment_ptr(),
                        reinterpret_cast<uint32_t*>(&chunk_rays[0][0]));
      return;
    }
  }

  const FrameUniforms& f = a.f;
  const SceneUniforms& su = a.s;
  constexpr bool kMb = is_mandelbulb(FAM);     // resumable body loop
  constexpr bool kHw = FAM == kMandelbulbHw;   // FRM_FLAG_HW_MATH
  // The lean service pass (below): the Mandelbulb launches (single, MULTI, ANIM, hardware math).
  // Not the ring grid (its register budget is fragile), nor the fixed-trip families.
  constexpr bool kLeanPass = kMb && !RES;
  // Round 12, the launches of the lean pass (whose masks they use): tap distances stored, not
  // summed; and, off: the per-lane `done` flag as the mask done_m; tap offsets without their
  // final selects
  constexpr bool kTapStore = kMb && !RES;
  constexpr bool kPassMasks = FRM_PASS_MASKS && kLeanPass;
  constexpr bool kTapOffset = FRM_TAP_OFFSET && kMb && !RES;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint64_t lane_bit = 1ull << lane;
  // fetch positions (host: < 2^32 - 1); a multi-frame launch pads each frame to whole chunks
  const uint32_t total = MULTI ? a.batch * ((a.npix + kChunk - 1u) / kChunk) * kChunk : a.npix;
  uint32_t chunk_frame = 0;  // wave-uniform: the frame of the wave's current chunk
  const uint32_t n_iter = iterations<ITERS>(su.n);
  static_assert(!ANIM || ((MULTI || RES) && is_mandelbulb(FAM)), "per-lane powers: multi-frame or ring Mandelbulb launches");
  float lane_power = su.mb_power;  // ANIM: the power of the lane's pixel's frame
  ShadeGeom* __restrict__ geom = a.geom;
  ShadeTail* __restrict__ tails = a.tails;

  // wave-uniform state: current chunk of 64 fetched pixels, how many were handed out
  uint32_t slots_used = kChunk;
  bool exhausted = false;
  // the work-queue partition the wave claims from (its XCD's first, kQueueParts in frm_internal.h)
  // and the partitions it has found drained
  const uint32_t nchunks = (total + kChunk - 1u) / kChunk;
  uint32_t part = queue_part();
  typedef typename DrainMask<!RES && (kQueueParts < 32u)>::type drain_t;
  drain_t drained = 0;  // bit x: partition x drained; bit kQueueParts: the head
  const uint32_t nhead = nchunks / kQueueHeadDiv;
  // work counters (frm_stats), each from the launch's debug start value (0 but for
  // FRM_DEBUG_COUNTER_START, the test of the carries), which the flush takes off again
  const uint32_t count0 = RES ? 0u : a.counter_start;
  WaveCounter n_pix(count0), n_hit(count0), n_prim(count0), n_shadow(count0), n_body(count0), n_bail(count0);
#ifdef FRM_COUNT_EXACT
  uint64_t n_dbg_total = 0, n_dbg_exact = 0;
#endif
  uint32_t r_slot = 0;                    // RES: the slot of the wave's current chunk
  if constexpr (RES) {
    uint32_t b = 0;
    if (lane == 0) {
      RING_GRID_TRACE(a.ring, 0);
      b = max(a.ring.first_seq, dev_poll(&a.ring.dev->base));
      ring_lds->host = a.ring.host;
      ring_lds->dev = a.ring.dev;
      ring_lds->order = a.ring.order;
      ring_lds->slots = a.ring.slots;
      ring_lds->grid_id = a.ring.grid_id;
      ring_lds->rec_stride = a.rec_stride;
      ring_lds->npix = a.npix;
    }
    __syncthreads();
    if (lane < (uint32_t)kRwWords) rw[lane] = 0u;
    rw_set(rw, kRwLo, uniform(__shfl(b, 0, 64)));
  }

  // per-lane state
  uint32_t pix = kIdle;      // local pixel index (lr * width + x) being marched
  uint32_t phase = kPrimary;
  bool done = false;         // the current DE has its result
  // kPassMasks: the same set as a wave-uniform mask (SGPRs), in place of `done`. As a flag it was
  // set under one branch and read under another, so each crossing widened it to 0/1 in a VGPR and
  // compared it back into a mask. Bits of lanes without a pixel mean nothing (masked by `live`).
  [[maybe_unused]] uint64_t done_m = 0;
  v3 o = mk(0.f, 0.f, 0.f), d = o, nsum = o, q = o, z = o;
  float t = 0.f, closeness = 0.f, dr = 1.f, mag = 0.f, de = 0.f;
  uint32_t it = 0, psteps = 0;
  [[maybe_unused]] uint32_t left = 0;  // kMb: the bodies the lane's DE has left (count_down())
  uint32_t pix_cost = 0;  // the lane's pixel's Mandelbulb bodies (other families: DEs) so far, for
                          // its scheduling key; the wave's body total is counted in SGPRs
#ifdef FRM_STAMPS
  uint64_t stamp_service = 0, n_service = 0, n_loop = 0, real_exhaust = 0;
  uint64_t stamp_consume = 0, stamp_refill = 0, n_fetch = 0, n_lean = 0;
  uint64_t stamp_sub[4] = {0, 0, 0, 0};  // consume: distance, primary, taps, shadow
  const uint64_t stamp_begin = __builtin_amdgcn_s_memtime();
  const uint64_t stamp_real0 = __builtin_amdgcn_s_memrealtime();
#define FRM_SUB_BEGIN() const uint64_t sub0 = __builtin_amdgcn_s_memtime()
#define FRM_SUB_END(k) stamp_sub[k] += __builtin_amdgcn_s_memtime() - sub0
#else
#define FRM_SUB_BEGIN()
#define FRM_SUB_END(k)
#endif

  for (;;) {
    // Body phase (Mandelbulb): one loop body per computing lane per iteration, until
    // a.service_min lanes wait for a service pass (finished DE, or idle with work left)
    // or no lane computes. The service pass costs the same however many lanes take part.
    [[maybe_unused]] uint64_t live_m = 0, cons_m = 0;  // kLeanPass: live lanes, consuming lanes (SGPRs)
    if constexpr (kMb) {
      // The loop keeps its lane sets as wave-uniform masks (SGPRs): `pending` predicates the
      // body directly (inverse ballot -> exec) and one ballot per iteration retires lanes,
      // instead of a per-lane flag merged under exec masks every iteration.
      const uint64_t live = ballot(pix != kIdle);
      uint64_t pending = live & ~(kPassMasks ? done_m : ballot(done));
      // lanes that count as waiting when not pending: finished DEs, and idle lanes while
      // the queue still has pixels
      const uint64_t waitable = exhausted ? live : ~0ull;
      for (;;) {
        if (pending == 0 || (uint32_t)__popcll(waitable & ~pending) >= a.service_min) break;
        // one body per computing lane this iteration (a DE that bails out at entry never
        // becomes pending, so this counts bodies exactly: fragment.wgsl:245-249)
        if constexpr (!RES) n_body.add((uint32_t)__popcll(pending));
#ifdef FRM_STAMPS
        n_loop++;
#endif
        // the count exits: by every lane, in front of the branch (the borrow-in selects the lanes)
        const uint64_t cnt_exit = count_down(left, pending);
        if (lane_in(pending)) {
#if defined(FRM_COUNT_EXACT) && defined(__HIP_DEVICE_COMPILE__)  // diagnostic: body-loop iterations, and those that ran the exact body
          n_dbg_total++;
          if (ballot(!mb_tame(z, mag)) != 0) n_dbg_exact++;
#endif
          if constexpr (ANIM)
            mb_step<kHw>(lane_power, lane_power - 1.0f, q, mag, z, dr);  // = the host's mb_power_m1
          else
            mb_step<kHw>(su, q, mag, z, dr);
          // N+1 bodies: the distance uses the last loop-top magnitude
          if (!lane_in(cnt_exit)) mag = mb_length<kHw>(z);
        }
        // the lanes whose DE ends, tested by every lane outside the body's branch (other lanes'
        // bits fall outside `pending`): a flag set inside it reached the mask through a VGPR
        // (the count exits are a mask already)
        pending &= ~(cnt_exit | ballot(mag > su.mb_bailout));
      }
      if constexpr (!kPassMasks) done = !lane_in(pending);  // idle lanes: masked by cons
      live_m = live;
      cons_m = live & ~pending;
    }

    // Service pass.
#ifdef FRM_STAMPS  // diagnostic build: wave cycles spent in service passes -> counters[7]
    const uint64_t stamp0 = __builtin_amdgcn_s_memtime();
#endif
    // 1. consume finished DEs. Branch-light: the bookkeeping of every phase is computed for
    //    every lane with selects; only the distance, the last-tap transition (normal, record,
    //    shadow ray) and the record store of a finished pixel are branches.
    // (kPassMasks: the consuming lanes are the body loop's mask, live & ~pending)
    const bool cons = kPassMasks ? lane_in(cons_m) : (pix != kIdle && done);
    bool ev_bail = false;
    if constexpr (kPassMasks) {
      // DEs that left by bailout (before the first body included), counted from the mask of one
      // compare by every lane: a flag set under `if (cons)` reached the count through a VGPR
      n_bail.add((uint32_t)__popcll(cons_m & ballot(left <= n_iter)));
    }
    // the distance's log without its special-value selects (and with the integer exponent
    // split) when every consuming lane's magnitude is positive, normal and finite
    // (wave-uniform test; same bits)
    bool plain_log = true;
    if constexpr (kMb && !kHw) {
      if constexpr (kPassMasks)  // the same class as an integer range of the bits, [2^-126, inf): the ballot of a
                                 // class test is widened to 0/1 and compared again, a compare's is its mask
        plain_log = (cons_m & ballot(__float_as_uint(mag) - 0x00800000u >= 0x7F000000u)) == 0;
      else
        plain_log = ballot(cons && !__builtin_amdgcn_classf(mag, 0x100 /* +normal */)) == 0;
    }
    if (cons) {
      done = false;
      if constexpr (kMb) {
        FRM_SUB_BEGIN();
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (kHw)
          de = mb_distance_hw(mag, dr);
        else
          de = plain_log ? mb_distance_posnormal(mag, dr) : mb_distance(mag, dr);
#else
        (void)plain_log;
        de = mb_distance(mag, dr);
#endif
        const uint32_t body = n_iter - left;  // wraps to N+1 on a count exit
        pix_cost += body;          // bodies this DE ran (N+1 on a count exit)
        ev_bail = body <= n_iter;  // exit by bailout (incl. before the first body)
        FRM_SUB_END(0);
      }
    }
    // Lean pass (wave-uniform): no live lane is in a tap or shadow phase and no consuming lane
    // hits in this pass, so every consuming lane is a primary ray that marches on or ends as a
    // miss. That holds from a wave's start until its first hit and again once the hit pixels of
    // the longest-first order have drained: the primary rays of miss pixels run under two bodies
    // per DE, so those waves need a pass after about every body iteration. A pass in which a
    // lane hits takes the full path below (de is computed, nothing is redone).
    bool lean = false;
    [[maybe_unused]] uint64_t prim_m = 0, hit_m = 0;  // consuming primary lanes; lanes with a hit distance
    if constexpr (kLeanPass) {  // (the body loop's masks: one compare per term, combined in SGPRs)
      const uint64_t other_m = ballot(phase != kPrimary);
      hit_m = ballot(de <= kMinDistance);
      prim_m = cons_m & ~other_m;
      lean = ((live_m & other_m) | (cons_m & hit_m)) == 0;
    }
    bool need_point = false;
    bool ev_prim = false, ev_hit = false, ev_shadow = false;  // what the full path's lanes consumed
    if (lean) {
      // the full path's primary miss step without the shadow closeness, the tap sums and the
      // phase updates no lane here can need; the same t, it and record bits
      if (cons) {
        t += de;
        it++;
        need_point = it < f.max_steps && t < kMaxTotalDistance;
        if (!need_point) {  // primary miss (flags 0: BACKGROUND_COLOR)
          const uint2 tail = make_uint2(__float_as_uint(closeness), psteps | (cost_key(pix_cost) << kRecKeyShift));
          *reinterpret_cast<uint2*>(&tails[pix]) = tail;
          pix = kIdle;
        }
      }
      n_prim.add((uint32_t)__popcll(cons_m));
#ifdef FRM_STAMPS
      n_lean++;
#endif
    } else {
    if constexpr (kLeanPass) {  // work counters, from the masks while they are at hand
      n_prim.add((uint32_t)__popcll(prim_m));
      n_hit.add((uint32_t)__popcll(prim_m & hit_m));
      n_shadow.add((uint32_t)__popcll(cons_m & ballot(phase == kShadow)));
    }
    ev_prim = cons && phase == kPrimary, ev_shadow = cons && phase == kShadow;
    const bool tap = cons && !ev_prim && !ev_shadow;  // normal taps k.xyy, k.yyx, k.yxy, k.xxx
    const bool hit = de <= kMinDistance;              // object_result.distance >= 0
    ev_hit = ev_prim && hit;
    // shadow closeness = min(closeness, d / t) before t moves (d / 0 on step 0, as in
    // fragment.wgsl:292); computed by every lane, kept by shadow lanes
    const float cl = min_(closeness, de / t);
    closeness = ev_shadow ? cl : closeness;
    const bool step = (ev_prim || ev_shadow) && !hit;  // march on: t += d, it++
    const float t_next = t + de;
    const uint32_t it_next = it + 1u;
    const bool more = it_next < f.max_steps && t_next < kMaxTotalDistance;
    t = step ? t_next : t;
    it = step ? it_next : it;
    psteps = ev_hit ? it : psteps;
    const bool fin = (step && !more) || (ev_shadow && hit);  // primary miss, or shadow march ends
    const bool sun_miss = ev_shadow && step && !more;
    need_point = ev_hit || (step && more) || tap;  // start a DE at the phase's next sample point
    // tap k adds s_k * d to the sum (k = 0 sets it); s_0..s_3 = (+--), (--+), (-+-), (+++)
    const uint32_t k = phase - kTap0;
    if constexpr (kTapStore) {
      // The sums are read at the fourth tap only, so until then nsum's registers hold the first
      // three taps' distances as they come (one select each; 4 % of the consumed DEs are taps)
      // and the fourth-tap branch below adds them up.
      nsum = mk((cons && k == 0u) ? de : nsum.x, (cons && k == 1u) ? de : nsum.y, (cons && k == 2u) ? de : nsum.z);
    } else {
    const float dx = (k == 0u || k == 3u) ? de : -de, dy = (k >= 2u) ? de : -de,
                dz = (k == 1u || k == 3u) ? de : -de;
    // (component-wise: a select of whole structs compiles to a select of stack addresses)
    const float sx = (k == 0u) ? dx : nsum.x + dx, sy = (k == 0u) ? dy : nsum.y + dy,
                sz = (k == 0u) ? dz : nsum.z + dz;
    nsum = mk(tap ? sx : nsum.x, tap ? sy : nsum.y, tap ? sz : nsum.z);
    }
    phase = ev_hit ? kTap0 : (tap ? phase + 1u : phase);  // after the last tap: kShadow
    if (tap && k == kTap3 - kTap0) {  // normal, then the shadow ray toward the sun
      FRM_SUB_BEGIN();
      // kTapStore: the same f32 additions in the same order as the running sums (tap 0 sets the
      // sum, taps 1..3 add s_k * d; a negation is exact)
      const float d0 = nsum.x, d1 = nsum.y, d2 = nsum.z;
      const v3 ns = kTapStore ? mk(((d0 + -d1) + -d2) + de, ((-d0 + -d1) + d2) + de, ((-d0 + d1) + -d2) + de) : nsum;
#if defined(__HIP_DEVICE_COMPILE__)  // one reciprocal for the three quotients when the lanes allow it (same bits)
      const v3 n = normalize_wave(ns);
#else
      const v3 n = normalize(ns);
#endif
      const v3 hp = ray_at(o, t, d);
      if constexpr (RES) {  // read by another wave's shading, maybe on another XCD (ring_flush)
        coherent_store(&geom[pix], make_float4(t, n.x, n.y, n.z));
      } else {
        *reinterpret_cast<float4*>(&geom[pix]) = make_float4(t, n.x, n.y, n.z);
      }
      o = shadow_origin(hp, n);
      d = to_sun();
      t = 0.f;
      it = 0;
      closeness = kInfinity;
      FRM_SUB_END(2);
    }
    if (fin) {  // primary miss (flags 0: BACKGROUND_COLOR) or end of the shadow march
      FRM_SUB_BEGIN();
      const uint32_t flags = ev_shadow ? (kRecHit | (sun_miss ? kRecSunMiss : 0u)) : 0u;
      const uint32_t ck = cost_key(pix_cost);
      const uint2 tail = make_uint2(__float_as_uint(closeness), psteps | flags | (ck << kRecKeyShift));
      if constexpr (RES)
        coherent_store(&tails[pix], tail);
      else
        *reinterpret_cast<uint2*>(&tails[pix]) = tail;
      if constexpr (RES)  // the finished pixel into its slot's count (published by ring_settle)
        atomicAdd(&rw[kRwPend + ring_slot_of(pix, rl_u32(ring_lds->rec_stride))], 1u);
      pix = kIdle;
      FRM_SUB_END(3);
    }
    }  // !lean
    if constexpr (kLeanPass && !kPassMasks) n_bail.add((uint32_t)count(ev_bail));
    if constexpr (RES) {  // drained slots whose last pixels left the lanes
      const uint32_t gone = rw_get(rw, kRwGone);
      if (gone) ring_settle(ring_lds, rw, gone, pix);
    }
    // 2. refill idle lanes from the wave's current chunk; fetch + ray-gen a new chunk
#ifdef FRM_STAMPS
    const uint64_t stamp1 = __builtin_amdgcn_s_memtime();
    stamp_consume += stamp1 - stamp0;
#endif
    const uint64_t want = ballot(pix == kIdle);
    if (want != 0 && !exhausted) {
      if (slots_used == kChunk) {
        uint32_t base = kIdle;
        if constexpr (RES) {
          base = ring_claim(ring_lds, rw, cam_lds, nchunks, nhead, pix, &r_slot);
        } else {
        constexpr drain_t kOne = 1, kAllParts = (drain_t)((1ull << kQueueParts) - 1ull);
        // the head of the order (its most expensive chunks) from the shared counter
        if (!(drained >> kQueueParts)) {
          uint32_t j = 0;
          if (lane == 0) j = atomicAdd(a.queue + kQueueParts * kQueuePartWords, 1u);
          j = uniform(__shfl(j, 0, 64));
          if (j < nhead)
            base = j * kChunk;
          else
            drained |= kOne << kQueueParts;
        }
        // then chunk j of the XCD's partition x is queue chunk nhead + j * kQueueParts + x; a
        // drained partition passes the wave on to the next one
        while (base == kIdle) {
          uint32_t j = 0;
          if (lane == 0) j = atomicAdd(a.queue + part * kQueuePartWords, 1u);
          j = uniform(__shfl(j, 0, 64));
          const uint32_t c = nhead + j * kQueueParts + part;
          if (c < nchunks) {
            base = c * kChunk;
            break;
          }
          drained |= kOne << part;
          if ((drained & kAllParts) == kAllParts) break;
          do part = (part + 1u) % kQueueParts;
          while ((drained >> part) & 1u);
        }
        }  // !RES
#ifdef FRM_STAMPS
        n_fetch++;
#endif
        if (base == kIdle) {
          exhausted = true;
#ifdef FRM_STAMPS
          real_exhaust = __builtin_amdgcn_s_memrealtime();
          if (lane == 0) atomicMin(a.debug + 2, (unsigned long long)real_exhaust);
#endif
        } else {
          // the i-th pixel fetched is pixel_order[i]: most expensive first (the previous
          // frame's cost keys, frm_sched.hip), row-major without history
          uint32_t p = kIdle;
          v3 ray = mk(0.f, 0.f, 0.f);
          uint32_t pos0 = base, lim = total;
          // RES: the chunk's frame's camera rows (wave-uniform, SGPRs): one LDS word per lane, then
          // lane reads (twelve loads into VGPRs before their readfirstlanes pushed the march state
          // into scratch). The load is pinned here, where every lane runs: the compiler would
          // otherwise sink it into the branch below, and a lane read of a lane outside that
          // branch's mask returns garbage.
          [[maybe_unused]] float row[3][4];
          if constexpr (RES) {
            uint32_t mine = __float_as_uint(cam_lds[r_slot][lane & 15u]);
            asm volatile("" : "+v"(mine));
#pragma unroll
            for (int i = 0; i < 12; ++i) row[i / 4][i % 4] = __uint_as_float(__builtin_amdgcn_readlane(mine, i));
          }
          if constexpr (MULTI) {
            const uint32_t c = base / kChunk;
            chunk_frame = uniform(c % a.batch);
            pos0 = (c / a.batch) * kChunk;
            lim = a.npix;
          }
          if (pos0 + lane < lim) {
            const uint32_t lp =
                RES ? dev_load(&rl_ptr(((const volatile RingLds*)ring_lds)->order)[r_slot * a.rec_stride + pos0 + lane])
                    : a.pixel_order[pos0 + lane];
            // (lean-pass kernels: the two divisors as this block's own values, so that the
            // divisions' reciprocals are worked out here, once per chunk, instead of living in
            // VGPRs across the whole march loop, where one of them spilled)
            uint32_t fw = f.width;
            BandGeometry bg = a.g;
            if constexpr (kLeanPass) asm volatile("" : "+s"(fw), "+s"(bg.band_rows));
            const uint32_t lr = lp / fw, x = lp - lr * fw, y = band_row_to_global(bg, lr);
            if constexpr (RES)
              ray = camera_ray_rows(f, row, x, y);
            else if constexpr (MULTI)
              ray = camera_ray_rows(f, a.cams[chunk_frame].row, x, y);
            else
              ray = camera_ray(f, x, y);
            p = (RES ? r_slot * a.rec_stride : chunk_frame * a.rec_stride) + lp;  // the pixel's record index
          }
          if constexpr (!RES) n_pix.add((uint32_t)count(p != kIdle));
          chunk_rays[wave][lane] = make_float4(ray.x, ray.y, ray.z, __uint_as_float(p));
          __builtin_amdgcn_wave_barrier();
          slots_used = 0;
        }
      }
      if (slots_used < kChunk) {
        const uint32_t slot = slots_used + __popcll(want & (lane_bit - 1ull));
        // RES: the chunk's frame's origin and power, read as the camera rows above
        [[maybe_unused]] float cam_o[4];
        if constexpr (RES) {
          uint32_t mine = __float_as_uint(cam_lds[r_slot][12u + (lane & 3u)]);
          asm volatile("" : "+v"(mine));
#pragma unroll
          for (int i = 0; i < 4; ++i) cam_o[i] = __uint_as_float(__builtin_amdgcn_readlane(mine, i));
        }
        if ((want & lane_bit) && slot < kChunk) {
          const float4 r = chunk_rays[wave][slot];
          pix = __float_as_uint(r.w);
          if (pix != kIdle) {
            // the frame's step 0 done once (KernelArgs::first_info; ring frames run it per pixel):
            // start at step 1 where consuming it would leave the pixel
            const uint32_t fy = RES ? 0u : a.first_info[chunk_frame];
            const bool first_skip = (fy & kFirstSkip) != 0u;
            pix_cost = first_skip ? (fy & kFirstCostMask) : 0u;
            d = mk(r.x, r.y, r.z);
            if constexpr (RES)
              o = mk(cam_o[0], cam_o[1], cam_o[2]);
            else
              o = MULTI ? a.cams[chunk_frame].origin : f.origin;
            if constexpr (RES && ANIM)
              lane_power = cam_o[3];
            else if constexpr (ANIM)
              lane_power = a.mb_powers[chunk_frame];
            t = first_skip ? a.first_t[chunk_frame] : 0.f;
            it = first_skip ? 1u : 0u;
            phase = kPrimary;
            need_point = true;
          }
        }
        slots_used = min(kChunk, slots_used + (uint32_t)__popcll(want));
      }
    }

#ifdef FRM_STAMPS
    stamp_refill += __builtin_amdgcn_s_memtime() - stamp1;
#endif
    // 3. start the next DE of every lane that needs one (the hit point of the normal
    //    taps is recomputed from the unchanged primary ray: ray_at(o, t_hit, d))
    if (need_point) {
      const v3 r = ray_at(o, t, d);
      // no tap among the lanes that start a DE (every lean pass: a refill only adds primary
      // lanes): the point itself. Tested here again: the lean flag carried across the refill is a
      // lane mask that the register allocator parks in two VGPR lanes, four lane moves per pass
      // (profiles/round9/sgpr/lean_carry.patch).
      bool no_tap = false;
      if constexpr (kLeanPass) no_tap = ballot(phase - kTap0 <= kTap3 - kTap0) == 0;
      if (no_tap) {
        q = r;
      } else if constexpr (kTapOffset) {
        // The same point without the three final selects: a lane that is no tap adds -0.0f, which
        // leaves every x its bits (both zeros included; a NaN stays a NaN). A tap adds
        // +-MIN_DISTANCE with the sign bit looked up by the phase in a six-entry bit table
        // (entries 0 and 5, the march phases, are the -0.0f's sign): a shift and a v_lshl_or each
        // instead of the compare pairs. x is negative for taps 1 and 2, y for 0 and 1, z for 0 and 2.
        const bool is_tap = phase - kTap0 <= kTap3 - kTap0;
        const uint32_t e = is_tap ? __float_as_uint(kMinDistance) : 0u;
        constexpr uint32_t kNegX = 0x2Du, kNegY = 0x27u, kNegZ = 0x2Bu;  // bit `phase`: the offset is negative
        q = mk(r.x + __uint_as_float(((kNegX >> phase) << 31) | e), r.y + __uint_as_float(((kNegY >> phase) << 31) | e),
               r.z + __uint_as_float(((kNegZ >> phase) << 31) | e));
      } else {
        // normal tap k samples r + s_k * MIN_DISTANCE (normal_tap_pos), with selects
        const uint32_t kq = phase - kTap0;
        const bool is_tap = kq <= kTap3 - kTap0;
        const float e = kMinDistance;
        const float ex = (kq == 0u || kq == 3u) ? e : -e, ey = (kq >= 2u) ? e : -e, ez = (kq == 1u || kq == 3u) ? e : -e;
        q = mk(is_tap ? r.x + ex : r.x, is_tap ? r.y + ey : r.y, is_tap ? r.z + ez : r.z);
      }
      if constexpr (kMb) {
        z = q;
        dr = 1.f;
        left = n_iter;
        mag = mb_length<kHw>(q);
        if constexpr (!kPassMasks) done = mag > su.mb_bailout;
      } else {
        DeCount unused = {0u, 0u};
        de = scene_de<FAM, ITERS>(su, q, unused);
        done = true;
        pix_cost++;  // fixed-trip families: the scheduling cost unit is one DE
      }
    }
    // kPassMasks: the DEs that bailed out at entry, one compare by every lane outside the branch
    // (a mask assigned inside it joins the other path's through a VGPR, and so does one combined
    // with need_point). The other lanes need no masking: a lane that holds a pixel here and did
    // not start a DE was still pending when the body loop left, so its magnitude is not above the
    // bailout (the loop retires such a lane at once), and a consumed lane either started a DE or
    // gave up its pixel.
    if constexpr (kPassMasks) done_m = ballot(mag > su.mb_bailout);

    // work counters (frm_stats); a ring grid's frames report none (frm_render with stats renders
    // outside the ring), so it keeps no counters
    if constexpr (!RES && !kLeanPass) {
      n_prim.add((uint32_t)count(ev_prim));
      n_hit.add((uint32_t)count(ev_hit));
      n_shadow.add((uint32_t)count(ev_shadow));
      n_bail.add((uint32_t)count(ev_bail));
    }
#ifdef FRM_STAMPS
    stamp_service += __builtin_amdgcn_s_memtime() - stamp0;
    n_service++;
#endif

    if (exhausted && ballot(pix != kIdle) == 0) break;
  }
  if constexpr (RES) {
#pragma unroll
    for (uint32_t sl = 0; sl < kRingSlots; ++sl)
      if (sl < a.ring.slots) ring_flush(ring_lds, rw, sl);
  }

#ifdef FRM_STAMPS
  if (lane == 0) {
    atomicAdd(&a.counters[7], (unsigned long long)stamp_service);
    atomicAdd(a.debug, (unsigned long long)(__builtin_amdgcn_s_memtime() - stamp_begin));
    atomicAdd(a.debug + 1, (unsigned long long)n_service);
    atomicMin(a.debug + 3, (unsigned long long)stamp_real0);  // first wave start (100 MHz)
    atomicMax(a.debug + 4, (unsigned long long)__builtin_amdgcn_s_memrealtime());  // last wave end
  }
  {
    const uint32_t w = blockIdx.x * kMarchWaves + wave;
    uint32_t hw = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    if (lane == 0 && w < kWaveDebugSlots) {
      unsigned long long* r = g_wave_debug + 16u * w;
      r[8] = stamp_consume;
      r[9] = stamp_refill;
      r[10] = n_fetch;
      for (int k = 0; k < 4; ++k) r[11 + k] = stamp_sub[k];
      r[15] = n_lean;  // service passes that took the lean path
      r[0] = n_loop;
      r[1] = n_body.value();
      r[2] = n_service;
      r[3] = stamp_service;
      r[4] = __builtin_amdgcn_s_memtime() - stamp_begin;
      r[5] = stamp_real0;
      r[6] = real_exhaust;
      r[7] = ((unsigned long long)hw << 32) | (uint32_t)(__builtin_amdgcn_s_memrealtime() - stamp_real0);
    }
  }
#endif
  if (lane == 0 && !RES) {
#ifdef FRM_COUNT_EXACT
    atomicAdd(&a.counters[7], (unsigned long long)((n_dbg_total << 32) | n_dbg_exact));
#endif
    // the counts without the debug start value, in 64 bits; the value is read again here (a
    // volatile load of the kernel argument) so that it holds no register across the loops
    typedef const volatile __attribute__((address_space(4))) KernelArgs* kernarg_ptr;
    const uint64_t c0 = ((kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr())->counter_start;
    const uint64_t c_hit = n_hit.value() - c0;
    uint64_t c_prim = n_prim.value() - c0, c_body = n_body.value() - c0, c_bail = n_bail.value() - c0;
    if (blockIdx.x == 0 && wave == 0) {  // the launch's skipped steps 0 (KernelArgs::first_counts)
      c_prim += a.first_counts[0];
      c_body += a.first_counts[1];
      c_bail += a.first_counts[2];
    }
    unsigned long long v[7] = {n_pix.value() - c0, c_hit, c_prim, n_shadow.value() - c0, 4ull * c_hit, c_body, c_bail};
#pragma unroll
    for (int k = 0; k < 7; ++k)
      if (v[k]) atomicAdd(&a.counters[k], v[k]);
  }
}

// Exclusive prefix sum over the 256 threads of a block (4 waves), one value per thread.
__device__ __forceinline__ uint32_t block_exclusive_scan256(uint32_t v, uint32_t* wave_tot) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t inc = wave_inclusive_scan(v);
  if (lane == 63u) wave_tot[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (uint32_t w = 0; w < wave; ++w) before += wave_tot[w];
  return before + inc - v;
}

// The shading of one pixel's records (fragment.wgsl:333-348 + the Rgba8UnormSrgb store).
template <uint32_t FAM>
__device__ __forceinline__ void shade_record(const KernelArgs& a, uint2 r1, uint32_t rec, uint32_t fr, uint32_t idx,
                                             uint32_t x, uint32_t y, const float* table) {
  uint32_t word = 255u << 24;  // miss: BACKGROUND_COLOR
  if (r1.y & kRecHit) {
    const float4 r0 = *reinterpret_cast<const float4*>(&a.geom[rec]);
    const bool multi = a.batch > 1u;
    const v3 dir = multi ? camera_ray_rows(a.f, a.cams[fr].row, x, y) : camera_ray(a.f, x, y);
    const v3 hp = ray_at(multi ? a.cams[fr].origin : a.f.origin, r0.x, dir);
    const v3 n = mk(r0.y, r0.z, r0.w);
    float spec;
    v3 color = shade_hit_pre(a.f, scene_color<FAM>(hp), dir, n, r1.y & kRecStepsMask, &spec);
    color = shade_hit_post(color, spec, (r1.y & kRecSunMiss) ? -kInfinity : 0.0f, __uint_as_float(r1.x));
    word = pack_rgba(color, table);
  }
  a.out[(size_t)fr * a.out_stride + idx] = word;
}

// Coherent shading of the records written by march_persistent: fragment.wgsl:333-348
// (+ the Rgba8UnormSrgb store). A block shades kShadeBlockPixels local pixels, row-major, 256
// at a time (coalesced). With fused scheduling (KernelArgs::key_hist) it also counts the cost
// keys of the launch's last frame (an LDS histogram per block, one global add per key present:
// few blocks, so few adds on the hot keys' counters) and resets the slot's next launch.
template <uint32_t FAM>
__global__ __launch_bounds__(256) void shade_pass(KernelArgs a) {
  __shared__ float table[256];
  __shared__ uint32_t s_count[256];
  const uint32_t t = threadIdx.x;
  const uint32_t fr = blockIdx.y;  // frame of a multi-frame launch (0 otherwise)
  // fused scheduling: the key histogram of the launch's last frame (block-uniform)
  const bool hist = a.key_hist != nullptr && fr + 1u == a.batch;
  table[t] = kSrgbThresholds[t];
  if (hist) s_count[t] = 0u;
  __syncthreads();
  const uint32_t width = a.f.width, local = a.g.local_rows * width;
  for (uint32_t j = 0; j < kShadeBlockPixels / 256u; ++j) {
    const uint32_t idx = (blockIdx.x * (kShadeBlockPixels / 256u) + j) * 256u + t;
    if (idx >= local) break;
    const uint32_t lr = idx / width, x = idx - lr * width;
    const uint32_t y = band_row_to_global(a.g, lr);
    if (y >= a.f.height) break;  // the short last band's missing rows: the launch's last local rows
    const uint32_t rec = fr * a.rec_stride + idx;
    const uint2 r1 = *reinterpret_cast<const uint2*>(&a.tails[rec]);
    const uint32_t key = r1.y >> kRecKeyShift;
    // coalesced, for the next launch's order (a multi-frame launch: its last frame's costs)
    if (a.pixel_key && fr + 1u == a.batch) a.pixel_key[idx] = (uint8_t)key;
    if (hist) atomicAdd(&s_count[key], 1u);
    shade_record<FAM>(a, r1, rec, fr, idx, x, y, table);
  }
  if (!hist) return;
  __syncthreads();
  if (const uint32_t c = s_count[t]) atomicAdd(a.key_hist + t, c);
  if (blockIdx.x == 0) {  // the slot's next launch starts from zeroed counts, cursors and queue
    a.key_hist_next[t] = 0u;
    a.key_hist_next[256u + t] = 0u;
    for (uint32_t w = t; w < kQueueDebugWord; w += 256u) a.queue[w] = 0u;
  }
}

// Fused scheduling, after shade_pass: the next launch's fetch order, the local pixels by descending
// cost key (an 8-bit counting sort: bucket bases from the shading pass's histogram, one range per
// block and bucket reserved through the cursors key_hist[256..511], the block's kShadeBlockPixels
// pixels ranked in LDS). Ties are ordered by block, then as the LDS atomics happen to run: the
// order places pixels on lanes, it never changes a pixel's bytes.
__global__ __launch_bounds__(256) void rank_pass(const uint8_t* __restrict__ keys, uint32_t npix,
                                                 uint32_t* __restrict__ hist, uint32_t* __restrict__ order) {
  constexpr uint32_t kPer = kShadeBlockPixels / 256u;
  __shared__ uint32_t s_base[256], s_count[256], s_res[256], s_wave[4];
  const uint32_t t = threadIdx.x;
  s_count[t] = 0u;
  __syncthreads();
  uint32_t key[kPer], rank[kPer];
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) {
    const uint32_t idx = (blockIdx.x * kPer + j) * 256u + t;
    key[j] = idx < npix ? keys[idx] : 0u;
    rank[j] = idx < npix ? atomicAdd(&s_count[key[j]], 1u) : 0u;
  }
  // bucket bases in descending key order: base[k] = pixels with a key above k
  const uint32_t k_desc = 255u - t;
  s_base[k_desc] = block_exclusive_scan256(hist[k_desc], s_wave);  // its barrier completes s_count
  const uint32_t c = s_count[t];
  s_res[t] = c ? atomicAdd(hist + 256u + t, c) : 0u;
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < kPer; ++j) {
    const uint32_t idx = (blockIdx.x * kPer + j) * 256u + t;
    const uint32_t pos = s_base[key[j]] + s_res[key[j]] + rank[j];
    if (idx < npix && pos < npix) order[pos] = idx;  // pos < npix always, for a histogram of these keys
  }
}

}  // namespace frm
