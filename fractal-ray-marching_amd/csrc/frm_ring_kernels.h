// frm_ring_kernels.h — the resident frame ring's device side (frm_internal.h RingArgs; host side:
// frm_ring.hip): the coherence helpers, the march waves' claims from the ring's frames (ring_claim,
// ring_settle, ring_flush) and the service waves that shade, rank and publish them (ring_service).
// march_persistent<..., RES = true> (frm_render_kernels.h) is the ring's grid and the only user.
//
// It uses the wave helpers at the top of frm_render_kernels.h, which includes this file right
// below them. Included on its own, this file therefore goes through that header first, and it is
// that header's include of this file that defines the ring (hence the include ahead of the guard).
// Project headers only: the run-time compiler (frm_reload.hip) has no system headers.
#include "frm_render_kernels.h"
#ifndef FRM_RING_KERNELS_H
#define FRM_RING_KERNELS_H

namespace frm {

// The ring's memory is shared by waves on different XCDs, whose L2s are not coherent with each
// other, and with the host. The rules the code below follows:
//  * counters and flags are only touched by atomics, which are performed at the coherence point;
//    a poll is an atomic fetch (never a load that an acquire would have to make fresh: an acquire
//    invalidates the wave's whole L2, and polling with acquire loads ran the ring 3.5x slower);
//  * data one wave writes for another (records, cost keys, fetch orders) is stored with agent-scope
//    stores, which write through the L2, and the writer waits for its stores (ring_wait_mem) before
//    the atomic that publishes them;
//  * such data is read with agent-scope loads, which never return a stale line of the reader's
//    XCD L2 (an acquire fence instead invalidates that whole L2: one per shade/rank task and per
//    frame a march wave entered, ~10^4 per frame, slowed every wave on the XCD);
//  * host memory (RingHost: posted, descriptors; zero-copy images) is uncached: system-scope loads
//    and stores, ordered by waiting.
__device__ __forceinline__ uint32_t sys_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void sys_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
template <class T>
__device__ __forceinline__ T dev_poll(T* p) {
  return __hip_atomic_fetch_add(p, (T)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ T dev_load(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ void dev_store(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Waits until this wave's memory accesses so far have completed.
__device__ __forceinline__ void ring_wait_mem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ uint64_t realtime() { return __builtin_amdgcn_s_memrealtime(); }  // 100 MHz
constexpr uint64_t kRingWatchdogTicks = 200000000ull;  // 2 s of the 100 MHz clock without progress
constexpr unsigned long long kEpochMask = 0xFFFFFFFF00000000ull;
__device__ __forceinline__ unsigned long long epoch_of(uint32_t seq) { return (unsigned long long)seq << 32; }
#ifdef FRM_RING_TRACE
#define RING_TRACE_MIN(r, seq, k) atomicMin(&(r).dev->trace[(seq) & 63u][k], (unsigned long long)realtime())
#define RING_TRACE_MAX(r, seq, k) atomicMax(&(r).dev->trace[(seq) & 63u][k], (unsigned long long)realtime())
#define RING_GRID_TRACE(r, k) atomicMin(&(r).dev->grid_trace[(r).grid_id & 63u][k], (unsigned long long)realtime())
#else
#define RING_TRACE_MIN(r, seq, k)
#define RING_TRACE_MAX(r, seq, k)
#define RING_GRID_TRACE(r, k)
#endif
__device__ __forceinline__ RingFrameCtl& ring_ctl(const RingArgs& r, uint32_t seq) {
  return r.dev->set[(seq - 1u) & (2u * r.slots - 1u)];
}
// The ring arguments a march wave needs, kept in LDS and read (volatile) where they are used: held
// in kernel-argument SGPRs for the whole march loop they pushed its SGPRs into VGPR lanes and those
// into scratch, reloaded on every service pass (the ring ran at 60 % of the batched march's rate).
struct RingLds {
  RingHost* host;
  RingDev* dev;
  uint32_t* order;
  uint32_t slots, grid_id, rec_stride, npix;
};
__device__ __forceinline__ uint32_t rl_u32(const volatile uint32_t& v) { return uniform(v); }
template <class T>
__device__ __forceinline__ T* rl_ptr(T* const volatile& v) {
  const uint64_t x = reinterpret_cast<uint64_t>(v);
  return reinterpret_cast<T*>((uint64_t)uniform((uint32_t)x) | ((uint64_t)uniform((uint32_t)(x >> 32)) << 32));
}
// The march-path view of the ring arguments (see RingLds), fields read at this point.
__device__ __forceinline__ RingArgs ring_view(const volatile RingLds* rl) {
  RingArgs r;
  r.host = rl_ptr(rl->host);
  r.dev = rl_ptr(rl->dev);
  r.order = rl_ptr(rl->order);
  r.slots = rl_u32(rl->slots);
  r.grid_id = rl_u32(rl->grid_id);
  r.first_seq = 0;
  r.service_waves = 0;
  r.out = nullptr;
  r.keys = nullptr;
  return r;
}

// Lane 0 adds v to an epoch-tagged counter of frame `seq` (frm_internal.h RingFrameCtl); broadcast:
// the count before the add, or ~0u when the word counts another frame.
__device__ __forceinline__ uint32_t epoch_add(unsigned long long* w, uint32_t seq, uint32_t v) {
  unsigned long long old = 0;
  if ((threadIdx.x & 63u) == 0) old = atomicAdd(w, (unsigned long long)v);
  old = __shfl(old, 0, 64);
  return (old & kEpochMask) == epoch_of(seq) ? (uint32_t)old : 0xFFFFFFFFu;
}
// A claim of one of n items: its index, or ~0u (all claimed, or another frame's counter).
__device__ __forceinline__ uint32_t epoch_claim(unsigned long long* w, uint32_t seq, uint32_t n) {
  const uint32_t t = epoch_add(w, seq, 1u);
  return t < n ? t : 0xFFFFFFFFu;
}

// The frames a grid may serve: those up to min(posted, grid_stop - 1), and after the grid has
// closed (a march wave found nothing left to claim), those up to the limit its closer fixed.
struct RingView {
  uint32_t limit;  // the last seq this wave knows it may serve
  bool closed;     // `limit` is the grid's final limit
};
__device__ __forceinline__ void ring_refresh(const RingArgs& r, RingView& v) {
  if (v.closed) return;
  uint32_t lim = 0, closed = 0;
  if ((threadIdx.x & 63u) == 0) {
    closed = dev_poll(&r.dev->grid.limit_valid);
    if (closed) {
      lim = dev_poll(&r.dev->grid.limit);
    } else {
      const uint32_t posted = sys_load(&r.host->posted);
      const uint32_t stop = sys_load(&r.host->grid_stop[r.grid_id % kRingGridIds][0]);
      lim = min(posted, stop - 1u);
#ifdef FRM_RING_TRACE
      if (lim >= 1u) RING_TRACE_MIN(r, lim, 0);
#endif
    }
  }
  v.closed = uniform(__shfl(closed, 0, 64)) != 0;
  v.limit = uniform(__shfl(lim, 0, 64));
}
// A march wave with nothing left to claim up to v.limit closes the grid: the first to get there
// publishes `closed` to the host, waits for that store, reads `posted` once more and fixes the last
// frame the grid serves; every other wave waits for that limit. Frames posted later belong to the
// next grid, which the host launches when it sees `closed` after its own post (frm_ring.hip
// ring_render: each side stores, then loads the other's word, so one of them sees the other's store).
__device__ __forceinline__ void ring_close(const RingArgs& r, RingView& v) {
  uint32_t lim = 0, ok = 1;
  if ((threadIdx.x & 63u) == 0) {
    if (atomicCAS(&r.dev->grid.closed, 0u, 1u) == 0u) {
      sys_store(&r.host->closed, r.grid_id);
      RING_GRID_TRACE(r, 1);
      ring_wait_mem();
      const uint32_t posted = sys_load(&r.host->posted);
      const uint32_t stop = sys_load(&r.host->grid_stop[r.grid_id % kRingGridIds][0]);
      lim = min(posted, stop - 1u);
      atomicExch(&r.dev->grid.limit, lim);
      atomicExch(&r.dev->base, lim + 1u);
      ring_wait_mem();
      atomicExch(&r.dev->grid.limit_valid, 1u);
    } else {
      const uint64_t t0 = realtime();
      while (!dev_poll(&r.dev->grid.limit_valid)) {
        if (realtime() - t0 > 1000000ull) { ok = 0; break; }  // 10 ms: the closer stalled; stop here
        __builtin_amdgcn_s_sleep(2);
      }
      lim = dev_poll(&r.dev->grid.limit);
    }
  }
  v.closed = true;
  v.limit = uniform(__shfl(ok ? lim : 0u, 0, 64));
}

// The camera (and zero-copy image) of ring frame slot `slot`, from its RingFrame in host memory.
struct RingCam {
  float row[3][4];
  v3 origin;
  float power;
  uint32_t* host_img;
};
// The first 16 words of the RingFrame (camera rows, origin, power) into LDS (march waves).
__device__ __forceinline__ void ring_camera_lds(const RingArgs& r, uint32_t slot, float* lds) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&r.host->frames[slot]);
  const uint32_t lane = threadIdx.x & 63u;
  if (lane < 16u) lds[lane] = __uint_as_float(sys_load(w + lane));
  __syncthreads();  // one-wave workgroup: orders the LDS accesses
}
__device__ __forceinline__ RingCam ring_camera(const RingArgs& r, uint32_t slot) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&r.host->frames[slot]);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t mine = lane < 20u ? sys_load(w + lane) : 0u;  // row[12], origin[3], power, seq, pad, host_img
  RingCam c;
#pragma unroll
  for (int i = 0; i < 12; ++i) c.row[i / 4][i % 4] = __uint_as_float(uniform(__shfl(mine, i, 64)));
  c.origin = mk(__uint_as_float(uniform(__shfl(mine, 12, 64))), __uint_as_float(uniform(__shfl(mine, 13, 64))),
                __uint_as_float(uniform(__shfl(mine, 14, 64))));
  c.power = __uint_as_float(uniform(__shfl(mine, 15, 64)));
  const uint64_t lo = uniform(__shfl(mine, 18, 64)), hi = uniform(__shfl(mine, 19, 64));
  c.host_img = reinterpret_cast<uint32_t*>(lo | (hi << 32));
  return c;
}

// A ring march wave's claim state, all of it in LDS (SGPRs and VGPRs are the march's): the oldest
// frame it has not drained, the grid's frames as it last saw them, and per slot the frame the slot's
// state belongs to, its camera, its queue drain state and the pixels of that frame whose march
// ended in this wave and that the frame's pix_done does not count yet; and the slots whose frames
// the wave has drained. A slot's count goes out once the wave has drained the frame (it never
// claims from it again) and none of its lanes holds a pixel of it (ring_settle), so a frame's count
// completes only after every wave is done with it.
enum RingWaveWord : uint32_t {
  kRwLo = 0,       // the oldest frame the wave has not drained
  kRwLimit,        // the grid's frames as this wave last saw them (RingView)
  kRwClosed,
  kRwSeqOf,        // + slot: the frame the slot's state (camera, drain state) belongs to
  kRwPart = kRwSeqOf + kRingSlots,       // + slot: the queue partition the wave claims from
  kRwDrainLo = kRwPart + kRingSlots,     // + slot: drained partitions (bits 0..31; bit kQueueParts: the head)
  kRwDrainHi = kRwDrainLo + kRingSlots,  // + slot: high half
  kRwPend = kRwDrainHi + kRingSlots,     // + slot: finished pixels not yet added to pix_done
  kRwGone = kRwPend + kRingSlots,        // bit s: the wave has drained slot s's frame
  kRwWords
};
__device__ __forceinline__ uint32_t rw_get(const uint32_t* rw, uint32_t i) { return uniform(rw[i]); }
__device__ __forceinline__ void rw_set(uint32_t* rw, uint32_t i, uint32_t v) {
  if ((threadIdx.x & 63u) == 0) rw[i] = v;
}
// Records of a ring frame are read by the service waves' shading, maybe on another XCD: written
// through (agent-scope stores) and waited for (ring_add_done) before their pixels are counted, and
// read with agent-scope loads (never from a stale line of the reader's L2).
__device__ __forceinline__ void coherent_store(ShadeTail* p, uint2 v) {
  dev_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v.x | ((unsigned long long)v.y << 32));
}
__device__ __forceinline__ void coherent_store(ShadeGeom* p, float4 v) {
  unsigned long long* w = reinterpret_cast<unsigned long long*>(p);
  dev_store(w, (unsigned long long)__float_as_uint(v.x) | ((unsigned long long)__float_as_uint(v.y) << 32));
  dev_store(w + 1, (unsigned long long)__float_as_uint(v.z) | ((unsigned long long)__float_as_uint(v.w) << 32));
}
__device__ __forceinline__ uint2 coherent_load(const ShadeTail* p) {
  const unsigned long long v = dev_load(reinterpret_cast<const unsigned long long*>(p));
  return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}
__device__ __forceinline__ float4 coherent_load(const ShadeGeom* p) {
  const unsigned long long* w = reinterpret_cast<const unsigned long long*>(p);
  const unsigned long long lo = dev_load(w), hi = dev_load(w + 1);
  return make_float4(__uint_as_float((uint32_t)lo), __uint_as_float((uint32_t)(lo >> 32)), __uint_as_float((uint32_t)hi),
                     __uint_as_float((uint32_t)(hi >> 32)));
}
// Adds n finished pixels to frame seq's pix_done, after the wave's record stores have completed.
__device__ __forceinline__ void ring_add_done(const volatile RingLds* rl, uint32_t seq, uint32_t n) {
  ring_wait_mem();
  const RingArgs r = ring_view(rl);
  const uint32_t before = epoch_add(&ring_ctl(r, seq).pix_done[0], seq, n);
#ifdef FRM_RING_TRACE
  if (before + n == rl_u32(rl->npix) && (threadIdx.x & 63u) == 0) RING_TRACE_MIN(r, seq, 3);
#else
  (void)before;
#endif
}
// Slot s's finished pixels into its frame's pix_done (see ring_settle).
__device__ __forceinline__ void ring_flush(const volatile RingLds* rl, uint32_t* rw, uint32_t s) {
  const uint32_t n = rw_get(rw, kRwPend + s);
  if (n) {
    ring_add_done(rl, rw_get(rw, kRwSeqOf + s), n);
    rw_set(rw, kRwPend + s, 0u);
  }
}
// A slot the wave has drained (bit s of kRwGone) whose pixels have all left its lanes (pix: the
// lanes' pixels now) is settled: its count goes out and the bit clears, once per wave and frame.
// (Counts added at every claim and every finished pixel of a drained frame were an atomic on one
// word per service pass of every wave, each behind a wait for the wave's stores: the ring marched
// at 60 % of the batched rate.)
__device__ __forceinline__ void ring_settle(const volatile RingLds* rl, uint32_t* rw, uint32_t gone, uint32_t pix) {
  const uint32_t rs = rl_u32(rl->rec_stride);
#pragma unroll
  for (uint32_t sl = 0; sl < kRingSlots; ++sl) {
    if (!((gone >> sl) & 1u) || ballot(pix - sl * rs < rs) != 0) continue;
    ring_flush(rl, rw, sl);
    rw_set(rw, kRwGone, rw_get(rw, kRwGone) & ~(1u << sl));
  }
}
// The slot of a record index (slot * rec_stride + local pixel; at most kRingSlots slots).
__device__ __forceinline__ uint32_t ring_slot_of(uint32_t pix, uint32_t rs) {
  return (uint32_t)(pix >= rs) + (uint32_t)(pix >= 2u * rs) + (uint32_t)(pix >= 3u * rs);
}
// One claim from frame seq's queue (slot s): the head of its order first, then the partitions, as
// the single-frame claim. Returns the chunk's first fetch position or kIdle (drained for this wave).
__device__ __forceinline__ uint32_t ring_claim_frame(const RingArgs& r, uint32_t* rw, uint32_t seq, uint32_t s,
                                                     uint32_t nchunks, uint32_t nhead) {
  unsigned long long* q = ring_ctl(r, seq).queue;
  constexpr uint32_t kW = kQueuePartWords / 2u;
  uint64_t drained = (uint64_t)rw_get(rw, kRwDrainLo + s) | ((uint64_t)rw_get(rw, kRwDrainHi + s) << 32);
  uint32_t part = rw_get(rw, kRwPart + s);
  uint32_t base = kIdle;
  if (!(drained >> kQueueParts)) {
    const uint32_t j = epoch_claim(q + kQueueParts * kW, seq, nhead);
    if (j != kIdle)
      base = j * kChunk;
    else
      drained |= 1ull << kQueueParts;
  }
  while (base == kIdle) {
    // partition `part` holds chunks nhead + j * kQueueParts + part below nchunks
    const uint32_t jmax = nchunks > nhead + part ? (nchunks - nhead - part + kQueueParts - 1u) / kQueueParts : 0u;
    const uint32_t j = jmax ? epoch_claim(q + part * kW, seq, jmax) : kIdle;
    if (j != kIdle) {
      base = (nhead + j * kQueueParts + part) * kChunk;
      break;
    }
    drained |= 1ull << part;
    if ((drained & ((1ull << kQueueParts) - 1ull)) == (1ull << kQueueParts) - 1ull) break;
    do part = (part + 1u) % kQueueParts;
    while ((drained >> part) & 1u);
  }
  rw_set(rw, kRwDrainLo + s, (uint32_t)drained);
  rw_set(rw, kRwDrainHi + s, (uint32_t)(drained >> 32));
  rw_set(rw, kRwPart + s, part);
  return base;
}
// The claim's rare steps, as calls (inlined, their registers pushed the march state into scratch):
// a new look at the grid's frames (and closing it), and the wave's first claim from a frame.
__device__ __noinline__ void ring_update_view(const volatile RingLds* rl, uint32_t* rw, uint32_t lo) {
  const RingArgs r = ring_view(rl);
  RingView v = {rw_get(rw, kRwLimit), rw_get(rw, kRwClosed) != 0};
  ring_refresh(r, v);
  if (lo > v.limit && !v.closed) ring_close(r, v);
  rw_set(rw, kRwLimit, v.limit);
  rw_set(rw, kRwClosed, v.closed ? 1u : 0u);
  __builtin_amdgcn_wave_barrier();
}
__device__ __noinline__ void ring_enter_frame(const volatile RingLds* rl, uint32_t* rw, float* cam, uint32_t s,
                                              uint32_t f) {
  const RingArgs r = ring_view(rl);
  ring_camera_lds(r, s, cam);
  rw_set(rw, kRwSeqOf + s, f);
  rw_set(rw, kRwDrainLo + s, 0u);
  rw_set(rw, kRwDrainHi + s, 0u);
  rw_set(rw, kRwPart + s, queue_part());
  __builtin_amdgcn_wave_barrier();
}
// The next chunk for a ring march wave. Returns the chunk's first fetch position (kIdle: nothing
// left for this grid) and its slot (*out_slot); the slot's camera is in cam_lds[slot].
// Frames in posting order: the wave claims from the oldest frame it has not drained and moves on
// when that frame's queue is empty for it. Each frame's claims thus end while the next frame still
// has most of its chunks, so the frame completes (is shaded and published, its slot freed) while
// the grid marches the next one, and the host posts the frame after that before the grid runs
// dry: with two slots the grid never closes in a steady loop. (Round-robin claims over the posted
// frames drained two frames together, as a 2-frame multi-frame launch: the grid then closed after
// every pair and paid a drain per pair; measured no faster.)
__device__ __forceinline__ uint32_t ring_claim(const volatile RingLds* rl, uint32_t* rw, float (*cam_lds)[16],
                                               uint32_t nchunks, uint32_t nhead, uint32_t pix, uint32_t* out_slot) {
  const uint32_t R = rl_u32(rl->slots);
  for (;;) {
    const uint32_t f = rw_get(rw, kRwLo);
    if (f > rw_get(rw, kRwLimit)) {
      ring_update_view(rl, rw, f);
      if (f > rw_get(rw, kRwLimit)) return kIdle;  // nothing left for this grid
    }
    const uint32_t s = (f - 1u) & (R - 1u);
    if (rw_get(rw, kRwSeqOf + s) != f) {  // the wave's first claim from frame f
      ring_enter_frame(rl, rw, cam_lds[s], s, f);
      rw_set(rw, kRwGone, rw_get(rw, kRwGone) & ~(1u << s));
    }
    const RingArgs r = ring_view(rl);
    const uint32_t base = ring_claim_frame(r, rw, f, s, nchunks, nhead);
    if (base != kIdle) {
#ifdef FRM_RING_TRACE
      if ((threadIdx.x & 63u) == 0) {
        RING_TRACE_MIN(r, f, 1);
        RING_TRACE_MAX(r, f, 2);
      }
#endif
      *out_slot = s;
      return base;
    }
    rw_set(rw, kRwGone, rw_get(rw, kRwGone) | (1u << s));  // drained for this wave: it never claims from frame f again
    ring_settle(rl, rw, 1u << s, pix);
    rw_set(rw, kRwLo, f + 1u);
  }
}

// Wave-wide exclusive prefix sum of one value per lane.
__device__ __forceinline__ uint32_t wave_exclusive_scan(uint32_t v) { return wave_inclusive_scan(v) - v; }

// Shade task t of ring frame `seq` (slot s): kRingTaskPixels local pixels, 64 at a time, as
// shade_pass (fragment.wgsl:333-348 + the Rgba8UnormSrgb store) with the frame's ring camera; the
// cost keys go out for the slot's next fetch order and into the frame's key histogram.
template <uint32_t FAM>
__device__ void ring_shade_task(const KernelArgs& a, const RingCam& cam, uint32_t seq, uint32_t s, uint32_t t,
                                const float* table, uint32_t* cnt) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t width = a.f.width, npix = a.npix, rs = a.rec_stride;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) cnt[lane * 4u + k] = 0u;
  __syncthreads();  // one-wave workgroup: orders the LDS accesses
  for (uint32_t j = 0; j < kRingTaskPixels / 64u; ++j) {
    const uint32_t idx = t * kRingTaskPixels + j * 64u + lane;
    if (idx >= npix) break;
    const uint32_t lr = idx / width, x = idx - lr * width;
    const uint32_t y = band_row_to_global(a.g, lr);
    const uint32_t rec = s * rs + idx;
    const uint2 r1 = coherent_load(&a.tails[rec]);
    const uint32_t key = r1.y >> kRecKeyShift;
    dev_store(&a.ring.keys[rec], (uint8_t)key);
    atomicAdd(&cnt[key], 1u);
    uint32_t word = 255u << 24;  // miss: BACKGROUND_COLOR
    if (r1.y & kRecHit) {
      const float4 r0 = coherent_load(&a.geom[rec]);
      const v3 dir = camera_ray_rows(a.f, cam.row, x, y);
      const v3 hp = ray_at(cam.origin, r0.x, dir);
      const v3 n = mk(r0.y, r0.z, r0.w);
      float spec;
      v3 color = shade_hit_pre(a.f, scene_color<FAM>(hp), dir, n, r1.y & kRecStepsMask, &spec);
      color = shade_hit_post(color, spec, (r1.y & kRecSunMiss) ? -kInfinity : 0.0f, __uint_as_float(r1.x));
      word = pack_rgba(color, table);
    }
    a.ring.out[rec] = word;
    if (cam.host_img) cam.host_img[idx] = word;  // zero-copy readback (pinned host image)
  }
  __syncthreads();
  uint32_t* hist = ring_ctl(a.ring, seq).hist;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k)
    if (const uint32_t c = cnt[lane * 4u + k]) atomicAdd(&hist[lane * 4u + k], c);
}

// Rank task t of ring frame `seq` (slot s): kRingTaskPixels local pixels into the slot's next fetch
// order, by descending cost key (rank_pass's counting sort: bucket bases from the frame's complete
// histogram, a range per task and key reserved through the cursors hist[256..511]; a pixel's place in
// its range from an LDS atomic on a second pass over the keys). Placement only: never a pixel's bytes.
__device__ __forceinline__ void ring_rank_task(const KernelArgs& a, uint32_t seq, uint32_t s, uint32_t t,
                                               uint32_t* cnt) {
  const uint32_t lane = threadIdx.x & 63u, npix = a.npix, rs = a.rec_stride;
  const uint8_t* keys = a.ring.keys + (size_t)s * rs;
  uint32_t* order = a.ring.order + (size_t)s * rs;
  uint32_t* hist = ring_ctl(a.ring, seq).hist;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) cnt[lane * 4u + k] = 0u;
  __syncthreads();
  for (uint32_t j = 0; j < kRingTaskPixels / 64u; ++j) {
    const uint32_t idx = t * kRingTaskPixels + j * 64u + lane;
    if (idx >= npix) break;
    atomicAdd(&cnt[dev_load(&keys[idx])], 1u);
  }
  __syncthreads();
  // descending key order: lane l holds keys 255 - 4l .. 252 - 4l; base[k] = pixels with a key above
  // k plus this task's reserved offset in bucket k
  uint32_t h[4], sum = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    h[i] = dev_load(&hist[255u - (lane * 4u + i)]);
    sum += h[i];
  }
  uint32_t before = wave_exclusive_scan(sum);
  uint32_t b[4];
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    const uint32_t k = 255u - (lane * 4u + i);
    const uint32_t c = cnt[k];
    b[i] = before + (c ? atomicAdd(&hist[256u + k], c) : 0u);
    before += h[i];
  }
  __syncthreads();  // every lane has read its counts: the array now takes the bases
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) cnt[255u - (lane * 4u + i)] = b[i];
  __syncthreads();
  for (uint32_t j = 0; j < kRingTaskPixels / 64u; ++j) {
    const uint32_t idx = t * kRingTaskPixels + j * 64u + lane;
    if (idx >= npix) break;
    const uint32_t pos = atomicAdd(&cnt[dev_load(&keys[idx])], 1u);
    if (pos < npix) dev_store(&order[pos], idx);  // always, for a histogram of these keys
  }
}

// Every task of ring frame `seq` (slot s) is done: set up the counters of frame seq + slots (its
// epoch, zero counts, histogram and cursors), then publish the frame.
__device__ __forceinline__ void ring_finish(const KernelArgs& a, uint32_t seq, uint32_t s) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t next_seq = seq + a.ring.slots;
  RingFrameCtl& c = ring_ctl(a.ring, next_seq);
  const unsigned long long next = epoch_of(next_seq);
  if (lane <= kQueueParts) dev_store(&c.queue[lane * (kQueuePartWords / 2u)], next);
  if (lane == 16u) dev_store(&c.pix_done[0], next);
  if (lane == 17u) dev_store(&c.shade_next[0], next);
  if (lane == 18u) dev_store(&c.shade_done[0], next);
  if (lane == 19u) dev_store(&c.rank_next[0], next);
  if (lane == 20u) dev_store(&c.rank_done[0], next);
#pragma unroll
  for (uint32_t k = 0; k < kRankWords / 64u; ++k) dev_store(&c.hist[k * 64u + lane], 0u);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope: before the host sees the frame done
  if (lane == 0) {
    RING_TRACE_MIN(a.ring, seq, 5);
    atomicExch(&a.ring.dev->done_seq[s][0], seq);
    sys_store(&a.ring.host->done[s][0], seq);
  }
}

// An idle service wave's pause between polls, ~13 us (4 x 127 x 64 clocks): its polls are atomics at
// the coherence point, which the march's claims and counts also go through; polling every half
// microsecond from 128 waves slowed the march to about half its rate (128 -> 512 waves: 4x worse).
__device__ __forceinline__ void ring_idle() {
#pragma unroll
  for (int i = 0; i < 4; ++i) __builtin_amdgcn_s_sleep(127);
}

// A ring grid's service wave: shades, ranks and publishes the grid's frames as their marches
// complete (oldest first, any of the `slots` frames in flight), until the grid has closed and
// every frame up to its limit is done. Sleeps between polls; gives up after kRingWatchdogTicks
// without progress (the host then reports the frame as never completed, frm_ring.hip).
template <uint32_t FAM>
__device__ __noinline__ void ring_service(const KernelArgs& a, uint32_t* cnt) {
  const RingArgs& R = a.ring;
  const uint32_t lane = threadIdx.x & 63u;
  const float* table = kSrgbThresholds;  // (global: the service waves share the march waves' LDS budget)
  const uint32_t npix = a.npix;
  const uint32_t ntask = (npix + kRingTaskPixels - 1u) / kRingTaskPixels;
  uint32_t seq0 = 0;
  if (lane == 0) seq0 = max(R.first_seq, dev_poll(&R.dev->base));
  seq0 = uniform(__shfl(seq0, 0, 64));
  RingView rv = {0u, false};
  uint64_t last_progress = realtime();
  unsigned long long last_pd = 0;
  for (;;) {
    if (seq0 > rv.limit) ring_refresh(R, rv);
    // skip the frames already done (another service wave finished them)
    for (;;) {
      if (seq0 > rv.limit) break;
      uint32_t d = 0;
      if (lane == 0) d = dev_poll(&R.dev->done_seq[(seq0 - 1u) & (R.slots - 1u)][0]);
      if (uniform(__shfl(d, 0, 64)) < seq0) break;
      ++seq0;
    }
    if (seq0 > rv.limit) {
      if (rv.closed) return;  // every frame of this grid is done
      if (realtime() - last_progress > kRingWatchdogTicks) return;
      ring_idle();
      continue;
    }
    bool worked = false;
    for (uint32_t g = seq0; g <= rv.limit && g < seq0 + R.slots && !worked; ++g) {
      const uint32_t s = (g - 1u) & (R.slots - 1u);
      RingFrameCtl& c = ring_ctl(R, g);
      unsigned long long pd = 0, sd = 0;
      if (lane == 0) {
        pd = dev_poll(&c.pix_done[0]);
        sd = dev_poll(&c.shade_done[0]);
      }
      pd = __shfl(pd, 0, 64);
      sd = __shfl(sd, 0, 64);
      if (g == seq0 && pd != last_pd) {  // the oldest frame's march moves: progress
        last_pd = pd;
        last_progress = realtime();
      }
      if (pd != (epoch_of(g) | npix)) continue;  // its march has not ended yet
      if (sd == (epoch_of(g) | ntask)) {
        const uint32_t t = epoch_claim(&c.rank_next[0], g, ntask);
        if (t == kIdle) continue;
        ring_rank_task(a, g, s, t, cnt);
        ring_wait_mem();  // its order entries and cursors, before it counts as done
        if (epoch_add(&c.rank_done[0], g, 1u) == ntask - 1u) ring_finish(a, g, s);
        worked = true;
      } else {
        const uint32_t t = epoch_claim(&c.shade_next[0], g, ntask);
        if (t == kIdle) continue;
        const RingCam cam = ring_camera(R, s);
        ring_shade_task<FAM>(a, cam, g, s, t, table, cnt);
        // its pixels, keys and histogram counts first; the zero-copy image's stores reach the host
        // before the frame is published (a system-scope release: the image is read by the host)
        if (cam.host_img)
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        else
          ring_wait_mem();
        if (epoch_add(&c.shade_done[0], g, 1u) == ntask - 1u && lane == 0) RING_TRACE_MIN(R, g, 4);
        worked = true;
      }
    }
    if (worked) {
      last_progress = realtime();
    } else {
      if (realtime() - last_progress > kRingWatchdogTicks) return;
      ring_idle();
    }
  }
}

}  // namespace frm
#endif  // FRM_RING_KERNELS_H
