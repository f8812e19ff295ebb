// frm_refine_kernels.h — adaptive supersampling (frm_set_adaptive, frm_refine; DESIGN.md
// "Adaptive supersampling"): edge_pass finds the pixels of a plain frame whose 3 x 3 neighbourhood
// has contrast, refine_samples<FAM, ITERS, S> marches the S x S samples of those pixels only and
// resolves them as resolve_box does. Included by frm_kernels.hip only: the kernels are not part of
// the source frm_reload compiles at run time.
#pragma once
#include "frm_render_kernels.h"

namespace frm {

// The control words of one adaptive pass (device memory, zeroed on the stream before edge_pass):
// the length of the list of refined pixels and the claim cursor of the refine waves, each in its
// own 256-byte line.
constexpr uint32_t kRefineCountWord = 0, kRefineCursorWord = 64, kRefineCtlWords = 128;
static_assert(kRefineCtlWords * sizeof(uint32_t) == kRefineCtlBytes, "control words of an adaptive pass");

// Edge mask + copy. Output pixel (x, y) is refined iff, over its 3 x 3 window clipped to the frame,
// max over R, G, B of (max - min) of the 8-bit codes is >= threshold (0: every pixel, 256: none;
// alpha is ignored). Every pixel is copied to dst with alpha 255; the linear index of each refined
// one is appended to `list` (capacity w * h), one atomic per wave: the wave's count from the ballot,
// each lane's place from the refined lanes below it. One wave per 8 x 8 tile, as render_simple, so
// that list neighbours are spatial neighbours and a refine wave marches coherent rays. The order of
// the tiles in the list follows the atomics; nothing downstream depends on it.
__global__ __launch_bounds__(256) void edge_pass(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                 uint32_t w, uint32_t h, uint32_t threshold,
                                                 uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t x = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
  const uint32_t y = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
  bool refine = false;
  uint32_t idx = 0;
  if (x < w && y < h) {
    const uint32_t x0 = x ? x - 1u : 0u, x1 = min(x + 1u, w - 1u);
    const uint32_t y0 = y ? y - 1u : 0u, y1 = min(y + 1u, h - 1u);
    uint32_t lo[3] = {255u, 255u, 255u}, hi[3] = {0u, 0u, 0u};
    for (uint32_t yy = y0; yy <= y1; ++yy)
      for (uint32_t xx = x0; xx <= x1; ++xx) {
        const uint32_t t = src[(size_t)yy * w + xx];
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
          const uint32_t v = (t >> (8u * c)) & 255u;
          lo[c] = min(lo[c], v);
          hi[c] = max(hi[c], v);
        }
      }
    const uint32_t contrast = max(max(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    refine = contrast >= threshold;
    idx = y * w + x;
    dst[idx] = src[idx] | (255u << 24);
  }
  const unsigned long long m = __ballot(refine);
  if (m) {  // wave-uniform
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, 0, 64);
    if (refine) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = idx;
  }
}

struct RefineArgs {
  FrameUniforms f;  // of the (S * width) x (S * height) frame: its pixel centres are the samples
  SceneUniforms s;
  const uint32_t* list;   // linear indices of the refined output pixels
  const uint32_t* count;  // their number (device memory: edge_pass's, complete in stream order)
  uint32_t* cursor;       // chunks claimed so far
  uint32_t* dst;          // the output frame, pitch = width
  uint32_t width;         // output pixels per row
  unsigned long long* counters;  // FRM_NUM_COUNTERS, added to (or nullptr)
};

// One lane per sample: a wave holds 64 / (S * S) refined pixels (16, 7 or 4; the lanes left over
// idle), S * S consecutive lanes per pixel in the resolve's order (row by row, left to right). A
// fixed resident grid of one-wave workgroups claims chunks of that many list entries through the
// cursor. Each lane shades its sample as render_simple shades a pixel of the S x frame
// (shade_pixel, pack_rgba); the codes reach every lane of the pixel's group by __shfl, and the
// group's first lane stores the pinned resolve of them (resolve_box: decode, f32 sum in order,
// divide by S * S, encode), one dword per refined pixel. Work counters: each lane's totals live in
// LDS over the wave's chunks (seven 64-bit words a lane: 14 VGPRs less across the march), then per
// wave one atomic per counter, as render_simple.
template <uint32_t FAM, bool ITERS, uint32_t S>
__global__ __launch_bounds__(64) void refine_samples(RefineArgs a) {
  __shared__ float enc[256], dec[256];
  __shared__ unsigned long long total[7][64];
  for (uint32_t t = threadIdx.x; t < 256u; t += 64u) {
    enc[t] = kSrgbThresholds[t];
    dec[t] = kSrgbDecode[t];
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) total[c][threadIdx.x] = 0ull;
  __syncthreads();
  constexpr uint32_t kSamples = S * S, kPixels = 64u / kSamples;
  const uint32_t lane = threadIdx.x;
  const uint32_t group = lane / kSamples, k = lane - group * kSamples;
  const uint32_t count = *a.count;
  for (;;) {
    uint32_t chunk = 0;
    if (lane == 0) chunk = atomicAdd(a.cursor, 1u);
    chunk = __shfl(chunk, 0, 64);
    const uint32_t first = chunk * kPixels;  // < count + grid * kPixels: no wrap (count <= 2^30)
    if (first >= count) break;
    const bool active = group < kPixels && first + group < count;
    uint32_t code = 0, pix = 0;
    if (active) {
      pix = a.list[first + group];
      const uint32_t py = pix / a.width, px = pix - py * a.width;
      PixelCount pc = {0u, 0u, 0u, 0u, {0u, 0u}};
      const v3 color = shade_pixel<FAM, ITERS>(a.f, a.s, S * px + k % S, S * py + k / S, pc);
      code = pack_rgba(color, enc);
      const uint32_t v[7] = {1u, pc.hit, pc.primary, pc.shadow, pc.normal, pc.de.bodies, pc.de.bailouts};
#pragma unroll
      for (int c = 0; c < 7; ++c) total[c][lane] += v[c];  // the lane's own words
    }
    float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < kSamples; ++i) {
      const uint32_t t = __shfl(code, (int)((lane - k + i) & 63u), 64);  // (an idle lane's group runs past 63)
      r = r + dec[t & 255u];
      g = g + dec[(t >> 8) & 255u];
      b = b + dec[(t >> 16) & 255u];
    }
    constexpr float n = (float)kSamples;
    if (active && k == 0)
      a.dst[pix] = encode_srgb(r / n, enc) | (encode_srgb(g / n, enc) << 8) | (encode_srgb(b / n, enc) << 16) |
                   (255u << 24);
  }
  if (a.counters) {
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      const unsigned long long s = wave_sum(total[c][lane]);
      if (lane == 0 && s) atomicAdd(&a.counters[c], s);
    }
  }
}

// ---- launchers ----------------------------------------------------------------------------------
template <uint32_t FAM, bool ITERS, uint32_t S>
static hipError_t refine_one(const RefineArgs& a, uint32_t npix, int cu_count, hipStream_t stream) {
  static int blocks_per_cu = 0;  // occupancy of this instantiation (per process)
  if (blocks_per_cu == 0) {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, refine_samples<FAM, ITERS, S>, 64, 0);
    if (e != hipSuccess) return e;
    blocks_per_cu = n > 0 ? n : 1;
  }
  // the list's length stays on the device: a resident grid, never more waves than chunks of a
  // frame whose every pixel is refined
  constexpr uint32_t kPixels = 64u / (S * S);
  uint32_t blocks = (uint32_t)(blocks_per_cu * cu_count);
  const uint32_t max_blocks = (npix + kPixels - 1u) / kPixels;
  if (blocks > max_blocks) blocks = max_blocks;
  if (blocks == 0) blocks = 1;
  hipLaunchKernelGGL((refine_samples<FAM, ITERS, S>), dim3(blocks), dim3(64), 0, stream, a);
  return hipGetLastError();
}

template <uint32_t FAM, bool ITERS>
static hipError_t refine_factor(const RefineArgs& a, uint32_t factor, uint32_t npix, int cu_count, hipStream_t stream) {
  switch (factor) {
    case 2: return refine_one<FAM, ITERS, 2>(a, npix, cu_count, stream);
    case 3: return refine_one<FAM, ITERS, 3>(a, npix, cu_count, stream);
    case 4: return refine_one<FAM, ITERS, 4>(a, npix, cu_count, stream);
    default: return hipErrorInvalidValue;
  }
}

template <uint32_t FAM>
static hipError_t refine_family(const RefineArgs& a, uint32_t factor, uint32_t npix, int cu_count, hipStream_t stream) {
  return a.s.n ? refine_factor<FAM, true>(a, factor, npix, cu_count, stream)
               : refine_factor<FAM, false>(a, factor, npix, cu_count, stream);
}

hipError_t launch_adaptive(const FrameUniforms& f, const SceneUniforms& s, const uint8_t* src, uint8_t* dst,
                           uint32_t width, uint32_t height, uint32_t factor, uint32_t threshold, uint32_t* list,
                           uint32_t* ctl, unsigned long long* counters, int cu_count, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(ctl, 0, kRefineCtlWords * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(edge_pass, dim3((width + 15u) / 16u, (height + 15u) / 16u), dim3(256), 0, stream,
                     (const uint32_t*)src, (uint32_t*)dst, width, height, threshold, list, ctl + kRefineCountWord);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (factor == 1u) return hipSuccess;  // every sample is the pixel itself: the copy is the frame
  RefineArgs a;
  a.f = f;
  a.s = s;
  a.list = list;
  a.count = ctl + kRefineCountWord;
  a.cursor = ctl + kRefineCursorWord;
  a.dst = (uint32_t*)dst;
  a.width = width;
  a.counters = counters;
  const uint32_t npix = width * height;
  switch (s.family) {
    case kMenger: return refine_family<kMenger>(a, factor, npix, cu_count, stream);
    case kSierpinski: return refine_family<kSierpinski>(a, factor, npix, cu_count, stream);
    case kKoch: return refine_family<kKoch>(a, factor, npix, cu_count, stream);
    case kMandelbulb: return refine_family<kMandelbulb>(a, factor, npix, cu_count, stream);
    case kMandelbulbHw: return refine_family<kMandelbulbHw>(a, factor, npix, cu_count, stream);
    default: return refine_family<kSphere>(a, factor, npix, cu_count, stream);
  }
}

}  // namespace frm
