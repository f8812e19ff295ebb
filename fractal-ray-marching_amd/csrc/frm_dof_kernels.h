// frm_dof_kernels.h — depth of field (frm_set_depth_of_field, frm_depth_of_field, frm_read_depth;
// DESIGN.md "Depth of field"): depth_pass turns a persistent launch's records into an f32 depth
// plane, dof_gather blurs a frame in linear light by each pixel's circle of confusion. Included by
// frm_kernels.hip; frm_host.cpp takes the per-pixel functions below for frm_dof_coc.
//
// Per pixel q, all f32, no contraction, IEEE divisions (tests/dof_reference.py pins this order):
//   c = A * fabsf(1.0f - F / Z[q]);  if (!(c >= 0.0f)) c = 0.0f;  if (c > (float)R) c = (float)R
//   a = c * c;   w = 1.0f / (kPi * a + 1.0f)
// Per output pixel p: sw = sr = sg = sb = 0.0f; for dy = -R..R (outer), dx = -R..R (inner), q = p +
// (dx, dy) inside the frame:
//   use_p = (Z[q] > Z[p]) && (c[p] < c[q]);  a_e = use_p ? a[p] : a[q];  w_e = use_p ? w[p] : w[q]
//   if ((float)(dx*dx + dy*dy) <= a_e):  sw = sw + w_e;  sr = sr + w_e * D[S[q].r]  (likewise g, b)
// out[p] = encode(sr / sw), encode(sg / sw), encode(sb / sw), 255.
#pragma once
#include "frm_math.h"

namespace frm {

constexpr float kDofPi = 0x1.921fb6p+1f;  // f32(pi)

// c of one depth; rf = (float)R.
FRM_HD float dof_coc(float aperture, float focus, float rf, float z) {
  float c = aperture * fabsf(1.0f - focus / z);
  if (!(c >= 0.0f)) c = 0.0f;  // NaN: in focus
  if (c > rf) c = rf;
  return c;
}
// w of a = c * c.
FRM_HD float dof_weight(float a) { return 1.0f / (kDofPi * a + 1.0f); }

#if defined(__HIPCC__)

// Z[idx] = the primary hit distance of local pixel idx, +inf for a miss. One thread per pixel.
// Misses never read geom: their records are stale by design (frm_internal.h ShadeGeom).
__global__ __launch_bounds__(256) void depth_pass(const ShadeGeom* __restrict__ geom,
                                                  const ShadeTail* __restrict__ tails, float* __restrict__ z,
                                                  uint32_t npix) {
  const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
  if (idx >= npix) return;
  float t = __uint_as_float(0x7f800000u);
  if (tails[idx].word & kRecHit) t = geom[idx].t;
  z[idx] = t;
}

hipError_t launch_depth(const ShadeGeom* geom, const ShadeTail* tails, float* z, uint32_t npix, hipStream_t stream) {
  hipLaunchKernelGGL(depth_pass, dim3((npix + 255u) / 256u), dim3(256), 0, stream, geom, tails, z, npix);
  return hipGetLastError();
}

// A block of 16 x 16 threads owns a 16 x 16 tile of output pixels and stages the tile with a halo of
// R pixels in LDS: per staged pixel the decoded linear colour with Z (one float4) and a, w (one
// float2), so a sample costs one 16-byte and one 8-byte LDS read. Staged positions outside the frame
// hold a = -1 (no distance passes), Z = -inf (use_p is false) and w = 0. The LDS is dynamic,
// 24 * (16 + 2R)^2 + 2064 bytes: 57360 at R = 16 (two blocks per CU), 12816 at R = 3.
//
// c[p] < c[q] is tested as a[p] < a[q]: squaring is monotonic, and where it maps two different c
// to one a the two candidates (a, w) are the same pair. A sample that does not pass adds 0.0f, the
// same bits as skipping it (the sums are never negative). No sample passes beyond the largest a of
// the staged pixels, so the window is walked only as far as that: rows |dy| <= r with r*r <= amax,
// and in row dy the columns with dx*dx + dy*dy <= amax. Both bounds are the block's, not a lane's.
constexpr uint32_t kDofTile = 16;
constexpr size_t kDofLdsTail = 2u * 256u * sizeof(float) + 16u;  // decode and encode tables, amax
static inline size_t dof_lds_bytes(uint32_t radius) {
  const size_t side = kDofTile + 2u * radius;
  return side * side * (sizeof(float4) + sizeof(float2)) + kDofLdsTail;
}

__global__ __launch_bounds__(256) void dof_gather(const uint32_t* __restrict__ src, const float* __restrict__ depth,
                                                  uint32_t* __restrict__ dst, uint32_t width, uint32_t height,
                                                  float aperture, float focus, uint32_t radius) {
  extern __shared__ float4 dof_lds[];
  const uint32_t side = kDofTile + 2u * radius, n = side * side;
  float4* cz = dof_lds;                              // r, g, b, Z
  float2* aw = reinterpret_cast<float2*>(cz + n);    // a, w
  float* dec = reinterpret_cast<float*>(aw + n);
  float* enc = dec + 256;
  uint32_t* amax_bits = reinterpret_cast<uint32_t*>(enc + 256);
  const uint32_t t = threadIdx.y * kDofTile + threadIdx.x;
  dec[t] = kSrgbDecode[t];
  enc[t] = kSrgbThresholds[t];
  if (t == 0) *amax_bits = 0u;
  __syncthreads();
  const int x0 = (int)(blockIdx.x * kDofTile) - (int)radius, y0 = (int)(blockIdx.y * kDofTile) - (int)radius;
  const float rf = (float)radius;
  float amax = 0.0f;
  for (uint32_t i = t; i < n; i += 256u) {
    const uint32_t ly = i / side, lx = i - ly * side;
    const int gx = x0 + (int)lx, gy = y0 + (int)ly;
    float4 c4 = make_float4(0.0f, 0.0f, 0.0f, -__uint_as_float(0x7f800000u));
    float2 a2 = make_float2(-1.0f, 0.0f);
    if (gx >= 0 && gy >= 0 && gx < (int)width && gy < (int)height) {
      const size_t g = (size_t)gy * width + (uint32_t)gx;
      const uint32_t tx = src[g];
      const float z = depth[g];
      const float c = dof_coc(aperture, focus, rf, z);
      const float a = c * c;
      c4 = make_float4(dec[tx & 255u], dec[(tx >> 8) & 255u], dec[(tx >> 16) & 255u], z);
      a2 = make_float2(a, dof_weight(a));
      amax = fmaxf(amax, a);
    }
    cz[i] = c4;
    aw[i] = a2;
  }
  atomicMax(amax_bits, __float_as_uint(amax));  // a >= 0: the bit patterns order as the values do
  __syncthreads();
  const uint32_t px = blockIdx.x * kDofTile + threadIdx.x, py = blockIdx.y * kDofTile + threadIdx.y;
  if (px >= width || py >= height) return;
  // every lane reads the same LDS word (complete since the barrier), so the first lane's value is
  // the wave's: the loop bounds below are scalar
  const float amax_all = __uint_as_float(__builtin_amdgcn_readfirstlane(*amax_bits));
  int r = 0;
  while (r < (int)radius && (float)((r + 1) * (r + 1)) <= amax_all) ++r;
  const int pc = (int)((threadIdx.y + radius) * side + threadIdx.x + radius);
  const float zp = cz[pc].w, ap = aw[pc].x, wp = aw[pc].y;
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
  for (int dy = -r; dy <= r; ++dy) {
    int m = r;  // the row's reach: dx*dx + dy*dy <= amax_all (dx = 0 passes: |dy| <= r)
    while ((float)(m * m + dy * dy) > amax_all) --m;
    const int row = pc + dy * (int)side;
#pragma unroll 4
    for (int dx = -m; dx <= m; ++dx) {
      const float4 q = cz[row + dx];
      const float2 e = aw[row + dx];
      const bool use_p = (q.w > zp) && (ap < e.x);
      const float a_e = use_p ? ap : e.x, w_e = use_p ? wp : e.y;
      const float wz = (float)(dx * dx + dy * dy) <= a_e ? w_e : 0.0f;
      sw = sw + wz;
      sr = sr + wz * q.x;
      sg = sg + wz * q.y;
      sb = sb + wz * q.z;
    }
  }
  dst[(size_t)py * width + px] = encode_srgb(sr / sw, enc) | (encode_srgb(sg / sw, enc) << 8) |
                                 (encode_srgb(sb / sw, enc) << 16) | (255u << 24);
}

// src, dst: height rows of width RGBA8 sRGB texels; depth: as many floats; all 4-byte aligned, dst
// overlapping neither input; radius <= FRM_MAX_DOF_RADIUS (the LDS stays below 64 KB).
hipError_t launch_dof(const uint8_t* src, const float* depth, uint8_t* dst, uint32_t width, uint32_t height,
                      float aperture, float focus, uint32_t radius, hipStream_t stream) {
  if (radius > FRM_MAX_DOF_RADIUS) return hipErrorInvalidValue;
  const dim3 grid((width + kDofTile - 1u) / kDofTile, (height + kDofTile - 1u) / kDofTile), block(kDofTile, kDofTile);
  hipLaunchKernelGGL(dof_gather, grid, block, dof_lds_bytes(radius), stream, (const uint32_t*)src, depth,
                     (uint32_t*)dst, width, height, aperture, focus, radius);
  return hipGetLastError();
}

#endif  // __HIPCC__

}  // namespace frm
