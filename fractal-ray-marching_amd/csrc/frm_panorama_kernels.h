// frm_panorama_kernels.h — 360-degree panoramas (frm_set_panorama, frm_project_equirect; DESIGN.md
// "Panorama"): six cube faces of M x M texels (M = N + 2: N texels of a 90-degree face and one
// guard texel all round) projected to a W x H equirectangular frame. Included by frm_kernels.hip;
// the pixel layout is resolve_box's, the filter is blit_kernel's linear path.
//
// For output pixel (X, Y), all f32, no contraction (tests/panorama_reference.py pins this order):
//   dx = cos_lat[Y]*sin_lon[X];  dy = sin_lat[Y];  dz = cos_lat[Y]*cos_lon[X]
//   face: |dz| >= |dx| && |dz| >= |dy| ? (dz > 0 ? 0 : 1)
//       : |dx| >= |dy|                 ? (dx > 0 ? 2 : 3)
//       :                                (dy > 0 ? 4 : 5)
//   (A, B, m) = (dx,dy,dz) (-dx,dy,-dz) (-dz,dy,dx) (dz,dy,-dx) (dx,-dz,dy) (dx,dz,-dy)  for face 0..5
//   u = A / m;  v = B / m
//   fx = u*(0.5f*N) + (0.5f*M - 0.5f);  fy = (0.5f*M - 0.5f) - v*(0.5f*N)
//   x0 = floor(fx); tx = fx - x0;  y0 = floor(fy); ty = fy - y0
//   x0, x0 + 1, y0, y0 + 1 clamped to [0, M - 1]
//   per channel: top = mix(D[t00], D[t10], tx); bot = mix(D[t01], D[t11], tx); c = mix(top, bot, ty)
//   with mix(a, b, t) = a*(1.0f - t) + b*t and D = kSrgbDecode; stored as the sRGB store, alpha 255.
#pragma once

namespace frm {

__device__ __forceinline__ float pano_mix(float a, float b, float t) { return a * (1.0f - t) + b * t; }

// One thread per output pixel, one wave per 64 consecutive pixels of an output row (resolve_box's
// layout), so sin_lat / cos_lat are wave-uniform. The four taps are dword gathers: near the poles a
// wave reads a handful of texels, at the equator it walks two face rows. face_stride: texels.
__global__ __launch_bounds__(256) void project_equirect(const uint32_t* __restrict__ faces, size_t face_stride,
                                                        uint32_t n, const float* __restrict__ sin_lon,
                                                        const float* __restrict__ cos_lon,
                                                        const float* __restrict__ sin_lat,
                                                        const float* __restrict__ cos_lat,
                                                        uint32_t* __restrict__ dst, uint32_t dw, uint32_t dh) {
  __shared__ float dec[256], enc[256];
  const uint32_t t = threadIdx.y * 64u + threadIdx.x;
  dec[t] = kSrgbDecode[t];
  enc[t] = kSrgbThresholds[t];
  __syncthreads();
  const uint32_t x = blockIdx.x * 64u + threadIdx.x;
  const uint32_t y = __builtin_amdgcn_readfirstlane(blockIdx.y * 4u + threadIdx.y);  // a wave is one row
  if (x >= dw || y >= dh) return;
  const float sl = sin_lon[x], cl = cos_lon[x], sp = sin_lat[y], cp = cos_lat[y];
  const float dx = cp * sl, dy = sp, dz = cp * cl;
  const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
  uint32_t f;
  float A, B, m;
  if (az >= ax && az >= ay) {
    const bool pos = dz > 0.0f;
    f = pos ? 0u : 1u, A = pos ? dx : -dx, B = dy, m = pos ? dz : -dz;
  } else if (ax >= ay) {
    const bool pos = dx > 0.0f;
    f = pos ? 2u : 3u, A = pos ? -dz : dz, B = dy, m = pos ? dx : -dx;
  } else {
    const bool pos = dy > 0.0f;
    f = pos ? 4u : 5u, A = dx, B = pos ? -dz : dz, m = pos ? dy : -dy;
  }
  const float u = A / m, v = B / m;
  const uint32_t mm = n + 2u;
  const float half_n = 0.5f * (float)n, centre = 0.5f * (float)mm - 0.5f, last = (float)(mm - 1u);
  const float fx = u * half_n + centre, fy = centre - v * half_n;
  const float x0f = floorf(fx), y0f = floorf(fy);
  const float tx = fx - x0f, ty = fy - y0f;
  // clamped as floats (a NaN clamps to 0): no index leaves the face whatever the tables hold
  const uint32_t x0 = (uint32_t)fminf(fmaxf(x0f, 0.0f), last), x1 = (uint32_t)fminf(fmaxf(x0f + 1.0f, 0.0f), last);
  const uint32_t y0 = (uint32_t)fminf(fmaxf(y0f, 0.0f), last), y1 = (uint32_t)fminf(fmaxf(y0f + 1.0f, 0.0f), last);
  const uint32_t* face = faces + f * face_stride;
  const uint32_t t00 = face[y0 * mm + x0], t10 = face[y0 * mm + x1], t01 = face[y1 * mm + x0], t11 = face[y1 * mm + x1];
  uint32_t code = 255u << 24;
#pragma unroll
  for (uint32_t k = 0; k < 3u; ++k) {
    const uint32_t sh = 8u * k;
    const float top = pano_mix(dec[(t00 >> sh) & 255u], dec[(t10 >> sh) & 255u], tx);
    const float bot = pano_mix(dec[(t01 >> sh) & 255u], dec[(t11 >> sh) & 255u], tx);
    code |= encode_srgb(pano_mix(top, bot, ty), enc) << sh;
  }
  dst[(size_t)y * dw + x] = code;
}

// faces: six faces face_stride_bytes (a multiple of 4, at least 4*(n+2)^2) apart, each n+2 rows of
// n+2 RGBA8 sRGB texels, 4-byte aligned; tables: sin_lon[dw], cos_lon[dw], sin_lat[dh], cos_lat[dh]
// back to back in device memory (frm_equirect_tables); dst: dh rows of dw texels.
hipError_t launch_project_equirect(const uint8_t* faces, size_t face_stride_bytes, uint32_t n, const float* tables,
                                   uint8_t* dst, uint32_t dw, uint32_t dh, hipStream_t stream) {
  const dim3 grid((dw + 63u) / 64u, (dh + 3u) / 4u), block(64, 4);
  hipLaunchKernelGGL(project_equirect, grid, block, 0, stream, (const uint32_t*)faces, face_stride_bytes / 4u, n,
                     tables, tables + dw, tables + 2u * (size_t)dw, tables + 2u * (size_t)dw + dh, (uint32_t*)dst, dw, dh);
  return hipGetLastError();
}

}  // namespace frm
