// frm_shutter_kernels.h — motion blur (frm_render_shutter, frm_accumulate; DESIGN.md "Motion
// blur"): the mean, in linear light, of the S x S texels under an output pixel over `count`
// sub-frames of one shutter interval. Included by frm_kernels.hip; the pixel layout and the row
// loads are resolve_box's.
//
// For output pixel (X, Y) and each of R, G, B (tests/shutter_reference.py pins this order):
//   sum = acc ? acc[pixel] : 0
//   for k in 0..count-1, j in 0..S-1, i in 0..S-1:  sum = sum + kSrgbDecode[frame k [S*Y+j][S*X+i]]
//   acc[pixel] = (sum, 0)                                     (if acc)
//   dst[pixel] = encode_srgb(sum / (float)divisor), alpha 255 (if dst)
// The adds form one f32 chain in exactly this order, so a sum carried through acc between launches
// gives the bits of one launch over all the sub-frames.
#pragma once

namespace frm {

// One thread per output pixel, one wave per 64 consecutive pixels of an output row (resolve_box's
// layout: each source row of a sub-frame is one contiguous run of 64*S texels per wave). VEC: a
// lane reads its S texels of a row with one uint2 / uint4 load; the source base and the frame
// stride must then be 4*S-byte aligned. The add chain is sequential, the loads are not: the texels
// of kShutterUnroll sub-frames are loaded before the first of them is consumed, so that several
// frames' loads are in flight per lane.
constexpr uint32_t kShutterUnroll = 4;

template <uint32_t S, bool VEC>
__device__ __forceinline__ void shutter_load(const uint32_t* p, size_t pitch, uint32_t (&tx)[S * S]) {
#pragma unroll
  for (uint32_t j = 0; j < S; ++j, p += pitch) {
    if constexpr (VEC && S == 2) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      tx[2 * j] = v.x, tx[2 * j + 1] = v.y;
    } else if constexpr (VEC && S == 4) {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      tx[4 * j] = v.x, tx[4 * j + 1] = v.y, tx[4 * j + 2] = v.z, tx[4 * j + 3] = v.w;
    } else {
#pragma unroll
      for (uint32_t i = 0; i < S; ++i) tx[S * j + i] = p[i];
    }
  }
}

template <uint32_t S>
__device__ __forceinline__ void shutter_add(const uint32_t (&tx)[S * S], const float* dec, float& r, float& g, float& b) {
#pragma unroll
  for (uint32_t i = 0; i < S * S; ++i) {  // row by row, left to right
    r = r + dec[tx[i] & 255u];
    g = g + dec[(tx[i] >> 8) & 255u];
    b = b + dec[(tx[i] >> 16) & 255u];
  }
}

template <uint32_t S, bool VEC>
__global__ __launch_bounds__(256) void shutter_accumulate(const uint32_t* __restrict__ src, size_t frame_stride,
                                                          uint32_t count, float4* __restrict__ acc,
                                                          uint32_t* __restrict__ dst, uint32_t dw, uint32_t dh,
                                                          float divisor) {
  __shared__ float dec[256], enc[256];
  const uint32_t t = threadIdx.y * 64u + threadIdx.x;
  dec[t] = kSrgbDecode[t];
  enc[t] = kSrgbThresholds[t];
  __syncthreads();
  const uint32_t x = blockIdx.x * 64u + threadIdx.x, y = blockIdx.y * 4u + threadIdx.y;
  if (x >= dw || y >= dh) return;
  const size_t pitch = (size_t)S * dw;  // source texels per row
  const size_t pix = (size_t)y * dw + x;
  const uint32_t* p = src + (size_t)S * y * pitch + (size_t)S * x;  // sub-frame 0; k: + k * frame_stride
  float r = 0.0f, g = 0.0f, b = 0.0f;
  if (acc) {
    const float4 a = acc[pix];
    r = a.x, g = a.y, b = a.z;
  }
  uint32_t k = 0;
  for (; k + kShutterUnroll <= count; k += kShutterUnroll, p += kShutterUnroll * frame_stride) {
    uint32_t tx[kShutterUnroll][S * S];
#pragma unroll
    for (uint32_t u = 0; u < kShutterUnroll; ++u) shutter_load<S, VEC>(p + u * frame_stride, pitch, tx[u]);
#pragma unroll
    for (uint32_t u = 0; u < kShutterUnroll; ++u) shutter_add<S>(tx[u], dec, r, g, b);
  }
  for (; k < count; ++k, p += frame_stride) {
    uint32_t tx[S * S];
    shutter_load<S, VEC>(p, pitch, tx);
    shutter_add<S>(tx, dec, r, g, b);
  }
  if (acc) acc[pix] = make_float4(r, g, b, 0.0f);
  if (dst)
    dst[pix] = encode_srgb(r / divisor, enc) | (encode_srgb(g / divisor, enc) << 8) |
               (encode_srgb(b / divisor, enc) << 16) | (255u << 24);
}

template <uint32_t S>
static void shutter_one(const uint8_t* src, size_t frame_stride_bytes, uint32_t count, float* acc, uint8_t* dst,
                        uint32_t dw, uint32_t dh, uint32_t divisor, hipStream_t stream) {
  const dim3 grid((dw + 63u) / 64u, (dh + 3u) / 4u), block(64, 4);
  const bool vec = (S == 2 || S == 4) && reinterpret_cast<uintptr_t>(src) % (4u * S) == 0 &&
                   frame_stride_bytes % (4u * S) == 0;
  if (vec)
    hipLaunchKernelGGL((shutter_accumulate<S, true>), grid, block, 0, stream, (const uint32_t*)src,
                       frame_stride_bytes / 4u, count, (float4*)acc, (uint32_t*)dst, dw, dh, (float)divisor);
  else
    hipLaunchKernelGGL((shutter_accumulate<S, false>), grid, block, 0, stream, (const uint32_t*)src,
                       frame_stride_bytes / 4u, count, (float4*)acc, (uint32_t*)dst, dw, dh, (float)divisor);
}

// src: `count` (>= 1) sub-frames frame_stride_bytes (a multiple of 4) apart, each factor*dh rows of
// factor*dw RGBA8 sRGB texels, 4-byte aligned; acc: nullptr or dw*dh float4 (16-byte aligned, read
// and written); dst: nullptr or dh rows of dw texels; factor 1..4.
hipError_t launch_shutter(const uint8_t* src, size_t frame_stride_bytes, uint32_t count, float* acc, uint8_t* dst,
                          uint32_t dw, uint32_t dh, uint32_t factor, uint32_t divisor, hipStream_t stream) {
  switch (factor) {
    case 1: shutter_one<1>(src, frame_stride_bytes, count, acc, dst, dw, dh, divisor, stream); break;
    case 2: shutter_one<2>(src, frame_stride_bytes, count, acc, dst, dw, dh, divisor, stream); break;
    case 3: shutter_one<3>(src, frame_stride_bytes, count, acc, dst, dw, dh, divisor, stream); break;
    case 4: shutter_one<4>(src, frame_stride_bytes, count, acc, dst, dw, dh, divisor, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace frm
