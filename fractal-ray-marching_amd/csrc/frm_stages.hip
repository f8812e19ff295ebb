// frm_stages.hip — the stream-level stages of include/frm.h: each works on device buffers of the
// caller's, on the caller's stream, without touching the context's frames (frm_resolve, frm_refine,
// frm_blit, frm_accumulate, frm_project_equirect, frm_depth_of_field, frm_unshuffle_bands), the pure
// helpers that go with them, and the one check of their buffers.
#include "frm_ctx.h"

// A frame size for `factor` samples per pixel and axis: [1, FRM_MAX_DIMENSION / factor]^2.
int check_size(frm_ctx* ctx, uint32_t width, uint32_t height, uint32_t factor, const char* noun) {
  const uint32_t limit = FRM_MAX_DIMENSION / factor;
  if (width == 0 || height == 0 || width > limit || height > limit)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "%s %ux%u outside [1, %u]^2 (factor %u)", noun, width, height, limit,
                factor);
  return FRM_OK;
}

// The output size and blit flags of frm_present, frm_present_async and frm_blit.
int check_output(frm_ctx* ctx, uint32_t out_width, uint32_t out_height, uint32_t flags) {
  if (int rc = check_size(ctx, out_width, out_height, 1, "output size")) return rc;
  if (flags & ~(FRM_BLIT_SRGB | FRM_BLIT_BGRA)) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
  return FRM_OK;
}

// The lens of frm_dof_coc, frm_depth_of_field and frm_set_depth_of_field.
int check_lens(frm_ctx* ctx, float aperture, float focus, uint32_t max_radius) {
  if (max_radius > FRM_MAX_DOF_RADIUS)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "depth-of-field radius %u above %u", max_radius, FRM_MAX_DOF_RADIUS);
  if (!(aperture >= 0.0f) || aperture > 3.402823466e+38f)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "depth-of-field aperture %g: not finite or negative", (double)aperture);
  if (!(focus > 0.0f) || focus > 3.402823466e+38f)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "depth-of-field focus %g: not finite and positive", (double)focus);
  return FRM_OK;
}

// The buffers (frm_ctx.h Span) of one call, reported in this order: every alignment, then every size
// in list order, then every pair that overlaps with one of the two written (two inputs may share
// bytes). The band entry points of frm_api.hip check theirs here too.
int check_spans(frm_ctx* ctx, std::initializer_list<Span> spans) {
  for (const Span& s : spans)
    if (reinterpret_cast<uintptr_t>(s.p) % s.align)
      return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "%s not %u-byte aligned", s.name, s.align);
  for (const Span& s : spans)
    if (s.held < s.need || s.need == SIZE_MAX)
      return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "%s holds %zu bytes, the call needs %zu", s.name, s.held, s.need);
  for (const Span* a = spans.begin(); a != spans.end(); ++a)
    for (const Span* b = a + 1; b != spans.end(); ++b) {
      const uintptr_t pa = reinterpret_cast<uintptr_t>(a->p), pb = reinterpret_cast<uintptr_t>(b->p);
      if (a->need && b->need && (a->written || b->written) && pa < pb + b->need && pb < pa + a->need)
        return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "%s and %s overlap", a->name, b->name);
    }
  return FRM_OK;
}

namespace {

// *need: the bytes that `count` frames of frame_need bytes, stride bytes apart, span (SIZE_MAX: more
// than any buffer holds). A stride below a frame or not a multiple of 4 is refused.
int strided_need(frm_ctx* ctx, size_t stride, size_t frame_need, uint32_t count, size_t* need) {
  if (stride % 4u || stride < frame_need)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "stride %zu: below the %zu bytes of a frame or not a multiple of 4", stride,
                frame_need);
  *need = count - 1u > (SIZE_MAX - frame_need) / stride ? SIZE_MAX : (count - 1u) * stride + frame_need;
  return FRM_OK;
}

}  // namespace

extern "C" {

int frm_resolve(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, uint32_t out_width, uint32_t out_height,
                uint32_t factor, uint8_t* dev_dst, size_t dst_bytes, void* stream) {
  if (!ctx || !dev_src || !dev_dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_src/dev_dst is NULL");
  if (factor == 0 || factor > FRM_MAX_SUPERSAMPLE)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "supersampling factor %u outside [1, %u]", factor, FRM_MAX_SUPERSAMPLE);
  if (int rc = check_size(ctx, out_width, out_height, factor, "output size")) return rc;
  const size_t need = (size_t)out_width * out_height * 4u;
  if (int rc = check_spans(ctx, {{"dev_src", dev_src, src_bytes, need * factor * factor, 4, false},
                                 {"dev_dst", dev_dst, dst_bytes, need, 4, true}}))
    return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  FRM_HIP(ctx, launch_resolve(dev_src, dev_dst, out_width, out_height, factor, s));
  return FRM_OK;
}

int frm_refine(frm_ctx* ctx, const frm_parameters* params, const uint8_t* dev_src, size_t src_bytes, uint32_t width,
               uint32_t height, uint32_t factor, uint32_t threshold, uint8_t* dev_dst, size_t dst_bytes,
               uint64_t* dev_counters, void* stream) {
  if (!ctx || !dev_src || !dev_dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_src/dev_dst is NULL");
  if (factor == 0 || factor > FRM_MAX_SUPERSAMPLE || threshold > 256u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "adaptive factor %u outside [1, %u] or edge threshold %u above 256", factor,
                FRM_MAX_SUPERSAMPLE, threshold);
  if (int rc = check_size(ctx, width, height, factor, "frame size")) return rc;
  const size_t need = (size_t)width * height * 4u;
  if (int rc = check_spans(ctx, {{"dev_src", dev_src, src_bytes, need, 4, false},
                                 {"dev_dst", dev_dst, dst_bytes, need, 4, true},
                                 {"dev_counters", dev_counters, 0, 0, 8, true}}))
    return rc;
  frm_parameters p;
  SceneUniforms su;
  if (params) {
    p = *params;
    compute_scene_uniforms(p, ctx->flags, &su);
    if (int rc = check_parameters(ctx, su, p)) return rc;
  } else {
    if (!ctx->has_params) return fail(ctx, FRM_ERR_NOT_READY, "params is NULL and frm_set_parameters has not been called");
    p = ctx->params;
    su = ctx->scene;
  }
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // scratch per call, allocated and released in the order of the call's stream: calls in flight on
  // different streams never share it
  uint32_t *list = nullptr, *ctl = nullptr;
  int rc = dev_alloc(ctx, (void**)&list, need, s);
  if (rc) return rc;
  if ((rc = dev_alloc(ctx, (void**)&ctl, kRefineCtlBytes, s))) {
    (void)hipFreeAsync(list, s);
    return rc;
  }
  FrameUniforms f;
  compute_frame_uniforms(p, factor * width, factor * height, ctx->max_steps, &f);
  const hipError_t e = launch_adaptive(f, su, dev_src, dev_dst, width, height, factor, threshold, list, ctl,
                                       (unsigned long long*)dev_counters, ctx->cu_count, s);
  const int r1 = dev_release(ctx, list, s), r2 = dev_release(ctx, ctl, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "launch_adaptive");
  return r1 ? r1 : r2;
}

int frm_blit(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, uint32_t src_width, uint32_t src_height,
             uint8_t* dev_dst, size_t dst_bytes, uint32_t out_width, uint32_t out_height, uint32_t flags, void* stream) {
  if (!ctx || !dev_src || !dev_dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_src/dev_dst is NULL");
  if (int rc = check_size(ctx, src_width, src_height, 1, "source size")) return rc;
  if (int rc = check_output(ctx, out_width, out_height, flags)) return rc;
  if (int rc = check_spans(ctx, {{"dev_src", dev_src, src_bytes, (size_t)src_width * src_height * 4u, 4, false},
                                 {"dev_dst", dev_dst, dst_bytes, (size_t)out_width * out_height * 4u, 4, true}}))
    return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  FRM_HIP(ctx, launch_blit(dev_src, src_width, src_height, dev_dst, out_width, out_height, flags, s));
  return FRM_OK;
}

int frm_accumulate(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, size_t frame_stride_bytes, uint32_t count,
                   uint32_t out_width, uint32_t out_height, uint32_t factor, float* dev_acc, size_t acc_bytes,
                   uint32_t divisor, uint8_t* dev_dst, size_t dst_bytes, void* stream) {
  if (!ctx || !dev_src || (!dev_acc && !dev_dst))
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_src is NULL, or both dev_acc and dev_dst are");
  if (factor == 0 || factor > FRM_MAX_SUPERSAMPLE || count == 0 || count > FRM_MAX_SHUTTER_SAMPLES)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "factor %u outside [1, %u] or count %u outside [1, %u]", factor,
                FRM_MAX_SUPERSAMPLE, count, FRM_MAX_SHUTTER_SAMPLES);
  if (int rc = check_size(ctx, out_width, out_height, factor, "output size")) return rc;
  if (dev_dst && divisor == 0) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "divisor is 0");
  const size_t npix = (size_t)out_width * out_height;
  size_t src_need = 0;
  if (int rc = strided_need(ctx, frame_stride_bytes, npix * factor * factor * 4u, count, &src_need)) return rc;
  if (int rc = check_spans(ctx, {{"dev_src", dev_src, src_bytes, src_need, 4, false},
                                 {"dev_acc", dev_acc, acc_bytes, dev_acc ? npix * sizeof(float4) : 0, 16, true},
                                 {"dev_dst", dev_dst, dst_bytes, dev_dst ? npix * 4u : 0, 4, true}}))
    return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  FRM_HIP(ctx, launch_shutter(dev_src, frame_stride_bytes, count, dev_acc, dev_dst, out_width, out_height, factor, divisor, s));
  return FRM_OK;
}

int frm_panorama_face_size(uint32_t width, uint32_t* out_face_size) {
  if (!out_face_size || width == 0 || width > FRM_MAX_DIMENSION)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "out_face_size is NULL or width %u outside [1, %u]", width,
                FRM_MAX_DIMENSION);
  *out_face_size = (width + 3u) / 4u;
  return FRM_OK;
}

int frm_equirect_tables(uint32_t width, uint32_t height, float* sin_lon, float* cos_lon, float* sin_lat,
                        float* cos_lat) {
  if (!sin_lon || !cos_lon || !sin_lat || !cos_lat || width == 0 || height == 0 || width > FRM_MAX_DIMENSION ||
      height > FRM_MAX_DIMENSION)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "a table is NULL or size %ux%u outside [1, %u]^2", width, height,
                FRM_MAX_DIMENSION);
  float* t = new (std::nothrow) float[2u * (size_t)width + 2u * (size_t)height];
  if (!t) return fail(nullptr, FRM_ERR_OUT_OF_MEMORY, "host allocation failed");
  equirect_tables(width, height, t);
  memcpy(sin_lon, t, width * sizeof(float));
  memcpy(cos_lon, t + width, width * sizeof(float));
  memcpy(sin_lat, t + 2u * (size_t)width, height * sizeof(float));
  memcpy(cos_lat, t + 2u * (size_t)width + height, height * sizeof(float));
  delete[] t;
  return FRM_OK;
}

int frm_project_equirect(frm_ctx* ctx, const uint8_t* dev_faces, size_t faces_bytes, size_t face_stride_bytes,
                         uint32_t face_size, uint8_t* dev_dst, size_t dst_bytes, uint32_t out_width,
                         uint32_t out_height, void* stream) {
  if (!ctx || !dev_faces || !dev_dst) return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_faces/dev_dst is NULL");
  if (face_size == 0 || face_size > FRM_MAX_DIMENSION - 2u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "face size %u outside [1, %u]", face_size, FRM_MAX_DIMENSION - 2u);
  if (int rc = check_size(ctx, out_width, out_height, 1, "output size")) return rc;
  const size_t m = (size_t)face_size + 2u;
  size_t faces_need = 0;
  if (int rc = strided_need(ctx, face_stride_bytes, m * m * 4u, 6, &faces_need)) return rc;
  if (int rc = check_spans(ctx, {{"dev_faces", dev_faces, faces_bytes, faces_need, 4, false},
                                 {"dev_dst", dev_dst, dst_bytes, (size_t)out_width * out_height * 4u, 4, true}}))
    return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // the tables are scratch per call, allocated and released in the order of the call's stream: calls
  // in flight on different streams never share them
  float* tables = nullptr;
  int rc = dev_alloc(ctx, (void**)&tables, (2u * (size_t)out_width + 2u * (size_t)out_height) * sizeof(float), s);
  if (rc) return rc;
  hipError_t e = hipSuccess;
  if (!(rc = upload_tables(ctx, tables, out_width, out_height, s)))
    e = launch_project_equirect(dev_faces, face_stride_bytes, face_size, tables, dev_dst, out_width, out_height, s);
  const int r1 = dev_release(ctx, tables, s);
  if (rc) return rc;
  if (e != hipSuccess) return hip_fail(ctx, e, "launch_project_equirect");
  return r1;
}

int frm_dof_coc(float aperture, float focus, uint32_t max_radius, const float* depth, size_t n, float* out_c) {
  if (!depth || !out_c) return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "depth/out_c is NULL");
  if (int rc = check_lens(nullptr, aperture, focus, max_radius)) return rc;
  dof_coc_host(aperture, focus, max_radius, depth, n, out_c);
  return FRM_OK;
}

int frm_depth_of_field(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, const float* dev_depth,
                       size_t depth_bytes, uint32_t width, uint32_t height, float aperture, float focus,
                       uint32_t max_radius, uint8_t* dev_dst, size_t dst_bytes, void* stream) {
  if (!ctx || !dev_src || !dev_depth || !dev_dst)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "ctx/dev_src/dev_depth/dev_dst is NULL");
  if (int rc = check_size(ctx, width, height, 1, "frame size")) return rc;
  if (int rc = check_lens(ctx, aperture, focus, max_radius)) return rc;
  const size_t need = (size_t)width * height * 4u;  // of each of the three
  // the frame and the output first, then the depth plane and the output: a fault of the first pair is
  // reported before any of the plane's
  const Span src{"dev_src", dev_src, src_bytes, need, 4, false}, dst{"dev_dst", dev_dst, dst_bytes, need, 4, true};
  if (int rc = check_spans(ctx, {src, dst})) return rc;
  if (int rc = check_spans(ctx, {{"dev_depth", dev_depth, depth_bytes, need, 4, false}, dst})) return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ring_leave(ctx)) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  FRM_HIP(ctx, launch_dof(dev_src, dev_depth, dev_dst, width, height, aperture, focus, max_radius, s));
  return FRM_OK;
}

int frm_group_band_rows(uint32_t height, uint32_t devices, uint32_t* out_band_rows) {
  if (!out_band_rows || height == 0 || devices == 0 || devices > FRM_MAX_DEVICES)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "invalid height %u or device count %u", height, devices);
  *out_band_rows = group_band_rows(height, devices);
  return FRM_OK;
}

int frm_band_rows_for(uint32_t height, uint32_t band_rows, uint32_t first_band, uint32_t band_stride,
                      uint32_t* out_rows) {
  if (!out_rows || height == 0 || band_rows == 0 || band_stride == 0)
    return fail(nullptr, FRM_ERR_INVALID_ARGUMENT, "invalid band geometry");
  return band_rows_u32(nullptr, height, band_rows, first_band, band_stride, out_rows);
}

int frm_unshuffle_bands(frm_ctx* ctx, const uint8_t* dev_src, size_t rank_stride_bytes, uint8_t* dev_dst,
                        size_t dst_bytes, uint32_t band_rows, uint32_t ranks, void* stream) {
  if (!ctx || !dev_src || !dev_dst || band_rows == 0 || ranks == 0)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "invalid unshuffle arguments");
  if (frame_mode(ctx) != kPlain) return refuse_mode(ctx, "frm_unshuffle_bands");
  if (!ctx->width) return fail(ctx, FRM_ERR_NOT_READY, "frm_resize has not been called");
  size_t need = (size_t)ctx->width * ctx->height * 4u;
  if (dst_bytes < need)
    return fail(ctx, FRM_ERR_BUFFER_TOO_SMALL, "dst holds %zu bytes, frame needs %zu", dst_bytes, need);
  uint32_t rows = 0;
  if (int rc = band_rows_u32(ctx, ctx->height, band_rows, 0, ranks, &rows)) return rc;
  if (rank_stride_bytes < (size_t)rows * ctx->width * 4u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "rank stride %zu below one rank's bands", rank_stride_bytes);
  if (rank_stride_bytes % 4u)
    return fail(ctx, FRM_ERR_INVALID_ARGUMENT, "rank stride must be a multiple of 4");
  // what the call reads of dev_src: from its start to the end of the rows of the last rank that holds
  // a band (the ranks beyond the frame's bands are never touched)
  const uint32_t nb = num_bands(ctx->height, band_rows), holders = ranks < nb ? ranks : nb;
  uint32_t last_rows = 0;
  if (int rc = band_rows_u32(ctx, ctx->height, band_rows, holders - 1u, ranks, &last_rows)) return rc;
  size_t src_need = 0;
  if (int rc = strided_need(ctx, rank_stride_bytes, (size_t)last_rows * ctx->width * 4u, holders, &src_need)) return rc;
  if (int rc = check_spans(ctx, {{"dev_src", dev_src, src_need, src_need, 4, false},
                                 {"dev_dst", dev_dst, dst_bytes, need, 4, true}}))
    return rc;
  FRM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  FRM_HIP(ctx, launch_unshuffle(dev_src, rank_stride_bytes, dev_dst, ctx->width, ctx->height, band_rows,
                                ranks, s));
  return FRM_OK;
}

}  // extern "C"
