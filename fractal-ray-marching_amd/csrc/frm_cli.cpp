// frm_render — offscreen CLI over libfrm: renders frames of a
// reference scene and writes binary PPMs (P6, sRGB bytes), replacing the reference's
// `present` (graphics.rs:101-108) for offline use. With --frames F > 1 it is a scripted
// fly-through: each frame runs the reference's update order (initialized_app.rs:43-48)
// through libfrm's restatement of Timing and Camera (frm_timing_*, frm_camera_*):
// time += time_factor * dt; camera.update(held keys, dt); parameters.update_camera.
//   frm_render [--width W] [--height H] [--scene S] [--iters N] [--time T]
//              [--max-steps M] [--pos X Y Z] [--yaw A] [--pitch B] [--device D]
//              [--simple] [--sphere] [--out file.ppm | pattern_%04d.ppm]
//              [--frames F] [--dt S] [--keys BITS] [--orbit RAD_PER_S]
//              [--lock-yaw 0..4] [--lock-pitch] [--time-factor X] [--gpus N] [--batch B]
//              [--ssaa K] [--adaptive S] [--edge-threshold T] [--shutter-samples T] [--shutter F]
//              [--panorama] [--face-size N]
//              [--dof-aperture A --dof-focus F [--dof-radius R]] [--depth-out file.pfm]
// With --dof-aperture A and --dof-focus F every frame is blurred by a thin lens
// (frm_set_depth_of_field): A is the blur radius, in pixels, of a point at infinity, F the ray
// distance in focus, R (--dof-radius, 1..16, default 16) the largest radius. Works with --frames /
// --orbit / --out pattern; not with --ssaa, --adaptive, --shutter-samples, --panorama, --batch or
// --gpus. --depth-out writes the last frame's depth plane (frm_read_depth: the primary hit distance,
// +inf for a miss) as a little-endian single-channel PFM, bottom row first as the format has it; it
// needs a single-GPU run whose frames are plain or depth-of-field frames on the persistent kernel.
// With --panorama every frame is a 360-degree equirectangular one around the camera
// (frm_set_panorama): --width / --height are the panorama's size, the six cube faces have N texels
// a side (--face-size, default frm_panorama_face_size(W) = ceil(W / 4)) and the JSON lines count all
// six. Works with --frames / --orbit / --out pattern; not with --ssaa, --adaptive,
// --shutter-samples, --batch or --gpus.
// With --shutter-samples T (1..32, default 1) every frame is motion-blurred: the mean, in linear
// light, of T sub-frames that step the frame's own state (time, camera) through the fraction F
// (--shutter, 0 < F <= 1, default 0.5) of --dt (frm_shutter_parameters, frm_render_shutter). The main
// trajectory advances by dt as without it; the JSON lines count all T sub-frames. Combines with
// --ssaa; not with --batch, --adaptive or --gpus (the shutter already batches its sub-frames).
// With --ssaa K (1..4) every frame is rendered with K x K samples per pixel and resolved in linear
// light (frm_set_supersampling); W x H stay the size of the written frames, the work counters in
// the JSON lines are those of the (K*W) x (K*H) frame rendered. With --batch the context stays plain
// at that size and each frame goes through frm_resolve before it is copied to the host.
// With --adaptive S (1..4) every frame is rendered plainly and the pixels whose 3 x 3 neighbourhood has a
// contrast of at least T sRGB codes (--edge-threshold, 0..256, default FRM_ADAPTIVE_DEFAULT_THRESHOLD)
// are replaced by the resolve of their S x S samples (frm_set_adaptive); the JSON lines count the
// plain frame plus the refined samples and give the number of refined pixels. With --batch each
// frame goes through frm_refine with its own parameters. Not together with --ssaa.
// With --batch B (one context) the fly-through's frames are rendered B per launch
// (frm_render_bands_batch: one work queue for B frames whose camera and, for the Mandelbulb,
// time differ), so a launch's tail is paid once per B frames; the frames' bytes are the same.
// With --gpus N every frame is row-tiled across devices 0..N-1 from this one process: the CLI
// creates a group context (frm_config.device_count = N, include/frm.h), in which device r renders
// the interleaved bands r, r+N, ..., RCCL point-to-point transfers gather the bands on device 0
// over xGMI and device 0 reassembles the frame. Everything else is the one-GPU
// loop: frm_render + frm_read_frame, the config alone selects the GPUs.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "frm.h"

static void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    fprintf(stderr, "frm_render: %s failed: %s\n", what, hipGetErrorString(e));
    exit(1);
  }
}

static int check(int rc, frm_ctx* ctx, const char* what) {
  if (rc != FRM_OK) {
    fprintf(stderr, "frm_render: %s failed (%d): %s\n", what, rc, frm_last_error(ctx));
    exit(1);
  }
  return rc;
}

// An option's integer in [lo, hi], or its float in (0, hi] (positive) or [0, hi]; anything else ends
// the run with the option's complaint.
static uint32_t parse_uint(const char* opt, const char* v, long lo, long hi) {
  char* end = nullptr;
  const long k = strtol(v, &end, 10);
  if (end == v || *end || k < lo || k > hi) {
    fprintf(stderr, "frm_render: %s %s outside [%ld, %ld]\n", opt, v, lo, hi);
    exit(2);
  }
  return (uint32_t)k;
}
static float parse_float(const char* opt, const char* v, bool positive, float hi, const char* complaint) {
  char* end = nullptr;
  const float x = strtof(v, &end);
  if (end == v || *end || !(positive ? x > 0.0f : x >= 0.0f) || x > hi) {
    fprintf(stderr, "frm_render: %s %s%s\n", opt, v, complaint);
    exit(2);
  }
  return x;
}

static int write_ppm(const char* out, uint32_t fr, const uint8_t* rgba, uint32_t width, uint32_t height,
                     char* name, size_t name_len) {
  if (strchr(out, '%')) snprintf(name, name_len, out, fr);
  else snprintf(name, name_len, "%s", out);
  FILE* f = fopen(name, "wb");
  if (!f) {
    perror(name);
    return 1;
  }
  fprintf(f, "P6\n%u %u\n255\n", width, height);
  for (size_t i = 0; i < (size_t)width * height; ++i) fwrite(&rgba[4 * i], 1, 3, f);
  fclose(f);
  return 0;
}

// --batch: the fly-through's Parameters first (the same update order as the per-frame loop),
// then B frames per frm_render_bands_batch launch into a device buffer, each written as a PPM.
// kernel_ms is the launch's wall time (frm_synchronize) over its frames; the work counters are
// the launch's, reported per launch.
static int render_batched(frm_ctx* ctx, frm_parameters p, frm_camera cam, frm_timing timing, uint32_t keys,
                          float dt, uint32_t frames, uint32_t batch, uint32_t width, uint32_t height,
                          uint32_t ssaa, uint32_t adaptive, uint32_t edge_threshold, float shutter, const char* out) {
  std::vector<frm_parameters> ps(frames);
  std::vector<frm_camera> cams(frames);
  for (uint32_t fr = 0; fr < frames; ++fr) {
    if (fr > 0) {
      const float delta = frm_timing_update(&timing, &p, dt);
      frm_camera_update(&cam, keys, delta);
      frm_parameters_update_camera_from(&p, &cam);
    }
    ps[fr] = p;
    cams[fr] = cam;
  }
  // the context renders ssaa x the output size; `width` x `height` frames of `ofb` bytes are written
  const uint32_t rh = ssaa * height;
  const size_t ofb = (size_t)width * height * 4, fb = ofb * ssaa * ssaa;
  uint8_t *dev = nullptr, *resolved = nullptr;
  uint64_t* dcnt = nullptr;
  hip_check(hipMalloc(&dev, fb * batch), "hipMalloc");
  if (ssaa > 1 || adaptive > 1) hip_check(hipMalloc(&resolved, ofb * batch), "hipMalloc");
  // the launch's counters, then one set per frame for its refined samples (--adaptive)
  hip_check(hipMalloc(&dcnt, (1 + (size_t)batch) * FRM_NUM_COUNTERS * sizeof(uint64_t)), "hipMalloc");
  std::vector<uint64_t> rc((size_t)batch * FRM_NUM_COUNTERS);
  std::vector<uint8_t> host(ofb * batch);
  char name[4096];
  for (uint32_t g = 0; g < frames; g += batch) {
    const uint32_t n = frames - g < batch ? frames - g : batch;
    hip_check(hipMemset(dcnt, 0, (1 + (size_t)batch) * FRM_NUM_COUNTERS * sizeof(uint64_t)), "hipMemset");
    const auto t0 = std::chrono::steady_clock::now();
    check(frm_render_bands_batch(ctx, n, &ps[g], dev, fb * n, fb, rh, 0, 1, nullptr, dcnt), ctx,
          "frm_render_bands_batch");
    for (uint32_t b = 0; b < n && ssaa > 1; ++b)  // on the context's stream, after the launch
      check(frm_resolve(ctx, dev + fb * b, fb, width, height, ssaa, resolved + ofb * b, ofb, nullptr), ctx,
            "frm_resolve");
    for (uint32_t b = 0; b < n && adaptive > 1; ++b)  // each frame's samples follow its own parameters
      check(frm_refine(ctx, &ps[g + b], dev + fb * b, fb, width, height, adaptive, edge_threshold, resolved + ofb * b,
                       ofb, dcnt + (1 + b) * FRM_NUM_COUNTERS, nullptr),
            ctx, "frm_refine");
    check(frm_synchronize(ctx), ctx, "frm_synchronize");
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    uint64_t c[FRM_NUM_COUNTERS];
    hip_check(hipMemcpy(c, dcnt, sizeof(c), hipMemcpyDeviceToHost), "hipMemcpy");
    hip_check(hipMemcpy(rc.data(), dcnt + FRM_NUM_COUNTERS, rc.size() * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy");
    for (uint32_t b = 0; b < n; ++b)  // the launch's work: its frames plus their refined samples
      for (uint32_t k = 0; k < FRM_NUM_COUNTERS; ++k) c[k] += rc[(size_t)b * FRM_NUM_COUNTERS + k];
    hip_check(hipMemcpy(host.data(), resolved ? resolved : dev, ofb * n, hipMemcpyDeviceToHost), "hipMemcpy");
    for (uint32_t b = 0; b < n; ++b) {
      const uint32_t fr = g + b;
      if (write_ppm(out, fr, &host[ofb * b], width, height, name, sizeof(name))) return 1;
      printf("{\"frame\": %u, \"out\": \"%s\", \"width\": %u, \"height\": %u, \"time\": %.6f, "
             "\"pos\": [%.5f, %.5f, %.5f], \"yaw\": %.5f, \"pitch\": %.5f, \"kernel_ms\": %.3f, "
             "\"batch\": %u, \"launch_march_steps\": %llu, \"launch_hit_pixels\": %llu, \"gsteps_per_s\": %.3f, "
             "\"ssaa\": %u, \"adaptive\": %u, \"edge_threshold\": %u, \"refined_pixels\": %llu, "
             "\"shutter_samples\": 1, \"shutter\": %.6f, \"panorama\": 0, \"face_size\": 0}\n",
             fr, name, width, height, ps[fr].time, cams[fr].position[0], cams[fr].position[1], cams[fr].position[2],
             cams[fr].yaw, cams[fr].pitch, ms / n, n, (unsigned long long)(c[2] + c[3]), (unsigned long long)c[1],
             (double)(c[2] + c[3]) / (ms * 1e-3) / 1e9, ssaa, adaptive, edge_threshold,
             (unsigned long long)(rc[(size_t)b * FRM_NUM_COUNTERS] / (adaptive * adaptive)), shutter);
    }
  }
  (void)hipFree(dev);
  (void)hipFree(resolved);
  (void)hipFree(dcnt);
  frm_destroy(ctx);
  return 0;
}

int main(int argc, char** argv) {
  uint32_t width = 1920, height = 1080, scene = 18, iters = 12, max_steps = 256;
  float time = 3.2175055f, pos[3] = {0.0f, 0.0f, -1.6f}, yaw = 0.0f, pitch = 0.0f;
  int device = 0;
  uint32_t flags = 0;
  const char* out = "frame.ppm";
  uint32_t frames = 1, keys = 0;
  float dt = 1.0f / 60.0f, orbit = 0.0f, time_factor = 1.0f;
  int lock_yaw = FRM_LOCK_YAW_NONE, lock_pitch = 0;
  uint32_t gpus = 0;  // 0: one GPU (--device); >= 1: a group context over devices 0..gpus-1
  uint32_t batch = 1;  // frames per launch (one context)
  uint32_t ssaa = 1;   // samples per pixel and axis
  uint32_t adaptive = 1, edge_threshold = FRM_ADAPTIVE_DEFAULT_THRESHOLD;  // --adaptive, --edge-threshold
  bool ssaa_given = false, adaptive_given = false;
  uint32_t shutter_samples = 1;  // sub-frames per frame
  float shutter = 0.5f;          // the fraction of dt they span
  bool panorama = false;
  uint32_t face_size = 0;  // 0: frm_panorama_face_size(width)
  float dof_aperture = 0.0f, dof_focus = 0.0f;
  uint32_t dof_radius = FRM_MAX_DOF_RADIUS;
  bool dof_aperture_given = false, dof_focus_given = false, dof_radius_given = false;
  const char* depth_out = nullptr;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    auto next = [&](void) -> const char* {
      if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", a); exit(2); }
      return argv[++i];
    };
    if (!strcmp(a, "--width")) width = (uint32_t)atoi(next());
    else if (!strcmp(a, "--height")) height = (uint32_t)atoi(next());
    else if (!strcmp(a, "--scene")) scene = (uint32_t)atoi(next());
    else if (!strcmp(a, "--iters")) iters = (uint32_t)atoi(next());
    else if (!strcmp(a, "--time")) time = (float)atof(next());
    else if (!strcmp(a, "--max-steps")) max_steps = (uint32_t)atoi(next());
    else if (!strcmp(a, "--pos")) { pos[0] = (float)atof(next()); pos[1] = (float)atof(next()); pos[2] = (float)atof(next()); }
    else if (!strcmp(a, "--yaw")) yaw = (float)atof(next());
    else if (!strcmp(a, "--pitch")) pitch = (float)atof(next());
    else if (!strcmp(a, "--device")) device = atoi(next());
    else if (!strcmp(a, "--simple")) flags |= FRM_FLAG_SIMPLE_KERNEL;
    else if (!strcmp(a, "--sphere")) flags |= FRM_FLAG_SCENE_SPHERE;
    else if (!strcmp(a, "--out")) out = next();
    else if (!strcmp(a, "--frames")) frames = (uint32_t)atoi(next());
    else if (!strcmp(a, "--dt")) dt = (float)atof(next());
    else if (!strcmp(a, "--keys")) keys = (uint32_t)strtoul(next(), nullptr, 0);
    else if (!strcmp(a, "--orbit")) orbit = (float)atof(next());
    else if (!strcmp(a, "--lock-yaw")) lock_yaw = atoi(next());
    else if (!strcmp(a, "--lock-pitch")) lock_pitch = 1;
    else if (!strcmp(a, "--time-factor")) time_factor = (float)atof(next());
    else if (!strcmp(a, "--gpus")) gpus = (uint32_t)atoi(next());
    else if (!strcmp(a, "--batch")) batch = (uint32_t)atoi(next());
    else if (!strcmp(a, "--ssaa")) { ssaa = parse_uint(a, next(), 1, FRM_MAX_SUPERSAMPLE); ssaa_given = true; }
    else if (!strcmp(a, "--adaptive")) { adaptive = parse_uint(a, next(), 1, FRM_MAX_SUPERSAMPLE); adaptive_given = true; }
    else if (!strcmp(a, "--edge-threshold")) { edge_threshold = parse_uint(a, next(), 0, 256); adaptive_given = true; }
    else if (!strcmp(a, "--shutter-samples")) shutter_samples = parse_uint(a, next(), 1, FRM_MAX_SHUTTER_SAMPLES);
    else if (!strcmp(a, "--shutter")) shutter = parse_float(a, next(), true, 1.0f, " outside (0, 1]");
    else if (!strcmp(a, "--panorama")) panorama = true;
    else if (!strcmp(a, "--face-size")) face_size = parse_uint(a, next(), 1, FRM_MAX_DIMENSION - 2);
    else if (!strcmp(a, "--dof-aperture")) {
      dof_aperture = parse_float(a, next(), false, 3.402823466e+38f, ": not a finite non-negative number");
      dof_aperture_given = true;
    }
    else if (!strcmp(a, "--dof-focus")) {
      dof_focus = parse_float(a, next(), true, 3.402823466e+38f, ": not a finite positive number");
      dof_focus_given = true;
    }
    else if (!strcmp(a, "--dof-radius")) { dof_radius = parse_uint(a, next(), 1, FRM_MAX_DOF_RADIUS); dof_radius_given = true; }
    else if (!strcmp(a, "--depth-out")) depth_out = next();
    else { fprintf(stderr, "unknown argument %s\n", a); return 2; }
  }
  const bool dof = dof_aperture_given || dof_focus_given || dof_radius_given;
  // what may not be combined: (the options given, what they exclude or lack, the complaint), the first
  // that holds is reported
  const bool many = batch > 1 || gpus > 0, blur = shutter_samples > 1;
  const struct {
    bool given, clash;
    const char* complaint;
  } rules[] = {
      {dof, !(dof_aperture_given && dof_focus_given), "depth of field needs both --dof-aperture and --dof-focus"},
      {dof, ssaa_given || adaptive_given || blur || panorama || many,
       "--dof-* excludes --ssaa, --adaptive, --shutter-samples, --panorama, --batch and --gpus "
       "(the gather works on one plain frame and its depth)"},
      {dof, (flags & FRM_FLAG_SIMPLE_KERNEL) != 0,
       "--dof-* excludes --simple (the depth plane comes from the persistent kernel)"},
      {depth_out != nullptr, many || panorama || blur,
       "--depth-out excludes --batch, --gpus, --panorama and --shutter-samples (no single frame's depth)"},
      {face_size != 0, !panorama, "--face-size needs --panorama"},
      {panorama, ssaa_given || adaptive_given || blur || many,
       "--panorama excludes --ssaa, --adaptive, --shutter-samples, --batch and --gpus (for an "
       "anti-aliased panorama project the faces to a larger frame with frm_project_equirect and "
       "frm_resolve it)"},
      {ssaa_given, adaptive_given, "--adaptive / --edge-threshold and --ssaa exclude each other"},
      {blur, many || adaptive > 1,
       "--shutter-samples excludes --batch, --adaptive and --gpus (frm_render_shutter batches "
       "its sub-frames on one plain or supersampled context)"},
  };
  for (const auto& r : rules)
    if (r.given && r.clash) {
      fprintf(stderr, "frm_render: %s\n", r.complaint);
      return 2;
    }
  if (panorama && !face_size && frm_panorama_face_size(width, &face_size) != FRM_OK) {
    fprintf(stderr, "frm_render: --panorama: %s\n", frm_last_error(nullptr));
    return 2;
  }
  frm_ctx* ctx = nullptr;
  frm_config cfg = {device, max_steps, flags, 0, 0, {0}};
  if (gpus > 0) {
    int count = 0;
    hip_check(hipGetDeviceCount(&count), "hipGetDeviceCount");
    if ((int)gpus > count || gpus > FRM_MAX_DEVICES) {
      fprintf(stderr, "frm_render: --gpus %u but %d devices (at most %u)\n", gpus, count, FRM_MAX_DEVICES);
      return 2;
    }
    cfg.device_count = gpus;  // a group context: devices 0..gpus-1
    for (uint32_t r = 0; r < gpus; ++r) cfg.devices[r] = (int32_t)r;
  }
  check(frm_create(&ctx, &cfg), nullptr, "frm_create");
  frm_parameters p;
  frm_parameters_default(&p);
  frm_parameters_update_aspect(&p, width, height);
  p.time = time;
  p.num_iterations = iters;
  p.scene_index = scene;
  frm_camera cam;
  frm_camera_default(&cam);
  for (int k = 0; k < 3; ++k) cam.position[k] = pos[k];
  cam.yaw = yaw;
  cam.pitch = pitch;
  cam.orbit_angle_per_second = orbit;
  cam.lock_yaw_mode = lock_yaw;
  cam.lock_pitch = lock_pitch;
  frm_timing timing;
  frm_timing_init(&timing);
  timing.time_factor = time_factor;
  frm_parameters_update_camera_from(&p, &cam);
  if (batch < 1 || batch > FRM_MAX_BATCH) {
    fprintf(stderr, "frm_render: --batch %u outside [1, %u]\n", batch, FRM_MAX_BATCH);
    return 2;
  }
  // --batch drives the bands itself: a plain context at the render size, resolved frame by frame
  if (batch > 1) {
    check(frm_resize(ctx, ssaa * width, ssaa * height), ctx, "frm_resize");
  } else {
    check(frm_set_supersampling(ctx, ssaa), ctx, "frm_set_supersampling");
    check(frm_resize(ctx, width, height), ctx, "frm_resize");
    check(frm_set_adaptive(ctx, adaptive, edge_threshold), ctx, "frm_set_adaptive");
    if (panorama) check(frm_set_panorama(ctx, face_size), ctx, "frm_set_panorama");
    if (dof) check(frm_set_depth_of_field(ctx, dof_aperture, dof_focus, dof_radius), ctx, "frm_set_depth_of_field");
  }
  std::vector<uint8_t> rgba((size_t)width * height * 4);
  if (batch > 1 && gpus > 0) {
    fprintf(stderr, "frm_render: --batch renders on one GPU (frm_render_bands_batch is a per-device entry point)\n");
    return 2;
  }
  if (batch > 1) return render_batched(ctx, p, cam, timing, keys, dt, frames, batch, width, height, ssaa, adaptive,
                                   edge_threshold, shutter, out);
  std::vector<frm_parameters> sub(shutter_samples);
  for (uint32_t fr = 0; fr < frames; ++fr) {
    if (fr > 0) {  // initialized_app.rs:43-48, with a fixed frame time
      const float delta = frm_timing_update(&timing, &p, dt);
      frm_camera_update(&cam, keys, delta);
      frm_parameters_update_camera_from(&p, &cam);
    }
    frm_stats st;
    memset(&st, 0, sizeof(st));
    if (shutter_samples > 1) {  // the frame's own state stepped through the shutter interval
      frm_shutter_parameters(&p, &cam, &timing, keys, dt, shutter_samples, shutter, sub.data());
      check(frm_render_shutter(ctx, shutter_samples, sub.data(), &st), ctx, "frm_render_shutter");
    } else {
      check(frm_set_parameters(ctx, &p), ctx, "frm_set_parameters");
      check(frm_render(ctx, &st), ctx, "frm_render");  // a group: render, gather and reassembly
    }
    check(frm_read_frame(ctx, rgba.data(), rgba.size()), ctx, "frm_read_frame");
    char name[4096];
    if (write_ppm(out, fr, rgba.data(), width, height, name, sizeof(name))) return 1;
    printf("{\"frame\": %u, \"out\": \"%s\", \"width\": %u, \"height\": %u, \"time\": %.6f, "
           "\"pos\": [%.5f, %.5f, %.5f], \"yaw\": %.5f, \"pitch\": %.5f, \"kernel_ms\": %.3f, "
           "\"march_steps\": %llu, \"hit_pixels\": %llu, \"gsteps_per_s\": %.3f, \"ssaa\": %u, "
           "\"adaptive\": %u, \"edge_threshold\": %u, \"refined_pixels\": %llu, \"shutter_samples\": %u, "
           "\"shutter\": %.6f, \"panorama\": %u, \"face_size\": %u, \"dof_aperture\": %.6f, "
           "\"dof_focus\": %.6f, \"dof_radius\": %u}\n",
           fr, name, width, height, p.time, cam.position[0], cam.position[1], cam.position[2], cam.yaw,
           cam.pitch, st.kernel_ms, (unsigned long long)st.march_steps, (unsigned long long)st.hit_pixels,
           st.march_steps / (st.kernel_ms * 1e-3) / 1e9, ssaa, adaptive, edge_threshold,
           (unsigned long long)(adaptive > 1 ? (st.pixels - (uint64_t)width * height) / (adaptive * adaptive) : 0),
           shutter_samples, shutter, panorama ? 1u : 0u, face_size, dof ? dof_aperture : 0.0f, dof ? dof_focus : 0.0f,
           dof ? dof_radius : 0u);
  }
  if (depth_out) {  // the last frame's; the render size (--ssaa: the supersampled frame's)
    const uint32_t dw = ssaa * width, dh = ssaa * height;
    std::vector<float> depth((size_t)dw * dh);
    check(frm_read_depth(ctx, depth.data(), depth.size()), ctx, "frm_read_depth");
    FILE* f = fopen(depth_out, "wb");
    if (!f) { perror(depth_out); return 1; }
    fprintf(f, "Pf\n%u %u\n-1.0\n", dw, dh);  // a negative scale: little-endian floats
    for (uint32_t y = dh; y-- > 0;) fwrite(&depth[(size_t)y * dw], sizeof(float), dw, f);
    fclose(f);
  }
  frm_destroy(ctx);
  return 0;
}
