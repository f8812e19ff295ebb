/*
 * frm.h — C ABI of the MI355X-native offscreen fractal ray-marcher (libfrm.so).
 *
 * This is the drop-in boundary that replaces the reference's wgpu graphics layer
 * (MariusDoe/fractal-ray-marching: src/graphics.rs, src/persistent_graphics.rs,
 * src/reloadable_graphics.rs, src/blit_graphics.rs) for the one hot path the
 * reference has: the per-pixel sphere tracer `fragment_main` in src/fragment.wgsl:327-349.
 * The caller keeps the reference's own `Parameters` uniform (src/parameters.rs:6-15)
 * byte for byte; `frm_parameters` below is that struct.
 *
 * Conventions
 *   - Every entry point returns an `int` status (FRM_OK = 0). Nothing aborts, throws
 *     or panics across the ABI. The message of the last failure on a context is
 *     available from frm_last_error(); failures before a context exists are available
 *     from frm_last_error(NULL) (thread-local).
 *   - A context drives one GPU, or with frm_config.device_count a group of GPUs row-tiling
 *     each frame, and is not thread-safe (one context per host thread), mirroring the
 *     reference's single winit event-loop thread (src/app.rs).
 *   - Rendering is stream-ordered. frm_render() with a NULL stats pointer is
 *     asynchronous; frm_read_frame()/frm_synchronize() wait for it. With
 *     frames_in_flight > 1, consecutive frm_render() calls run on rotating streams and
 *     may overlap on the GPU; frm_read_frame()/frm_present() see the last one.
 *   - Plain pointers and sizes only; `void* stream` is a hipStream_t (NULL = the
 *     context's own stream).
 */
#ifndef FRM_H
#define FRM_H

#if !defined(__HIPCC_RTC__) /* hiprtc (frm_reload) defines the fixed-width types itself */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FRM_ABI_VERSION 5u  /* 2: frm_config.frames_in_flight (was reserved); 3: frm_render_bands_batch
                               takes dst_bytes, frm_set_parameters bounds the fractal loop work;
                               4: asynchronous readback (frm_read_frame_async, frm_present_async,
                               frm_frame_pixels); 5: frm_config.device_count / devices (one context
                               row-tiles every frame over several GPUs, RCCL gather) */

/* ---- status codes -------------------------------------------------------- */
enum {
  FRM_OK = 0,
  FRM_ERR_INVALID_ARGUMENT = 1, /* NULL pointer, zero size, out-of-range value       */
  FRM_ERR_NO_DEVICE = 2,        /* no HIP device / device index out of range          */
  FRM_ERR_HIP = 3,              /* a HIP runtime call failed (message has the name)   */
  FRM_ERR_OUT_OF_MEMORY = 4,    /* device allocation failed                           */
  FRM_ERR_NOT_READY = 5,        /* frm_render before frm_resize / frm_set_parameters  */
  FRM_ERR_BUFFER_TOO_SMALL = 6, /* destination smaller than the frame or band set      */
  FRM_ERR_UNSUPPORTED = 7,      /* an operation this build does not support            */
  FRM_ERR_COMPILE = 8           /* frm_reload: the sources failed to compile (log in last_error) */
};

/* ---- the reference's uniform, byte for byte -------------------------------
 * src/parameters.rs:6-15 (#[repr(C)], bytemuck Pod) mirrored in WGSL at
 * src/fragment.wgsl:108-116. Offsets: camera_matrix 0, aspect_scale 64, time 72,
 * num_iterations 76, scene_index 80, padding 84; sizeof == 96.
 * camera_matrix holds the TRANSPOSE of the cgmath camera matrix in column-major
 * order (parameters.rs:23-25), i.e. camera_matrix[4*j + i] = C[row j][col i]; the
 * kernel computes C·v exactly like `(v * camera_matrix)` in fragment.wgsl:315-317. */
typedef struct frm_parameters {
  float camera_matrix[16];
  float aspect_scale[2];
  float time;
  uint32_t num_iterations;
  uint32_t scene_index;
  uint8_t padding[12];
} frm_parameters;

#if defined(__HIPCC_RTC__)
static_assert(sizeof(frm_parameters) == 96, "frm_parameters must be 96 bytes");
#elif defined(__cplusplus)
static_assert(sizeof(frm_parameters) == 96, "frm_parameters must be 96 bytes");
static_assert(offsetof(frm_parameters, aspect_scale) == 64, "aspect_scale @64");
static_assert(offsetof(frm_parameters, time) == 72, "time @72");
static_assert(offsetof(frm_parameters, num_iterations) == 76, "num_iterations @76");
static_assert(offsetof(frm_parameters, scene_index) == 80, "scene_index @80");
#else
_Static_assert(sizeof(frm_parameters) == 96, "frm_parameters must be 96 bytes");
#endif

#define FRM_NUM_SCENES 19u            /* parameters.rs:35 (NUM_SCENES)                 */
#define FRM_DEFAULT_MAX_STEPS 5000u   /* fragment.wgsl:4 (MAX_ITERATIONS)              */
/* Largest fractal loop trip count (Menger/Koch/Sierpinski folds, Mandelbulb bodies - 1) that
 * frm_set_parameters accepts without FRM_FLAG_UNBOUNDED_ITERATIONS. num_iterations is any u32
 * in the reference (update_num_iterations saturates, parameters.rs:31-33), and every DE runs
 * O(num_iterations) loop bodies (fragment.wgsl:181,207,226,245), so a frame near 2^32 runs for
 * days; such parameters get FRM_ERR_UNSUPPORTED unless the context opted out. Sierpinski's
 * i32 loop runs no fold for N >= 2^31 (fragment.wgsl:181), which is cheap and always accepted.
 * The Mandelbulb's `i <= N` loop (fragment.wgsl:245) never ends for N = 0xffffffff (the u32
 * counter wraps first; the reference hangs too): refused even with the opt-out. */
#define FRM_MAX_NUM_ITERATIONS 65536u
#define FRM_MAX_DIMENSION 32768u      /* width/height limit per frame                  */

/* config flags */
#define FRM_FLAG_SCENE_SPHERE 0x1u  /* build-only extension scene for BASELINE config C1:
                                       DE = length(p) - 0.5, colour = colorize(p). Not in
                                       the reference (its out-of-range scene ids map to 0). */
#define FRM_FLAG_SIMPLE_KERNEL 0x2u /* use the one-thread-per-pixel kernel instead of the
                                       persistent ray-regeneration kernel (same bytes). */
#define FRM_FLAG_PERSISTENT_KERNEL 0x4u /* always use the persistent kernel. With neither
                                       kernel flag the context picks per launch: simple
                                       below one resident persistent grid of pixels
                                       (frm_kernel_for_pixels), persistent above. */
#define FRM_FLAG_UNBOUNDED_ITERATIONS 0x8u /* accept num_iterations above FRM_MAX_NUM_ITERATIONS
                                       (the caller accepts frames whose cost grows with it) */
#define FRM_FLAG_HW_MATH 0x10u      /* OPT-IN, NOT BIT-EXACT: the Mandelbulb (scene 18) body, magnitude
                                       and distance on the GPU's hardware transcendentals (v_log,
                                       v_exp, v_sin, v_cos, v_sqrt, v_rcp), as a Vulkan driver lowers
                                       fragment.wgsl's builtins (WGSL leaves their precision to the
                                       implementation). Faster; frames differ from the oracle's and
                                       are checked by the classified comparison against precise
                                       builtins. Other scenes and the shading
                                       are unchanged (exact). Never the default. */

/* kernels (frm_kernel_for_pixels) */
#define FRM_KERNEL_PERSISTENT 0u
#define FRM_KERNEL_SIMPLE 1u

typedef struct frm_config {
  int32_t device;     /* HIP device ordinal (replaces the wgpu adapter request,
                         persistent_graphics.rs:43-50)                                 */
  uint32_t max_steps; /* march() step cap; 0 = FRM_DEFAULT_MAX_STEPS, at most
                         FRM_MAX_STEPS_LIMIT. It also feeds the ambient-occlusion term
                         (fragment.wgsl:289,342)                                         */
  uint32_t flags;     /* FRM_FLAG_*                                                    */
  uint32_t frames_in_flight; /* frames a context may have in flight on the GPU at once,
                         1..FRM_MAX_FRAMES_IN_FLIGHT (0 = 1). Each render launch (frm_render,
                         frm_render_bands) takes the next of this many slots of device scratch
                         (pixel records, scheduling arrays, work queue; frm_render: also a
                         framebuffer and a stream), so frame k+1 runs while frame k's longest
                         pixels finish instead of after them. No reference counterpart: the
                         reference renders one frame per submit (graphics.rs:91-110).        */
  uint32_t device_count; /* 0: one GPU, `device` (every field above as before). 1..FRM_MAX_DEVICES:
                         a GROUP context over devices[0..device_count-1] (`device` ignored): every
                         frm_render row-tiles the frame over those GPUs (device r renders the
                         interleaved bands r, r+N, ..., as frm_render_bands with first_band r and
                         band_stride N), gathers the bands on devices[0] with RCCL point-to-point
                         transfers over xGMI (grouped ncclSend/ncclRecv; device-to-device copies
                         when a device is listed twice, e.g. to rehearse N ranks on one GPU) and
                         reassembles the frame there; frm_read_frame, frm_present and their async
                         forms then see the whole frame, exactly as on one GPU. The per-rank band
                         entry points (frm_render_bands*, frm_unshuffle_bands, frm_debug_trace,
                         frm_debug_*pixel_keys, frm_debug_pixel_order) are FRM_ERR_UNSUPPORTED on a group. No reference
                         counterpart (the reference is single-device, graphics.rs:25-37).       */
  int32_t devices[16];  /* HIP device ordinals of a group (FRM_MAX_DEVICES)                        */
} frm_config;

#define FRM_MAX_FRAMES_IN_FLIGHT 8u
#define FRM_MAX_DEVICES 16u
/* Band height a group context uses for a frame of `height` rows over `devices` GPUs: the smallest
 * height >= 16 that splits the frame into a multiple of `devices` bands (else 16), so the
 * interleaved bands balance the devices' work. */
int frm_group_band_rows(uint32_t height, uint32_t devices, uint32_t* out_band_rows);
/* largest frm_config.max_steps: the persistent kernel packs a pixel's primary step count
   into 22 bits of its 8-byte record (the reference's MAX_ITERATIONS is 5000) */
#define FRM_MAX_STEPS_LIMIT 4194303u

/* Work counters of one render (exact; equal to the CPU oracle's counts). */
typedef struct frm_stats {
  uint64_t pixels;          /* pixels shaded                                           */
  uint64_t hit_pixels;      /* primary march hits (distance >= 0, fragment.wgsl:334)   */
  uint64_t primary_steps;   /* scene() evaluations inside the primary march loop       */
  uint64_t shadow_steps;    /* scene() evaluations inside the shadow march loop        */
  uint64_t normal_evals;    /* scene() evaluations in calculate_normal (4 per hit)     */
  uint64_t fractal_bodies;  /* Mandelbulb loop bodies that ran to completion           */
  uint64_t fractal_bailouts;/* Mandelbulb loop exits by bailout                        */
  uint64_t march_steps;     /* primary_steps + shadow_steps (the headline unit)        */
  uint64_t wom_ops;         /* algorithmic VALU lane-ops of the frame */
  double kernel_ms;         /* device time of the render kernel(s) (HIP events)        */
} frm_stats;

typedef struct frm_ctx frm_ctx;

/* ---- lifecycle (replaces Graphics::init, graphics.rs:25-37) ------------------ */
int frm_create(frm_ctx** out_ctx, const frm_config* config);
int frm_destroy(frm_ctx* ctx);
const char* frm_last_error(const frm_ctx* ctx);
uint32_t frm_abi_version(void);
int frm_device_count(int32_t* out_count);

/* ---- frame size (replaces BlitGraphics::init / update_render_texture_size,
 *      graphics.rs:54-57, render_texture_config.rs:1-22). Sizes the device RGBA8
 *      framebuffer(s), pitch = 4*width. The caller sets aspect_scale with
 *      frm_parameters_update_aspect(width, height) semantics (parameters.rs:18-21).
 *      Asynchronous: frames in flight finish at their own size and their pending
 *      readbacks (frm_read_frame_async tickets) keep their bytes; the buffers of the new
 *      size are allocated in stream order (no host wait), as a wgpu texture re-creation
 *      does not stall the frames already submitted. */
int frm_resize(frm_ctx* ctx, uint32_t width, uint32_t height);

/* ---- supersampled anti-aliasing (the offline counterpart of the reference's `>`/`<`
 *      render-texture factor, render_texture_config.rs:1-22: render larger than shown). With a
 *      factor S > 1 every frm_render renders the (S*width) x (S*height) frame, whose pixel centres
 *      are exactly the S x S sub-sample centres of the width x height frame (aspect_scale stays the
 *      caller's, from width and height), and resolves it on the same stream: each output channel is
 *      the box mean of its S*S texels in linear light, as a filtering sampler over the
 *      Rgba8UnormSrgb render texture averages them: decoded (the blit's table), added in f32 row
 *      by row, left to right, divided by S*S (correctly rounded) and stored as the sRGB store
 *      does; alpha 255. frm_resize takes the OUTPUT size (factor x width and height at most
 *      FRM_MAX_DIMENSION); frm_read_frame, frm_present, their async forms and frm_frame_pixels see
 *      the resolved frame at that size. frm_stats counts the rendered frame (pixels = S*S x width
 *      x height) and kernel_ms includes the resolve; frm_debug_trace, frm_debug_*pixel_keys and
 *      frm_debug_pixel_order stay at the render size. Factor 1 (the default) allocates nothing and changes no path.
 * frm_set_supersampling: factor 1..FRM_MAX_SUPERSAMPLE (FRM_ERR_INVALID_ARGUMENT otherwise, or when
 *      the current size times the factor exceeds FRM_MAX_DIMENSION; the old factor stays). With a
 *      size set, a change acts as frm_resize of the current output size: no drain, frames in flight
 *      and their tickets keep their bytes and shapes, async readbacks give FRM_ERR_NOT_READY until
 *      the next frm_render. A group context applies it to every member. On a supersampled context
 *      frm_render_bands, frm_render_bands_batch and frm_unshuffle_bands are FRM_ERR_UNSUPPORTED
 *      (render the bands at S x the size on a plain context, then frm_resolve).
 * frm_resolve: the resolve alone, on any context, asynchronous on `stream`: dev_src holds
 *      factor*out_height rows of factor*out_width RGBA8 sRGB texels (pitch 4*factor*out_width),
 *      dev_dst out_height rows of out_width, both device memory of the context's GPU (devices[0]
 *      of a group), 4-byte aligned, not overlapping (FRM_ERR_INVALID_ARGUMENT otherwise;
 *      FRM_ERR_BUFFER_TOO_SMALL when src_bytes or dst_bytes is short). The source alpha is
 *      ignored; factor 1 copies the texels with alpha 255. */
#define FRM_MAX_SUPERSAMPLE 4u
int frm_set_supersampling(frm_ctx* ctx, uint32_t factor);
int frm_get_supersampling(const frm_ctx* ctx, uint32_t* out_factor);
int frm_resolve(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, uint32_t out_width,
                uint32_t out_height, uint32_t factor, uint8_t* dev_dst, size_t dst_bytes, void* stream);

/* ---- adaptive supersampling: the S x S samples of frm_set_supersampling(S), taken only where the
 *      plain frame has contrast. With F1 the plain width x height frame (frm_render's bytes without
 *      this) and FS the frame frm_set_supersampling(S) gives for the same size and parameters:
 *      output pixel (X, Y) is REFINED iff, over the 3 x 3 window around it clipped to the frame,
 *      max over R, G, B of (max - min of the 8-bit sRGB codes of F1) >= threshold (alpha ignored;
 *      threshold 0 refines every pixel, 256 none). The adaptive frame is FS where refined and F1
 *      elsewhere, alpha 255, bit for bit. The render size stays the output size; the frame is rendered
 *      as without this, then an edge pass and a refine pass run on the same stream.
 *      frm_read_frame, frm_present, their async forms and frm_frame_pixels see the adaptive frame.
 *      frm_stats holds F1's counters plus those of every refined sample (pixels = width x height +
 *      S*S x refined pixels); kernel_ms includes both passes. Known limit: a feature thinner than a
 *      pixel that no pixel centre of F1 hits leaves no contrast there and is not found.
 * frm_set_adaptive: factor 1 (the default) switches it off; factor in 1..FRM_MAX_SUPERSAMPLE and
 *      threshold in 0..256, and factor x the current size at most FRM_MAX_DIMENSION (which frm_resize
 *      checks on an adaptive context too), else FRM_ERR_INVALID_ARGUMENT and the old values stay.
 *      FRM_ERR_UNSUPPORTED (old values stay) with factor > 1 on a supersampled context, as is
 *      frm_set_supersampling(k > 1) on an adaptive one, and with runtime-reloaded kernels active, as
 *      is frm_reload(dir) on an adaptive one (the refine kernel is built in). A change takes effect at
 *      the next frm_render without a drain: frames in flight and their tickets keep their bytes, async
 *      readbacks give FRM_ERR_NOT_READY until that frm_render. A group context runs the two passes on
 *      devices[0] after the reassembly. On an adaptive context frm_render_bands,
 *      frm_render_bands_batch and frm_unshuffle_bands are FRM_ERR_UNSUPPORTED (render the bands on a
 *      plain context, then frm_refine), and frames never go through the resident ring.
 * frm_refine: the two passes alone, on any context, asynchronous on `stream`: dev_src holds the
 *      plain frame (height rows of width RGBA8 sRGB texels; it need not be a frame of that scene,
 *      refined pixels never read it), dev_dst receives the adaptive one; both device memory of the
 *      context's GPU, 4-byte aligned, not overlapping (FRM_ERR_INVALID_ARGUMENT otherwise;
 *      FRM_ERR_BUFFER_TOO_SMALL when src_bytes or dst_bytes is short). The samples are those of
 *      `params` (checked as frm_set_parameters checks them; NULL: the context's, FRM_ERR_NOT_READY
 *      without any) with the context's max_steps and flags. factor 1 copies the texels with alpha
 *      255. dev_counters: NULL, or FRM_NUM_COUNTERS device words to which the refined samples' work
 *      is added. Calls in flight on different streams are independent.
 * frm_debug_refine_mask: the edge mask of the last frm_render, if it was adaptive (FRM_ERR_NOT_READY
 *      otherwise): out[i] = 1 where pixel i (row-major) was refined, else 0, for the first
 *      min(n, width x height) pixels; returns that count, or a negative frm_status. Synchronises
 *      the frame. Additive: FRM_ABI_VERSION stays 5. */
#define FRM_ADAPTIVE_DEFAULT_THRESHOLD 16u   /* sRGB codes; a product default, not a measured optimum */
int frm_set_adaptive(frm_ctx* ctx, uint32_t factor, uint32_t threshold);
int frm_get_adaptive(const frm_ctx* ctx, uint32_t* out_factor, uint32_t* out_threshold);
int frm_refine(frm_ctx* ctx, const frm_parameters* params, const uint8_t* dev_src, size_t src_bytes,
               uint32_t width, uint32_t height, uint32_t factor, uint32_t threshold, uint8_t* dev_dst,
               size_t dst_bytes, uint64_t* dev_counters, void* stream);
int frm_debug_refine_mask(frm_ctx* ctx, uint8_t* out, size_t n);

/* ---- uniform upload (replaces Graphics::update_parameters_buffer,
 *      graphics.rs:59-61 → queue.write_buffer, persistent_graphics.rs:167-173).
 *      The struct is copied; it reaches the kernel by value. FRM_ERR_UNSUPPORTED (the previous
 *      parameters stay) when the scene's fractal loop would exceed FRM_MAX_NUM_ITERATIONS trips
 *      on a context without FRM_FLAG_UNBOUNDED_ITERATIONS, or never end (see above). */
int frm_set_parameters(frm_ctx* ctx, const frm_parameters* parameters);

/* ---- draw (replaces Graphics::render, graphics.rs:91-110). One full frame into
 *      the context framebuffer. stats == NULL: asynchronous. stats != NULL: waits
 *      for every frame in flight, then for this one, and fills the counters and
 *      kernel time. */
int frm_render(frm_ctx* ctx, frm_stats* stats);

/* ---- readback (replaces the blit pass + present, graphics.rs:101-108). Copies the
 *      whole RGBA8 sRGB frame (row 0 = top, 4*width*height bytes) to host memory. */
int frm_read_frame(frm_ctx* ctx, uint8_t* dst, size_t dst_bytes);

/* Present the last rendered frame at out_width x out_height into host dst (RGBA8 or BGRA8,
 * pitch 4*out_width): the reference's blit pass, which draws the render texture on the
 * window surface (blit.wgsl:6-11; graphics.rs:91-110) through a clamp-to-edge sampler with
 * linear magnification and nearest minification (persistent_graphics.rs:55-64), texels
 * read as linear light (the texture is Rgba8UnormSrgb, blit_graphics.rs:14). The surface
 * format is platform-chosen (persistent_graphics.rs:95): FRM_BLIT_SRGB encodes the output
 * as sRGB (an ...UnormSrgb surface) instead of linear unorm, FRM_BLIT_BGRA writes B,G,R,A.
 * Synchronous. Same size + FRM_BLIT_SRGB reproduces frm_read_frame's bytes. */
#define FRM_BLIT_SRGB 0x1u
#define FRM_BLIT_BGRA 0x2u
int frm_present(frm_ctx* ctx, uint32_t out_width, uint32_t out_height, uint32_t flags, uint8_t* dst,
                size_t dst_bytes);
/* frm_blit: that blit alone, on any context, asynchronous on `stream` (NULL: the context's):
 * dev_src holds src_height rows of src_width RGBA8 sRGB texels (pitch 4*src_width), dev_dst
 * receives out_height rows of out_width, both device memory of the context's GPU (devices[0]
 * of a group), 4-byte aligned, not overlapping, every size in [1, FRM_MAX_DIMENSION]
 * (FRM_ERR_INVALID_ARGUMENT otherwise, or for unknown flags; FRM_ERR_BUFFER_TOO_SMALL when
 * src_bytes or dst_bytes is short). The source alpha is ignored, the output alpha is 255.
 * frm_present(w, h, flags) is frm_blit of frm_read_frame's bytes. */
int frm_blit(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, uint32_t src_width, uint32_t src_height,
             uint8_t* dev_dst, size_t dst_bytes, uint32_t out_width, uint32_t out_height, uint32_t flags,
             void* stream);
int frm_synchronize(frm_ctx* ctx);

/* ---- asynchronous readback: presentation with a frame of latency, as the reference's
 *      surface has it. The reference configures its surface with wgpu's default
 *      (persistent_graphics.rs:158-162, Surface::get_default_config:
 *      desired_maximum_frame_latency = 2): present() and submit() return before the GPU has
 *      drawn the frame, so the CPU prepares frame k+1 while frame k renders. With
 *      frames_in_flight >= 2 the same loop on libfrm is
 *          frm_render(k); frm_read_frame_async(&t[k]);      (both return at once)
 *          frm_frame_pixels(t[k-1], &pixels);                (waits for frame k-1 only)
 *      so frame k is already queued behind frame k-1 and fills the GPU while frame k-1's
 *      longest pixels finish.
 * frm_read_frame_async: enqueues the copy of the last frm_render's frame (frm_read_frame's
 *      bytes) into a library-owned pinned host image of that frame's slot; returns a ticket.
 * frm_present_async: the same for frm_present's blit output (out size, FRM_BLIT_* flags).
 * frm_frame_pixels: waits for a ticket's copy and returns its pixels (4*w*h bytes, row 0 =
 *      top). The image belongs to the render slot: it stays valid until frames_in_flight
 *      further frm_render calls have been made (a later async readback of the same slot
 *      replaces it); an expired or unknown ticket gives FRM_ERR_INVALID_ARGUMENT. */
int frm_read_frame_async(frm_ctx* ctx, uint64_t* out_ticket);
int frm_present_async(frm_ctx* ctx, uint32_t out_width, uint32_t out_height, uint32_t flags,
                      uint64_t* out_ticket);
int frm_frame_pixels(frm_ctx* ctx, uint64_t ticket, const uint8_t** out_pixels, size_t* out_bytes);

/* The kernel (FRM_KERNEL_*) a render or band launch of `pixels` pixels runs on this
 * context: the FRM_FLAG_*_KERNEL flag when set, otherwise FRM_KERNEL_SIMPLE when pixels
 * is below one resident persistent grid (1536 lanes per CU) and FRM_KERNEL_PERSISTENT
 * from there on. No reference counterpart (the reference has one fragment pipeline). */
int frm_kernel_for_pixels(const frm_ctx* ctx, uint64_t pixels, uint32_t* out_kernel);

/* Runtime kernel reload (the reference's `r` key: graphics.rs:39-48, reloadable_graphics.rs:
 * 15-52). Recompiles the render kernels with hiprtc from source_dir, a directory holding an
 * edited copy of this package's csrc/ headers (frm_render_kernels.h and the headers it
 * includes: scenes, distance estimators, builtins, shading), and renders every later frame
 * of this context with them. On failure (FRM_ERR_COMPILE, log in frm_last_error) the
 * previous kernels stay active, as the reference keeps its pipeline. source_dir = NULL
 * returns to the built-in kernels. Waits for the context's stream. */
int frm_reload(frm_ctx* ctx, const char* source_dir);

/* ---- row-tiled rendering for multi-GPU (no reference counterpart: the reference
 *      is single-device). Band b covers frame rows [b*band_rows, (b+1)*band_rows).
 *      This call renders bands first_band, first_band+band_stride, ... (below
 *      num_bands(H)) and stores them back to back, band-major, at dev_dst (device
 *      memory of this context's GPU), each row 4*width bytes. `stream` is a
 *      hipStream_t (NULL = context stream). dev_counters, if not NULL, is device
 *      memory of FRM_NUM_COUNTERS uint64 to which the work counters are ADDED.
 *      Asynchronous. With frames_in_flight = F the launch uses the next of F scratch
 *      slots; a slot last used on another stream is awaited on the device, so a caller
 *      that rotates F streams (and F destination buffers) overlaps F launches.
 * frm_band_rows_for: the rows such a call stores for a frame of `height` rows: whole bands, a
 *      short last band of the frame counted as band_rows rows (0 when first_band is at or beyond
 *      the band count). FRM_ERR_INVALID_ARGUMENT, *out_rows left alone, for a height, band_rows or
 *      band_stride of 0, and when the count does not fit 32 bits (it is below height + band_rows,
 *      so a height of at most FRM_MAX_DIMENSION always fits).
 * frm_render_bands: dev_dst holds dst_bytes bytes, at least frm_band_rows_for's rows of 4*width
 *      bytes (FRM_ERR_BUFFER_TOO_SMALL otherwise), and is 4-byte aligned; dev_counters, if not
 *      NULL, is 8-byte aligned (FRM_ERR_INVALID_ARGUMENT otherwise, reported after every other
 *      fault of the call; a refused call launches nothing). The rows a short last band lacks are
 *      padding: they are never written and keep the caller's bytes, as does every byte outside the
 *      call's rows. A call without bands (0 rows) succeeds with a dst_bytes of 0 and writes nothing. */
#define FRM_NUM_COUNTERS 8u
int frm_band_rows_for(uint32_t height, uint32_t band_rows, uint32_t first_band,
                      uint32_t band_stride, uint32_t* out_rows);
int frm_render_bands(frm_ctx* ctx, uint8_t* dev_dst, size_t dst_bytes, uint32_t band_rows,
                     uint32_t first_band, uint32_t band_stride, void* stream,
                     uint64_t* dev_counters);
/* Multi-frame launch: renders `count` frames (1..FRM_MAX_BATCH) of the context's size in ONE
 * launch, frame k with params[k], each as frm_render_bands would render it (this rank's bands,
 * band-major) into dev_dst + k * frame_stride_bytes. The frames' pixels share one work queue
 * (each frame's pixels longest first, the frames interleaved), so one frame's longest pixels
 * run beside the other frames' work instead of ending a launch with idle lanes: for short
 * launches (a rank's share of a row-split frame) the persistent kernel's tail is paid once
 * per batch. The frames may differ in camera, and the Mandelbulb's (scene 18) in time too (its
 * power is its one time-derived constant, fragment.wgsl:75; each lane then carries its frame's
 * power): otherwise params[k] must give the same scene, num_iterations, time-derived scene
 * constants and aspect as params[0] (FRM_ERR_INVALID_ARGUMENT otherwise). A scripted
 * fly-through (the CLI's, bench.py's HEADLINE_FLY) so renders several of its frames per launch. The context's parameters become params[count-1].
 * Counters are added over all frames. Bytes per frame are those of frm_render_bands; dev_dst
 * holds dst_bytes bytes, at least (count - 1) * frame_stride_bytes + one frame's bands
 * (FRM_ERR_BUFFER_TOO_SMALL otherwise); frame_stride_bytes is a multiple of 4 below 16 GiB.
 * dev_dst is 4-byte aligned and dev_counters, if not NULL, 8-byte aligned (FRM_ERR_INVALID_ARGUMENT
 * otherwise, reported after every other fault of the call; a refused call launches nothing). As
 * with frm_render_bands, the padding rows of a short last band are never written, nor are the
 * bytes between one frame's rows and the next frame's start. */
#define FRM_MAX_BATCH 32u
int frm_render_bands_batch(frm_ctx* ctx, uint32_t count, const frm_parameters* params,
                           uint8_t* dev_dst, size_t dst_bytes, size_t frame_stride_bytes, uint32_t band_rows,
                           uint32_t first_band, uint32_t band_stride, void* stream,
                           uint64_t* dev_counters);
/* ---- motion blur: one frame as the mean, in linear light, of `count` sub-frames sampled over a
 *      shutter interval (no reference counterpart: the reference renders instantaneous poses). With
 *      S the context's supersampling factor, sub-frame k the (S*width) x (S*height) frame frm_render
 *      would render with params[k], and D the sRGB decode table of the blit, output pixel (X, Y) is,
 *      for each of R, G, B:
 *          sum = 0.0f
 *          for k in 0..count-1, j in 0..S-1, i in 0..S-1:      (sub-frames in the order given, source
 *            sum = sum + D[frame[k][S*Y+j][S*X+i]]               rows top to bottom, texels left to right)
 *          code = encode(sum / (float)(count*S*S))              (f32 adds in exactly this order, one
 *                                                                correctly rounded division, the sRGB store)
 *      alpha 255. One sum over all count*S*S samples: not a resolve per sub-frame and a mean of
 *      codes. count = 1 gives frm_render's bytes; identical sub-frames give the plain frame.
 * frm_render_shutter: frm_render for one such frame. It takes one render slot and its stream as
 *      frm_render does (frames in flight, tickets, stats == NULL being asynchronous, frm_resize
 *      without a drain: all as there), and frm_read_frame, frm_present, their async forms and
 *      frm_frame_pixels see the blurred frame. Every params[k] is checked as frm_set_parameters
 *      checks it; all must share scene_index, num_iterations and aspect_scale
 *      (FRM_ERR_INVALID_ARGUMENT otherwise); time and camera may differ in every scene. The
 *      context's parameters become params[count-1]. Where frm_render_bands_batch's rules allow it
 *      (the same scene uniforms up to the Mandelbulb's power, the persistent kernel, no reloaded
 *      module) the sub-frames share one persistent launch, else each gets its own, with the same
 *      bytes. The sub-frames are rendered into a scratch of the slot in chunks (at most
 *      FRM_MAX_SHUTTER_SAMPLES, 1 GiB of scratch, and the environment variable FRM_SHUTTER_CHUNK
 *      read by frm_create, a tuning knob); each chunk is added to an f32 accumulator and the last
 *      one writes the frame, with the bytes of a single chunk. frm_stats is the sum over the
 *      sub-frames (pixels = count * S*S * width * height); kernel_ms includes the accumulation.
 *      FRM_ERR_UNSUPPORTED on a group or an adaptive context, FRM_ERR_NOT_READY before frm_resize,
 *      FRM_ERR_INVALID_ARGUMENT for NULL or a count outside 1..FRM_MAX_SHUTTER_SAMPLES; a refusal
 *      changes nothing. Shutter frames never go through the resident ring, and frm_debug_trace after
 *      one gives FRM_ERR_NOT_READY (there is no single frame to trace).
 * frm_accumulate: the accumulation alone, on any context, asynchronous on `stream` (NULL: the
 *      context's). dev_src holds `count` (1..FRM_MAX_SHUTTER_SAMPLES) frames frame_stride_bytes
 *      apart (a multiple of 4, at least a frame's bytes), each factor*out_height rows of
 *      factor*out_width RGBA8 sRGB texels; factor 1..FRM_MAX_SUPERSAMPLE and factor x each size
 *      at most FRM_MAX_DIMENSION. dev_acc: NULL, or 16 bytes per output pixel (float x, y, z: the
 *      sums of R, G, B; w is written as 0), 16-byte aligned, read AND written: the sum starts from
 *      it, so the caller zeroes it before the first chunk (all-zero bytes are 0.0f). dev_dst: NULL,
 *      or out_height rows of out_width texels that receive the frame of sum / divisor (divisor >= 1:
 *      the number of samples summed so far). Both NULL, misaligned or overlapping buffers and
 *      sizes out of range are FRM_ERR_INVALID_ARGUMENT, a short buffer FRM_ERR_BUFFER_TOO_SMALL.
 *      The source alpha is ignored. Additive: FRM_ABI_VERSION stays 5. */
#define FRM_MAX_SHUTTER_SAMPLES 32u   /* = FRM_MAX_BATCH */
int frm_render_shutter(frm_ctx* ctx, uint32_t count, const frm_parameters* params, frm_stats* stats);
int frm_accumulate(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, size_t frame_stride_bytes,
                   uint32_t count, uint32_t out_width, uint32_t out_height, uint32_t factor,
                   float* dev_acc, size_t acc_bytes, uint32_t divisor,
                   uint8_t* dev_dst, size_t dst_bytes, void* stream);
/* ---- panorama: a 360-degree equirectangular frame of W x H pixels, projected from the six faces
 *      of a cube map around the camera (no reference counterpart: the reference has one pinhole
 *      camera). N is the face size, M = N + 2 (one guard texel all round), q = (float)M / (float)N
 *      and a = kCameraDirectionZ * q (one f32 multiply; kCameraDirectionZ = f32(1/atan(pi/2)), the
 *      z of every camera ray).
 *      Face frames. Face f of a parameter set p is the M x M frame frm_render renders for p_f: p with
 *      aspect_scale = (a, a) (the caller's aspect is ignored) and the camera C_f = C * [r_f u_f w_f],
 *      C the 4x4 camera matrix of p and the face vectors in the camera's own basis (x right, y up,
 *      z forward); column 3 is unchanged:
 *          f  face       r (right)   u (up)      w (forward)
 *          0  +z front   ( 1,0, 0)   (0,1, 0)    ( 0, 0, 1)
 *          1  -z back    (-1,0, 0)   (0,1, 0)    ( 0, 0,-1)
 *          2  +x right   ( 0,0,-1)   (0,1, 0)    ( 1, 0, 0)
 *          3  -x left    ( 0,0, 1)   (0,1, 0)    (-1, 0, 0)
 *          4  +y up      ( 1,0, 0)   (0,0,-1)    ( 0, 1, 0)
 *          5  -y down    ( 1,0, 0)   (0,0, 1)    ( 0,-1, 0)
 *      r x u = w for every face. C_f is a signed permutation of C's first three columns, exact in
 *      f32: camera_matrix[4j+i] of p_f is + or - camera_matrix[4j+k] of p, for all four j. The inner
 *      N x N texels cover tan in [-1, 1]; their centres sit where those of an N x N 90-degree face
 *      would.
 *      Direction tables. Output pixel (X, Y) has longitude lon = ((2X+1)/W - 1) * pi and latitude
 *      lat = (1 - (2Y+1)/H) * pi/2: the image centre looks along the camera's forward axis, lon grows
 *      to the right, row 0 is the zenith side. sin_lon[X], cos_lon[X], sin_lat[Y], cos_lat[Y] are
 *      computed on the host in double precision and rounded once to f32.
 *      Per pixel, all f32, no contraction, IEEE divisions:
 *          dx = cos_lat*sin_lon;  dy = sin_lat;  dz = cos_lat*cos_lon
 *          face: |dz| >= |dx| && |dz| >= |dy| ? (dz > 0 ? 0 : 1)
 *              : |dx| >= |dy|                 ? (dx > 0 ? 2 : 3)
 *              :                                (dy > 0 ? 4 : 5)
 *          A = d.r_f;  B = d.u_f;  m = d.w_f        (each a signed component of d: no arithmetic)
 *          u = A / m;  v = B / m
 *          fx = u*(0.5f*N) + (0.5f*M - 0.5f);   fy = (0.5f*M - 0.5f) - v*(0.5f*N)
 *          x0 = floor(fx); tx = fx - x0;  y0 = floor(fy); ty = fy - y0
 *          x0, x0+1, y0, y0+1 clamped to [0, M-1]
 *      then the blit's linear filter over the four texels t00 (x0, y0), t10 (x0+1, y0), t01, t11 of
 *      face f: per channel top = mix(D[t00], D[t10], tx), bot = mix(D[t01], D[t11], tx),
 *      c = mix(top, bot, ty) with mix(a, b, t) = a*(1.0f - t) + b*t and D the blit's sRGB decode
 *      table; stored as the sRGB store does, alpha 255 (the source alpha is ignored). The filter
 *      is 2 x 2 everywhere: near the cube's corners, where face texels are denser than panorama
 *      pixels, it does not filter the minification.
 * frm_panorama_parameters: out[f] = p_f for f = 0..5 (host only; nothing for NULL or face_size 0).
 * frm_panorama_face_size: the product default N = ceil(width / 4) for a panorama `width` pixels
 *      wide: the customary cube size for an equirectangular width (the equator then has about one
 *      face texel per pixel), not a measured optimum. width in [1, FRM_MAX_DIMENSION].
 * frm_equirect_tables: the four tables above (width, width, height, height floats; host only).
 * frm_project_equirect: the projection alone, on any context, asynchronous on `stream` (NULL: the
 *      context's). dev_faces holds faces 0..5 face_stride_bytes apart (a multiple of 4, at least
 *      4*M*M), each M rows of M RGBA8 sRGB texels; dev_dst receives out_height rows of out_width
 *      texels. Both device memory of the context's GPU, 4-byte aligned, not overlapping; face_size
 *      in [1, FRM_MAX_DIMENSION - 2], the output sizes in [1, FRM_MAX_DIMENSION]
 *      (FRM_ERR_INVALID_ARGUMENT otherwise; FRM_ERR_BUFFER_TOO_SMALL when faces_bytes or dst_bytes
 *      is short). The tables are scratch of the call, allocated and released in its stream's order.
 * frm_set_panorama: face size N; 0 (the default) is off, allocates nothing and changes no path.
 *      With N >= 1 frm_resize keeps taking the output size W x H (any, up to FRM_MAX_DIMENSION)
 *      while the context renders M x M frames: every frm_render renders the six faces of the
 *      context's parameters into a scratch of its slot (one shared persistent launch where
 *      frm_render_bands_batch's rules allow it, else six launches, with the same bytes) and projects
 *      them into the frame that frm_read_frame, frm_present, their async forms and frm_frame_pixels
 *      see. It takes one render slot as frm_render does; a change acts as frm_resize does: no drain,
 *      frames in flight and their tickets keep their bytes, async readbacks give FRM_ERR_NOT_READY
 *      until the next frm_render. frm_stats is the sum over the faces (pixels = 6*M*M); kernel_ms
 *      includes the projection. frm_debug_trace after a panorama gives FRM_ERR_NOT_READY (no single
 *      frame to trace); panoramas never go through the resident ring. FRM_ERR_UNSUPPORTED, with
 *      nothing changed: N >= 1 on a group, supersampled or adaptive context; and on a panorama
 *      context frm_set_supersampling(k > 1), frm_set_adaptive(k > 1), frm_render_shutter,
 *      frm_render_bands, frm_render_bands_batch and frm_unshuffle_bands. FRM_ERR_INVALID_ARGUMENT
 *      (N unchanged) when M exceeds FRM_MAX_DIMENSION or the six faces 1 GiB.
 *      Additive: FRM_ABI_VERSION stays 5. */
void frm_panorama_parameters(const frm_parameters* p, uint32_t face_size, frm_parameters out[6]);
int frm_panorama_face_size(uint32_t width, uint32_t* out_face_size);
int frm_equirect_tables(uint32_t width, uint32_t height, float* sin_lon, float* cos_lon, float* sin_lat,
                        float* cos_lat);
int frm_project_equirect(frm_ctx* ctx, const uint8_t* dev_faces, size_t faces_bytes, size_t face_stride_bytes,
                         uint32_t face_size, uint8_t* dev_dst, size_t dst_bytes, uint32_t out_width,
                         uint32_t out_height, void* stream);
int frm_set_panorama(frm_ctx* ctx, uint32_t face_size);
int frm_get_panorama(const frm_ctx* ctx, uint32_t* out_face_size);
/* ---- depth of field: a depth plane and a thin-lens gather in linear light (no reference
 *      counterpart: the reference has a pinhole camera and hands out no depth).
 *      Inputs:
 *        - A frame S of W x H RGBA8 sRGB texels.
 *        - A depth plane Z of W x H f32 values.
 *        - A, the aperture: the blur radius, in pixels, of a point at infinity. Finite, >= 0.
 *        - F, the focus distance. Finite, > 0.
 *        - R, the largest radius: an integer in 0..FRM_MAX_DOF_RADIUS, with FRM_MAX_DOF_RADIUS = 16.
 *        - D, the blit's sRGB decode table.
 *        - kPi = f32(pi).
 *      All arithmetic is f32 with no contraction, and every division is an IEEE division.
 *      Per pixel q (depends on q alone):
 *          c = A * fabsf(1.0f - F / Z[q])      (thin lens; Z = +inf gives c = A; Z = 0 gives +inf, or NaN when A = 0)
 *          if (!(c >= 0.0f)) c = 0.0f          (NaN: in focus)
 *          if (c > (float)R) c = (float)R
 *          a = c * c;   w = 1.0f / (kPi * a + 1.0f)
 *      Per output pixel p: Start with sw = sr = sg = sb = 0.0f. Loop dy from -R to R, outer, top to
 *      bottom. Loop dx from -R to R, inner, left to right. Let q = p + (dx, dy). Skip q when it lies
 *      outside the frame: the window is clipped, not clamped.
 *          use_p = (Z[q] > Z[p]) && (c[p] < c[q])       (a sample behind p spreads no wider than p's own circle:
 *          a_e = use_p ? a[p] : a[q]                      no background bleeding onto a sharper foreground)
 *          w_e = use_p ? w[p] : w[q]
 *          if ((float)(dx*dx + dy*dy) <= a_e):
 *              sw = sw + w_e
 *              sr = sr + w_e * D[S[q].r]                  (one multiply, one add; likewise g, b)
 *      Then:
 *          out[p] = encode(sr / sw), encode(sg / sw), encode(sb / sw), 255
 *      encode is the sRGB store. The source alpha is ignored. q = p always passes, so sw >= w[p] > 0;
 *      adding 0.0f for a sample that does not pass gives the same bits as skipping it (the sums are
 *      never negative); a and w are functions of one pixel. A = 0 gives c = 0 everywhere, hence
 *      sw = 1 and the source frame's bytes with alpha 255; R = 0 does the same.
 *      Known limits. Z is the ray distance t, not the planar depth: the focus surface is a sphere
 *      around the camera. Taking t * dir.z instead would need the camera's normalize sequence pinned
 *      in a second reference; it is left for later. A point behind a blurred foreground object is
 *      not recovered: the frame holds one surface per pixel.
 * frm_dof_coc: out_c[i] = c of depth[i] for i < n, as above (host only; the code the kernel runs,
 *      compiled for the host). FRM_ERR_INVALID_ARGUMENT for NULL, max_radius above
 *      FRM_MAX_DOF_RADIUS, an aperture that is not finite and >= 0 or a focus that is not finite
 *      and > 0.
 * frm_depth_of_field: the gather alone, on any context, asynchronous on `stream` (NULL: the
 *      context's). dev_src and dev_dst hold height rows of width RGBA8 sRGB texels, dev_depth as many
 *      floats, row-major. All device memory of the context's GPU, 4-byte aligned; dev_dst overlaps
 *      neither input. FRM_ERR_INVALID_ARGUMENT for NULL, sizes outside [1, FRM_MAX_DIMENSION],
 *      max_radius above the limit, a non-finite or negative aperture, a focus that is not finite
 *      and positive, misalignment or overlap; FRM_ERR_BUFFER_TOO_SMALL for short buffers.
 * frm_set_depth_of_field: switches the effect on; max_radius = 0 (the default) is off: nothing is
 *      allocated and frm_render enqueues the launches it did before (the host tests the radius in
 *      kernel_for and resolve_frame; that the plain frame's time is unchanged rests on bench.py's
 *      comparison with the parent's library, DESIGN.md "Depth of field"). When on, every frm_render renders as before, always on the
 *      persistent kernel whatever the frame's size (the bytes are the same), then turns the slot's
 *      records into a depth plane (hit: the primary hit distance t; miss: +inf) and gathers on the
 *      slot's stream into the slot's second image, which frm_read_frame, frm_present, their async
 *      forms and frm_frame_pixels see. A change acts as frm_set_adaptive does: no drain, frames in
 *      flight and their tickets keep their bytes, async readbacks give FRM_ERR_NOT_READY until the
 *      next frm_render. frm_stats holds the plain frame's counters; kernel_ms includes both passes.
 *      Such frames never go through the resident ring. FRM_ERR_UNSUPPORTED, with nothing changed:
 *      max_radius >= 1 on a group, supersampled, adaptive or panorama context, on a context with
 *      FRM_FLAG_SIMPLE_KERNEL or with runtime-reloaded kernels active; and on a depth-of-field
 *      context frm_set_supersampling(k > 1), frm_set_adaptive(k > 1), frm_set_panorama(N >= 1),
 *      frm_render_shutter, frm_render_bands, frm_render_bands_batch, frm_unshuffle_bands and
 *      frm_reload(dir). FRM_ERR_INVALID_ARGUMENT (values unchanged) as for frm_dof_coc; with
 *      max_radius = 0 the aperture and focus are stored unchecked.
 * frm_read_depth: the depth plane of the last frm_render: width * height floats, row-major,
 *      synchronous. Available under frm_debug_trace's conditions: a whole frame on the persistent
 *      kernel whose slot no later launch has reused; otherwise FRM_ERR_NOT_READY.
 *      FRM_ERR_UNSUPPORTED on a group, FRM_ERR_BUFFER_TOO_SMALL for a short dst. On a depth-of-field
 *      context the plane is the one the gather used.
 *      Additive: FRM_ABI_VERSION stays 5. */
#define FRM_MAX_DOF_RADIUS 16u
int frm_dof_coc(float aperture, float focus, uint32_t max_radius, const float* depth, size_t n, float* out_c);
int frm_depth_of_field(frm_ctx* ctx, const uint8_t* dev_src, size_t src_bytes, const float* dev_depth,
                       size_t depth_bytes, uint32_t width, uint32_t height, float aperture, float focus,
                       uint32_t max_radius, uint8_t* dev_dst, size_t dst_bytes, void* stream);
int frm_set_depth_of_field(frm_ctx* ctx, float aperture, float focus, uint32_t max_radius);
int frm_get_depth_of_field(const frm_ctx* ctx, float* out_aperture, float* out_focus, uint32_t* out_max_radius);
int frm_read_depth(frm_ctx* ctx, float* dst, size_t n_floats);
/* Reassemble a frame from per-rank band buffers laid out rank-major in dev_src
 * (rank r's buffer starts at r*rank_stride_bytes, as written by frm_render_bands with
 * first_band = r, band_stride = ranks) into row-major dev_dst. Asynchronous on `stream` (NULL:
 * the context's). dev_dst holds dst_bytes bytes, at least the frame's 4*width*height
 * (FRM_ERR_BUFFER_TOO_SMALL otherwise); rank_stride_bytes is a multiple of 4, at least rank 0's
 * frm_band_rows_for rows of 4*width bytes. The call reads dev_src from its first byte to the end of
 * the rows (whole bands) of the last rank that holds a band, rank min(ranks, band count) - 1, and
 * of these only the rows that hold frame rows: padding rows, the bytes between a rank's rows and
 * the next rank's start and the shares of ranks beyond the band count are never read. dev_src
 * and dev_dst are device memory of the context's GPU, 4-byte aligned, and the frame at dev_dst
 * does not overlap that span of dev_src (FRM_ERR_INVALID_ARGUMENT otherwise, reported after every
 * other fault of the call; a refused call launches nothing). Rows move as 16-byte words when
 * 4*width, rank_stride_bytes, dev_src and dev_dst are all multiples of 16, else as 4-byte words:
 * the bytes are the same. */
int frm_unshuffle_bands(frm_ctx* ctx, const uint8_t* dev_src, size_t rank_stride_bytes,
                        uint8_t* dev_dst, size_t dst_bytes, uint32_t band_rows,
                        uint32_t ranks, void* stream);
/* Convert FRM_NUM_COUNTERS raw counters (host copy) to frm_stats for the context's
 * current parameters (fills wom_ops; kernel_ms = 0). */
int frm_stats_from_counters(const frm_ctx* ctx, const uint64_t* counters, frm_stats* out);

/* ---- diagnostics (parity tooling; synchronous, host pointers) -------------------
 * frm_eval_scene: evaluates the current scene's distance estimator and object colour
 * (scene(position), fragment.wgsl:18-78) at n points (xyz interleaved) on the GPU.
 * frm_eval_math: evaluates one frm builtin on the GPU, element-wise; fn = FRM_MATH_*. */
enum {
  FRM_MATH_SIN = 0, FRM_MATH_COS = 1, FRM_MATH_ACOS = 2, FRM_MATH_ATAN2 = 3,
  FRM_MATH_LOG = 4, FRM_MATH_LOG2 = 5, FRM_MATH_EXP2 = 6, FRM_MATH_POW = 7,
  FRM_MATH_SQRT = 8, FRM_MATH_DIV = 9,
  /* device fast paths (bit-identical to the builtin above on their stated domain, used by
     the Mandelbulb body when a whole wave qualifies; csrc/frm_fast.h) */
  FRM_MATH_SQRT_NOSMALL = 10, FRM_MATH_DIV_TAME = 11, FRM_MATH_DIV_TAME_NZ = 12,
  FRM_MATH_SIN_SMALL = 13, FRM_MATH_COS_SMALL = 14, FRM_MATH_ACOS_DEV = 15,
  FRM_MATH_ATAN2_TAME = 16, FRM_MATH_LOG2_TAME = 17, FRM_MATH_EXP2_TAME = 18,
  FRM_MATH_LOG_POSNORMAL = 19,
  /* the Rgba8UnormSrgb store's 8-bit code of a linear value (as a float; csrc/frm_scene.h) */
  FRM_MATH_SRGB_ENCODE = 20,
  /* the division ended by v_div_fixup (csrc/frm_fast.h div_fix), and the x / y component of the
     march's last-tap normalize of (a, b, b): guarded (per wave the reciprocal-based form when every
     lane allows it, csrc/frm_scene.h normalize_wave) and plain */
  FRM_MATH_DIV_FIX = 21, FRM_MATH_NORMALIZE_GUARDED_X = 22, FRM_MATH_NORMALIZE_GUARDED_Y = 23,
  FRM_MATH_NORMALIZE_X = 24, FRM_MATH_NORMALIZE_Y = 25,
  /* atan2_tame for two non-zero operands (csrc/frm_fast.h atan2_tame_nz; the Mandelbulb body's
     with profiles/round11/loop/atan2_nz.patch) */
  FRM_MATH_ATAN2_TAME_NZ = 26,
  FRM_MATH_LAST = 26
};
int frm_eval_scene(frm_ctx* ctx, const float* points, uint32_t n, float* out_distance,
                   float* out_color);
int frm_eval_math(frm_ctx* ctx, int32_t fn, const float* a, const float* b, uint32_t n,
                  float* out);
/* frm_debug_pixel_keys: the 8-bit scheduling cost keys (16 log2(bodies + 1), csrc/frm_sched.hip)
 * the context's last persistent launch recorded per local pixel, row-major; copies
 * min(n, pixels) bytes and returns that count, or a negative frm_status. */
int frm_debug_pixel_keys(frm_ctx* ctx, uint8_t* out, size_t n);
/* frm_debug_set_pixel_keys: replaces the keys the next persistent launch orders its pixels by
 * (n = width x height; the next slot must hold a whole frame of the current size). */
int frm_debug_set_pixel_keys(frm_ctx* ctx, const uint8_t* keys, size_t n);
/* frm_debug_pixel_order: the fetch order held by the slot of the context's last persistent launch:
 * a permutation of that launch's local pixels 0..pixels-1, most expensive key first; copies
 * min(n, pixels) entries and returns that count, or a negative frm_status (as frm_debug_pixel_keys:
 * the device is synchronised first, FRM_ERR_UNSUPPORTED on a group, FRM_ERR_INVALID_ARGUMENT before
 * any persistent launch). *out_ranked = 1: that launch ranked its own keys into the order, which
 * the slot's next launch of the same geometry fetches by (the default); 0: the buffer still holds
 * the order that launch itself fetched by (FRM_SCHED=sort, runtime-reloaded kernels): a stable
 * descending sort of the keys it started from, or 0..pixels-1 without history. Equal keys are in
 * pixel order only when out_ranked is 0. Additive: FRM_ABI_VERSION stays 5. */
int frm_debug_pixel_order(frm_ctx* ctx, uint32_t* out, size_t n, uint32_t* out_ranked);

/* frm_debug_trace: the geometric inputs of the shading of every pixel of the last frm_render (a
 * whole frame on the persistent kernel, with the size and parameters that render used; refused
 * with FRM_ERR_NOT_READY when a later launch has reused its slot), 10 floats per
 * pixel, row-major, in the layout of the oracle's per-pixel trace: hit, primary steps, normal xyz,
 * sun hit, sun closeness, object colour xyz (hits; zeros for misses). Parity tooling for frames
 * that are not bit-exact by design (FRM_FLAG_HW_MATH). n_floats >= 10 x width x height. */
int frm_debug_trace(frm_ctx* ctx, float* out, size_t n_floats);

/* ---- host-side mirrors of the reference's Parameters mutators (src/parameters.rs).
 *      These let a C/C++/Python host drive the same uniform without Rust. */
void frm_parameters_default(frm_parameters* p);                               /* #[derive(Default)] */
void frm_parameters_update_aspect(frm_parameters* p, uint32_t w, uint32_t h); /* parameters.rs:18-21 */
void frm_parameters_update_time(frm_parameters* p, float delta);             /* parameters.rs:27-29 */
void frm_parameters_update_num_iterations(frm_parameters* p, int32_t delta); /* parameters.rs:31-33 */
void frm_parameters_update_scene_index(frm_parameters* p, int32_t delta);    /* parameters.rs:37-40 */
/* parameters.rs:23-25 with Camera::to_matrix (camera.rs:26-44):
 * camera_matrix = transpose(T(position) * Ry(yaw) * Rx(pitch)), column-major. */
void frm_parameters_update_camera(frm_parameters* p, const float position[3], float yaw,
                                  float pitch);

/* ---- animation driver: host-side restatement of the reference's Camera (src/camera.rs)
 *      and Timing (src/timing.rs), for scripted fly-throughs without a window (SURVEY
 *      §8(f) row 2). Keyboard/mouse input becomes explicit arguments: held keys as a
 *      FRM_KEY_* bit set (held_keys.rs), the frame time as seconds (timing.rs uses
 *      Instant::now). All arithmetic is f32 in cgmath's operation order. */
#define FRM_KEY_MOVE_FORWARD (1u << 0)  /* held_keys.rs:6-17 */
#define FRM_KEY_MOVE_BACKWARD (1u << 1)
#define FRM_KEY_MOVE_RIGHT (1u << 2)
#define FRM_KEY_MOVE_LEFT (1u << 3)
#define FRM_KEY_MOVE_UP (1u << 4)
#define FRM_KEY_MOVE_DOWN (1u << 5)
#define FRM_KEY_PITCH_UP (1u << 6)
#define FRM_KEY_PITCH_DOWN (1u << 7)
#define FRM_KEY_YAW_RIGHT (1u << 8)
#define FRM_KEY_YAW_LEFT (1u << 9)

enum { /* camera.rs:16-23 */
  FRM_LOCK_YAW_NONE = 0,
  FRM_LOCK_YAW_INWARDS = 1,
  FRM_LOCK_YAW_RIGHT = 2,
  FRM_LOCK_YAW_OUTWARDS = 3,
  FRM_LOCK_YAW_LEFT = 4
};

typedef struct frm_camera { /* camera.rs:5-14 */
  float position[3];
  float pitch;                  /* radians, clamped to [-pi/2, pi/2]          */
  float yaw;                    /* radians, kept in (-2pi, 2pi) by fmod        */
  float movement_per_second;
  float orbit_angle_per_second; /* radians per second about the y axis         */
  int32_t lock_yaw_mode;        /* FRM_LOCK_YAW_*                              */
  int32_t lock_pitch;           /* bool                                        */
} frm_camera;

void frm_camera_default(frm_camera* c);                                  /* camera.rs:176-188 */
void frm_camera_update(frm_camera* c, uint32_t held_keys, float seconds); /* camera.rs:100-147 */
void frm_camera_update_speed(frm_camera* c, float delta);                /* camera.rs:60-62 */
void frm_camera_update_orbit_speed(frm_camera* c, float delta);          /* camera.rs:64-69 */
void frm_camera_reset_orbit_speed(frm_camera* c);                        /* camera.rs:71-73 */
void frm_camera_toggle_lock_pitch(frm_camera* c);                        /* camera.rs:75-77 */
void frm_camera_cycle_lock_yaw_mode(frm_camera* c, int32_t backwards);   /* camera.rs:79-98 */
void frm_camera_rotate_from_cursor(frm_camera* c, float yaw_pixels,
                                   float pitch_pixels);                  /* camera.rs:151-154 */
void frm_parameters_update_camera_from(frm_parameters* p, const frm_camera* c); /* parameters.rs:23-25 */

typedef struct frm_timing { /* timing.rs:5-10, minus the wall clock and the FPS log */
  float time_factor;
} frm_timing;

void frm_timing_init(frm_timing* t);                                     /* timing.rs:13-21 */
/* parameters.time += time_factor * delta_seconds (timing.rs:23-30); returns delta_seconds */
float frm_timing_update(frm_timing* t, frm_parameters* p, float delta_seconds);
void frm_timing_update_time_factor(frm_timing* t, float delta);          /* timing.rs:32-34 */
void frm_timing_stop_time(frm_timing* t);                                /* timing.rs:36-38 */

/* The sub-frames of one motion-blurred frame (frm_render_shutter) of a scripted fly-through, as
 * the CLI samples them: `samples` parameter sets that step the frame's state through the fraction
 * `shutter` of its frame time dt. out[0] = *p; for s >= 1, on private copies of p, c and t carried
 * on from s - 1: h = shutter * dt / (float)samples (f32, in this order);
 * delta = frm_timing_update(&t, &p, h); frm_camera_update(&c, held_keys, delta);
 * frm_parameters_update_camera_from(&p, &c); out[s] = p. The inputs are not modified. */
void frm_shutter_parameters(const frm_parameters* p, const frm_camera* c, const frm_timing* t,
                            uint32_t held_keys, float dt, uint32_t samples, float shutter,
                            frm_parameters* out /* samples entries */);

#ifdef __cplusplus
}
#endif
#endif /* FRM_H */
