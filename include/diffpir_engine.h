/*
 * diffpir_engine.h -- C ABI of the MI355X-native DiffPIR sampling engine (libdiffpir_hip.so).
 *
 * The reference (yuanzhi-zhu/DiffPIR) has no FFI: its "plugin surface" is three Python call
 * signatures used by main_ddpir.py's restoration loop.  Each entry point
 * below names the reference interface it replaces (paths relative to the reference root).
 * The Python shims in diffpir_amd/ (utils_model.model_fn, utils_sisr.pre_calculate /
 * data_solution, ...) mirror those signatures and call straight into these symbols via ctypes;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (DPIR_OK) or a negative dpir_status; nothing throws or aborts
 *     across the ABI; dpir_last_error() gives the message for the last failure on that engine.
 *   - "dev" pointers are raw device addresses (engine-allocated with dpir_malloc, or any other
 *     HIP allocation such as torch.Tensor.data_ptr()); "host" pointers are plain host memory.
 *   - tensors are fp32, NCHW, contiguous; images are in [-1,1] inside the loop and y in [0,1],
 *     exactly as in main_ddpir.py.  Masks are uint8 {0,1} (bit-exact integer semantics).
 *   - all work is enqueued on ONE engine-owned HIP stream; calls are asynchronous unless noted
 *     (dpir_sync, D2H copies).  One engine per device; an engine is not thread-safe, independent
 *     engines are.
 *   - shapes: the stepwise entries (dpir_prox_mask, dpir_repaint_mix, dpir_renoise, dpir_finalize, dpir_randn,
 *     dpir_bicubic_up, dpir_resize_down, dpir_prox_ibp, dpir_metrics, dpir_grad_and_value) check their shape before
 *     anything is divided, allocated or enqueued: B, H, W (and C of dpir_randn) >= 1, H * W <= 2^29 - 1 pixels per plane
 *     ("H * W is out of range"; the kernels decode 3 * H * W in an int; dpir_bicubic_up: (h sf) * (w sf)), and where the entry has a scale
 *     factor sf >= 1 dividing H and W (dpir_bicubic_up: sf >= 1; its h, w are the low-resolution sizes).  A violation
 *     returns DPIR_ERR_INVALID with a message naming the entry and leaves the engine usable.  Every entry selects the
 *     engine's device itself (hipSetDevice), whichever device is current in the calling thread.
 */
#ifndef DIFFPIR_ENGINE_H
#define DIFFPIR_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPIR_ABI_VERSION 2   /* 2 (round 5): dpir_dps_coef grew to 24 bytes and dpir_loop_desc gained ddim_sample in round 4 without a bump; bumped with every public struct layout change from here on */

typedef enum dpir_status {
    DPIR_OK = 0,
    DPIR_ERR_INVALID = -1,   /* bad argument / shape / missing weight */
    DPIR_ERR_HIP = -2,       /* a HIP runtime call failed */
    DPIR_ERR_NOMEM = -3,
    DPIR_ERR_STATE = -4,     /* e.g. forward before load_unet */
    DPIR_ERR_UNSUPPORTED = -5,
    DPIR_ERR_RANGE = -6      /* f16x3 mode: an activation left the f16 operand range (|v| > 65000) and was clamped; the
                              * result is wrong.  Reported by dpir_sync / dpir_d2h after the offending work; reload the
                              * weights with dpir_set_precision(e, 0).  Mirrors the reference's use_fp16 caveat
                              * (guided_diffusion/unet.py:618-632, fp16_util.py:15-32) -- but loudly.  The guard covers the
                              * TOP of the range only: a raw operand below about 2^-7 leaves R x fp32 silently, with the
                              * error max(2^-22 |v|, 2^-25) per value ("operand range of the f16
                              * modes"; 2^-6: E = 1.1e-6, 2^-14: 2.7e-4 of a layer's budget, measured). */
} dpir_status;

typedef struct dpir_engine dpir_engine;   /* opaque */
typedef struct dpir_prox dpir_prox;       /* opaque: FB / F2B / FBFy spectra of one batch */

/* ---- lifecycle -------------------------------------------------------------------------- */
int dpir_version(void);
/* number of HIP devices visible to this process (0 when there is none; never fails).  The reference reads
 * torch.cuda.device_count() for its unused world_size (main_ddpir.py:135); the multi-GPU launcher and tests use this. */
int dpir_device_count(int* n_out);
/* "<gcnArchName> | <device name> | pci <bus id> | <CUs> CUs | ordinal <n>" of the engine's device into buf (NUL-terminated, truncated to cap) */
int dpir_device_info(dpir_engine* e, char* buf, size_t cap);
/* device = HIP ordinal.  Fails with DPIR_ERR_HIP when no gfx950 device is visible. */
int dpir_create(int device, dpir_engine** out);
void dpir_destroy(dpir_engine* e);
const char* dpir_last_error(const dpir_engine* e);   /* never NULL */
/* hipStreamSynchronize on the engine stream, then the f16 operand range guard (DPIR_ERR_RANGE, above).  Also the point where a time-out of
 * conv7's fused GroupNorm hop (an inter-workgroup wait; only seen when 3+ engines / processes share the GPU) is handled: the engine switches
 * the hop off for its lifetime and, when the ONE eager forward (dpir_unet_forward / dpir_model_fn_xstart / dpir_p_sample) outstanding since the
 * last synchronisation is still the LAST work on the stream, its outputs do not alias its inputs and no dpir_free happened since, re-issues it on the
 * unfused path and returns DPIR_OK with correct results.  Anything else -- several un-synchronised forwards, or other calls (a prox step, dpir_finalize,
 * a copy) already queued behind the forward, which have consumed its invalid output -- cannot be repaired from here and returns DPIR_ERR_HIP ONCE
 * (not sticky: repeat the calls).  dpir_d2h does the same before it copies; dpir_run_loop re-runs itself. */
int dpir_sync(dpir_engine* e);
/* the engine's hipStream_t, for callers that enqueue their own work (e.g. RCCL) behind it */
void* dpir_stream(dpir_engine* e);

/* ---- device memory (plumbing) ------------------------------------------------------------ */
int dpir_malloc(dpir_engine* e, size_t bytes, void** dev_out);
int dpir_free(dpir_engine* e, void* dev);
int dpir_h2d(dpir_engine* e, void* dev_dst, const void* host_src, size_t bytes);   /* async */
int dpir_d2h(dpir_engine* e, void* host_dst, const void* dev_src, size_t bytes);   /* syncs  */
int dpir_d2d(dpir_engine* e, void* dev_dst, const void* dev_src, size_t bytes);    /* async  */

/* ---- denoiser: guided-diffusion UNet ----------------------------------------------------- */
/* Replaces script_util.create_model(...) hyper-parameters (guided_diffusion/script_util.py:130-184
 * as resolved by utils/utils_model.py:353-387 and main_ddpir.py:219-230). */
typedef struct dpir_unet_desc {
    int32_t image_size;          /* 256 / 512: only selects the default channel_mult */
    int32_t in_channels;         /* 3 */
    int32_t model_channels;      /* 128 (FFHQ) / 256 (ImageNet) */
    int32_t out_channels;        /* 6 (learn_sigma) */
    int32_t num_res_blocks;
    int32_t num_head_channels;   /* 64 */
    int32_t n_channel_mult;      /* 0 -> default for image_size (script_util.py:147-160) */
    float channel_mult[8];
    int32_t n_attention_ds;      /* downsample rates with attention, e.g. {16} */
    int32_t attention_ds[8];
    int32_t num_classes;         /* 0 = unconditional, else label_emb rows (class_cond) */
} dpir_unet_desc;

/* One entry of the reference state-dict (main_ddpir.py:234 torch.load -> load_state_dict). */
typedef struct dpir_tensor {
    const char* name;            /* reference key, e.g. "input_blocks.3.0.in_layers.2.weight" */
    const float* data;           /* HOST pointer, fp32, contiguous, reference layout (OIHW ...) */
    int32_t ndim;
    int64_t shape[4];
} dpir_tensor;

/* Replaces model.load_state_dict(...).to(device) (main_ddpir.py:231-240).  Copies and repacks the
 * weights into the engine's arena (caller keeps ownership of the host arrays).  Fails with
 * DPIR_ERR_INVALID naming the first missing / mis-shaped key. */
int dpir_load_unet(dpir_engine* e, const dpir_unet_desc* desc, const dpir_tensor* weights, int n_weights);

/* Arithmetic of the convolution / attention GEMMs, to be chosen BEFORE dpir_load_unet (weights are packed for it):
 *   0  exact fp32 MFMA (v_mfma_f32_32x32x2_f32), the default;
 *   1  operand-split f16 MFMA: x = hi + lo in f16, 3 x v_mfma_f32_32x32x16_f16 per product, fp32 accumulation --
 *      22-bit products, measured error <= the fp32 MFMA chain's, 5.3x its rate;
 *   2  f16x1: f16 operands (weights and activations rounded once to f16), ONE MFMA per product, fp32 accumulation, fp32
 *      GroupNorm / softmax / residual stream -- the reference's own reduced-precision recipe (guided_diffusion/fp16_util.py:15-32,
 *      unet.py:618-632 `use_fp16`).  NOT within the 1e-3 dB parity contract: its measured quality delta is reported by bench.py. */
int dpir_set_precision(dpir_engine* e, int mode);

/* Replaces UNetModel.forward (guided_diffusion/unet.py:634-663): x_dev [B,3,H,W], t_host [B] int64
 * timesteps (host), y_host [B] int64 labels or NULL -> out_dev [B,out_channels,H,W].  Asynchronous on the engine stream.  When all B timesteps
 * are equal and there are no labels (what utils_model.model_fn always passes: `[t_step] * x.shape[0]`) the timestep is written on the device by a
 * kernel (no host copy, no synchronisation) and the time embedding + FiLM projection are evaluated for one row and shared; otherwise t / y are
 * uploaded (one stream synchronisation). */
int dpir_unet_forward(dpir_engine* e, const float* x_dev, const int64_t* t_host, const int64_t* y_host,
                      float* out_dev, int B, int H, int W);

/* Replaces utils_model.model_fn(..., model_out_type='pred_xstart') (utils/utils_model.py:207-258)
 * = SpacedDiffusion.p_sample -> p_mean_variance (guided_diffusion/gaussian_diffusion.py:232-333):
 * x0 = clamp(c1*x - c2*eps, -1, 1), eps = UNet(x,t)[:, :3];  c1 = float32(sqrt(1/acp64[t])),
 * c2 = float32(sqrt(1/acp64[t]-1)) computed by the caller from the float64 schedule. */
int dpir_model_fn_xstart(dpir_engine* e, const float* x_dev, int t, float c1, float c2,
                         const int64_t* y_host, float* x0_dev, int B, int H, int W);

/* Optional per-layer tap for parity tests: copies the named layer's most recent output (the
 * reference module path, e.g. "input_blocks.3.0") to host.  numel_out receives the element count. */
int dpir_unet_read_tap(dpir_engine* e, const char* layer, float* host_dst, size_t cap_floats, size_t* numel_out);

/* ---- data-fidelity operators ------------------------------------------------------------- */
/* Replaces sr.pre_calculate(y, k, sf) (utils/utils_sisr.py:78-95): y_dev [B,3,H/sf,W/sf] in [0,1],
 * k_dev [B,1,kh,kw]; builds FB, F2B, FBFy (full c2c spectra of size HxW) in an engine-owned object.
 * Supported: 256 x 256 and 512 x 512 and 64 x 64 with sf 1, 2 or 4; H a power of two in [16, 1024], W one in [16, 2048] and sf 1, 2, 4, 8
 * or 16 (the generic kernels of csrc/fft.hip: H is bounded by the LDS of their column pass); and, where H or W is no power of two or sf is
 * another integer, any H in [8, 1024] and W in [8, 2048] without a prime factor above 31 with any sf in [1, 16] (the mixed-radix kernels of
 * csrc/fft_mixed.hip; launch modes 2 and 3 of dpir_set_prox_launch, 3 being the default -- under modes 0 and 1 these shapes are DPIR_ERR_UNSUPPORTED).  Checked here before anything is allocated or launched: DPIR_ERR_INVALID when sf does not divide H and W, B < 1, or
 * the PSF is empty or larger than the image; DPIR_ERR_UNSUPPORTED for any other sf or image size (the message names a prime factor above 31).  dpir_run_loop applies the same shape checks before it allocates the spectra (after
 * its own workspaces) and the PSF check before the first prox launch (after the loop's initialisation launches). */
int dpir_prox_fft_precalc(dpir_engine* e, const float* y_dev, const float* k_dev, int kh, int kw,
                          int sf, int B, int H, int W, dpir_prox** out);
void dpir_prox_free(dpir_engine* e, dpir_prox* p);
/* Copy spectra to host for cross-checks: which = 0 FB (complex64 [B,1,H,W]), 1 F2B (f32 [B,1,H,W]),
 * 2 FBFy (complex64 [B,3,H,W]). */
int dpir_prox_read(dpir_engine* e, const dpir_prox* p, int which, void* host_dst, size_t cap_bytes);
/* Replaces sr.data_solution(x, FB, FBC, F2B, FBFy, alpha, sf) (utils/utils_sisr.py:65-75):
 * x_dev [B,3,H,W] in [0,1] -> out_dev (may alias x_dev). */
int dpir_data_solution(dpir_engine* e, const dpir_prox* p, const float* x_dev, float alpha, float* out_dev);
/* Replaces main_ddpir.py:395-400: x0 <- x0 + g*(2*data_solution(x0/2+.5, tau) - 1 - x0), in place. */
int dpir_prox_fft_apply(dpir_engine* e, const dpir_prox* p, float* x0_dev, float tau, float guidance);
/* Measurement helper (bench.py `roofline_prox`): dpir_prox_fft_apply n times back to back between two HIP events on the engine stream -- eager launches
 * (use_graph 0) or ONE captured graph of the n applies (use_graph 1: how dpir_run_loop replays the step; no host launch cost, no event record between
 * applies) -> device microseconds per apply, launch boundaries included.  x0 is overwritten n + 1 (+ n) times. */
int dpir_prox_fft_apply_timed(dpir_engine* e, const dpir_prox* p, float* x0_dev, float tau, float guidance, int n, int use_graph, float* us_per_apply);
/* Which kernels run the half-spectrum data_solution (utils/utils_sisr.py:65-75).  mode 1 (and 3, the default), 256 x 256
 * and 512 x 512: one wave per 256- / 512-point transform (64 lanes x 4 / 8 points, permlane-swap / DPP register transposes, a wave-private LDS tile, no workgroup
 * barrier inside a transform) on a COLUMN-major half spectrum, csrc/fft4.hip.  mode 0, and every other size: the two-pass register kernels of csrc/fft2.hip (a thread holds
 * 16 points) on the row-major padded spectrum.  Same mathematics, results within a few 1e-6 of each other.  A dpir_prox keeps the layout of the mode it
 * was created in (dpir_prox_read returns natural order either way).  Drops the captured step graphs.
 * Modes 2 and 3 are 0 and 1 plus the mixed-radix kernels (csrc/fft_mixed.hip) for every shape the power-of-two families refuse: H or W no power of
 * two, or sf not 1, 2, 4, 8 or 16.  3 is the default (env DPIR_PROX_MODE = 0 .. 3 at dpir_create).  Modes 0 and 1 are the strict forms: only the
 * power-of-two families run and any other shape is DPIR_ERR_UNSUPPORTED, as it was before the mixed-radix kernels existed. */
int dpir_set_prox_launch(dpir_engine* e, int mode);
/* Replaces main_ddpir.py:392-394: x0_p = (m*(2y-1)+tau*x0)/(m+tau); x0 += g*(x0_p-x0).  mask u8 [B,3,H,W]. */
int dpir_prox_mask(dpir_engine* e, float* x0_dev, const float* y_dev, const uint8_t* mask_dev,
                   float tau, float guidance, int B, int H, int W);
/* Replaces Resizer(in_shape, 1/sf).forward (utils/utils_resizer.py:55-74, cubic, antialiasing):
 * x_dev [B,3,H,W] -> out_dev [B,3,H/sf,W/sf]. */
int dpir_resize_down(dpir_engine* e, const float* x_dev, float* out_dev, int sf, int B, int H, int W);
/* Replaces main_ddpir.py:401-406 (sr_mode 'cubic', iterative back-projection), in place on x0:
 * in_iter times { x0 <- 2*(z + gamma*up_nearest(y - down(z))/(1+rho)) - 1, z = x0/2+.5 }. */
int dpir_prox_ibp(dpir_engine* e, float* x0_dev, const float* y_dev, float rho, float gamma,
                  int in_iter, int sf, int B, int H, int W);
/* Replaces F.interpolate(y, size=(h*sf,w*sf), mode='bicubic', align_corners=False) (main_ddpir.py:295). */
int dpir_bicubic_up(dpir_engine* e, const float* y_dev, float* out_dev, int sf, int B, int h, int w);

/* ---- loop arithmetic --------------------------------------------------------------------- */
/* Per-step scalars (SURVEY.md 8 a-S), all computed on the host exactly as the reference does. */
typedef struct dpir_step {
    int32_t t;            /* t_i: UNet timestep */
    int32_t last;         /* 1 on the final step: no prox / re-noise (main_ddpir.py:384,448) */
    float c1, c2;         /* eps -> x0 (gaussian_diffusion.py:328-333), float64 tables cast to f32 */
    float tau;            /* rhos[t_i] (main_ddpir.py:389) */
    float sa_t, s1m_t;    /* sqrt_alphas_cumprod[t_i], sqrt_1m_alphas_cumprod[t_i]  (float32 tables) */
    float sa_p;           /* sqrt_alphas_cumprod[t_im1] */
    float k1;             /* float32(np.sqrt(1-zeta)) */
    float q;              /* sqrt(s1m_p^2 - eta_sigma^2), float32 arithmetic as in the reference */
    float es;             /* eta_sigma = eta * s1m_p / s1m_t * sqrt(betas[t_i])  (0 when eta == 0) */
    float k2;             /* np.sqrt(zeta) * s1m_p */
} dpir_step;

/* Replaces main_ddpir.py:451-456 (re-noise to t_{i-1}); x_dev updated in place.
 * x = sa_p*x0 + k1*(q*eps + es*n1) + k2*n2, eps = (x - sa_t*x0)/s1m_t.  n1_dev may be NULL when es == 0. */
int dpir_renoise(dpir_engine* e, float* x_dev, const float* x0_dev, const dpir_step* s,
                 const float* n1_dev, const float* n2_dev, int B, int H, int W);
/* Replaces main_ddpir.py:470,482 + utils_image.tensor2uint_batch (utils/utils_image.py:238-242):
 * x_dev [B,3,H,W] in [-1,1] -> out_f32 [B,3,H,W] = x/2+.5 (optional) and out_u8 [B,H,W,3] (optional). */
/* main_ddpir.py:355-358: x = (sa_t*(2y-1) + s1m_t*n)*mask + (1-mask)*x  (coefficients from the step: sa_t, s1m_t) */
int dpir_repaint_mix(dpir_engine* e, float* x_dev, const float* y_dev, const uint8_t* mask_dev, const dpir_step* s,
                     const float* n_dev, int B, int H, int W);
int dpir_finalize(dpir_engine* e, const float* x_dev, float* out_f32_dev, uint8_t* out_u8_dev, int B, int H, int W);
/* N(0,1) on device (Philox4x32-10 + Box-Muller) keyed by (seed, image index offset, stream id):
 * the perf-mode replacement of torch.randn_like; parity mode feeds host noise. */
int dpir_randn(dpir_engine* e, float* out_dev, uint64_t seed, uint64_t stream_id, int64_t image_offset,
               int B, int C, int H, int W);

/* The loop body's own tensor arithmetic, for a loop that stays in the host language: main_ddpir.py:437 `x = xt - norm_grad * 1.`,
 * :440 `sa_t * (2*y-1) + s1m_t * randn_like(y)`, :444 `xt - norm_grad * lambda_ * norm / rhos[t_i] * 0.35`.  One float32 operation per
 * element, rounded once, like a torch elementwise op: out[i] = x[i] op rhs with rhs = y_dev[i] (y_numel == numel), y_dev[0]
 * (y_numel == 1: a 0-dim tensor such as `norm`) or `scalar` (y_dev NULL).  op: 0 add, 1 sub, 2 mul, 3 div, 4 rhs - x, 5 rhs / x.
 * out_dev may alias x_dev. */
int dpir_ewise(dpir_engine* e, int op, const float* x_dev, const float* y_dev, size_t y_numel, float scalar, float* out_dev, size_t numel);

/* ---- whole restoration loop (main_ddpir.py:291-470 for one batch) ------------------------- */
typedef enum dpir_task { DPIR_TASK_DEBLUR = 0, DPIR_TASK_SR_BLUR = 1, DPIR_TASK_INPAINT = 2, DPIR_TASK_SR_CUBIC = 3 } dpir_task;

typedef struct dpir_loop_desc {
    int32_t task;                 /* dpir_task */
    int32_t B, H, W;              /* H,W = restored (high-res) size */
    int32_t sf;                   /* 1 for deblur / inpaint */
    int32_t kh, kw;               /* PSF size (deblur / sr-blur) */
    int32_t in_iter;              /* sr-cubic */
    float gamma;                  /* sr-cubic */
    float guidance;               /* guidance_scale */
    float sa_start, s1m_start;    /* forward-noise coefficients at t_start (main_ddpir.py:315) */
    const float* y_dev;           /* [B,3,H/sf,W/sf] in [0,1] */
    const float* k_dev;           /* [B,1,kh,kw] or NULL */
    const uint8_t* mask_dev;      /* [B,3,H,W] or NULL */
    const int64_t* labels_host;   /* [B] or NULL (class-conditional UNet) */
    /* host-fed noise (parity mode): init [B,3,H,W]; n1/n2 [(n_steps-1),B,3,H,W]; any may be NULL ->
     * device Philox keyed by (seed, image_offset + b, draw index) */
    const float* noise_init_dev;
    const float* noise_n1_dev;
    const float* noise_n2_dev;
    uint64_t seed;
    int64_t image_offset;         /* global index of image 0 of this shard (multi-GPU invariance) */
    int32_t use_graph;            /* 1: capture one step as a hipGraph and replay it n_steps times */
    int32_t skip_dead_final_eval; /* 1: skip the last UNet call whose output is discarded (Q2) */
    /* generate_mode (main_ddpir.py:349-358, 384): 0 DiffPIR (prox every step), 1 repaint (inpainting only: the known region
     * is re-drawn at the current noise level before every denoiser call, no prox), 2 vanilla (inpainting only: no
     * conditioning inside the loop).  Re-noising is applied in all three (main_ddpir.py:448). */
    int32_t generate_mode;
    /* 1: sub_1_analytic = false -- the first-order data step of main_ddpir.py:420-430 instead of the closed-form prox:
     * x0 <- x0 - d||(2y-1) - Resizer(x0)|| / dx0 * ||.|| / rho (super-resolution tasks, DiffPIR mode; no network backward) */
    int32_t first_order;
    const float* noise_rp_dev;    /* repaint, host-fed noise: [n_steps,B,3,H,W] in step order; NULL -> device Philox (draw 3) */
    int32_t ddim_sample;          /* dpir_run_dps_loop: 1 -> x_prev from ddim_sample(eta=0) instead of p_sample (config.ddim_sample,
                                   * utils_model.py:219-240).  dpir_run_loop ignores it: 'pred_xstart' is the same tensor either way. */
} dpir_loop_desc;

/* Runs init -> n_steps x ([repaint mix ->] UNet -> [prox ->] re-noise) -> finalize.  Outputs (either may be NULL):
 * out_f32_dev [B,3,H,W] in [0,1] un-clamped (x_0 of main_ddpir.py:470), out_u8_dev [B,H,W,3].
 * Synchronisation: in the f32 mode, in gradient mode and once the fused hop is off the call returns as soon as the last step is enqueued
 * (asynchronous on the engine stream).  In the f16 modes with the fused hop on it BLOCKS until the loop has finished: it reads the guard word back
 * (one 8-byte D2H + hipStreamSynchronize) so that a hop time-out can re-run the whole loop on the unfused path before the caller sees a result --
 * callers that queue the next batch's uploads behind the loop lose that overlap; DPIR_FUSE_H1=0 trades ~2 % of the step for an asynchronous return. */
int dpir_run_loop(dpir_engine* e, const dpir_loop_desc* d, const dpir_step* steps_host, int n_steps,
                  float* out_f32_dev, uint8_t* out_u8_dev);

/* The three scalars of a step that depend on (lambda, zeta, sigma), for one image: rhos[t_i] (main_ddpir.py:277-286, 389) and the two zeta
 * coefficients of the re-noise (main_ddpir.py:454-456), computed on the host like dpir_step's (diffpir_amd/schedule.py build_image_table). */
typedef struct dpir_image_step { float tau, k1, k2, reserved; } dpir_image_step;

/* dpir_run_loop with per-image scalars: image b at step i uses per_image_host[i*B + b]. {tau, k1, k2}
 * in place of steps_host[i].{tau, k1, k2} (NULL: the step's own), and device Philox is keyed by
 * image_index_host[b] in place of d->image_offset + b (NULL: that default).  Both NULL == dpir_run_loop.
 * Replaces the outer sweep loop of main_ddpir.py:548-580 (one restoration per (lambda, zeta) point) by rows of one batch: every other field of a
 * step, the timesteps and the denoiser are shared.  Row b computes what dpir_run_loop computes for that image under uniform scalars equal to its
 * own (the same float32 operations in the same order).  Both tables are copied before the call returns.  DPIR_ERR_UNSUPPORTED before anything is
 * enqueued: d->first_order with a per-image table (that data step normalises by ONE residual norm of the whole batch, main_ddpir.py:425-427).
 * The gradient-mode loops and dpir_run_inpaint_loop have no per-image form. */
int dpir_run_loop_per_image(dpir_engine* e, const dpir_loop_desc* d, const dpir_step* steps_host, int n_steps,
                            const dpir_image_step* per_image_host, const int64_t* image_index_host,
                            float* out_f32_dev, uint8_t* out_u8_dev);

/* dpir_randn with an explicit image number per row: row b == dpir_randn(..., image_offset = image_index_host[b], B = 1)
 * (torch.randn_like's perf-mode replacement, SURVEY.md 8a-R, for a batch whose rows are not consecutive images).  Synchronises the stream once
 * (the image numbers are uploaded from the caller's array). */
int dpir_randn_indexed(dpir_engine* e, float* out_dev, uint64_t seed, uint64_t stream_id,
                       const int64_t* image_index_host, int B, int C, int H, int W);

/* ---- inpainting with resampling (main_ddpir_inpainting.py:147-317, iter_num_U >= 1) ------- */
/* One row per sub-step (i, u) of the standalone inpainting program, all computed on the host as that program does
 * (diffpir_amd/schedule.py build_inpaint_rows).  The first ten scalars are dpir_step's. */
typedef struct dpir_inpaint_row {
    int32_t t;            /* t_i: UNet timestep */
    int32_t last;         /* 1 where seq[i] == seq[-1]: a dead denoiser call, nothing else (:261, :285, :296) */
    int32_t pos;          /* position of t_i among the visited timesteps: the U sub-steps of one i share it (hoisted FiLM row) */
    int32_t back;         /* 1: set back to t_i after the re-noise (u < iter_num_U - 1, :296-300) */
    float c1, c2, tau, sa_t, s1m_t, sa_p, k1, q, es, k2;      /* the scalars of dpir_step, main_ddpir_inpainting.py:267, :288-293 */
    float sae;            /* sqrt_alphas_cumprod[t_i] / sqrt_alphas_cumprod[t_im1] (:298) */
    float sb;             /* sqrt(s1m[t_i]^2 - sae^2 * s1m[t_im1]^2) (:299-300); exactly 0 when t_im1 == t_i */
    float sa_n, s1m_n;    /* sqrt_alphas_cumprod / sqrt_1m_alphas_cumprod at the NEXT row's t_i (repaint mix of the next sub-step, :244-246) */
    int32_t mix_next;     /* 1: a next row exists (generate_mode repaint applies its mix at the end of this sub-step) */
    int32_t reserved;
} dpir_inpaint_row;

/* The data side of one sub-step in one pass, in place on x_dev [B,3,H,W] (main_ddpir_inpainting.py:249-300 behind the network call):
 *   x0 = clamp(c1 x - c2 eps)  [-> x0_out_dev when given]; generate_mode 0: x0 += guidance ((mask (2y-1) + tau x0)/(mask + tau) - x0);
 *   x = sa_p x0 + k1 (q (x - sa_t x0)/s1m_t + es n1) + k2 n2; back: x = sae x + sb n_back; generate_mode 1 and mix_next:
 *   x = (sa_n (2y-1) + s1m_n n_repaint_next) mask + (1 - mask) x.  A row with last = 1 only takes the mix.
 * eps_dev [B,eps_channels,H,W] (eps_channels 3 or 6: the UNet's output, channels 0..2 used), y_dev in [0,1], mask_dev uint8 {0,1}.
 * Noise: n2_dev non-NULL -> host-fed tensors [B,3,H,W] (n1 needed when es != 0, n_back when back, n_repaint_next when the mix applies);
 * n2_dev NULL -> Philox in place, streams 1 + 4s / 2 + 4s / 2^32 + s / 3 + 4(s+1) for sub-step ordinal s = `substep`, keyed by (seed, image_offset + b)
 * exactly as dpir_randn would produce them.  Bit-identical to dpir_prox_mask -> dpir_renoise -> dpir_ewise -> dpir_repaint_mix.
 * Asynchronous on the engine stream like its siblings: the row travels by value in the kernel arguments (no copy, no synchronisation). */
int dpir_inpaint_step(dpir_engine* e, float* x_dev, const float* eps_dev, int eps_channels, const float* y_dev, const uint8_t* mask_dev,
                      const dpir_inpaint_row* row, int generate_mode, float guidance, const float* n1_dev, const float* n2_dev,
                      const float* n_back_dev, const float* n_repaint_next_dev, uint64_t seed, int64_t image_offset, int substep,
                      float* x0_out_dev, int B, int H, int W);

/* Runs init -> n_rows x (UNet -> dpir_inpaint_step) -> finalize: the standalone inpainting program's loop for one batch, one captured graph
 * for every sub-step (use_graph).  d as in dpir_run_loop with task DPIR_TASK_INPAINT and sa_start / s1m_start from the t_y initialisation
 * (:190-193); d->generate_mode 0 / 1 / 2.  Host-fed noise (parity mode; all four NULL -> device Philox): d->noise_init_dev [B,3,H,W], and
 * [n_rows,B,3,H,W] in sub-step order for d->noise_n1_dev (eta != 0), d->noise_n2_dev, noise_back_dev (some row has back) and
 * d->noise_rp_dev (repaint).  Synchronisation and the fused-hop guard: as dpir_run_loop. */
int dpir_run_inpaint_loop(dpir_engine* e, const dpir_loop_desc* d, const dpir_inpaint_row* rows_host, int n_rows, const float* noise_back_dev,
                          float* out_f32_dev, uint8_t* out_u8_dev);

/* ---- progressive snapshots (save_progressive / log_process / save_progressive_mask) ----------- */
/* dpir_progress_snapshot replaces main_ddpir_deblur.py:359-371 = main_ddpir_sisr.py:386-398 = main_ddpir_inpainting.py:302-313 for one panel
 * (x_show = x/2+.5 kept where seq[i] is in progress_seq, np.max / np.min of it for log_process), the cv2.hconcat of the kept panels
 * (main_ddpir_deblur.py:400-406, main_ddpir_inpainting.py:356-359: each panel is written at its column block of the strip instead) and
 * main_ddpir_inpainting.py:361-366 (y_t mask + (1 - mask) x_show; that program's y is in [-1,1], hence its y/2+0.5 -- y_dev here is in [0,1]).
 * One pass over x_dev [B,3,H,W] for panel `panel` of `n_panels`; every output is optional (NULL: not written):
 *   strip_f32 [B,3,H,n_panels W] = x/2+.5 and strip_u8 [B,H,n_panels W,3], both bit-equal to dpir_finalize's outputs of the same x;
 *   masked_f32 / masked_u8: the same two layouts of the masked blend (need y_dev and mask_dev [B,3,H,W], mask uint8 {0,1});
 *   minmax_dev [n_panels,B,2]: (max, min) of image b's panel at [panel][b], exact, float32 (4-byte aligned).
 * Only the panel's columns (and its minmax row) are written.  Asynchronous on the engine stream.  DPIR_ERR_INVALID, nothing launched: panel
 * outside [0, n_panels), a masked output without y_dev and mask_dev, a bad shape (see the conventions above; n_panels W must fit an int). */
int dpir_progress_snapshot(dpir_engine* e, const float* x_dev, const float* y_dev, const uint8_t* mask_dev, int panel, int n_panels,
                           float* strip_f32, uint8_t* strip_u8, float* masked_f32, uint8_t* masked_u8, float* minmax_dev, int B, int H, int W);

/* The same film strip out of the whole-loop entries, which never return to the host between steps.  Replaces the `if save_progressive and
 * (seq[i] in progress_seq)` blocks cited above inside the loops of main_ddpir.py:336-338, main_ddpir_deblur.py:242-254 and
 * main_ddpir_inpainting.py:217-228 (diffpir_amd/schedule.py progress_panels computes panel_of_step_host from those recipes). */
typedef struct dpir_progress_desc {
    const int32_t* panel_of_step_host;   /* [n_entries]: the panel taken after step i (dpir_run_loop, dpir_run_dps_loop, dpir_run_deblur_grad_loop) or
                                          * after row r (dpir_run_inpaint_loop: the last sub-step of the timestep; dpir_run_ancestral_loop), or -1 for none.  Copied. */
    int32_t n_entries;                   /* must equal the loop call's n_steps / n_rows */
    int32_t n_panels;
    float* strip_f32; uint8_t* strip_u8; /* as dpir_progress_snapshot, for the loop's B, H, W; any may be NULL */
    float* masked_f32; uint8_t* masked_u8;   /* inpainting loops only (the descriptor's y_dev and mask_dev) */
    float* minmax_dev;
} dpir_progress_desc;
/* Arms the NEXT call of dpir_run_loop / dpir_run_inpaint_loop / dpir_run_ancestral_loop / dpir_run_dps_loop / dpir_run_deblur_grad_loop on this engine, and only that call: the
 * arming is cleared when the call returns, whether it succeeded or not.  NULL disarms.  A step skipped by skip_dead_final_eval still yields its
 * panel (the unchanged x).  The snapshots are launched on the engine stream between the steps, outside the captured step graphs: an armed
 * call replays the same graphs as an unarmed one and computes the same result; an unarmed call launches nothing new.  The loop call returns
 * DPIR_ERR_INVALID before anything is launched when n_entries differs from its n_steps / n_rows or a masked strip is armed for a loop without a
 * mask.  DPIR_ERR_INVALID here: n_panels < 1, an entry outside [-1, n_panels), n_entries < 1 or a NULL table. */
int dpir_set_progress(dpir_engine* e, const dpir_progress_desc* desc);

/* ---- gradient-based sampling (generate_mode 'DPS_y0') ---------------------- */
/* Replaces what torch.autograd does for the reference's DPS branch (main_ddpir.py:370-373, 434-438 with
 * utils_model.grad_and_value, utils/utils_model.py:390-394).  Gradient mode must be switched on BEFORE dpir_load_unet: it builds
 * the dgrad weight packs and makes every forward record what the backward needs (the fused elementwise prologues are off). */
int dpir_enable_grad(dpir_engine* e, int on);
/* Vector-Jacobian product of UNetModel.forward w.r.t. its input: runs the forward (out_dev [B,out_channels,H,W], may be NULL) and
 * returns dx_dev [B,3,H,W] = J(x)^T gout_dev, gout_dev [B,out_channels,H,W].  The unit the parity tests compare with
 * torch.autograd.grad on the reference network; per-layer gradients are readable as taps named "grad:<layer>". */
int dpir_unet_vjp(dpir_engine* e, const float* x_dev, const int64_t* t_host, const int64_t* y_host, const float* gout_dev,
                  float* out_dev, float* dx_dev, int B, int H, int W);
/* Per-step p_sample coefficients (gaussian_diffusion.py:153-167, 268-276: float64 tables cast to float32 by
 * _extract_into_tensor): posterior_mean_coef1/2[t], posterior_log_variance_clipped[t], log(betas[t]). */
typedef struct dpir_dps_coef {
    float pc1, pc2, min_log, max_log;
    float sa_prev, s1m_prev;      /* ddim_sample(eta=0) only: sqrt(alphas_cumprod_prev[t]), sqrt(1 - alphas_cumprod_prev[t]) in float32
                                   * (gaussian_diffusion.py:568-580) */
} dpir_dps_coef;
/* generate_mode 'DPS_y0' for the super-resolution tasks (the only DPS variant the reference can run as shipped: its deblurring
 * operator raises at main_ddpir.py:302 and the inpainting branch never defines xt).  Per step:
 *   xt, x0 = p_sample(x)                       (model_fn 'pred_x_prev_and_start', utils_model.py:207-258)
 *   norm   = || (2y - 1) - Resizer(x0) ||_2    over the whole batch          (grad_and_value)
 *   x      = xt - step_scale * d norm / d x    (main_ddpir.py:437, step_scale = 1), no re-noising (:448)
 * variant 1 = 'DPS_yt' (main_ddpir.py:439-445): y_t = sa_t (2y-1) + s1m_t n;  norm = || y_t - Resizer(xt) ||_2;
 *   x = xt - d norm / d xt * lambda * norm / rho_t * 0.35   -- differentiated w.r.t. xt itself, no network backward (gradient mode not needed).
 * d / steps_host as in dpir_run_loop (task DPIR_TASK_SR_BLUR or _SR_CUBIC; k / mask / n1 / n2 unused); coefs_host [n_steps];
 * noise_ps_dev: host-fed p_sample noise [n_steps, B,3,H,W] in step order or NULL -> device Philox (stream 4*(step+1));
 * noise_yt_dev (variant 1): host-fed y_t noise [n_steps, B,3,H/sf,W/sf] or NULL -> Philox (stream 4*(step+1)+1).
 * This entry and dpir_run_deblur_grad_loop below are ONE loop body over a measurement operator (here Resizer(1/sf)); what is said here of the
 * steps, the dead final step (skip_dead_final_eval), the noise layouts, the Philox streams (init: 0, rows keyed by image_offset) and the
 * progressive strip holds for both.  A steps table in which a non-final step follows a final one is DPIR_ERR_INVALID. */
int dpir_run_dps_loop(dpir_engine* e, const dpir_loop_desc* d, const dpir_step* steps_host, const dpir_dps_coef* coefs_host, int n_steps,
                      int variant, float lambda_, const float* noise_ps_dev, const float* noise_yt_dev, float step_scale,
                      float* out_f32_dev, uint8_t* out_u8_dev);

/* The two plugs the reference's DPS / first-order branches call, for a loop body that stays in the host language (round 4):
 *
 * dpir_p_sample = utils_model.model_fn(x, ..., model_out_type='pred_x_prev_and_start' | 'pred_x_prev') (utils/utils_model.py:207-246,
 *   called at main_ddpir.py:370-373): one denoiser call, then GaussianDiffusion.p_sample with the learned-range variance
 *   (gaussian_diffusion.py:232-326, 395-439) or, with c->ddim, ddim_sample(eta = 0) (:537-585).  noise_dev [B,3,H,W] is the
 *   randn_like draw of the sampler (required; ddim consumes it with sigma = 0).  Outputs xt ("sample") and x0 ("pred_xstart").
 *   In gradient mode the call leaves the forward's tape and the clamp mask on the engine for dpir_grad_and_value.
 *   Needs a learn_sigma model (out_channels == 6), else DPIR_ERR_UNSUPPORTED. */
typedef struct dpir_psample_coef {
    float c1, c2;                 /* sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t] */
    float pc1, pc2, min_log, max_log;   /* as dpir_dps_coef */
    int32_t ddim;
    float sa_prev, s1m_prev;      /* as dpir_dps_coef */
} dpir_psample_coef;
int dpir_p_sample(dpir_engine* e, const float* x_dev, int t, const dpir_psample_coef* c, const float* noise_dev, const int64_t* y_host,
                  float* xt_out_dev, float* x0_out_dev, int B, int H, int W);
/* model_out_type 'epsilon' / 'score' (utils/utils_model.py:247-255): out = (x - sqrt_ac x0) / sqrt_1m_ac  [score: * -1 / sqrt_1m_ac]. */
int dpir_eps_from_xstart(dpir_engine* e, const float* x_dev, const float* x0_dev, float sqrt_ac, float sqrt_1m_ac, int score,
                         float* out_dev, size_t numel);
/* dpir_grad_and_value = utils_model.grad_and_value(operator=Resizer(1/sf), x, x_hat, measurement) (utils/utils_model.py:390-394):
 *   difference = measurement - Resizer(x_hat);  norm = ||difference||_2 over the WHOLE batch (all ranks of the communicator when one
 *   with more than one rank is attached);  norm_grad = d norm / d x.
 * through_network = 1: x is the input of the LAST dpir_p_sample on this engine and x_hat_dev its pred_xstart output (checked) -- the
 *   gradient runs through the clamp and the denoiser (main_ddpir.py:436, generate_mode DPS_y0); gradient mode required.
 * through_network = 0: x is x_hat itself (main_ddpir.py:425 first-order data step, :443 DPS_yt): norm_grad = -Resizer^T(difference) / norm.
 * measurement_dev [B,3,H/sf,W/sf] in the operator's range (the reference passes 2y-1 or y_t).  norm_grad_out_dev [B,3,H,W];
 * norm_out_dev: one device float (may be NULL).  Asynchronous. */
int dpir_grad_and_value(dpir_engine* e, int through_network, const float* x_hat_dev, const float* measurement_dev, int sf,
                        float* norm_grad_out_dev, float* norm_out_dev, int B, int H, int W);

/* ---- the standalone deblurring program's gradient modes (main_ddpir_deblur.py) ------------------------------------------------ */
/* main_ddpir.py cannot run DPS_y0 / DPS_yt / the first-order data step for deblurring (its batched-k einsum raises at :302), and the entries
 * above keep refusing it.  The reference's second driver, main_ddpir_deblur.py, does run them, with its own operator and initialisation;
 * the entries below are that program's semantics, selected explicitly.
 *
 * dpir_blur_reflect replaces Tx (main_ddpir_deblur.py:307-311, 317-321): F.conv2d(ReflectionPad2d(K // 2)(x / 2 + 0.5), eye(3) (x) k), :179-180:
 *   out[n,c,i,j] = sum_{a,b} k[n,a,b] v[n,c, r_H(i+a-p), r_W(j+b-p)],  v = x xa + xb,  p = K / 2,  r_L the reflection -t -> t, L-1+t -> L-1-t
 *   (cross-correlation, the edge sample not repeated).  x_dev, out_dev [B,3,H,W]; k_dev [B,1,kh,kw], one PSF per image.  The loop passes
 *   xa = xb = 0.5.  fp32 fmaf accumulation in ascending (a, b) order, independent of tiling and batch: image n equals the same image run alone.
 * dpir_blur_reflect_adjoint replaces what torch.autograd derives from Tx inside utils_model.grad_and_value (utils/utils_model.py:390-394):
 *   gx = xa R^T C^T g (the transposed correlation on the padded grid, the reflected border folded back), a gather without atomics.
 * Both return DPIR_ERR_INVALID before anything is allocated or enqueued when kh != kw, K is even (the reference's output would not have y's
 * size), K / 2 >= H or W (ReflectionPad2d refuses it) or B <= 0, and DPIR_ERR_UNSUPPORTED for K > 79. */
int dpir_blur_reflect(dpir_engine* e, const float* x_dev, const float* k_dev, int kh, int kw, float xa, float xb, float* out_dev, int B, int H, int W);
int dpir_blur_reflect_adjoint(dpir_engine* e, const float* g_dev, const float* k_dev, int kh, int kw, float xa, float* gx_dev, int B, int H, int W);
/* utils_model.grad_and_value(operator=Tx, x, x_hat, measurement) as main_ddpir_deblur.py:312, 324, 334 call it: difference = measurement - Tx(x_hat),
 * measurement_dev [B,3,H,W] in [0,1] (y, or y_t / 2 + 0.5).  The program restores one image at a time, so the norm is PER IMAGE:
 * norm_out_dev [B] (may be NULL), norm_grad_out_dev[n] = d norm_n / d x_n.  through_network and its tape preconditions as dpir_grad_and_value. */
int dpir_grad_and_value_blur(dpir_engine* e, int through_network, const float* x_hat_dev, const float* measurement_dev, const float* k_dev, int kh, int kw,
                             float* norm_grad_out_dev, float* norm_out_dev, int B, int H, int W);
/* The loop of main_ddpir_deblur.py:257-360 in its gradient modes, task DPIR_TASK_DEBLUR, sf 1, k_dev required: the body of dpir_run_dps_loop
 * over the operator Tx.  What differs: the measurement (y in [0,1]), the norm (each image's own, no collective), the initial x (y itself,
 * not its bicubic up-sampling), the full-size y_t draw, a unit DPS_y0 step, and variant 2:
 *   variant 0 'DPS_y0' (:323-327): xt, x0 = p_sample(x);  x = xt - d || y - Tx(x0) || / d x  (through the denoiser; gradient mode), no re-noising;
 *   variant 1 'DPS_yt' (:329-336): y_t = sa_t (2y-1) + s1m_t n;  x = xt - d || (y_t/2+.5) - Tx(xt) || / d xt * lambda * norm / rho_t * 0.35, no re-noising;
 *   variant 2 first-order data step (sub_1_analytic false, :305-314): x0 = pred_xstart;  x0 <- x0 - d || y - Tx(x0) || / d x0 * norm / rho_t, then the
 *             DiffPIR re-noise (:339-347; noise_n1_dev / noise_n2_dev of the descriptor, [n_steps - 1, B,3,H,W], or device Philox).
 * norm is each image's own.  The initial x = sa_start (2y-1) + s1m_start n0 takes the descriptor's coefficients, which the host computes from t_y
 * (:228-231): sqrt_ac[t_start] / sqrt_ac[t_y] and sqrt(s1m[t_start]^2 - that^2 s1m[t_y]^2) on the driver's float32 tables.  The analytic DiffPIR
 * mode of that program is dpir_run_loop with the same two coefficients.  coefs_host (variants 0, 1), noise_ps_dev, noise_yt_dev [n_steps, B,3,H,W]
 * and the Philox streams as dpir_run_dps_loop.  Eager launches (no step graph); single GPU. */
int dpir_run_deblur_grad_loop(dpir_engine* e, const dpir_loop_desc* d, const dpir_step* steps_host, const dpir_dps_coef* coefs_host, int n_steps,
                              int variant, float lambda_, const float* noise_ps_dev, const float* noise_yt_dev, float* out_f32_dev, uint8_t* out_u8_dev);

/* ---- ancestral inpainting loops (main_ddpir.py:341-470, model_output_type 'pred_x_prev') ------ */
/* task 'inpaint' with generate_mode 'repaint' (RePaint-style ancestral sampling) or 'vanilla' (plain DDPM ancestral sampling, the body of
 * p_sample_loop) and iter_num_U 1: per visited timestep [the repaint mix, :356-358 ->] x = model_fn(x, 'pred_x_prev') (:365-366), i.e.
 * diffusion.p_sample(clip_denoised=True) with the learned-range variance or, with ddim_sample, diffusion.ddim_sample(eta=0).  Nothing else
 * happens in a step (:384-445 has no branch for these modes, the re-noise at :448 requires 'pred_xstart', the set-back at :462 requires
 * u < iter_num_U - 1), and the final step is LIVE: x is replaced by the sample at t_i there too (t = 0: nonzero = 0).
 * One row per visited step, all computed on the host (diffpir_amd/schedule.py build_ancestral_rows). */
typedef struct dpir_ancestral_row {
    int32_t t;            /* t_i: UNet timestep */
    int32_t nonzero;      /* t != 0: p_sample's nonzero_mask (gaussian_diffusion.py:431-433) */
    int32_t mix_next;     /* 1: a next row exists (generate_mode repaint applies its mix at the end of this step) */
    int32_t reserved;
    float c1, c2;         /* sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t]: eps -> x0 (gaussian_diffusion.py:328-333) */
    float pc1, pc2, min_log, max_log;   /* as dpir_dps_coef */
    float sa_prev, s1m_prev;            /* ddim_sample(eta = 0) only, as dpir_dps_coef */
    float sa_t, s1m_t;    /* sqrt_alphas_cumprod / sqrt_1m_alphas_cumprod at t_i (driver's float32 tables): the mix ahead of the FIRST row */
    float sa_n, s1m_n;    /* the same pair at the NEXT row's t_i (repaint mix of the next step, :356-358) */
} dpir_ancestral_row;

/* The data side of one step in one pass, in place on x_dev [B,3,H,W], behind the network call:
 *   x0 = clamp(c1 x - c2 eps, -1, 1)  [-> x0_out_dev when given];  eps = out6[:, 0:3], v = out6[:, 3:6];
 *   p_sample:  mean = pc1 x0 + pc2 x;  lv = frac max_log + (1 - frac) min_log, frac = (v + 1) / 2;  x = mean + nonzero expf(0.5 lv) n;
 *   ddim != 0: x = x0 sa_prev + s1m_prev (c1 x - x0) / c2   (eta = 0: the sampler's draw is multiplied by 0 and not read);
 *   generate_mode 1 (repaint) and mix_next: x = (sa_n (2y-1) + s1m_n n_repaint_next) mask + (1 - mask) x.
 * Every expression is psample_kernel's / repaint_mix_kernel's, operation for operation: the pass equals dpir_p_sample's arithmetic followed by
 * dpir_repaint_mix bit for bit.  out6_dev [B,out_channels,H,W] is the UNet's output; out_channels must be 6 (a learn_sigma model), else
 * DPIR_ERR_UNSUPPORTED.  generate_mode: 1 repaint (y_dev in [0,1] and mask_dev uint8 {0,1} required) or 2 vanilla (both unused, may be NULL).
 * Noise: n_ps_dev non-NULL -> host-fed tensors [B,3,H,W] (n_repaint_next_dev needed when the mix applies); n_ps_dev NULL -> Philox in place,
 * keyed by (seed, image_offset + b) exactly as dpir_randn would produce them: stream 4 (step + 1) for the sampler's draw (as dpir_run_dps_loop)
 * and 3 + 4 (step + 1) for the next step's mix (as dpir_run_loop / dpir_inpaint_step); ddim and nonzero = 0 draw nothing for the sampler.
 * Asynchronous on the engine stream: the row travels by value in the kernel arguments.  DPIR_ERR_INVALID before any launch: a NULL engine,
 * x, out6 or row, y / mask missing in repaint mode, generate_mode not 1 or 2, step < 0, a bad shape (see the conventions above), host noise
 * without n_repaint_next_dev where the mix applies, n_repaint_next_dev without n_ps_dev. */
int dpir_ancestral_step(dpir_engine* e, float* x_dev, const float* out6_dev, int out_channels, const float* y_dev, const uint8_t* mask_dev,
                        const dpir_ancestral_row* row, int generate_mode, int ddim, const float* n_ps_dev, const float* n_repaint_next_dev,
                        uint64_t seed, int64_t image_offset, int step, float* x0_out_dev, int B, int H, int W);

/* Runs init -> [the first row's repaint mix ->] n_rows x (UNet -> dpir_ancestral_step) -> finalize for one batch, one captured graph for
 * every step (d->use_graph).  d as in dpir_run_loop with task DPIR_TASK_INPAINT, sf 1; read from it: generate_mode (1 or 2), ddim_sample,
 * sa_start / s1m_start, y / mask / labels, seed / image_offset, noise_init_dev and noise_rp_dev.  Host-fed noise (parity mode; all NULL ->
 * device Philox, init: stream 0): noise_ps_dev [n_rows,B,3,H,W] in step order selects it and then needs d->noise_init_dev [B,3,H,W] and, in
 * repaint mode, d->noise_rp_dev [n_rows,B,3,H,W].  d->skip_dead_final_eval is ignored: the final evaluation is live.  A model without
 * learn_sigma is DPIR_ERR_UNSUPPORTED.  Progress panels (dpir_set_progress): the panel of row r shows x after that row's sample, before the
 * next row's mix.  Synchronisation and the fused-hop guard: as dpir_run_loop. */
int dpir_run_ancestral_loop(dpir_engine* e, const dpir_loop_desc* d, const dpir_ancestral_row* rows_host, int n_rows, const float* noise_ps_dev,
                            float* out_f32_dev, uint8_t* out_u8_dev);

/* ---- multi-GPU: the one collective of the path ------------------------------ */
/* One process and one engine per GPU; images are block-partitioned over ranks, no exchange inside the loop (the reference is
 * single-GPU: main_ddpir.py:135 sets world_size and never uses it).  After a batch, ONE all-gather of the uint8 results over
 * RCCL / xGMI, enqueued on the engine stream behind the loop.  librccl.so is bound at run time (dlopen).
 *   dpir_comm_unique_id : rank 0 creates the 128-byte ncclUniqueId; the host side ships it to the other ranks;
 *   dpir_comm_init      : ncclCommInitRank on this engine's device;
 *   dpir_allgather_results(send [bytes_per_rank], recv [world * bytes_per_rank]) : ncclAllGather(ncclUint8);
 *   dpir_comm_allreduce_max / dpir_comm_barrier : the two rendezvous primitives a multi-GPU driver needs around its timed region
 *                         (MAX over ranks of one host double; a barrier is the same exchange with the value ignored) -- with
 *                         them the N-GPU launch needs no other communication library;
 *   dpir_comm_destroy   : also done by dpir_destroy. */
int dpir_comm_unique_id(void* id128_out);
/* ncclGetVersion() of the bound librccl.so (diagnostics of the multi-GPU bench line); DPIR_ERR_UNSUPPORTED when librccl cannot be loaded */
int dpir_comm_version(int* version_out);
int dpir_comm_init(dpir_engine* e, int world, int rank, const void* id128);
int dpir_allgather_results(dpir_engine* e, const void* send_dev, void* recv_dev, size_t bytes_per_rank);
int dpir_comm_allreduce_max(dpir_engine* e, double* value_inout);
int dpir_comm_barrier(dpir_engine* e);
int dpir_comm_destroy(dpir_engine* e);

/* ---- degradation synthesis and metrics: the steps either side of the loop ------------------ */
/* Replaces CustomDataset.__getitem__'s arithmetic (main_ddpir.py:84-114) on the device.  gt_u8_dev: ground truth, uint8
 * [B,H,W,3] (what util.imread_uint returns).  deblur: scipy.ndimage.convolve(img_H, k, mode='wrap') on the uint8 image (float64
 * accumulation, result cast back to uint8) / 255; sr (both sr_modes): utils_image.imresize_np(img_H / 255, 1 / sf) (== the Resizer
 * weights); inpaint: img_H * mask / 255.  Then img_L*2-1 + N(0, (2*noise_level_img)^2), /2 + 0.5 in float64 (:112-114) and, for
 * inpainting, * mask (:311-313).  noise_dev: [B,3,h,w] standard-normal floats (host-fed) or NULL -> device Philox keyed by
 * (seed, image_offset + b).  y_out_dev: [B,3,H/sf,W/sf] float32 in [0,1]. */
typedef struct dpir_degrade_desc {
    int32_t task;                 /* dpir_task */
    int32_t B, H, W, sf;
    int32_t kh, kw;               /* deblur PSF size */
    float noise_level_img;        /* already / 255 (main_ddpir.py:138) */
    uint64_t seed;
    int64_t image_offset;
} dpir_degrade_desc;
int dpir_degrade(dpir_engine* e, const dpir_degrade_desc* d, const uint8_t* gt_u8_dev, const float* k_dev, const uint8_t* mask_dev,
                 const float* noise_dev, float* y_out_dev);
/* Replaces main_ddpir.py:482-517: per image, PSNR of x_0*2-1 against img_H/255*2-1 (utils_image.calculate_psnr_batch terms,
 * max_pixel 2, eps 1e-10) and the same on the Y channel of rgb2ycbcr_batch(only_y) (utils_image.py:470-490; its two zero
 * channels are part of the mean, as in the reference).  x0_dev [B,3,H,W] in [0,1]; outputs: HOST arrays of B floats (syncs).
 * Precision: the inputs are the reference's float32 images (x0 and uint2single(img_H)); the differences, the Y combination, the mean and
 * the logarithm are evaluated in float64 and the result is rounded to float once.  This is NOT the reference's float32 evaluation of
 * calculate_psnr_batch: it is within 2e-5 dB of the float64 value at every image size, which the float32 evaluation is not (1.7e-4 dB on
 * a 63-pixel image at 87 dB); the two agree to 2e-5 dB on the reference's fixture.  Identical images give +inf in both. */
int dpir_metrics(dpir_engine* e, const float* x0_dev, const uint8_t* gt_u8_dev, int B, int H, int W, float* psnr_host, float* psnr_y_host);
/* The 8-bit protocol of the reference's standalone programs: util.calculate_psnr(img_E, img_H, border=border) on tensor2uint bytes
 * (main_ddpir_deblur.py:380, main_ddpir_inpainting.py:325, main_ddpir_sisr.py:406), the same on the Y channel through
 * rgb2ycbcr(only_y=True) (main_ddpir_sisr.py:459; utils_image.py:446-467), and util.calculate_ssim (utils_image.py:616-661) on both;
 * border = sf for super-resolution (main_ddpir.py:552, main_ddpir_sisr.py:166).  The estimate is exactly one of est_u8_dev, uint8 [B,H,W,3]
 * (what dpir_finalize writes), and est_f32_dev, float32 [B,3,H,W] in [0,1] and NOT clamped, which is quantised as tensor2uint does (clamp,
 * x 255.0 in float32, round half to even: dpir_finalize's bytes).  gt_u8_dev: uint8 [B,H,W,3].  `border` pixels are cropped from all four
 * sides first.  out_host: HOST array [B][4] of doubles (syncs): psnr, psnr_y, ssim, ssim_y.
 *   psnr    20 log10(255 / sqrt(mse)) in float64 from the exact integer sum of squared byte differences over the three channels
 *           (utils_image.py:586-599); +inf when the sum is 0.
 *   Y byte  rint(fma(b, 24.966, fma(g, 128.553, r * 65.481)) / 255.0 + 16.0) in float64, half to even: the summation order that equals
 *           numpy's dot on all 194 byte triplets that are exact .5 ties.  psnr_y and ssim_y are the same measures on the Y bytes.
 *   ssim    float64 throughout.  Window g[i] = exp(-(i - 5)^2 / (2 1.5^2)), 11 taps, normalised to sum 1 (cv2.getGaussianKernel(11, 1.5)),
 *           its outer product applied as a correlation at the valid positions only ([5:-5, 5:-5]), evaluated separably; five maps per
 *           plane (x, y, x^2, y^2, xy); C1 = (0.01 255)^2, C2 = (0.03 255)^2; the mean of
 *           ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)) over all valid positions of all three channels (the
 *           reference's loop over range(3) passes the whole H x W x 3 array each time: its mean of three equal numbers is that value).
 * An image's four numbers have the same bits wherever it sits in a batch, for every B and on every repeat (per-tile partial sums reduced
 * in a fixed order, no floating-point atomics); identical images give +inf and exactly 1.  DPIR_ERR_INVALID before anything is enqueued: a
 * null argument, both estimates or neither, B < 1, border < 0, H - 2 border < 11 or W - 2 border < 11 (the reference takes the mean of an
 * empty map there). */
int dpir_metrics_u8(dpir_engine* e, const uint8_t* est_u8_dev, const float* est_f32_dev, const uint8_t* gt_u8_dev, int B, int H, int W, int border,
                    double* out_host);

/* ---- saved results (save_L / save_LEH) ------------------------------------------------------ */
/* The bytes of the reference's saved measurement and of its L / E / H comparison strip for one batch, in one pass, asynchronous on the engine
 * stream (like dpir_finalize).  Replaces
 *   the measurement   util.single2uint(img_L) at its own h x w: main_ddpir.py:508-511, main_ddpir_deblur.py:423-424,
 *                     main_ddpir_inpainting.py:343-344;
 *   the strip, mode 0 main_ddpir_deblur.py:412-421 = main_ddpir_sisr.py:440-451: img_I = cv2.resize(img_L, x sf, INTER_NEAREST), the kernel
 *                     bytes zoomed x 3 (INTER_NEAREST) written at img_I[:3kh, -3kw:], THEN img_L pasted at img_I[:h, :w], and
 *                     np.concatenate([img_I, img_E, img_H], axis=1);
 *   the strip, mode 1 main_ddpir_inpainting.py:346-347: np.concatenate([single2uint(img_L), img_E, img_H], axis=1) (sf = 1, no inset).
 * y_dev float32 [B,3,h,w], h = H / sf, w = W / sf: what dpir_degrade wrote.  The L bytes are rint(clamp(y, 0, 1) 255) in float32, half to even
 * (dpir_finalize's conversion): single2uint of the ENGINE's float32 measurement, bit for bit np.uint8((y.clip(0, 1) * 255.).round()); not
 * single2uint of the reference's float64 img_L.  kv_u8_dev uint8 [B,kh,kw]: the host's single2uint(k / k.max()), or NULL for no inset (ignored
 * in mode 1).  est_u8_dev, gt_u8_dev uint8 [B,H,W,3]: the loop's out_u8 and img_H.  Outputs, each may be NULL (not written; the inputs only it
 * needs may then be NULL too): L_u8_out_dev [B,h,w,3]; leh_u8_out_dev [B,H,3W,3], whose panel 0 is per pixel the native L inside [0,h) x [0,w),
 * else the inset (grey on three channels, source kv[Y / 3][(X - (W - 3kw)) / 3]) inside rows [0,3kh) and columns [W - 3kw, W), else the zoom
 * (source pixel (Y / sf, X / sf)) -- the reference's write order as a priority; with sf = 1 the paste hides the inset entirely, as there.  Panels
 * 1 and 2 are est and gt.  DPIR_ERR_INVALID before anything is launched: B < 1, sf < 1 or not dividing H and W, a mode other than 0 / 1, mode
 * 1 with sf != 1, kernel bytes with 3kh > H or 3kw > W (the reference's slice assignment raises there), a missing input. */
typedef struct dpir_result_desc {
    int32_t B, H, W, sf, kh, kw;
    int32_t mode;                        /* 0: kernel-inset strip (deblurring / super-resolution); 1: inpainting strip */
} dpir_result_desc;
int dpir_result_panels(dpir_engine* e, const dpir_result_desc* d, const float* y_dev, const uint8_t* kv_u8_dev, const uint8_t* est_u8_dev,
                       const uint8_t* gt_u8_dev, uint8_t* L_u8_out_dev, uint8_t* leh_u8_out_dev);

/* ---- LPIPS (calc_LPIPS: main_ddpir.py:489-493, 532-535, 543-545) --------------------------- */
/* Replaces loss_fn_vgg = lpips.LPIPS(net='vgg') and its call loss_fn_vgg(x_0*2-1, img_H/255*2-1) (LPIPS v0.1, eval, normalize=False, spatial=False):
 * the scaling layer (shift -.030 -.088 -.188, scale .458 .448 .450, applied before the first convolution's zero padding), the 13 convolutions of
 * VGG16 `features` (3x3 pad 1 + bias + ReLU; 2x2 stride-2 max-pool, floor, behind convolutions 2, 4, 7, 10), taps behind the ReLU of convolutions
 * 2, 4, 7, 10, 13, and per tap n = f / (sqrt(sum_c f^2) + 1e-10), d = sum_c w_c (n0 - n1)^2, spatial mean; the score is the sum of the five means.
 * dpir_lpips_load copies and packs the weights (caller keeps the host arrays).  Canonical keys: features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,
 * bias} (OIHW / [Cout]) and lin{0..4}.weight (64, 128, 256, 512, 512 values, any rank); DPIR_ERR_INVALID naming the first missing / mis-shaped key.
 * Independent of dpir_load_unet and dpir_set_precision: the trunk always runs the exact-fp32 MFMA convolution. */
int dpir_lpips_load(dpir_engine* e, const dpir_tensor* weights, int n_weights);
/* x0_dev [B,3,H,W] float32 in [0,1] and NOT clamped (x_0 of main_ddpir.py:470); the ground truth as uint8 [B,H,W,3] (gt_u8_dev; img_H/255 formed
 * as dpir_metrics forms it) or float32 [B,3,H,W] in [0,1] (gt_f32_dev) -- exactly one of the two.  lpips_host: HOST array of B floats (syncs).
 * Features are float32; the channel norms, the distance and the means are evaluated in float64 and rounded to float once.  An image's score has
 * the same bits wherever it sits in a batch, for every B and on every repeat (no atomics; fixed-order reductions); identical images give 0.
 * The 2B rows run in chunks through an engine-owned arena of at most 8 rows at 256 x 256 (about 0.8 GB; one pair at least for larger images);
 * env DPIR_LPIPS_CHUNK=<rows> forces a smaller chunk (tests) -- chunking changes no bit.  DPIR_ERR_INVALID before anything is enqueued: H or W
 * below 16 (relu5_3 would be empty), no weights loaded, both or neither ground truth. */
int dpir_lpips(dpir_engine* e, const float* x0_dev, const uint8_t* gt_u8_dev, const float* gt_f32_dev, int B, int H, int W, float* lpips_host);
/* Parity taps: with keep on, every dpir_lpips call keeps its five post-ReLU feature maps (relu1_2 ... relu5_3) and dpir_lpips_read_tap copies
 * tap k of the last call to host as [2B,C_k,H_k,W_k]: rows [0,B) the estimate, rows [B,2B) the ground truth.  Off by default (a B = 16 call at
 * 256 x 256 would keep 1 GB).  host_dst NULL: only numel_out is written. */
int dpir_lpips_keep_taps(dpir_engine* e, int on);
int dpir_lpips_read_tap(dpir_engine* e, int k, float* host_dst, size_t cap_floats, size_t* numel_out);

/* ---- FID (calc_FID; the FID column of the paper's tables, reference README.md:119-141) ------ */
/* The `pool3` features of the FID Inception-v3 as pytorch-fid defines them (README.md:119-141 reports FID beside PSNR and LPIPS; the reference
 * computes it with pytorch-fid on saved images).  Entry: v = u8 / 255, bilinear resize to 299 x 299 (align_corners = False, no antialias), 2 v - 1.
 * Network: 94 BasicConv layers (convolution without bias, eval-mode BatchNorm with eps 1e-3 folded in by the host, ReLU) in the stem and the
 * blocks Mixed_5b/5c/5d, 6a, 6b..6e, 7a, 7b/7c; avg-pools 3x3 s1 p1 that do not count the padding; Mixed_7c's pool branch is a max-pool;
 * the features are the mean over the 8 x 8 positions (float64, rounded once).  Mean, covariance and the Frechet distance are the host's
 * (diffpir_amd/fid.py).  dpir_fid_load copies and packs the weights (caller keeps the host arrays).  Keys: "<layer>.weight" [Cout,Cin,KH,KW]
 * and "<layer>.bias" [Cout], BatchNorm already folded; DPIR_ERR_INVALID naming the first missing / mis-shaped key.  A second load replaces
 * the first.  Independent of dpir_load_unet and dpir_set_precision: the network always runs the exact-fp32 MFMA convolution, whose
 * accumulators are added to a float64 running sum every 64 products. */
int dpir_fid_load(dpir_engine* e, const dpir_tensor* weights, int n_weights);
/* Exactly one image pointer: img_u8_dev uint8 [B,H,W,3] (what dpir_finalize writes, what a saved PNG holds -- pytorch-fid reads PNGs) or
 * img_f32_dev float32 [B,3,H,W] in [0,1].  feat_host: HOST array of B * 2048 floats (syncs).  An image's features have the same bits
 * wherever it sits in a batch, for every B, chunk size and repeat (no atomics, no split-K; every sum has one order).  The images run in
 * chunks of 16 through an engine-owned arena (about 250 MB); env DPIR_FID_CHUNK=<images> forces a smaller chunk -- chunking changes no bit.
 * DPIR_ERR_STATE without a prior dpir_fid_load; DPIR_ERR_INVALID for B < 1, both pointers or neither. */
int dpir_fid_features(dpir_engine* e, const uint8_t* img_u8_dev, const float* img_f32_dev, int B, int H, int W, float* feat_host);
/* Parity taps (pytorch-fid's block boundaries): with keep on, every dpir_fid_features call keeps 13 tensors and dpir_fid_read_tap copies tap k
 * of the last call to host: k = 0, 1 the stem behind its two max-pools [B,64,73,73], [B,192,35,35]; 2..4 Mixed_5b/5c/5d [B,256|288|288,35,35];
 * 5..9 Mixed_6a..6e [B,768,17,17]; 10 Mixed_7a [B,1280,8,8]; 11, 12 Mixed_7b/7c [B,2048,8,8]; k = 13 the features [B,2048] (kept always).
 * host_dst NULL: only numel_out is written. */
int dpir_fid_keep_taps(dpir_engine* e, int on);
int dpir_fid_read_tap(dpir_engine* e, int k, float* host_dst, size_t cap_floats, size_t* numel_out);

/* ---- instrumentation --------------------------------------------------------------------- */
/* Kernel-time accounting with HIP events on the engine stream.  class ids: 0 conv3x3, 1 conv1x1,
 * 2 groupnorm-stats, 3 attention, 4 fft-prox, 5 elementwise/other, 6 whole unet forward.
 * dpir_prof_enable(1) makes every launch of a class bracketed by events (slow; bench only). */
#define DPIR_PROF_CLASSES 8
int dpir_prof_enable(dpir_engine* e, int on);
int dpir_prof_reset(dpir_engine* e);
/* ms_out / count_out: arrays of DPIR_PROF_CLASSES */
int dpir_prof_read(dpir_engine* e, double* ms_out, int64_t* count_out);
/* FLOPs (2*MAC, conv+linear+attention) of one UNet forward for one image at HxW; 0 if no model */
double dpir_unet_flops(dpir_engine* e, int H, int W);
/* number of captured step graphs currently cached by dpir_run_loop (one per shape / task / mode, shared by all batches) */
int dpir_graph_cache_size(dpir_engine* e);
/* the same split by profiling class (0 conv3x3, 1 conv1x1 incl. qkv/proj_out, 3 attention matmuls, 5 linears; -1 total) */
double dpir_unet_flops_class(dpir_engine* e, int H, int W, int cls);

#ifdef __cplusplus
}
#endif
#endif /* DIFFPIR_ENGINE_H */
