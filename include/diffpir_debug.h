/* diffpir_debug.h -- development-only entry points of libdiffpir_hip.so (not part of the drop-in boundary). */
#ifndef DIFFPIR_DEBUG_H
#define DIFFPIR_DEBUG_H
#include "diffpir_engine.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Average time (ms) of one convolution launch of the given shape on synthetic operands; `dbg` disables parts of the
 * kernel for ablation (1 no MFMA, 2 no prologue transform, 4 no global loads, 8 no LDS stores, 16 no epilogue stores);
 * mode 0 plain / 1 nearest-up source / 2 avg-pool source; with_prm: fused GroupNorm+SiLU prologue on/off. */
int dpir_debug_conv_bench(dpir_engine* e, int B, int Cin, int Cout, int H, int W, int ks, int mode, int with_prm,
                          int dbg, int iters, double* ms_out);
/* Concurrency probe: `blocks` workgroups of `threads` threads park a pattern in `lds_bytes` of LDS and in 32 registers per
 * thread, wait `spin_ticks` of the 100 MHz wall clock, verify; *bad_out = LDS mismatches (low 32 bits) + register mismatches << 32. */
int dpir_debug_victim(dpir_engine* e, int lds_bytes, int threads, int blocks, long long spin_ticks, int iters, unsigned long long* bad_out);
/* ALU probe: threads run `iters_in_kernel` dependent exact-integer fp32 operations (mode 0 v_add_f32, 1 v_pk_add_f32, 2 v_pk_fma_f32,
 * 3 v_pk_mul_f32) and check the closed-form result; *bad_out = number of threads whose result was wrong. */
int dpir_debug_victim_alu(dpir_engine* e, int mode, int blocks, int iters_in_kernel, int launches, unsigned long long* bad_out);
/* Register-FFT probe (csrc/dbg_fft.inc): same source built with (pk) and without (nopk) packed-fp32 instructions; *bad_out =
 * threads whose two identical computations disagreed. */
int dpir_debug_victim_fft_pk(dpir_engine* e, int blocks, int iters_in_kernel, int launches, unsigned long long* bad_out);
int dpir_debug_victim_fft_nopk(dpir_engine* e, int blocks, int iters_in_kernel, int launches, unsigned long long* bad_out);
/* conv7 (csrc/conv7.hip: 64 co x 128 px per wave, weights straight into registers; every launch class) against conv6 (csrc/conv6.hip,
 * still built for the 8 x 32 geometry, W >= 32) on the same split planes and weight pack, with the residual form res_mode (-1 none,
 * 0 same shape, 1 half resolution, 2 double resolution).  x1: f16x1 planes / products; split: allow split-K (the partial slabs are
 * compared instead of output + fused GroupNorm statistics; *ksplit_out = slabs); scaled: a device output scale (the dgrad route).
 * *mismatches_out = elements whose bits differ (expected 0: same MFMA order per accumulator), *maxdiff_out their largest absolute
 * difference, *ms6_out / *ms7_out the average launch times over `iters` back-to-back launches. */
int dpir_debug_conv7_check(dpir_engine* e, int B, int Cin, int Cout, int H, int W, int res_mode, int x1, int split, int scaled, int iters,
                           double* ms6_out, double* ms7_out, unsigned long long* mismatches_out, float* maxdiff_out, int* ksplit_out);
/* 1 when a 3x3 launch of this shape may take conv7's fused GroupNorm hop (Conv6Emit), 0 when the dispatch falls back to the unfused path;
 * *capacity_out = resident EMIT workgroups of the device (CUs x occupancy) the waiting-set limit is derived from. */
int dpir_debug_conv7_emit_supported(dpir_engine* e, int B, int Cout, int H, int W, int* capacity_out);
/* One 1x1 convolution layer on host operands through the forward's dispatch: out[B][Cout][H][W] = W[Cout][ca+cb] * concat(xa, xb)
 * (+ bias, + res); prm: optional [B][ca+cb][4] {mean, scale, shift, SiLU flag} GroupNorm prologue; res: optional residual of the output's
 * shape.  tile 0: launch_conv5's own choice (DPIR_CONV5_SMALL), or the general fp32 kernel where conv5 refuses the shape; 1 / 2: the
 * 128 x 256 / 64 x 128 conv5 tile whatever the workgroup count.  *path_out = 0 fp32 kernel, 1 / 2 the conv5 tile that ran.  The engine's
 * precision (f16x3 / f16x1) selects the products. */
int dpir_debug_conv5_layer(dpir_engine* e, int B, int ca, int cb, int Cout, int H, int W, int tile, const float* xa, const float* xb,
                           const float* w, const float* bias, const float* prm, const float* res, float* out, int* path_out);
/* One 3x3 convolution layer on host operands through the routes of the forward (Fwd::conv / Fwd::gn_conv): prologue, then launch_conv6
 * (conv6 / conv7, all three tile geometries, whole K or split-K), launch_conv8 or the general fp32 kernel.  Sources are at the resolution
 * `mode` implies (0 plain, 1 nearest-up: H/2 x W/2, 2 average pool: 2H x 2W); H x W is the output resolution.
 *   prologue 0 none; 1 the table prm[B][ca+cb][4] {mean, scale, shift, SiLU flag} (act_split, or the fp32 kernel's own prologue); 2 GroupNorm32
 *     (gamma, beta, optional per-image FiLM rows film[B][2C] = {scale, shift}) + SiLU through gn_act_small, which computes the statistics.
 *   res_mode -1 none, 0 same shape, 1 half resolution (nearest-up), 2 double resolution (2x2 mean); scaled: a device output scale of 0.25.
 *   route 0: the engine precision's own dispatch (f16x3 / f16x1: planes + launch_conv6; f32, or a shape conv6 refuses: launch_conv);
 *     6 / 7: force_kernel; 8: launch_conv8 (prologue 1 with the SiLU flag, one source, mode 0).
 *   split 0: no slab buffer; 1: a slab buffer, launch_conv6's own rule decides.
 *   defer (split, route 0 / 7): the split-K combine is left to a second stage, gn_act_small(gamma2, beta2, SiLU) with the pending convolution
 *     followed by a second 3x3 layer (w2 [Cout2][Cout][3][3], bias2): out = the first layer as gn_act_small stored it, out2 = the second layer.
 * Outputs: out; stat_out[B][Cout][2] fp64 {sum, sum of squares} where the launch produced statistics (stat_kind_out 1: epilogue slots,
 * folded here; 2: the split-K combine's per-plane records; 0 none; 3 left pending); path_out 0 fp32 kernel / 6 / 7 / 8; ksplit_out. */
typedef struct dpir_debug_conv3_desc {
    int32_t B, ca, cb, Cout, H, W, mode, res_mode, scaled, prologue, route, split, defer, Cout2;
    const float *xa, *xb, *w, *bias, *res, *prm, *gamma, *beta, *film, *gamma2, *beta2, *w2, *bias2;
    float* out; double* stat_out; float* out2;
    int32_t stat_kind_out, path_out, ksplit_out, reserved;
} dpir_debug_conv3_desc;
int dpir_debug_conv3_layer(dpir_engine* e, dpir_debug_conv3_desc* d);
/* One 8 x 8 3x3 layer on host operands through conv9 (csrc/conv9.hip: one workgroup per image and 32 output channels, whole K), as the
 * forward launches it above its workgroup threshold (the probe has no threshold: one image can be run alone).  x[B][Cin][H][W] is at the output
 * resolution; prm: optional table [B][Cin][4] {mean, scale, shift, SiLU flag} applied by act_split; res / res_mode as dpir_debug_conv3_desc.
 *   hop 0: out[B][Cout][H][W] and stat_out[B][Cout][2] fp64 {sum, sum of squares} of the stored planes.
 *   hop 1: the first layer's epilogue writes the second layer's operand planes -- GroupNorm32(gamma2, beta2), optional per-image FiLM rows
 *     film2[B][2 Cout] = {scale, shift}, SiLU -- and the second layer (w2 [Cout2][Cout][3][3], bias2) runs on conv9 as well: out2[B][Cout2][H][W].
 * A refusal (shape, gradient-mode engine, f32 precision) is a non-zero return code with dpir_last_error's text; ran_out = 1 when conv9 ran.
 * iters > 0: the launch (hop: both launches) is repeated back to back that many times and ms_out is the average time of one repeat. */
typedef struct dpir_debug_conv9_desc {
    int32_t B, Cin, Cout, H, W, res_mode, hop, Cout2;
    const float *x, *w, *bias, *res, *prm, *gamma2, *beta2, *film2, *w2, *bias2;
    float* out; double* stat_out; float* out2;
    int32_t ran_out, iters;
    double ms_out;
} dpir_debug_conv9_desc;
int dpir_debug_conv9_layer(dpir_engine* e, dpir_debug_conv9_desc* d);
/* One 3x3 layer of the 8 x 32 geometry on host operands through conv11 (csrc/conv11.hip: conv7's tile with the 16x16x32 MFMA), without the
 * forward's workgroup threshold.  x, prm, res / res_mode, out, stat_out (the epilogue's slots, folded here) as dpir_debug_conv9_desc.
 *   route 0: conv11; route 7: the same planes through launch_conv6 with conv7 forced (the arm conv11 is timed against).
 *   ksplit: the split-K factor the caller would have used; conv11 refuses anything but 1.
 *   hop 1 (route 0): the first layer's epilogue writes the second layer's planes -- GroupNorm32(gamma2, beta2), optional FiLM rows film2[B][2 Cout],
 *     SiLU -- and the second layer (w2 [Cout2][Cout][3][3], bias2) runs through launch_conv6: out2[B][Cout2][H][W].
 * A refusal (Cin, Cout, tile shape, split-K, gradient-mode engine, f32 / f16x1 precision, a hop whose groups straddle waves) is a non-zero return
 * code with dpir_last_error's text; ran_out = 11 when conv11 ran, 12 for its hop, 7 for conv7.  iters > 0: the convolution launch alone (planes
 * already built; hop: both launches, the hop's arena cleared in between) is repeated back to back that many times, ms_out = average of one repeat. */
typedef struct dpir_debug_conv11_desc {
    int32_t B, Cin, Cout, H, W, res_mode, route, ksplit, hop, Cout2;
    const float *x, *w, *bias, *res, *prm, *gamma2, *beta2, *film2, *w2, *bias2;
    float* out; double* stat_out; float* out2;
    int32_t ran_out, iters;
    double ms_out;
} dpir_debug_conv11_desc;
int dpir_debug_conv11_layer(dpir_engine* e, dpir_debug_conv11_desc* d);
/* conv1 of an up-sampling ResBlock (3x3 on the nearest-x2 up-sampled x) on host operands.  x[B][Cin][Hs][Ws] is at the SOURCE resolution, out
 * [B][Cout][2 Hs][2 Ws]; prm: optional table [B][Cin][4] {mean, scale, shift, SiLU flag} applied by act_split at the source resolution.
 *   route 0: conv_up (csrc/conv_up.hip: four 2x2 phase convolutions of the source image); route 1: the up-sampled planes + launch_conv6.
 *   hop 0: out and stat_out[B][Cout][2] fp64 {sum, sum of squares} (the epilogue's slots, folded here).
 *   hop 1: the first layer's epilogue writes the second layer's planes -- GroupNorm32(gamma2, beta2), optional FiLM rows film2[B][2 Cout], SiLU --
 *     and the second layer (w2 [Cout2][Cout][3][3], bias2) runs through launch_conv6: out2[B][Cout2][2 Hs][2 Ws].
 *   force_hop: the hop without the forward's lower bound of workgroups (kHopMinWg, csrc/conv_plan.h; small test shapes).
 * A refusal (shape, residual, gradient-mode engine, f32 precision) is a non-zero return code with dpir_last_error's text; ran_out = 1 conv_up,
 * 2 conv_up's hop, 7 launch_conv6's route.  iters > 0: the whole route (act_split and every launch) is repeated that many times, ms_out = average. */
typedef struct dpir_debug_conv_up_desc {
    int32_t B, Cin, Cout, Hs, Ws, hop, force_hop, Cout2, route, reserved;
    const float *x, *w, *bias, *res, *prm, *gamma2, *beta2, *film2, *w2, *bias2;
    float* out; double* stat_out; float* out2;
    int32_t ran_out, iters;
    double ms_out;
} dpir_debug_conv_up_desc;
int dpir_debug_conv_up_layer(dpir_engine* e, dpir_debug_conv_up_desc* d);
/* What the engine's last eager forward ran (recorded while taps are collected): one record per convolution launch, in launch order.
 *   kernel: 0 fp32 kernel, 5 conv5, 6 conv6, 7 conv7, 17 conv7's narrow variant, 8 conv8, 9 conv9, 11 conv11, 12 conv_up, 60 the split-K combine
 *     launch_conv6_resolve (same layer name as the convolution it finishes); ks: 3 or 1.
 *   hop: 0 none, 1 conv7 / conv11 through the arena, 2 conv9 inside one workgroup, 3 conv_up through the arena.
 *   stat_kind: 0 none, 1 epilogue slots, 2 fp64 per plane, 3 the split-K combine was done by the next layer's fused prologue (gn_act_small).
 * Up to `cap` records are written; *n_out is the number there are. */
typedef struct dpir_debug_route_rec {
    char layer[80];
    int32_t kernel, ks, ksplit, hop, stat_kind, reserved;
    long long workgroups;
} dpir_debug_route_rec;
int dpir_debug_route_log(dpir_engine* e, dpir_debug_route_rec* recs, int cap, int* n_out);
/* The planner of the 3x3 routes (csrc/conv_plan.h) on its own: no engine, no GPU.  Capacities (resident workgroups of the conv7 / conv11 /
 * conv_up emitting kernels) are arguments; knobs == NULL means the built-in defaults, whatever the environment says.  Fields as Conv3Query /
 * Conv3Plan / ResblockQuery / ResblockPlan there; slab_floats 0 = no slab buffer offered; stats: statistics buffers offered. */
typedef struct dpir_debug_conv_knobs {
    int32_t conv8, conv9, conv9_min_wg, conv11, conv_up, split_below, split_target, fuse_small, fuse_h1, emit_skip;
} dpir_debug_conv_knobs;
void dpir_debug_conv_knobs_default(dpir_debug_conv_knobs* k);
typedef struct dpir_debug_conv3_query {
    int32_t B, Cin, Cout, H, W, precision, grad, w16, w8, w11, conv8_source, defer, hop, has_res, stats, force_kernel;
    long long slab_floats;
} dpir_debug_conv3_query;
typedef struct dpir_debug_conv_plan {
    int32_t kernel, hop, geo, ksplit, chunks_per_split, stat_kind, stat_slots, refused;
    long long workgroups;
} dpir_debug_conv_plan;
/* n queries -> n plans */
int dpir_debug_conv3_plan(const dpir_debug_conv3_query* q, int n, const dpir_debug_conv_knobs* knobs, int cap7, int cap11, int cap_up,
                          dpir_debug_conv_plan* out);
/* One ResBlock (H x W: its input resolution; mode 0 plain, 1 up, 2 down; a 1x1 skip projection when Cin != Cout) with the weight packs
 * load_conv makes for `precision`. */
typedef struct dpir_debug_resblock_query {
    int32_t B, Cin, Cout, H, W, mode, concat, precision, grad, hop_allowed;
    long long arena_words_left, slab_floats;
} dpir_debug_resblock_query;
typedef struct dpir_debug_resblock_plan_out {
    int32_t up, skip_emit, hop, arena_counters;
    dpir_debug_conv_plan conv1, conv2;
} dpir_debug_resblock_plan_out;
int dpir_debug_resblock_plan(const dpir_debug_resblock_query* q, const dpir_debug_conv_knobs* knobs, int cap7, int cap11, int cap_up,
                             dpir_debug_resblock_plan_out* out);
/* The attention core (csrc/attn.hip) and its backward (csrc/grad.hip: launch_attention_bwd) on host operands, through the product's launchers.
 *   qkv[B][3C][T] in the legacy order: heads first, then q | k | v inside each head (QKVAttentionLegacy); head_ch as the model's num_head_channels.
 *   out[B][C][T] = launch_attention.  dAtt[B][C][T] (optional): dqkv[B][3C][T] = launch_attention_bwd, its T x T scratch allocated here.
 * Every buffer a kernel writes has 256 floats of a fixed bit pattern in front of and behind it and starts out filled with that pattern (a NaN);
 * guard_bad_out = guard words that changed, over all of them.  Operands are allocated at their exact size.  A launcher's refusal (head_ch != 64,
 * C no multiple of 64, backward with T > 1024 -- for which no T x T scratch is allocated) is a non-zero return code with dpir_last_error's text. */
typedef struct dpir_debug_attention_desc {
    int32_t B, C, T, head_ch;
    const float *qkv, *dAtt;
    float *out, *dqkv;
    uint64_t guard_bad_out;
} dpir_debug_attention_desc;
int dpir_debug_attention(dpir_engine* e, dpir_debug_attention_desc* d);
/* One GroupNorm32 (+ FiLM, + SiLU) site on host operands, forward table and backward, through the product's launchers.
 *   The source is the virtual concat of xa[B][ca][Hs][Ws] and xb[B][cb][Hs][Ws] (cb may be 0); gamma, beta [ca+cb]; film (optional) [B][2(ca+cb)]
 *   = {scale, shift} rows; silu: the SiLU flag of the table.
 *   Forward: launch_gn_stats per source, then launch_gn_prm, as Fwd::gn (csrc/unet.hip) chains them.  prm_out[B][C][4] = {mean, a, b, SiLU flag}
 *   with GN+FiLM(x) = (x - mean) * a + b; stats_out[B][32][2] = {mean, rstd} per (image, group).
 *   Backward (dA given): launch_gn_bwd on that same device table and statistics.  dA[B][C][Ho][Wo] is the gradient w.r.t. the activated and resampled
 *   tensor: mode 0 Ho x Wo = Hs x Ws, 1 (nearest-up) 2Hs x 2Ws, 2 (2x2 mean) Hs/2 x Ws/2.  acc_a / acc_b: accumulate into the prior contents
 *   ga_init / gb_init instead of overwriting; extra (optional, mode 0, cb = 0): a tensor shaped like xa added into ga before dx.
 *   ga_out[B][ca][Hs][Ws], gb_out[B][cb][Hs][Ws]; ns_out = gn_bwd_parts(C, Hs, Ws), the partial workgroups per group.
 * Guard words as for dpir_debug_attention.  A launcher's refusal (C no multiple of 32, mode 2 with an odd source) is a non-zero return code. */
typedef struct dpir_debug_groupnorm_desc {
    int32_t B, ca, cb, Hs, Ws, mode, silu, acc_a, acc_b, reserved;
    const float *xa, *xb, *gamma, *beta, *film, *dA, *ga_init, *gb_init, *extra;
    float *prm_out, *stats_out, *ga_out, *gb_out;
    int32_t ns_out, reserved2;
    uint64_t guard_bad_out;
} dpir_debug_groupnorm_desc;
int dpir_debug_groupnorm(dpir_engine* e, dpir_debug_groupnorm_desc* d);
/* The engine's f16 operand range guard word (DPIR_ERR_RANGE), read in stream order behind whatever was enqueued; clear != 0 zeroes it afterwards.
 * *count is the WHOLE word: bits 0 .. 39 are the lanes that clamped a value (or saw a NaN) since the word was last cleared -- waves that share an
 * operand may each count it, so only zero / non-zero is a contract --, bits 40 and up count the fused-hop time-outs (csrc/conv_epilogue.h).
 * The layer probes above synchronise without checking or clearing the word; dpir_sync / dpir_d2h check it, a forward or a loop clears it. */
int dpir_debug_range_counter(dpir_engine* e, unsigned long long* count, int clear);
/* The dgrad's per-image operand scale (csrc/grad.hip launch_grad_scale, then launch_grad_unscale with the factors it made) on a host tensor
 * x[B][per_img], for a table of C channels: sn_out[2B] = {s_n, then s_min / s_n}, scal_out[2] = {s_min, 1 / s_min}, prm_out[B][C][4] =
 * {0, s_n, 0, 0} (s_min for an all-zero image), x_out[B][per_img] = x after the un-scale; parts_out = grad_scale_parts(B).  Guard words as for
 * dpir_debug_attention. */
typedef struct dpir_debug_grad_scale_desc {
    int32_t B, C;
    int64_t per_img;
    const float* x;
    float *sn_out, *scal_out, *prm_out, *x_out;
    int32_t parts_out, reserved;
    uint64_t guard_bad_out;
} dpir_debug_grad_scale_desc;
int dpir_debug_grad_scale(dpir_engine* e, dpir_debug_grad_scale_desc* d);
/* The plan of the mixed-radix FFT prox (csrc/fft_plan.h) on its own: no engine, no GPU.
 * dpir_debug_fft_plan: the radix list of an N-point transform in forward order (up to radix_cap written, *n_radices = how many there are; the
 *   trailing ones multiply to sf) and, when perm != NULL, perm[f] = the stored position of frequency f (N ints).  DPIR_ERR_INVALID when sf does not
 *   divide N, DPIR_ERR_UNSUPPORTED when N has a prime factor above 31.
 * dpir_debug_prox_layout: the layout dpir_prox_fft_precalc stores a (H, W, sf) problem in under launch mode prox_mode (dpir_set_prox_launch, 0 .. 3) --
 *   0 FullBitrev, 1 HalfRows, 2 HalfCols, 3 FullDigitrev -- and, for the two full layouts, the column strips of the solve: strip_count strips of
 *   strip_width columns over [0, W), the last one strip_last wide.  A shape no kernel serves returns the error code dpir_prox_fft_precalc returns
 *   for it, with its text in msg (msg_cap bytes; may be NULL). */
int dpir_debug_fft_plan(int N, int sf, int* radices, int radix_cap, int* n_radices, int* perm);
int dpir_debug_prox_layout(int H, int W, int sf, int prox_mode, int* layout, int* strip_width, int* strip_count, int* strip_last, char* msg, int msg_cap);
#ifdef __cplusplus
}
#endif
#endif
