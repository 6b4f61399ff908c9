// Declarations for ancestral.hip: the fused data side of one ancestral inpainting step (main_ddpir.py:341-470, model_output_type 'pred_x_prev').
#pragma once
#include "common.h"
#include "elem.h"

namespace dpir {

// Device-resident copy of the CURRENT row of dpir_run_ancestral_loop (fixed address, like InpaintRowDev: one captured graph serves every step, the
// host copies rows_dev[r] -> cur between replays).  `st` comes first so that the UNet's hoisted FiLM table reads it as a StepDev: st.i is the
// row's position among the visited timesteps, which here is the step ordinal itself (iter_num_U = 1).  Of st only t, i, c1, c2 are set.
struct AncestralRowDev {
    StepDev st;
    int s;                  // step ordinal: host-noise slice and the Philox stream offset (sampler 4 (s + 1), next mix 3 + 4 (s + 1))
    int nonzero;            // t != 0 (gaussian_diffusion.py:431-433)
    int mix_next;           // 1: apply the NEXT step's repaint mix (main_ddpir.py:356-358) at the end of this pass
    int emit;               // 1 (armed progress panel, loop only): write x as it stands BEFORE the next step's mix to AncestralLoopDev::premix
    float pc1, pc2, min_log, max_log;   // posterior mean and learned-range variance bounds (gaussian_diffusion.py:268-276, 318)
    float sa_prev, s1m_prev;            // ddim_sample(eta = 0) (gaussian_diffusion.py:568-580)
    float sa_n, s1m_n;      // sa / s1m at the next step's timestep (repaint mix)
};

// Per-batch values of dpir_run_ancestral_loop that the kernel reads on the device: host-fed noise is [n_rows, B, 3, H, W] per draw kind, indexed by
// the step ordinal; both null -> Philox in place.
struct AncestralLoopDev {
    const float* y; const uint8_t* mask;
    const float* nps; const float* nrp;
    unsigned long long seed; long long image_offset;
    float* premix;          // [B,3,H,W] scratch for rows with `emit`, or null (no progress strip armed)
};

struct AncestralStepArgs {
    float* x;                   // [B,3,H,W], updated in place
    const float* out6;          // UNet output [B,6,H,W]: channels 0..2 eps, 3..5 the variance interpolation v
    const float* y; const uint8_t* mask;
    int mode;                   // generate_mode: 1 repaint, 2 vanilla
    int ddim;                   // 1: ddim_sample(eta = 0) instead of p_sample
    int device_noise;           // 1: every draw is Philox in place (seed / image offset below or from lp), 0: the two pointers below
    const float *nps, *nrp_next;    // host noise of THIS call (plug entry), or null with lp (loop: lp's tensors + row->s slices)
    unsigned long long seed; long long image_offset;
    float* x0_out;              // optional: the clamped x0 prediction
    float* premix_out;          // optional: x of this step before the next step's repaint mix is applied to it; with lp: lp->premix on rows with `emit`
    const AncestralRowDev* row; // device (the loop: the fixed-address current row), or null -> row_val
    AncestralRowDev row_val;    // the row by value in the kernel arguments (plug entry: no copy, no synchronisation)
    const AncestralLoopDev* lp; // device or null
    int B, HW, cus;
    int scalar_only;            // 1: a tensor behind lp is not 16-byte aligned (the launcher cannot see those pointers)
};
Status launch_ancestral_step(hipStream_t s, const AncestralStepArgs& a);

}  // namespace dpir
