// Declarations for inpaint.hip: the fused data side of one inpainting sub-step (main_ddpir_inpainting.py:249-300).
#pragma once
#include "common.h"
#include "elem.h"

namespace dpir {

// Device-resident copy of the CURRENT sub-step's row of dpir_run_inpaint_loop (fixed address, like StepDev for dpir_run_loop: one captured
// graph serves every sub-step, the host copies rows_dev[r] -> cur between replays).  `st` comes first so that the UNet's hoisted FiLM table
// and xstart-style consumers read it as a StepDev: st.i is the position of t_i among the visited timesteps (the U sub-steps of one timestep
// share a FiLM row), NOT the sub-step ordinal.
struct InpaintRowDev {
    StepDev st;
    int s;                  // sub-step ordinal: host-noise slice and the Philox stream offset (draw + 4 s; set-back 2^32 + s)
    int back;               // 1: set back to t_i after the re-noise (u < U - 1, main_ddpir_inpainting.py:296-300)
    int mix_next;           // 1: apply the NEXT sub-step's repaint mix (:244-246) at the end of this pass
    int emit;               // 1 (armed progress panel, loop only): write x as it stands BEFORE the next sub-step's mix to InpaintLoopDev::premix
    float sae, sb;          // set-back pair: sa[t_i] / sa[t_im1], sqrt(s1m[t_i]^2 - sae^2 s1m[t_im1]^2)
    float sa_n, s1m_n;      // sa / s1m at the next sub-step's timestep (repaint mix)
};

// Per-batch values of dpir_run_inpaint_loop that the kernel reads on the device (see LoopDev): host-fed noise is [n_rows, B, 3, H, W] per
// draw kind, indexed by the sub-step ordinal; all null -> Philox in place.
struct InpaintLoopDev {
    const float* y; const uint8_t* mask;
    const float* n1; const float* n2; const float* nback; const float* nrp;
    unsigned long long seed; long long image_offset;
    float* premix;          // [B,3,H,W] scratch for rows with `emit`, or null (no progress strip armed)
};

struct InpaintStepArgs {
    float* x;                   // [B,3,H,W], updated in place
    const float* eps; int eps_ch;   // UNet output [B,eps_ch,H,W]: channels 0..2 are eps
    const float* y; const uint8_t* mask;
    int mode;                   // generate_mode: 0 DiffPIR, 1 repaint, 2 vanilla
    float guidance;
    int device_noise;           // 1: every draw is Philox in place (seed / image offset below or from lp), 0: the four pointers below
    const float *n1, *n2, *nback, *nrp_next;    // host noise of THIS call (plug entry), or null with lp (loop: lp's tensors + row->s slices)
    unsigned long long seed; long long image_offset;
    float* x0_out;              // optional: the clamped x0 prediction, before the prox
    float* premix_out;          // optional: x of this sub-step before the next sub-step's repaint mix is applied to it (what a progress panel shows,
                                // main_ddpir_inpainting.py:303 precedes :245 of the next iteration); with lp: lp->premix on rows with `emit`
    const InpaintRowDev* row;   // device (the loop: the fixed-address current row), or null -> row_val
    InpaintRowDev row_val;      // the row by value in the kernel arguments (plug entry: no copy, no synchronisation)
    const InpaintLoopDev* lp;   // device or null
    int B, HW, cus;
    int scalar_only;            // 1: a tensor behind lp is not 16-byte aligned (the launcher cannot see those pointers)
};
Status launch_inpaint_step(hipStream_t s, const InpaintStepArgs& a);

}  // namespace dpir
