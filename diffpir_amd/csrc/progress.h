// Declarations for progress.hip: one panel of the progressive "process" strip (save_progressive / log_process).
#pragma once
#include "common.h"

namespace dpir {

// Panel `panel` of `n_panels`: x [B,3,H,W] in [-1,1] -> column block [panel W, (panel + 1) W) of the strips, whose row pitch is n_panels W.
// Every output is optional (null: not written).  y in [0,1] and mask uint8 {0,1}, both [B,3,H,W], are read for the masked pair only.
struct ProgressArgs {
    const float* x;
    const float* y; const uint8_t* mask;
    float* strip_f32; uint8_t* strip_u8;        // [B,3,H,P W] = x/2+.5 ; [B,H,P W,3] = rint(clamp(x/2+.5, 0, 1) 255)
    float* masked_f32; uint8_t* masked_u8;      // the same layouts for y mask + (1 - mask) (x/2+.5)
    float* minmax;                              // [P,B,2]: (max, min) of image n's panel at minmax[(panel B + n) 2]
    int B, H, W, panel, n_panels, cus;
};
Status launch_progress_snapshot(hipStream_t s, const ProgressArgs& a);

}  // namespace dpir
