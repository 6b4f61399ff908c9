// Declarations for results.hip: the saved measurement (save_L) and the L / E / H comparison strip (save_LEH) of one batch.
#pragma once
#include "common.h"

namespace dpir {

// y [B,3,h,w] float32 in [0,1] (un-clamped), h = H / sf, w = W / sf; kv [B,kh,kw] bytes (null: no inset); est, gt [B,H,W,3] bytes.
// Every output is optional (null: not written): L_u8 [B,h,w,3] = rint(clamp(y, 0, 1) 255); leh_u8 [B,H,3W,3] = zoomed L with the kernel inset and
// the native L on top | est | gt.  The caller has checked: sf divides H and W, 3 kh <= H and 3 kw <= W when kv is given.
struct ResultArgs {
    const float* y; const uint8_t* kv; const uint8_t* est; const uint8_t* gt;
    uint8_t* L_u8; uint8_t* leh_u8;
    int B, H, W, sf, kh, kw, cus;
};
Status launch_result_panels(hipStream_t s, const ResultArgs& a);

}  // namespace dpir
