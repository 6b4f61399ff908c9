// conv11.hip: conv7's 8 x 32 geometry (128 output channels x 8 rows x 32 columns per workgroup, 64 co x 128 px per wave, whole K) with
// v_mfma_f32_16x16x32_f16 in the main loop instead of 32x32x16.  f16x3 only.
#pragma once
#include "common.h"
#include "conv6_params.h"
#include <vector>
namespace dpir {

struct Conv11Args {
    const void* xhi = nullptr; const void* xlo = nullptr;   // blocked split activations [n][Cin / 8][H][W][16 B] (act.hip), as conv6 / conv7
    const void* w11 = nullptr; float w_scale = 1.f;         // pack_weights_conv11 layout, the scale pack_weights_conv6 returned
    const float* bias = nullptr; float* out = nullptr; const float* res = nullptr; int res_mode = 0;
    int B = 0, Cin = 0, Cout = 0, H = 0, W = 0;
    float2* stat = nullptr;            // optional [B][Cout][conv6_stat_slots(H, W)] epilogue partial sums (conv7's slot records)
    int ksplit = 1;                    // the caller's split-K factor for this launch; anything but 1 is refused
    int precision = 1;                 // engine precision: 0 f32, 1 f16x3, 2 f16x1; only 1 is taken
    bool grad = false;                 // gradient-mode forward: refused
    // fused hop to the next convolution of a ResBlock (Conv6Emit, conv7's contract): no fp32 output, no statistics, no residual
    const Conv6Emit* emit = nullptr;
};

// conv11_shape_ok / conv11_hop_ok (conv_plan.h) on this device: Cin % 32 == 0, Cout % 128 == 0, W % 32 == 0, H % 8 == 0; which layers take
// this kernel is the planner's decision
bool conv11_supported(int Cin, int Cout, int H, int W);
bool conv11_emit_supported(int Cout, int H, int W);
Status launch_conv11(hipStream_t s, const Conv11Args& a);
// Host: OIHW fp32 -> one 1 KiB record per (pair step, co-block, wave co-half, M-tile, hi | lo) in A-fragment lane order of the 16x16x32
// instruction; `scale` is the power of two pack_weights_conv6 chose for the same layer (every f16 half equals that pack's).
void pack_weights_conv11(const float* w_oihw, int cout, int cin, float scale, std::vector<uint16_t>& out);

}  // namespace dpir
