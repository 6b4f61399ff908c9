// conv9.hip: whole-image 3x3 convolution for 8 x 8 layers (one workgroup per image and 32 output channels, whole K, no split-K slabs).
#pragma once
#include "common.h"
#include "conv6_params.h"
namespace dpir {

struct Conv9Args {
    const void* xhi = nullptr; const void* xlo = nullptr;   // blocked split activations [n][Cin / 8][H][W][16 B] (act.hip)
    const void* w16 = nullptr; float w16_scale = 1.f;       // pack_weights_conv6 layout
    const float* bias = nullptr; float* out = nullptr; const float* res = nullptr; int res_mode = 0;
    int B = 0, Cin = 0, Cout = 0, H = 0, W = 0;
    double2* stat_plane = nullptr;     // optional [B][Cout] fp64 {sum, sum of squares} of the stored planes (the split-K combine's record format)
    bool x1 = false;                   // single-product mode (f16x1): hi planes / hi weight halves only
    // fused hop to the next convolution of a ResBlock: gamma / beta / FiLM / planes / range guard of Conv6Emit are used; its accumulators,
    // arrival counters and spin fields are ignored (a GroupNorm group is whole inside one workgroup).  No fp32 output, no residual.
    const Conv6Emit* emit = nullptr;
};

struct Conv9K {
    const char* xhi; const char* xlo; int C8;
    const char* w16; const float* bias; float* out; const float* res; int res_mode;
    int B, Cout, n_chunks, n_co_blocks;
    float out_scale;
    double2* stat;
    Conv6Emit em;
};

// conv9_refusal (conv_plan.h): H = W = 8, Cin % 16 == 0, Cout % 32 == 0; emit: GroupNorm groups never straddle a 32-channel tile.  When a layer
// takes this kernel (kConv9MinWg workgroups) is the planner's decision.
bool conv9_supported(int B, int Cin, int Cout, int H, int W, bool emit);
Status launch_conv9(hipStream_t s, const Conv9Args& a);

}  // namespace dpir
