// conv_up.hip: the 3x3 convolution of a nearest-x2 up-sampled image as four 2x2 phase convolutions of the SOURCE image (f16x3 / f16x1).
#pragma once
#include "common.h"
#include "conv6_params.h"
#include <vector>
namespace dpir {

struct ConvUpArgs {
    const void* xhi = nullptr; const void* xlo = nullptr;   // blocked split activations at the SOURCE resolution [n][Cin / 8][Hs][Ws][16 B] (act.hip, mode 0)
    const void* wup = nullptr; float wup_scale = 1.f;       // pack_weights_conv_up layout
    const float* bias = nullptr; float* out = nullptr;      // out [B][Cout][2 Hs][2 Ws]
    const float* res = nullptr;                             // refused: conv1 of a ResBlock never has a residual
    int B = 0, Cin = 0, Cout = 0, Hs = 0, Ws = 0;
    float2* stat = nullptr;            // optional [B][Cout][conv_up_stat_slots(Hs, Ws)] fp32 partial sums of 64 stored values each (conv6's epilogue record)
    bool x1 = false;                   // single-product mode (f16x1): hi planes / hi weight halves only
    const Conv6Emit* emit = nullptr;   // fused hop: the next convolution's planes at 2 Hs x 2 Ws instead of `out`; cnt holds B x Cout / 64 counters
    int min_wg_hop = 0;                // the hop is refused below this many workgroups (Fwd: kHopMinWg; tests: 0)
};

// conv_up_refusal (conv_plan.h) on this device: null when the launch is supported, else the refusal text
const char* conv_up_supported(int B, int Cin, int Cout, int Hs, int Ws, bool emit, int min_wg_hop = 0);
int conv_up_stat_slots(int Hs, int Ws);          // == conv6_stat_slots(2 Hs, 2 Ws)
// OIHW fp32 3x3 -> phase pack; returns the power-of-two scale (max |combined weight| * scale in [512, 1024))
float pack_weights_conv_up(const float* w_oihw, int cout, int cin, std::vector<uint16_t>& out);
Status launch_conv_up(hipStream_t s, const ConvUpArgs& a);

}  // namespace dpir
