// LPIPS v0.1, net = 'vgg' (lpips.LPIPS(net='vgg'), eval, normalize=False, spatial=False): scaling layer, the 13 convolutions of VGG16
// `features` and the five bias-free 1x1 heads.  The convolutions go through launch_conv (exact fp32 MFMA, conv2.hip) whatever the engine's
// precision mode; everything else is in lpips.hip.
#pragma once
#include "common.h"

struct dpir_engine;

namespace dpir {

constexpr int kLpipsConvs = 13, kLpipsTaps = 5;
// pairs per chunk: 4 image pairs (8 rows) at 256 x 256, more at smaller sizes, never fewer than one pair
constexpr long long kLpipsChunkPixels = 4ll * 256 * 256;

struct LpipsConv { float* w = nullptr; float* bias = nullptr; int cin = 0, cout = 0, coutp = 0; };

struct LpipsState {
    bool loaded = false;
    LpipsConv conv[kLpipsConvs];
    float* lin[kLpipsTaps] = {};
    float* zero_bias = nullptr;                     // 512 zeros: the slab launches of launch_conv add no bias
    std::vector<void*> weight_allocs;
    // arena of one chunk: the scaled input [2P,3,H,W], two ping-pong activation buffers [2P,64,H,W] and the per-slab convolution sums
    // [2P,256,H,W] (Cin / 16 partial tensors of a layer); grown on demand, bounded by the chunk rule: 0.8 GB at 256 x 256
    float *in = nullptr, *act[2] = {nullptr, nullptr}, *slabs = nullptr;
    size_t in_cap = 0, act_cap = 0;                 // floats
    double* partial = nullptr; size_t partial_cap = 0;       // [P][blocks] per-workgroup sums of one tap
    double* score_d = nullptr; float* score_f = nullptr; size_t score_cap = 0;   // [B]
    // the five post-ReLU feature maps of the last call, rows [0,B) the estimate and [B,2B) the ground truth (dpir_lpips_keep_taps)
    float* tap[kLpipsTaps] = {}; size_t tap_cap[kLpipsTaps] = {}; size_t tap_numel[kLpipsTaps] = {};
};

Status lpips_load(dpir_engine* e, const dpir_tensor* weights, int n);
void lpips_free(dpir_engine* e);
// scores -> the state's score_f [B] (device); asynchronous on the engine stream.  Exactly one of gt_u8 / gt_f32.
Status lpips_run(dpir_engine* e, const float* x0, const uint8_t* gt_u8, const float* gt_f32, int B, int H, int W);

}  // namespace dpir
