// FID Inception-v3 (pytorch-fid's FIDInceptionA/C/E_1/E_2 network, `pool3` output): 94 BasicConv layers (convolution + folded eval-mode
// BatchNorm + ReLU), the three 3x3 pools and the final 8 x 8 mean -> 2048 features per image.  Everything is in fid.hip: the convolutions
// are fid_conv (exact-fp32 MFMA implicit GEMM, general kernel / stride / padding), whatever the engine's precision mode.
#pragma once
#include "common.h"
#include <string>
#include <vector>

struct dpir_engine;

namespace dpir {

constexpr int kFidConvs = 94, kFidTaps = 14, kFidFeat = 2048, kFidSide = 299;
constexpr int kFidChunk = 16;                      // images per pass through the arena (about 16 MB of activations per image)
constexpr int kFidFlush = 64;                      // products an MFMA accumulator takes before it is added to the float64 running sum
constexpr int kFidBufs = 5;                        // X, Y (block input / output, ping-pong), T0, T1 (branch chains), T2 (the s1 pools)

struct FidLayer {
    std::string name; int cin, cout, kh, kw, stride, ph, pw;
    int hin = 0, win = 0, ho = 0, wo = 0;          // fixed by the network (the entry is always 299 x 299)
    int kp = 0, coutp = 0;                         // K = cin kh kw rounded up to the K chunk, Cout rounded up to the co tile
    float* w = nullptr; float* bias = nullptr; int2* ktab = nullptr;
};
enum FidOpKind { FID_CONV, FID_MAXPOOL_S2, FID_AVG3, FID_MAX3, FID_TAP };
struct FidOp {
    int kind, layer;                               // layer: FID_CONV only
    int src, src_c0, src_ct, dst, dst_c0, dst_ct;  // buffer ids, first channel and channel count of the whole tensor in that buffer
    int c, hin, win, ho, wo;                       // pools / taps: channels and sizes
    int tap;                                       // FID_TAP: tap number; its tensor is [c, hin, win] in buffer src
};

struct FidState {
    bool loaded = false;
    std::vector<FidLayer> layers;
    std::vector<FidOp> ops;
    size_t buf_floats[kFidBufs] = {};              // per image
    int out_buf = 0;                               // buffer holding Mixed_7c's output
    std::vector<void*> weight_allocs;
    float* buf[kFidBufs] = {}; int buf_imgs = 0;   // the arena: buf_floats[i] * buf_imgs floats each
    float* feat = nullptr; size_t feat_cap = 0;    // [B, 2048] of the last call
    float* tap[kFidTaps - 1] = {}; size_t tap_cap[kFidTaps - 1] = {}; size_t tap_numel[kFidTaps] = {};
    int tap_c[kFidTaps - 1] = {}, tap_hw[kFidTaps - 1] = {};
};

Status fid_load(dpir_engine* e, const dpir_tensor* weights, int n);
void fid_free(dpir_engine* e);
// features -> the state's feat [B, 2048] (device); asynchronous on the engine stream.  Exactly one of img_u8 (NHWC) / img_f32 (NCHW in [0,1]).
Status fid_run(dpir_engine* e, const uint8_t* img_u8, const float* img_f32, int B, int H, int W);

}  // namespace dpir
