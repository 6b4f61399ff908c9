// The planner of the 3x3 convolution routes: which kernel a layer runs on, with which tiling, split-K factor and statistics, and which
// fused hop a ResBlock takes.  Fwd (unet.hip), launch_conv6 / launch_conv7, the launchers' shape checks and the probes (dbg_conv.hip) all ask
// here, so a rule is written once.  Plain C++: no HIP call, no device query (capacities come in as DeviceCaps) and one getenv site
// (ConvKnobs::from_env), so the whole policy runs -- and is tested -- on a machine without a GPU.
#pragma once
#include <cstddef>
namespace dpir {

// A fused hop (conv1's epilogue writes conv2's operand planes) is taken when conv1's launch has at least this many workgroups: the rule
// launch_conv6 used for "runs whole K" when the hop was built (rounds 2-4).  DPIR_SPLIT_BELOW moved the plain launches to 256 later.
constexpr int kHopMinWg = 384;
// Workgroups (B x Cout / 32) from which conv9 is preferred to the split-K route (profiles/conv9/README.md has the per-layer table).
constexpr int kConv9MinWg = 128;
constexpr int kConv5EmitMaxC = 384;     // channels of the GroupNorm table conv5's plane-emitting variant stages in LDS (a capacity, not a threshold)
constexpr int kConv8MaxC = 256;         // channels of the GroupNorm table conv8 stages in LDS

// Every A/B switch of the dispatch.  Defaults are the measured settings; tests and tools/ compare routes by setting them in the environment.
struct ConvKnobs {
    bool conv8 = true;          // DPIR_CONV8=0: the output layer takes the planes route
    bool conv9 = true;          // DPIR_CONV9=0: 8 x 8 layers keep conv6 / conv7
    int conv9_min_wg = kConv9MinWg;   // DPIR_CONV9_MIN_WG
    bool conv11 = true;         // DPIR_CONV11=0: whole-K 8 x 32 layers keep conv7
    bool conv_up = true;        // DPIR_CONV_UP=0: up-sampling ResBlocks convolve the up-sampled planes
    // split-K when a launch has fewer than split_below workgroups, up to about split_target of them.  Rounds 2-4 used 384 / 512; measured in
    // round 5 (profiles/r05/split_rule_layer_roofline_and_forward_ab.log, five settings interleaved in one call): 256 / 256 is faster on every
    // affected shape -- 512 -> 512 @ 32^2 215 -> 185 us, 256 -> 256 @ 32^2 65 -> 60, 512 -> 512 @ 16^2 64 -> 58.5, 1024 -> 512 @ 16^2 108 -> 99 -- and
    // 18.88 -> 18.73 ms per forward; larger targets (768, 1024) lose 0.7 ms.
    int split_below = 256;      // DPIR_SPLIT_BELOW (conv6 / conv7, conv11 and conv_up all follow it)
    int split_target = 256;     // DPIR_SPLIT_TARGET
    bool fuse_small = true;     // DPIR_FUSE_SMALL=0: no fused low-resolution prologue, split-K combines are never left pending
    bool fuse_h1 = true;        // DPIR_FUSE_H1=0: no fused hop of any kind
    // conv5 emits conv1's operand planes in ResBlocks with a 1x1 skip projection: 0 never, 1 when the projection has ONE 128-channel output
    // block (each input row is then read exactly once; with two blocks only one of them emits and the other re-reads -- measured slower on
    // the ImageNet-256 topology, profiles/r03), 2 always
    int emit_skip = 1;          // DPIR_EMIT_SKIP
    static const ConvKnobs& from_env();     // the environment, read once per process
};

// Resident workgroups (CUs x occupancy) of the three kernels whose hop waits across workgroups; 0 = unknown (no hop)
struct DeviceCaps { int conv7 = 0, conv11 = 0, conv_up = 0; };

// The three tilings of conv6 / conv7 (conv11 and conv8 share the first): geo 0 = 8 x 32 pixels, 1 = 16 x 16, 2 = four images x 8 x 8
struct Conv3Geometry {
    int geo = -1;               // -1: not tiled (W % 4, or an image below 8 x 8): the fp32 kernel
    int tw = 0, th = 0, ti = 0; // tile width, height, images per tile
    int tiles_x = 0, tiles_y = 0;
    int stat_slots = 0;         // epilogue statistics records per (image, channel) plane: one per 64 stored pixels of every tile
    bool ok() const { return geo >= 0; }
    int pixel_tiles(int B) const { return tiles_x * tiles_y * ((B + ti - 1) / ti); }
};
Conv3Geometry geometry(int H, int W);

// A GroupNorm group (Cout / 32 channels) must lie inside the channels ONE wave owns, because the emitting epilogues fold a group's sums
// inside a wave: 64 channels for conv7 / conv11, 32 for conv9 / conv_up
bool group_in_wave(int Cout, int wave_channels);
// conv7's NARROW variant spreads a launch of at most 32 output channels (the 128 -> 6 output layer) over all four waves
inline bool conv7_narrow(int geo, int Cout) { return geo == 0 && Cout <= 32; }

// Shapes each kernel is built for (the launchers validate their arguments with the same functions)
bool conv8_shape_ok(int B, int C, int Cout, int H, int W);
const char* conv9_refusal(int B, int Cin, int Cout, int H, int W, bool hop);        // null = supported
bool conv11_shape_ok(int Cin, int Cout, int H, int W);
bool conv11_hop_ok(int Cout, int H, int W, int capacity);
long long conv_up_workgroups(int B, int Cout, int Hs, int Ws);                        // source tiles x 64-channel blocks x 2 row parities x images
const char* conv_up_refusal(int B, int Cin, int Cout, int Hs, int Ws, bool hop, int min_wg_hop, int capacity);   // null = supported
bool conv7_hop_ok(int B, int Cout, int H, int W, int capacity);

enum ConvKernel { CK_FP32 = 0, CK_CONV5 = 5, CK_CONV6 = 6, CK_CONV7 = 7, CK_CONV8 = 8, CK_CONV9 = 9, CK_CONV11 = 11, CK_CONV_UP = 12,
                  CK_CONV7_NARROW = 17, CK_RESOLVE = 60 };
enum StatKind { ST_NONE = 0, ST_SLOTS = 1, ST_PLANE = 2, ST_PENDING = 3 };    // none / epilogue slots / fp64 per plane / split-K combine left to the consumer
enum HopKind { HOP_NONE = 0, HOP_ARENA = 1, HOP_CONV9 = 2, HOP_CONV_UP = 3 }; // conv7 / conv11 through the arena, conv9 inside one workgroup, conv_up through the arena

struct Conv3Query {
    int B = 0, Cin = 0, Cout = 0, H = 0, W = 0;     // H, W: the output resolution
    int precision = 1;          // 0 f32, 1 f16x3, 2 f16x1
    bool grad = false;          // the forward records a tape
    bool w16 = false, w8 = false, w11 = false;      // weight packs the layer has
    bool conv8_source = false;  // GroupNorm table prologue on ONE source tensor at the output resolution (what conv8 fuses)
    bool slab = false; size_t slab_floats = 0;      // a split-K slab buffer is offered, its capacity
    bool defer = false;         // the caller can leave a split-K combine pending
    bool hop = false;           // the launch emits the next convolution's planes instead of its output
    bool has_res = false, out_scale_dev = false;
    bool stat_slots = false, stat_plane = false;    // statistics buffers offered
    int force_kernel = 0;       // tests: CK_CONV6 / CK_CONV7, or CK_CONV9 / CK_CONV11 without their workgroup thresholds and switches
};
struct Conv3Plan {
    int kernel = CK_FP32;
    bool hop = false;
    int geo = -1;
    long long workgroups = 0;   // 0 for the fp32 kernel (conv.hip tiles it itself)
    int ksplit = 1, chunks_per_split = 0;
    int stat_kind = ST_NONE, stat_slots = 0;
    const char* refusal = nullptr;      // the request cannot run (a hop or a forced kernel on a launch that has none)
};
// conv6 / conv7 on prepared planes: the tiling, the split-K rule and the choice between the two kernels (what launch_conv6 executes)
Conv3Plan plan_conv67(const Conv3Query& q, const ConvKnobs& knobs, const DeviceCaps& caps);
// the whole choice: conv8, the fp32 kernel, conv9, conv11, then plan_conv67
Conv3Plan plan_conv3(const Conv3Query& q, const ConvKnobs& knobs, const DeviceCaps& caps);

struct ResblockQuery {
    int B = 0, Cin = 0, Cout = 0, H = 0, W = 0;     // H, W: the INPUT resolution
    int mode = 0;               // 0 plain, 1 up, 2 down
    bool concat = false, has_skip = false;
    int gn1_c = 0, gn2_c = 0;
    int precision = 1; bool grad = false;
    bool hop_allowed = false;   // engine state: no time-out replay in progress (the knob, the precision and the tape are checked by the planner)
    size_t arena_words_left = 0;        // 8-byte words left in the hop arena (0: no arena)
    bool conv1_w16 = false, conv1_w11 = false, conv1_wup = false, conv2_w16 = false, conv2_w11 = false, skip_w16 = false;
    bool small_prologue = false;        // gn_act_small takes conv1's input (mode 0)
    bool conv5_ok = false;              // conv5's large tile takes the skip projection
    bool slab = false; size_t slab_floats = 0;
};
struct ResblockPlan {
    bool up = false;            // conv1 as four 2x2 phase convolutions of the source image (conv_up)
    bool skip_emit = false;     // conv5 runs the skip projection and emits conv1's planes
    int hop = HOP_NONE;
    int arena_counters = 0;     // arrival counters per image the hop takes from the arena
    Conv3Plan conv1, conv2;
};
ResblockPlan plan_resblock(const ResblockQuery& q, const ConvKnobs& knobs, const DeviceCaps& caps);

}  // namespace dpir
