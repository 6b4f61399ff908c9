// conv_plan.h: every rule of the 3x3 convolution dispatch, once.  Plain C++ (also compiled alone by a host compiler for the sanitizer walk).
#include "conv_plan.h"
#include <stdlib.h>
namespace dpir {

static bool env_on(const char* name) { const char* v = getenv(name); return !(v && atoi(v) == 0); }
static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }

const ConvKnobs& ConvKnobs::from_env() {
    static const ConvKnobs knobs = [] {
        ConvKnobs k;
        k.conv8 = env_on("DPIR_CONV8");
        k.conv9 = env_on("DPIR_CONV9");
        k.conv9_min_wg = env_int("DPIR_CONV9_MIN_WG", k.conv9_min_wg);
        k.conv11 = env_on("DPIR_CONV11");
        k.conv_up = env_on("DPIR_CONV_UP");
        k.split_below = env_int("DPIR_SPLIT_BELOW", k.split_below);
        k.split_target = env_int("DPIR_SPLIT_TARGET", k.split_target);
        k.fuse_small = env_on("DPIR_FUSE_SMALL");
        k.fuse_h1 = env_on("DPIR_FUSE_H1");
        k.emit_skip = env_int("DPIR_EMIT_SKIP", k.emit_skip);
        return k;
    }();
    return knobs;
}

static const size_t k4GiB = (size_t)1 << 32;      // range of a buffer descriptor

Conv3Geometry geometry(int H, int W) {
    Conv3Geometry g;
    if ((W & 3) || W < 8 || H < 8) return g;
    g.geo = W >= 32 ? 0 : (W >= 16 ? 1 : 2);
    g.tw = g.geo == 0 ? 32 : (g.geo == 1 ? 16 : 8);
    g.th = g.geo == 1 ? 16 : 8;
    g.ti = g.geo == 2 ? 4 : 1;
    g.tiles_x = (W + g.tw - 1) / g.tw;
    g.tiles_y = (H + g.th - 1) / g.th;
    g.stat_slots = g.tiles_x * g.tiles_y * ((g.tw * g.th) / 64);
    return g;
}

bool group_in_wave(int Cout, int wave_channels) { return Cout >= 32 && Cout % 32 == 0 && wave_channels % (Cout / 32) == 0; }

// ------------------------------------------------------------------------------------------ shapes each kernel is built for
bool conv8_shape_ok(int B, int C, int Cout, int H, int W) {
    return B > 0 && Cout >= 1 && Cout <= 16 && C % 32 == 0 && C >= 32 && C <= kConv8MaxC && H % 8 == 0 && W % 32 == 0 &&
           (size_t)C * H * W < ((size_t)1 << 30);      // one image's bytes fit the 32-bit range of a buffer descriptor
}

const char* conv9_refusal(int B, int Cin, int Cout, int H, int W, bool hop) {
    if (B <= 0 || Cin <= 0 || Cout <= 0) return "conv9: empty launch";
    if (H != W) return "conv9: whole-image tiles need a square image";
    if (H != 8) return "conv9: the whole-image tile is built for 8 x 8 layers only";
    if (Cin % 16) return "conv9: the input channels must be a multiple of 16";
    if (Cout % 32) return "conv9: the output channels must be a multiple of 32";
    if (hop && !group_in_wave(Cout, 32)) return "conv9: fused emission needs GroupNorm groups that do not straddle a 32-channel tile";
    if ((size_t)B * (Cin / 8) * H * W * 16 >= k4GiB) return "conv9: split activation plane exceeds the 4 GiB buffer-descriptor range";
    return nullptr;
}

bool conv11_shape_ok(int Cin, int Cout, int H, int W) {
    return Cin > 0 && Cin % 32 == 0 && Cout > 0 && Cout % 128 == 0 && W > 0 && W % 32 == 0 && H > 0 && H % 8 == 0;
}
// the waiting set -- the tiles of one (image, co-block), consecutive ids -- takes at most half of the resident workgroups, so that it is
// resident together with room to spare
bool conv11_hop_ok(int Cout, int H, int W, int capacity) {
    if (Cout <= 0 || Cout % 128 || W <= 0 || W % 32 || H <= 0 || H % 8 || !group_in_wave(Cout, 64)) return false;
    return (W / 32) * (H / 8) <= capacity / 2;
}

long long conv_up_workgroups(int B, int Cout, int Hs, int Ws) { return (long long)B * (Ws / 32) * (Hs / 8) * ((Cout + 63) / 64) * 2; }

const char* conv_up_refusal(int B, int Cin, int Cout, int Hs, int Ws, bool hop, int min_wg_hop, int capacity) {
    if (B <= 0 || Cin <= 0 || Cout <= 0 || Hs <= 0 || Ws <= 0) return "conv_up: bad shape";
    if (Ws & 31) return "conv_up: the source width must be a multiple of 32";
    if (Hs & 7) return "conv_up: the source height must be a multiple of 8";
    if (Cin & 15) return "conv_up: the input channels must be a multiple of 16";
    if (Cout & 31) return "conv_up: the output channels must be a multiple of 32";
    const size_t HW = (size_t)Hs * Ws;
    if ((size_t)B * (Cin / 8) * HW * 16 >= k4GiB || (size_t)Cout * HW * 16 >= k4GiB || conv_up_workgroups(B, Cout, Hs, Ws) >= ((long long)1 << 31))
        return "conv_up: operand planes or one image's output exceed the 4 GiB buffer-descriptor range";
    if (hop) {
        if ((Cout & 63) || !group_in_wave(Cout, 32)) return "conv_up: GroupNorm groups of the hop must not straddle a wave's 32 channels (Cout 128, 256, 512 or 1024)";
        const int wait_set = 2 * (Ws / 32) * (Hs / 8);
        if (wait_set > capacity / 2) return "conv_up: the hop's wait set exceeds half of the resident workgroups";
        if (conv_up_workgroups(B, Cout, Hs, Ws) < min_wg_hop) return "conv_up: too few workgroups for the hop";
        if ((size_t)B * (Cout / 8) * HW * 4 * 16 >= k4GiB) return "conv_up: the emitted planes exceed the 4 GiB range";
    }
    return nullptr;
}

// conv7's hop: whole K (kHopMinWg workgroups), 8 x 32 tiles inside the image, full 128-channel blocks, and the workgroups of one (image,
// co-block) -- the set that waits for one another, consecutive in dispatch order -- at most half of the resident ones
bool conv7_hop_ok(int B, int Cout, int H, int W, int capacity) {
    if (geometry(H, W).geo != 0 || (W & 31) || (H & 7) || Cout <= 0 || (Cout & 127) || !group_in_wave(Cout, 64)) return false;
    const long long tiles = (long long)(W / 32) * (H / 8);
    return tiles <= capacity / 2 && tiles * (Cout / 128) * B >= kHopMinWg;
}

// ------------------------------------------------------------------------------------------ one convolution
static Conv3Plan refuse(const char* why, int geo = -1) { Conv3Plan p; p.refusal = why; p.geo = geo; return p; }

Conv3Plan plan_conv67(const Conv3Query& q, const ConvKnobs& knobs, const DeviceCaps& caps) {
    const Conv3Geometry g = geometry(q.H, q.W);
    if (!g.ok()) return refuse("conv6: shape not tiled");
    Conv3Plan p;
    p.geo = g.geo;
    const int chunks = (q.Cin + 15) / 16;
    const long long blocks = (long long)g.pixel_tiles(q.B) * ((q.Cout + 127) / 128);
    if (blocks < 1 || chunks < 1) return refuse("conv6: empty launch", g.geo);
    // split-K when the launch cannot give every CU ONE workgroup (low-resolution layers); deterministic slabs.  Every slice writes a full fp32
    // slab, so splitting trades co-resident workgroups for slab traffic (ConvKnobs has the measurements behind the two constants).
    int S = 1;
    if (q.slab && blocks < knobs.split_below) {
        S = (int)((knobs.split_target + blocks - 1) / blocks);
        if (S > chunks / 2) S = chunks / 2;
        if (S > 16) S = 16;
        if (S < 1) S = 1;
        if ((size_t)S * q.B * q.Cout * q.H * q.W > q.slab_floats) S = 1;
    }
    p.chunks_per_split = (chunks + S - 1) / S;
    S = (chunks + p.chunks_per_split - 1) / p.chunks_per_split;      // no empty slice: every workgroup owns at least one chunk
    p.ksplit = S;
    p.workgroups = blocks * S;
    if (q.hop) {
        if (S != 1 || !conv7_hop_ok(q.B, q.Cout, q.H, q.W, caps.conv7) || q.has_res || q.out_scale_dev)
            return refuse("conv6: this launch cannot emit the next convolution's planes", g.geo);
        p.kernel = CK_CONV7; p.hop = true;
        return p;
    }
    // conv7 (same results bit for bit) is the 3x3 kernel; conv6 keeps the two launch classes of the 8 x 32 geometry it is measurably faster at
    // (profiles/r04/conv7x_check.log): split-K launches (x1.07) and a last co-block with at most 64 live channels (x1.05) -- unless the whole
    // launch has at most 32 output channels (the 128 -> 6 output convolution), which conv7's NARROW variant spreads over all four waves.
    const bool idle_half = (q.Cout & 127) != 0 && (q.Cout & 127) <= 64 && q.Cout > 32;
    const bool use6 = q.force_kernel == CK_CONV6 || (q.force_kernel != CK_CONV7 && g.geo == 0 && (S > 1 || idle_half));
    if (use6 && g.geo != 0) return refuse("conv6 is built for the 8 x 32 geometry only (conv7 has the 16 x 16 and 8 x 8 ones)", g.geo);
    p.kernel = use6 ? CK_CONV6 : (conv7_narrow(g.geo, q.Cout) ? CK_CONV7_NARROW : CK_CONV7);
    if (S > 1) p.stat_kind = q.defer ? ST_PENDING : (q.stat_plane ? ST_PLANE : ST_NONE);
    else if (q.stat_slots) { p.stat_kind = ST_SLOTS; p.stat_slots = g.stat_slots; }
    return p;
}

Conv3Plan plan_conv3(const Conv3Query& q, const ConvKnobs& knobs, const DeviceCaps& caps) {
    const Conv3Geometry g = geometry(q.H, q.W);
    const bool forced = q.force_kernel != 0;
    Conv3Plan p;
    // the output layer (128 -> 6): GroupNorm / SiLU / split happen in the convolution's own LDS fill; gradient mode keeps the planes route
    // (the backward pass reads the planes)
    if (!forced && knobs.conv8 && q.w8 && q.conv8_source && !q.grad && !q.hop && !q.has_res && conv8_shape_ok(q.B, q.Cin, q.Cout, q.H, q.W)) {
        p.kernel = CK_CONV8; p.geo = 0;
        p.workgroups = (long long)(q.W / 32) * (q.H / 8) * q.B;
        return p;
    }
    if (!q.w16 || !g.ok()) {        // f32 engine, or a shape the f16 tilings refuse (W % 4, images below 8 x 8)
        if (q.hop) return refuse("conv: fused emission was requested for a launch that is not on the f16 3x3 path");
        if (forced) return refuse("conv: a kernel cannot be forced here (f32 engine or a shape the f16 path refuses)");
        return p;
    }
    const bool f16_infer = !q.grad && q.precision != 0;
    // 8 x 8: one workgroup per (image, 32 output channels), whole K -- no slabs, nothing pending.  Below the threshold the split-K route,
    // tuned for small batches, stays.
    if (q.force_kernel == CK_CONV9 || (!forced && knobs.conv9 && (long long)q.B * (q.Cout / 32) >= knobs.conv9_min_wg)) {
        const char* why = conv9_refusal(q.B, q.Cin, q.Cout, q.H, q.W, q.hop);
        if (f16_infer && !why) {
            p.kernel = CK_CONV9; p.hop = q.hop; p.geo = g.geo;
            p.workgroups = (long long)q.B * (q.Cout / 32);
            if (!q.hop && q.stat_plane) p.stat_kind = ST_PLANE;
            return p;
        }
        if (forced) return refuse(why ? why : "conv9: an f16 inference forward only");
    }
    // conv11: conv7's 8 x 32 tile with the 16x16x32 MFMA (x0.93 of conv7's time per layer, profiles/conv11/README.md), f16x3 and whole K only:
    // where plan_conv67 would not split (the hop: kHopMinWg, and an image's tiles in half of conv11's own resident workgroups)
    if (q.force_kernel == CK_CONV11 || (!forced && knobs.conv11)) {
        const long long wgs = (long long)(q.W / 32) * (q.H / 8) * q.B * (q.Cout / 128);
        const bool shape = f16_infer && q.precision == 1 && q.w11 && conv11_shape_ok(q.Cin, q.Cout, q.H, q.W);
        const bool enough = forced || wgs >= (q.hop ? kHopMinWg : knobs.split_below);
        if (shape && enough && (!q.hop || conv11_hop_ok(q.Cout, q.H, q.W, caps.conv11))) {
            p.kernel = CK_CONV11; p.hop = q.hop; p.geo = 0; p.workgroups = wgs;
            if (!q.hop && q.stat_slots) { p.stat_kind = ST_SLOTS; p.stat_slots = g.stat_slots; }
            return p;
        }
        if (forced) return refuse("conv11: f16x3 inference, Cin % 32 == 0, Cout % 128 == 0, 8 x 32 tiles inside the image; the hop: groups inside a wave and an image's tiles resident");
    }
    return plan_conv67(q, knobs, caps);
}

// ------------------------------------------------------------------------------------------ one ResBlock
ResblockPlan plan_resblock(const ResblockQuery& q, const ConvKnobs& knobs, const DeviceCaps& caps) {
    ResblockPlan rp;
    const int Ho = q.mode == 1 ? q.H * 2 : (q.mode == 2 ? q.H / 2 : q.H), Wo = q.mode == 1 ? q.W * 2 : (q.mode == 2 ? q.W / 2 : q.W);
    const Conv3Geometry g = geometry(Ho, Wo);
    const bool stats = g.stat_slots > 0 && q.Cout % 32 == 0;
    const bool hops = q.hop_allowed && knobs.fuse_h1 && !q.grad && q.precision != 0;
    const bool arena = hops && q.arena_words_left > 0;
    auto arena_room = [&](int counters) { return (size_t)q.B * 64 + (size_t)q.B * counters <= q.arena_words_left; };
    Conv3Query c1, c2;
    c1.B = c2.B = q.B; c1.H = c2.H = Ho; c1.W = c2.W = Wo; c1.Cout = c2.Cout = c2.Cin = q.Cout; c1.Cin = q.Cin;
    c1.precision = c2.precision = q.precision; c1.grad = c2.grad = q.grad;
    c1.w16 = q.conv1_w16; c1.w11 = q.conv1_w11; c2.w16 = q.conv2_w16; c2.w11 = q.conv2_w11;
    c1.slab = c2.slab = q.slab; c1.slab_floats = c2.slab_floats = q.slab_floats;
    c1.defer = c2.defer = knobs.fuse_small;
    c1.stat_slots = c1.stat_plane = c2.stat_slots = c2.stat_plane = stats;
    c2.has_res = true;

    // conv1 of an up-sampling ResBlock as four 2x2 phase convolutions of the source image: an f16 precision, no tape, the phase pack loaded,
    // the shape supported, and enough workgroups that plan_conv67 would not have split K.  Everything else -- source widths below 32,
    // gradient mode, f32 -- keeps the route through the up-sampled planes.
    rp.up = knobs.conv_up && q.mode == 1 && !q.grad && q.precision != 0 && q.conv1_wup && !q.concat && q.Cin == q.gn1_c &&
            !conv_up_refusal(q.B, q.Cin, q.Cout, q.H, q.W, false, 0, 0) && conv_up_workgroups(q.B, q.Cout, q.H, q.W) >= knobs.split_below;
    if (rp.up) {
        const bool hop = arena && q.gn2_c == q.Cout && q.conv2_w16 && g.ok() && !conv_up_refusal(q.B, q.Cin, q.Cout, q.H, q.W, true, kHopMinWg, caps.conv_up) &&
                         arena_room(q.Cout / 64);
        rp.conv1.kernel = CK_CONV_UP; rp.conv1.hop = hop; rp.conv1.geo = 0;
        rp.conv1.workgroups = conv_up_workgroups(q.B, q.Cout, q.H, q.W);
        if (hop) { rp.hop = HOP_CONV_UP; rp.arena_counters = q.Cout / 64; }
        else { rp.conv1.stat_kind = ST_SLOTS; rp.conv1.stat_slots = g.stat_slots; }
        rp.conv2 = plan_conv3(c2, knobs, caps);
        return rp;
    }
    // ResBlock with a 1x1 skip projection at a resolution the fused low-resolution prologue does not take: ONE pass over the (concat) input
    // feeds both the skip projection and in_layers -- conv5 emits conv1's split operand planes
    rp.skip_emit = (knobs.emit_skip == 2 || (knobs.emit_skip == 1 && q.Cout <= 128)) && q.has_skip && q.mode == 0 && q.conv1_w16 && q.skip_w16 && g.ok() &&
                   q.conv5_ok && q.Cin % 16 == 0 && q.Cin <= kConv5EmitMaxC && (Ho * Wo) % 256 == 0 &&
                   (size_t)q.B * (2 * ((q.Cin + 15) / 16)) * Ho * Wo * 16 < k4GiB && !(knobs.fuse_small && q.small_prologue);
    // the hop through the arena (conv7's rule; conv1 then runs on conv11 where plan_conv3 says so)
    const bool hop_arena = arena && q.conv1_w16 && q.conv2_w16 && q.gn2_c == q.Cout && conv7_hop_ok(q.B, q.Cout, Ho, Wo, caps.conv7) &&
                           arena_room(q.Cout / 128) && (size_t)q.B * (2 * ((q.Cout + 15) / 16)) * Ho * Wo * 16 < k4GiB;
    // 8 x 8 with both convolutions on conv9: a GroupNorm group of h1 is whole inside one workgroup of conv1, which writes conv2's planes
    // itself -- nothing of the arena is used
    c1.hop = true;
    const bool hop9 = !rp.skip_emit && hops && q.gn2_c == q.Cout && plan_conv3(c1, knobs, caps).kernel == CK_CONV9 &&
                      plan_conv3(c2, knobs, caps).kernel == CK_CONV9;
    rp.hop = hop9 ? HOP_CONV9 : (hop_arena ? HOP_ARENA : HOP_NONE);
    if (rp.hop == HOP_ARENA) rp.arena_counters = q.Cout / 128;
    c1.hop = rp.hop != HOP_NONE;
    if (c1.hop) { c1.slab = false; c1.slab_floats = 0; c1.stat_slots = c1.stat_plane = false; }
    rp.conv1 = plan_conv3(c1, knobs, caps);
    rp.conv2 = plan_conv3(c2, knobs, caps);
    return rp;
}

}  // namespace dpir
