"""The dispatch of the 3x3 convolution layers, stated in Python from the documents that describe it -- DESIGN.md (section 3.1 and the per-layer
test description), profiles/conv9/README.md, profiles/conv11/README.md, profiles/conv_up/README.md and INTEGRATION.md's switch table -- not from
csrc/conv_plan.cpp, which the tests hold to this statement.

Kernels: 0 the fp32 kernel, 6 conv6, 7 conv7, 17 conv7's narrow variant, 8 conv8, 9 conv9, 11 conv11, 12 conv_up.
Statistics: 0 none, 1 epilogue slots, 2 fp64 per plane, 3 left pending for the consumer's fused prologue.
Hops: 0 none, 1 conv7 / conv11 through the arena, 2 conv9 inside one workgroup, 3 conv_up through the arena."""
HOP_MIN_WG = 384            # "whole K" for the hops (the rule of rounds 2-4)
KNOBS = dict(conv8=1, conv9=1, conv9_min_wg=128, conv11=1, conv_up=1, split_below=256, split_target=256, fuse_small=1, fuse_h1=1, emit_skip=1)
GiB4 = 1 << 32
TILES = ((32, 8, 1), (16, 16, 1), (8, 8, 4))        # tile width, height, images per tile of the three geometries


def cdiv(a, b):
    return -(-a // b)


def geo(H, W):
    if W % 4 or W < 8 or H < 8:
        return -1
    return 0 if W >= 32 else (1 if W >= 16 else 2)


def stat_slots(H, W):
    g = geo(H, W)
    if g < 0:
        return 0
    tw, th, _ = TILES[g]
    return cdiv(W, tw) * cdiv(H, th) * (tw * th // 64)


def group_in_wave(cout, wave_channels):
    """A GroupNorm group (cout / 32 channels) lies inside the channels one wave owns."""
    return cout >= 32 and cout % 32 == 0 and wave_channels % (cout // 32) == 0


def hop7_ok(B, cout, H, W, cap):
    """conv7's hop: 8 x 32 tiles inside the image, full 128-channel blocks, groups inside a wave's 64 channels, an image's tiles in half of
    the resident workgroups, and at least 384 workgroups."""
    if geo(H, W) != 0 or W % 32 or H % 8 or cout <= 0 or cout % 128 or not group_in_wave(cout, 64):
        return False
    tiles = (W // 32) * (H // 8)
    return tiles <= cap // 2 and tiles * (cout // 128) * B >= HOP_MIN_WG


def conv67(q, knobs=KNOBS, caps=(512, 512, 512)):
    """launch_conv6's rule: tiles of 8x32 / 16x16 / 4 images x 8x8; split-K only with a slab buffer and fewer than split_below workgroups, up to
    split_target of them, at most chunks / 2 and 16 slabs, no empty slab, and only if the slabs fit; conv6 only in the 8x32 geometry, for
    split-K launches and for a last 128-channel block with at most 64 live channels (unless the whole launch has at most 32 output channels:
    conv7's narrow variant)."""
    B, cin, cout, H, W = q["B"], q["Cin"], q["Cout"], q["H"], q["W"]
    g = geo(H, W)
    if g < 0:
        return dict(refused=1)
    tw, th, ti = TILES[g]
    blocks = cdiv(W, tw) * cdiv(H, th) * cdiv(B, ti) * cdiv(cout, 128)
    chunks = cdiv(cin, 16)
    S = 1
    if q["slab_floats"] > 0 and blocks < knobs["split_below"]:
        S = max(1, min(cdiv(knobs["split_target"], blocks), chunks // 2, 16))
        if S * B * cout * H * W > q["slab_floats"]:
            S = 1
    per = cdiv(chunks, S)
    S = cdiv(chunks, per)
    out = dict(refused=0, hop=0, geo=g, ksplit=S, chunks_per_split=per, workgroups=blocks * S, stat_kind=0, stat_slots=0)
    if q["hop"]:
        if S != 1 or not hop7_ok(B, cout, H, W, caps[0]) or q["has_res"]:
            return dict(refused=1)
        return dict(out, kernel=7, hop=1)
    idle_half = cout % 128 != 0 and cout % 128 <= 64 and cout > 32
    force = q.get("force_kernel", 0)
    use6 = force == 6 or (force != 7 and g == 0 and (S > 1 or idle_half))
    if use6 and g != 0:
        return dict(refused=1)
    out["kernel"] = 6 if use6 else (17 if g == 0 and cout <= 32 else 7)
    if S > 1:
        out["stat_kind"] = 3 if q["defer"] else (2 if q["stats"] else 0)
    elif q["stats"]:
        out["stat_kind"], out["stat_slots"] = 1, stat_slots(H, W)
    return out


def conv8_ok(B, C, cout, H, W):
    return B > 0 and 1 <= cout <= 16 and C % 32 == 0 and 32 <= C <= 256 and H % 8 == 0 and W % 32 == 0 and C * H * W < (1 << 30)


def conv9_ok(B, cin, cout, H, W, hop):
    return (B > 0 and H == W == 8 and cin > 0 and cin % 16 == 0 and cout > 0 and cout % 32 == 0 and (not hop or group_in_wave(cout, 32)) and
            B * (cin // 8) * H * W * 16 < GiB4)


def plan(q, knobs=KNOBS, caps=(512, 512, 512)):
    """One 3x3 layer.  q: B, Cin, Cout, H, W (output resolution), precision (0 f32, 1 f16x3, 2 f16x1), grad, w16 / w8 / w11 (weight packs),
    conv8_source, slab_floats (0: no slab), defer, hop, has_res, stats."""
    B, cin, cout, H, W = q["B"], q["Cin"], q["Cout"], q["H"], q["W"]
    none = dict(refused=0, hop=0, ksplit=1, stat_kind=0, stat_slots=0)
    # the output layer: conv8 fuses the GroupNorm table prologue; not in gradient mode
    if (knobs["conv8"] and q["w8"] and q["conv8_source"] and not q["grad"] and not q["hop"] and not q["has_res"] and conv8_ok(B, cin, cout, H, W)):
        return dict(none, kernel=8, workgroups=(W // 32) * (H // 8) * B)
    if not q["w16"] or geo(H, W) < 0:       # f32 engine, W % 4 != 0, images below 8 x 8: the fp32 kernel (which cannot hop)
        return dict(refused=1) if q["hop"] else dict(none, kernel=0, workgroups=0)
    infer16 = not q["grad"] and q["precision"] != 0
    # conv9 (profiles/conv9): 8 x 8, outside gradient mode, the f16 precisions, from 128 workgroups B x Cout / 32
    if knobs["conv9"] and infer16 and conv9_ok(B, cin, cout, H, W, q["hop"]) and B * (cout // 32) >= knobs["conv9_min_wg"]:
        return dict(none, kernel=9, hop=int(q["hop"]), workgroups=B * (cout // 32), stat_kind=2 if q["stats"] and not q["hop"] else 0)
    # conv11 (profiles/conv11): f16x3, no tape, pack loaded, Cin % 32 == 0, Cout % 128 == 0, W % 32 == 0, H % 8 == 0, whole K by launch_conv6's rule
    # (256 workgroups; the hop 384, groups inside a wave, an image's tiles in half of conv11's resident workgroups)
    if (knobs["conv11"] and infer16 and q["precision"] == 1 and q["w11"] and cin > 0 and cin % 32 == 0 and cout > 0 and cout % 128 == 0 and
            W % 32 == 0 and H % 8 == 0):
        wgs = (W // 32) * (H // 8) * B * (cout // 128)
        if q["hop"]:
            ok = wgs >= HOP_MIN_WG and group_in_wave(cout, 64) and (W // 32) * (H // 8) <= caps[1] // 2
        else:
            ok = wgs >= knobs["split_below"]
        if ok:
            slots = q["stats"] and not q["hop"]
            return dict(none, kernel=11, hop=int(q["hop"]), workgroups=wgs, stat_kind=1 if slots else 0, stat_slots=stat_slots(H, W) if slots else 0)
    return conv67(q, knobs, caps)


def expected(prec, shape, route=0, split=0):
    """(path, ksplit) of the per-layer probe dpir_debug_conv3_layer (conv9 / conv11 / conv8 off): the fp32 kernel, conv6 or conv7."""
    B, ca, cb, cout, H, W = shape
    if prec == "f32" or geo(H, W) < 0:
        return 0, 0
    p = conv67(dict(B=B, Cin=ca + cb, Cout=cout, H=H, W=W, slab_floats=16 * B * cout * H * W if split else 0, hop=0, has_res=0, defer=0, stats=0,
                    force_kernel=route))
    return (6 if p["kernel"] == 6 else 7), p["ksplit"]


# ---------------------------------------------------------------------------------------------------- ResBlocks
def gn_small_ok(C, Hs, Ws):
    """gn_act_small (the fused low-resolution prologue) takes a source of C channels at Hs x Ws"""
    return C > 0 and C % 32 == 0 and C // 32 <= 64 and (Hs * Ws) % 4 == 0 and Hs * Ws <= 1024 and (C // 32) * Hs * Ws <= 49152


def conv5_ok(B, cout, H, W):
    return (H * W) % 4 == 0 and cdiv(B * H * W, 256) * cdiv(cout, 128) >= 32


def conv_up_ok(B, cin, cout, Hs, Ws):
    return B > 0 and Ws % 32 == 0 and Hs % 8 == 0 and cin % 16 == 0 and cout % 32 == 0 and B * (cin // 8) * Hs * Ws * 16 < GiB4 and cout * Hs * Ws * 16 < GiB4


def resblock(q, knobs=KNOBS, caps=(512, 512, 512)):
    """One ResBlock.  q: B, Cin, Cout, H, W (INPUT resolution), mode (0 plain, 1 up, 2 down), concat, precision, grad, hop_allowed,
    arena_words_left, slab_floats.  A 1x1 skip projection when Cin != Cout.  -> up, skip_emit, hop, conv1 / conv2 plans."""
    B, cin, cout, H, W, mode = q["B"], q["Cin"], q["Cout"], q["H"], q["W"], q["mode"]
    Ho, Wo = (2 * H, 2 * W) if mode == 1 else ((H // 2, W // 2) if mode == 2 else (H, W))
    f16 = q["precision"] != 0
    stats = stat_slots(Ho, Wo) > 0 and cout % 32 == 0
    arena = q["hop_allowed"] and knobs["fuse_h1"] and q["arena_words_left"] > 0
    room = lambda counters: B * 64 + B * counters <= q["arena_words_left"]
    base = dict(B=B, H=Ho, W=Wo, Cout=cout, precision=q["precision"], grad=q["grad"], w16=f16, w8=0, conv8_source=0, slab_floats=q["slab_floats"],
                defer=knobs["fuse_small"], stats=stats, hop=0, has_res=0)
    w11 = lambda ci: q["precision"] == 1 and ci % 32 == 0 and cout % 128 == 0
    c1, c2 = dict(base, Cin=cin, w11=w11(cin)), dict(base, Cin=cout, w11=w11(cout), has_res=1)
    # conv_up (profiles/conv_up): mode 1, an f16 precision, no tape, the shape, at least split_below workgroups; the hop: Cout in {128, 256, 512,
    # 1024} (groups inside a wave's 32 channels), a wait set of at most half of the resident workgroups and 384 workgroups
    wgs_up = B * (W // 32) * (H // 8) * cdiv(cout, 64) * 2
    if knobs["conv_up"] and mode == 1 and not q["grad"] and f16 and not q["concat"] and conv_up_ok(B, cin, cout, H, W) and wgs_up >= knobs["split_below"]:
        hop = (arena and geo(Ho, Wo) >= 0 and cout % 64 == 0 and group_in_wave(cout, 32) and 2 * (W // 32) * (H // 8) <= caps[2] // 2 and
               wgs_up >= HOP_MIN_WG and B * (cout // 8) * H * W * 4 * 16 < GiB4 and room(cout // 64))
        conv1 = dict(kernel=12, hop=int(hop), workgroups=wgs_up, ksplit=1, stat_kind=0 if hop else 1)
        return dict(up=1, skip_emit=0, hop=3 if hop else 0, conv1=conv1, conv2=plan(c2, knobs, caps))
    has_skip = cin != cout
    skip_emit = ((knobs["emit_skip"] == 2 or (knobs["emit_skip"] == 1 and cout <= 128)) and has_skip and mode == 0 and f16 and geo(Ho, Wo) >= 0 and
                 conv5_ok(B, cout, Ho, Wo) and cin % 16 == 0 and cin <= 384 and (Ho * Wo) % 256 == 0 and B * 2 * cdiv(cin, 16) * Ho * Wo * 16 < GiB4 and
                 not (knobs["fuse_small"] and gn_small_ok(cin, H, W)))
    hop_arena = (arena and f16 and not q["grad"] and hop7_ok(B, cout, Ho, Wo, caps[0]) and room(cout // 128) and
                 B * 2 * cdiv(cout, 16) * Ho * Wo * 16 < GiB4)
    # conv9's hop: 8 x 8 with both convolutions on conv9; obeys fuse_h1, uses nothing of the arena
    hop9 = (not skip_emit and q["hop_allowed"] and knobs["fuse_h1"] and plan(dict(c1, hop=1), knobs, caps).get("kernel") == 9 and
            plan(c2, knobs, caps).get("kernel") == 9)
    hop = 2 if hop9 else (1 if hop_arena else 0)
    if hop:
        c1 = dict(c1, hop=1, slab_floats=0, stats=0)
    return dict(up=0, skip_emit=int(skip_emit), hop=hop, conv1=plan(c1, knobs, caps), conv2=plan(c2, knobs, caps))
