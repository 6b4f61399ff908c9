// Walks the planner of the 3x3 routes (csrc/conv_plan.cpp, compiled alone by a host compiler) over the grid of tests/test_conv_plan_host.py and
// every ResBlock on it, for a sanitizer run without a GPU or Python:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diffpir_amd/csrc tools/conv_plan_walk.cpp diffpir_amd/csrc/conv_plan.cpp -o conv_plan_walk
// Prints the number of plans per kernel; invariants that hold for every plan are checked on the way.
#include "conv_plan.h"
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
using namespace dpir;

static void check(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "conv_plan_walk: %s\n", what); exit(1); }
}

int main() {
    const int Bs[] = {1, 2, 3, 4, 5, 8, 16, 32, 64};
    const int Cs[] = {3, 6, 16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 640, 1024};
    const int HWs[][2] = {{4, 4}, {8, 8}, {12, 12}, {16, 16}, {24, 24}, {32, 32}, {40, 40}, {64, 64}, {128, 128}, {256, 256},
                          {8, 32}, {16, 64}, {32, 8}, {12, 20}, {64, 128}, {8, 16}};
    const ConvKnobs knobs = ConvKnobs::from_env();
    long long count[64] = {0}, refused = 0, blocks = 0;
    for (int cap : {512, 64})
        for (int B : Bs) for (int cin : Cs) for (int cout : Cs) for (auto& hw : HWs)
            for (int prec = 0; prec < 3; ++prec) for (int grad = 0; grad < 2; ++grad) for (int slab = 0; slab < 2; ++slab) for (int hop = 0; hop < 2; ++hop) {
                const DeviceCaps caps{cap, cap, cap};
                Conv3Query q;
                q.B = B; q.Cin = cin; q.Cout = cout; q.H = hw[0]; q.W = hw[1]; q.precision = prec; q.grad = grad;
                q.w16 = prec != 0; q.w11 = prec == 1 && cin % 32 == 0 && cout % 128 == 0; q.w8 = prec != 0 && cout <= 16 && cin % 32 == 0;
                q.conv8_source = slab; q.slab = slab && !hop; q.slab_floats = q.slab ? (size_t)16 << 20 : 0; q.defer = true; q.hop = hop;
                q.stat_slots = q.stat_plane = geometry(q.H, q.W).stat_slots > 0 && cout % 32 == 0 && !hop;
                const Conv3Plan p = plan_conv3(q, knobs, caps);
                if (p.refusal) { ++refused; continue; }
                check(p.kernel >= 0 && p.kernel < 64, "kernel id");
                ++count[p.kernel];
                check(p.ksplit >= 1 && p.ksplit <= 16 && p.workgroups >= 0 && p.workgroups < (1ll << 31), "split factor / workgroups");
                check(p.kernel == CK_FP32 || p.kernel == CK_CONV8 || p.kernel == CK_CONV9 || p.kernel == CK_CONV11 ||
                      p.ksplit * p.chunks_per_split >= (cin + 15) / 16, "slices cover K");
                check(!p.hop || (hop && p.ksplit == 1 && p.stat_kind == ST_NONE), "a hop runs whole K and keeps no statistics");
                check(p.stat_kind != ST_PENDING || p.ksplit > 1, "only a split launch is left pending");
                if (hop || !slab) continue;       // one ResBlock per shape and engine state: input resolution H x W, every mode
                for (int mode = 0; mode < 3; ++mode) {
                    ResblockQuery r;
                    r.B = B; r.Cin = cin; r.Cout = cout; r.H = hw[0]; r.W = hw[1]; r.mode = mode; r.has_skip = cin != cout; r.concat = r.has_skip;
                    r.gn1_c = cin; r.gn2_c = cout; r.precision = prec; r.grad = grad; r.hop_allowed = true; r.arena_words_left = (size_t)B * 4096;
                    r.conv1_w16 = r.conv2_w16 = r.skip_w16 = prec != 0; r.conv1_w11 = q.w11; r.conv2_w11 = prec == 1 && cout % 128 == 0;
                    r.conv1_wup = prec != 0 && mode == 1 && cin % 16 == 0 && cout % 32 == 0;
                    r.small_prologue = hw[0] * hw[1] <= 1024; r.conv5_ok = true; r.slab = true; r.slab_floats = (size_t)16 << 20;
                    const ResblockPlan rp = plan_resblock(r, knobs, caps);
                    check(!(rp.up && rp.skip_emit), "one ResBlock route");
                    check((rp.hop != HOP_NONE) == rp.conv1.hop || rp.conv1.refusal, "the hop is conv1's");
                    check(rp.hop == HOP_NONE || (!grad && prec != 0), "no hop with a tape or in f32");
                    ++blocks;
                }
            }
    for (int k = 0; k < 64; ++k)
        if (count[k]) printf("kernel %2d: %lld plans\n", k, count[k]);
    printf("refused: %lld, ResBlock plans: %lld\n", refused, blocks);
    return 0;
}
