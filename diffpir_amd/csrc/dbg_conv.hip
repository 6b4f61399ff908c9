// Development-only: one convolution shape timed in isolation (include/diffpir_debug.h).  Part of libdiffpir_dbg.so, which links
// against the product library and uses its internal launchers; nothing here is on the product path.
#include "engine.h"
#include "conv6_params.h"
#include "conv9.h"
#include "conv11.h"
#include "conv_up.h"
#include "../../include/diffpir_debug.h"
#include <string.h>
#include <vector>
using namespace dpir;
static int fail(dpir_engine* e, const Status& s) {
    if (e) e->last_error = s.msg;
    return s.code;
}
#define API_TRY(e, expr)                          \
    do {                                          \
        Status _s = (expr);                       \
        if (!_s.ok()) return fail((e), _s);       \
    } while (0)
#define API_HIP(e, expr)                                                                  \
    do {                                                                                  \
        hipError_t _h = (expr);                                                           \
        if (_h != hipSuccess)                                                             \
            return fail((e), Status{DPIR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_h)}); \
    } while (0)

// elements whose bit patterns differ (out[0]) and their largest absolute difference as ordered uint bits (out[1])
__global__ void dbg_bitdiff_kernel(const float* a, const float* b, size_t n, unsigned long long* out) {
    unsigned long long cnt = 0; unsigned mx = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float x = a[i], y = b[i];
        if (__builtin_bit_cast(unsigned, x) != __builtin_bit_cast(unsigned, y)) {
            ++cnt;
            const float d = fabsf(x - y);
            const unsigned u = d == d ? __builtin_bit_cast(unsigned, d) : 0x7fc00000u;
            mx = u > mx ? u : mx;
        }
    }
    if (cnt) { atomicAdd(&out[0], cnt); atomicMax(&out[1], (unsigned long long)mx); }
}

// `launch` repeated `iters` times back to back on the stream: *ms_out = average time of one repeat (untouched when iters <= 0)
template <class F>
static Status time_repeats(hipStream_t s, int iters, F&& launch, double* ms_out) {
    if (iters <= 0) return Status{};
    hipEvent_t e0, e1;
    DPIR_HIP(hipEventCreate(&e0)); DPIR_HIP(hipEventCreate(&e1));
    DPIR_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) DPIR_TRY(launch());
    DPIR_HIP(hipEventRecord(e1, s));
    DPIR_HIP(hipEventSynchronize(e1));
    float ms = 0; DPIR_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms_out = ms / iters;
    return Status{};
}

// epilogue slots [planes][slots] (fp32 partial sums of at most 256 values) folded in fp64 (gn_prm's contract) into stat_out[planes][2]
static Status fold_slots(const float2* st, size_t planes, int slots, double* stat_out) {
    std::vector<float2> hs(planes * slots);
    DPIR_HIP(hipMemcpy(hs.data(), st, hs.size() * 8, hipMemcpyDeviceToHost));
    for (size_t pl = 0; pl < planes; ++pl) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < slots; ++k) { s1 += (double)hs[pl * slots + k].x; s2 += (double)hs[pl * slots + k].y; }
        stat_out[2 * pl] = s1; stat_out[2 * pl + 1] = s2;
    }
    return Status{};
}

// The second layer of a two-layer hop probe (fields gamma2, beta2, film2, w2, bias2, Cout2 of the descriptors): its poisoned planes and output,
// GroupNorm affine, FiLM rows, bias and conv6-layout weights on the device, and the Conv6Emit the first layer's epilogue is given.
// counters > 0: an arena with the accumulators and that many arrival counters per image (to be zeroed before every launch of the first layer).
struct HopStage {
    char* s16b = nullptr; size_t plane2 = 0, no2 = 0, arena_words = 0;
    float *dbias2 = nullptr, *dout2 = nullptr; void* wp2 = nullptr; float w2_scale = 1.f; long long* arena = nullptr;
    Conv6Emit em;
};
template <class Desc>
static Status hop_stage(dpir_engine* e, const std::string& tag, const Desc* d, int B, int Cout, size_t HW, bool x1, int counters, HopStage* h) {
    const int Co2 = d->Cout2, C8b = 2 * ((Cout + 15) / 16);
    h->plane2 = (size_t)B * C8b * HW * 16; h->no2 = (size_t)B * Co2 * HW;
    float *dg = nullptr, *db = nullptr, *df = nullptr;
    DPIR_TRY(e->ws.getT(tag + "#s16b", 2 * h->plane2, &h->s16b));
    DPIR_TRY(e->ws.getT(tag + "#gamma2", (size_t)Cout, &dg));
    DPIR_TRY(e->ws.getT(tag + "#beta2", (size_t)Cout, &db));
    DPIR_TRY(e->ws.getT(tag + "#film2", (size_t)B * 2 * Cout, &df));
    DPIR_TRY(e->ws.getT(tag + "#b2", (size_t)round_up(Co2, 64), &h->dbias2));
    DPIR_TRY(e->ws.getT(tag + "#o2", h->no2, &h->dout2));
    DPIR_HIP(hipMemsetAsync(h->s16b, 0xFF, 2 * h->plane2, e->stream));
    DPIR_HIP(hipMemcpy(dg, d->gamma2, (size_t)Cout * 4, hipMemcpyHostToDevice));
    DPIR_HIP(hipMemcpy(db, d->beta2, (size_t)Cout * 4, hipMemcpyHostToDevice));
    if (d->film2) DPIR_HIP(hipMemcpy(df, d->film2, (size_t)B * 2 * Cout * 4, hipMemcpyHostToDevice));
    DPIR_HIP(hipMemset(h->dbias2, 0, (size_t)round_up(Co2, 64) * 4));
    DPIR_HIP(hipMemcpy(h->dbias2, d->bias2, (size_t)Co2 * 4, hipMemcpyHostToDevice));
    DPIR_HIP(hipMemsetAsync(h->dout2, 0xFF, h->no2 * 4, e->stream));
    std::vector<uint16_t> w16b;
    h->w2_scale = pack_weights_conv6(d->w2, Co2, Cout, w16b);
    DPIR_TRY(e->ws.get(tag + "#w16b", w16b.size() * 2, &h->wp2));
    DPIR_HIP(hipMemcpy(h->wp2, w16b.data(), w16b.size() * 2, hipMemcpyHostToDevice));
    Conv6Emit& em = h->em;
    em.hi = h->s16b; em.lo = x1 ? nullptr : h->s16b + h->plane2; em.C8 = C8b; em.gamma = dg; em.beta = db;
    em.film = d->film2 ? df : nullptr; em.film_stride = 2 * Cout; em.film_off = 0; em.frows = 2 * Cout; em.fstep = nullptr;
    em.range_ctr = e->range_ctr;
    if (counters > 0) {
        h->arena_words = (size_t)B * 64 + ((size_t)B * counters + 1) / 2;
        DPIR_TRY(e->ws.getT(tag + "#arena", h->arena_words, &h->arena));
        em.acc = h->arena; em.cnt = reinterpret_cast<unsigned*>(h->arena + (size_t)B * 64);
    }
    return Status{};
}
// the second layer through launch_conv6
static Conv6Args second_conv6(const HopStage& h, int B, int Cin, int Cout, int H, int W, bool x1) {
    Conv6Args c6;
    c6.x1 = x1; c6.xhi = h.s16b; c6.xlo = h.s16b + h.plane2; c6.w16 = h.wp2; c6.w16_scale = h.w2_scale;
    c6.bias = h.dbias2; c6.out = h.dout2; c6.B = B; c6.Cin = Cin; c6.Cout = Cout; c6.H = H; c6.W = W;
    return c6;
}

extern "C" {
// Times one convolution shape in isolation (synthetic operands already on the device).  mode bits: 0 = exact-fp32 kernels,
// 1 = f16x3 (conv6 for 3x3 incl. its act_split pre-pass, conv5 for 1x1), 2 = f16x3 without the pre-pass (planes prepared once).
// Not part of the product path; used by tools/ only.
int dpir_debug_conv_bench(dpir_engine* e, int B, int Cin, int Cout, int H, int W, int ks, int mode, int with_prm,
                          int dbg, int iters, double* ms_out) {
    if (!e || !ms_out || iters <= 0) return DPIR_ERR_INVALID;
    (void)hipSetDevice(e->device);
    int taps = ks * ks, coutp = round_up(Cout, 64), cinp = round_up(Cin, 16);
    float *x = nullptr, *w = nullptr, *bias = nullptr, *out = nullptr, *partial = nullptr; float4* prm = nullptr;
    API_TRY(e, e->ws.getT("dbg#x", (size_t)B * Cin * H * W, &x));
    API_TRY(e, e->ws.getT("dbg#w", (size_t)cinp * taps * coutp, &w));
    API_TRY(e, e->ws.getT("dbg#b", (size_t)coutp, &bias));
    API_TRY(e, e->ws.getT("dbg#o", (size_t)B * Cout * H * W, &out));
    API_TRY(e, e->ws.getT("dbg#prm", (size_t)B * Cin, &prm));
    API_TRY(e, e->ws.getT("conv#partial", (size_t)16 * 1024 * 1024, &partial));
    API_TRY(e, launch_randn(e->stream, x, 1, 1, 0, 1, (size_t)B * Cin * H * W));
    API_TRY(e, launch_randn(e->stream, w, 2, 1, 0, 1, (size_t)cinp * taps * coutp));
    API_TRY(e, launch_randn(e->stream, bias, 3, 1, 0, 1, (size_t)coutp));
    API_TRY(e, launch_randn(e->stream, reinterpret_cast<float*>(prm), 4, 1, 0, 1, (size_t)B * Cin * 4));
    ConvArgs a;
    a.src.a = x; a.src.ca = Cin; a.src.Hs = H; a.src.Ws = W; a.src.mode = 0; a.src.prm = with_prm ? prm : nullptr;
    a.w = w; a.bias = bias; a.out = out; a.B = B; a.Cin = Cin; a.Cout = Cout; a.CoutP = coutp; a.H = H; a.W = W; a.ks = ks;
    a.partial = partial; a.partial_capacity = (size_t)16 * 1024 * 1024;
    const void* w16 = nullptr; float w16_scale = 1.f;
    if (dbg != 0) {   // operand-split f16 path with synthetic split weights
        std::vector<float> hw((size_t)Cout * Cin * taps);
        for (size_t i = 0; i < hw.size(); ++i) hw[i] = (float)((i * 2654435761u) % 2001) / 1000.0f * 0.05f - 0.05f;
        std::vector<uint16_t> w16v;
        w16_scale = ks == 1 ? pack_weights_f16x3_1x1(hw.data(), Cout, Cin, w16v) : pack_weights_conv6(hw.data(), Cout, Cin, w16v);
        void* wp = nullptr;
        API_TRY(e, e->ws.get("dbg#w16", w16v.size() * 2, &wp));
        API_HIP(e, hipMemcpy(wp, w16v.data(), w16v.size() * 2, hipMemcpyHostToDevice));
        w16 = wp;
    }
    Conv5Args a5;
    Conv6Args a6;
    const bool use5 = dbg != 0 && ks == 1, use6 = dbg != 0 && ks == 3;
    if (use5) {
        a5.src = CatSrc{x, Cin, nullptr, 0}; a5.prm = a.src.prm; a5.w16 = w16; a5.w16_scale = w16_scale; a5.bias = bias; a5.out = out;
        a5.B = B; a5.Cout = Cout; a5.H = H; a5.W = W; a5.x1 = e->precision == 2;      // f16x1 engine: single-product kernels (hi planes only)
    }
    if (use6) {
        int C8 = 2 * ((Cin + 15) / 16);
        size_t plane = (size_t)B * C8 * H * W * 16;
        char* s16 = nullptr;
        API_TRY(e, e->ws.getT("dbg#s16", 2 * plane, &s16));
        API_TRY(e, launch_act_split(e->stream, CatSrc{x, Cin, nullptr, 0}, a.src.prm, 0, B, H, W, s16, s16 + plane));
        a6.xhi = s16; a6.xlo = s16 + plane; a6.w16 = w16; a6.w16_scale = w16_scale; a6.bias = bias; a6.out = out;
        a6.B = B; a6.Cin = Cin; a6.Cout = Cout; a6.H = H; a6.W = W; a6.partial = partial; a6.partial_capacity = a.partial_capacity;
        a6.x1 = e->precision == 2;
    }
    auto run_once = [&]() -> Status {
        if (use5) return launch_conv5(e->stream, a5);
        if (use6) {
            if (dbg == 1) DPIR_TRY(launch_act_split(e->stream, CatSrc{x, Cin, nullptr, 0}, a.src.prm, 0, B, H, W, const_cast<void*>(a6.xhi), const_cast<void*>(a6.xlo)));
            return launch_conv6(e->stream, a6);
        }
        return launch_conv(e->stream, a);
    };
    API_TRY(e, run_once());
    API_TRY(e, time_repeats(e->stream, iters, run_once, ms_out));
    return DPIR_OK;
}

// conv7 (csrc/conv7.hip) against conv6 (8 x 32 geometry: the only one conv6 is still built for) on the same split planes and weight
// pack: outputs + fused GroupNorm statistics (whole K) or the split-K partial slabs must agree bit for bit; then both are timed back to back.  x1: f16x1 planes / products; split: give both kernels a partial buffer so that the
// launch is split along K when launch_conv6's rule says so; scaled: a device output scale of 0.25 (the dgrad route).
int dpir_debug_conv7_check(dpir_engine* e, int B, int Cin, int Cout, int H, int W, int res_mode, int x1, int split, int scaled, int iters,
                            double* ms6_out, double* ms7_out, unsigned long long* mismatches_out, float* maxdiff_out, int* ksplit_out) {
    if (!e || !ms6_out || !ms7_out || !mismatches_out || !maxdiff_out || !ksplit_out || iters <= 0 || res_mode < -1 || res_mode > 2) return DPIR_ERR_INVALID;
    (void)hipSetDevice(e->device);
    if (!conv6_supported(H, W) || W < 32) return fail(e, invalid("conv7 check: conv6 only has the 8 x 32 geometry (W >= 32) to compare with"));
    const size_t nx = (size_t)B * Cin * H * W, no = (size_t)B * Cout * H * W;
    const size_t nres = res_mode == 1 ? no / 4 : (res_mode == 2 ? no * 4 : no);
    const int slots = conv6_stat_slots(H, W);
    const size_t nst = (size_t)B * Cout * slots;
    const size_t pcap = (size_t)16 * no;                       // room for 16 slabs
    float *x = nullptr, *bias = nullptr, *o6 = nullptr, *o7 = nullptr, *res = nullptr, *p6 = nullptr, *p7 = nullptr, *scale = nullptr;
    float2 *st6 = nullptr, *st7 = nullptr;
    unsigned long long* cmp = nullptr;
    API_TRY(e, e->ws.getT("c7#x", nx, &x));
    API_TRY(e, e->ws.getT("c7#b", (size_t)round_up(Cout, 64), &bias));
    API_TRY(e, e->ws.getT("c7#o6", no, &o6));
    API_TRY(e, e->ws.getT("c7#o7", no, &o7));
    API_TRY(e, e->ws.getT("c7#res", nres, &res));
    API_TRY(e, e->ws.getT("c7#st6", nst, &st6));
    API_TRY(e, e->ws.getT("c7#st7", nst, &st7));
    API_TRY(e, e->ws.getT("c7#cmp", (size_t)2, &cmp));
    API_TRY(e, e->ws.getT("c7#scale", (size_t)4, &scale));
    if (split) { API_TRY(e, e->ws.getT("c7#p6", pcap, &p6)); API_TRY(e, e->ws.getT("c7#p7", pcap, &p7)); }
    API_TRY(e, launch_randn(e->stream, x, 11, 1, 0, 1, nx));
    API_TRY(e, launch_randn(e->stream, bias, 12, 1, 0, 1, (size_t)round_up(Cout, 64)));
    API_TRY(e, launch_randn(e->stream, res, 13, 1, 0, 1, nres));
    const float quarter = 0.25f;
    API_HIP(e, hipMemcpyAsync(scale, &quarter, 4, hipMemcpyHostToDevice, e->stream));
    std::vector<float> hw((size_t)Cout * Cin * 9);
    for (size_t i = 0; i < hw.size(); ++i) hw[i] = (float)((i * 2654435761u) % 2001) / 1000.0f * 0.05f - 0.05f;
    std::vector<uint16_t> w16v;
    const float w16_scale = pack_weights_conv6(hw.data(), Cout, Cin, w16v);
    void* wp = nullptr;
    API_TRY(e, e->ws.get("c7#w16", w16v.size() * 2, &wp));
    API_HIP(e, hipMemcpy(wp, w16v.data(), w16v.size() * 2, hipMemcpyHostToDevice));
    const int chunks = (Cin + 15) / 16, C8 = 2 * chunks;
    const size_t plane = (size_t)B * C8 * H * W * 16;
    char* s16 = nullptr;
    API_TRY(e, e->ws.getT("c7#s16", 2 * plane, &s16));
    API_TRY(e, launch_act_split(e->stream, CatSrc{x, Cin, nullptr, 0}, nullptr, 0, B, H, W, s16, x1 ? nullptr : s16 + plane));
    Conv6Args a6;
    a6.xhi = s16; a6.xlo = x1 ? nullptr : s16 + plane; a6.w16 = wp; a6.w16_scale = w16_scale; a6.bias = bias;
    a6.B = B; a6.Cin = Cin; a6.Cout = Cout; a6.H = H; a6.W = W; a6.x1 = x1 != 0;
    if (res_mode >= 0) { a6.res = res; a6.res_mode = res_mode; }
    if (scaled) a6.out_scale_dev = scale;
    a6.out = o6; a6.stat = st6; a6.force_kernel = 6;
    if (split) { a6.partial = p6; a6.partial_capacity = pcap; }
    // the parameter block launch_conv6 builds, for conv7: the same plan with the other kernel forced
    Conv3Query q;
    q.B = B; q.Cin = Cin; q.Cout = Cout; q.H = H; q.W = W; q.w16 = true; q.slab = split != 0; q.slab_floats = pcap; q.defer = true;
    q.has_res = res_mode >= 0; q.out_scale_dev = scaled != 0; q.stat_slots = true; q.force_kernel = CK_CONV7;
    const Conv3Plan plan7 = plan_conv67(q, ConvKnobs::from_env(), DeviceCaps{});
    if (plan7.refusal) return fail(e, invalid(plan7.refusal));
    const Conv3Geometry g = geometry(H, W);
    const int S = plan7.ksplit, blocks = (int)(plan7.workgroups / S);
    Conv6K k;
    k.xhi = reinterpret_cast<const char*>(a6.xhi); k.xlo = reinterpret_cast<const char*>(a6.xlo);
    k.w16 = reinterpret_cast<const char*>(wp); k.bias = bias; k.out = o7; k.res = a6.res; k.res_mode = a6.res_mode;
    k.B = B; k.Cout = Cout; k.H = H; k.W = W; k.n_chunks_total = chunks; k.C8 = C8;
    k.out_scale = 1.0f / w16_scale; k.out_scale_dev = a6.out_scale_dev; k.zeros = nullptr;
    k.tiles_x = g.tiles_x; k.tiles_y = g.tiles_y; k.n_co_blocks = (Cout + 127) / 128;
    k.chunks_per_split = plan7.chunks_per_split; k.ksplit = S; k.partial = S > 1 ? p7 : nullptr;
    k.stat = S == 1 ? st7 : nullptr; k.stat_slots = plan7.stat_slots;
    *ksplit_out = S;
    API_HIP(e, hipMemsetAsync(o6, 0xFF, no * 4, e->stream));
    API_HIP(e, hipMemsetAsync(o7, 0x7F, no * 4, e->stream));
    API_HIP(e, hipMemsetAsync(st6, 0xFF, nst * 8, e->stream));
    API_HIP(e, hipMemsetAsync(st7, 0x7F, nst * 8, e->stream));
    if (split) { API_HIP(e, hipMemsetAsync(p6, 0xFF, (size_t)S * no * 4, e->stream)); API_HIP(e, hipMemsetAsync(p7, 0x7F, (size_t)S * no * 4, e->stream)); }
    API_HIP(e, hipMemsetAsync(cmp, 0, 16, e->stream));
    Conv3Plan plan6;
    PendingConv pend;
    API_TRY(e, launch_conv6(e->stream, a6, &plan6, &pend));
    if (plan6.kernel != CK_CONV6 || plan6.ksplit != S) return fail(e, Status{DPIR_ERR_INVALID, "conv7 check: forcing the kernel changed the plan"});
    API_TRY(e, launch_conv7(e->stream, k, blocks * S, x1 != 0));
    API_HIP(e, hipGetLastError());
    if (S > 1) {
        hipLaunchKernelGGL(dbg_bitdiff_kernel, dim3(2048), dim3(256), 0, e->stream, p6, p7, (size_t)S * no, cmp);
    } else {
        hipLaunchKernelGGL(dbg_bitdiff_kernel, dim3(2048), dim3(256), 0, e->stream, o6, o7, no, cmp);
        hipLaunchKernelGGL(dbg_bitdiff_kernel, dim3(256), dim3(256), 0, e->stream, reinterpret_cast<const float*>(st6), reinterpret_cast<const float*>(st7), nst * 2, cmp);
    }
    unsigned long long h[2] = {0, 0};
    API_HIP(e, hipMemcpyAsync(h, cmp, 16, hipMemcpyDeviceToHost, e->stream));
    API_HIP(e, hipStreamSynchronize(e->stream));
    *mismatches_out = h[0];
    const unsigned mb = (unsigned)h[1];
    *maxdiff_out = __builtin_bit_cast(float, mb);
    hipEvent_t e0, e1, e2;
    API_HIP(e, hipEventCreate(&e0)); API_HIP(e, hipEventCreate(&e1)); API_HIP(e, hipEventCreate(&e2));
    for (int i = 0; i < 3; ++i) { API_TRY(e, launch_conv6(e->stream, a6, &plan6, &pend)); API_TRY(e, launch_conv7(e->stream, k, blocks * S, x1 != 0)); }
    API_HIP(e, hipEventRecord(e0, e->stream));
    for (int i = 0; i < iters; ++i) API_TRY(e, launch_conv6(e->stream, a6, &plan6, &pend));
    API_HIP(e, hipEventRecord(e1, e->stream));
    for (int i = 0; i < iters; ++i) API_TRY(e, launch_conv7(e->stream, k, blocks * S, x1 != 0));
    API_HIP(e, hipEventRecord(e2, e->stream));
    API_HIP(e, hipEventSynchronize(e2));
    float m6 = 0, m7 = 0;
    API_HIP(e, hipEventElapsedTime(&m6, e0, e1)); API_HIP(e, hipEventElapsedTime(&m7, e1, e2));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2);
    *ms6_out = m6 / iters; *ms7_out = m7 / iters;
    return DPIR_OK;
}

// One 1x1 layer on caller-supplied host operands through the forward's own dispatch (Fwd::conv, unet.hip): conv5 on the tile
// launch_conv5 picks (tile 0) or on a forced tile (1 = 128 x 256, 2 = 64 x 128), the general fp32 kernel where conv5 refuses the shape.
int dpir_debug_conv5_layer(dpir_engine* e, int B, int ca, int cb, int Cout, int H, int W, int tile, const float* xa, const float* xb,
                           const float* w, const float* bias, const float* prm, const float* res, float* out, int* path_out) {
    if (!e || !xa || !w || !bias || !out || !path_out || B <= 0 || ca <= 0 || cb < 0 || (cb > 0 && !xb) || Cout <= 0 || tile < 0 || tile > 2) return DPIR_ERR_INVALID;
    if (e->precision == 0) return fail(e, invalid("conv5 layer: the engine is in f32 mode"));
    (void)hipSetDevice(e->device);
    const int C = ca + cb, HW = H * W;
    const size_t na = (size_t)B * ca * HW, nb = (size_t)B * cb * HW, no = (size_t)B * Cout * HW;
    float *dxa = nullptr, *dxb = nullptr, *dbias = nullptr, *dout = nullptr, *dres = nullptr, *dw = nullptr, *partial = nullptr; float4* dprm = nullptr;
    API_TRY(e, e->ws.getT("c5#xa", na, &dxa));
    API_TRY(e, e->ws.getT("c5#xb", nb + 1, &dxb));
    API_TRY(e, e->ws.getT("c5#b", (size_t)round_up(Cout, 64), &dbias));
    API_TRY(e, e->ws.getT("c5#o", no, &dout));
    API_TRY(e, e->ws.getT("c5#res", no, &dres));
    API_TRY(e, e->ws.getT("c5#prm", (size_t)B * C, &dprm));
    API_HIP(e, hipMemcpy(dxa, xa, na * 4, hipMemcpyHostToDevice));
    if (cb) API_HIP(e, hipMemcpy(dxb, xb, nb * 4, hipMemcpyHostToDevice));
    API_HIP(e, hipMemset(dbias, 0, (size_t)round_up(Cout, 64) * 4));
    API_HIP(e, hipMemcpy(dbias, bias, (size_t)Cout * 4, hipMemcpyHostToDevice));
    if (prm) API_HIP(e, hipMemcpy(dprm, prm, (size_t)B * C * 16, hipMemcpyHostToDevice));
    if (res) API_HIP(e, hipMemcpy(dres, res, no * 4, hipMemcpyHostToDevice));
    API_HIP(e, hipMemset(dout, 0xFF, no * 4));
    std::vector<uint16_t> w16v;
    const float w16_scale = pack_weights_f16x3_1x1(w, Cout, C, w16v);
    void* wp = nullptr;
    API_TRY(e, e->ws.get("c5#w16", w16v.size() * 2, &wp));
    API_HIP(e, hipMemcpy(wp, w16v.data(), w16v.size() * 2, hipMemcpyHostToDevice));
    const bool has_prm = prm != nullptr;
    const bool use5 = !(has_prm && C % 16) && (tile != 0 || conv5_supported(B, Cout, H, W, has_prm) || conv5_small_supported(B, ca, cb, Cout, H, W, has_prm));
    Status st;
    if (use5) {
        Conv5Args a5;
        a5.src = CatSrc{dxa, ca, cb ? dxb : nullptr, cb}; a5.prm = has_prm ? dprm : nullptr; a5.w16 = wp; a5.w16_scale = w16_scale;
        a5.bias = dbias; a5.out = dout; a5.res = res ? dres : nullptr; a5.B = B; a5.Cout = Cout; a5.H = H; a5.W = W;
        a5.x1 = e->precision == 2; a5.force_tile = tile; a5.range_ctr = e->range_ctr;
        *path_out = tile ? tile : (conv5_small_supported(B, ca, cb, Cout, H, W, has_prm) ? 2 : 1);
        st = launch_conv5(e->stream, a5);
    } else {
        // load_conv's packing of the fp32 operand: [CinP][taps][CoutP]
        const int coutp = round_up(Cout, 64), cinp = round_up(C, 16);
        std::vector<float> packed((size_t)cinp * coutp, 0.f);
        for (int co = 0; co < Cout; ++co)
            for (int ci = 0; ci < C; ++ci) packed[(size_t)ci * coutp + co] = w[(size_t)co * C + ci];
        API_TRY(e, e->ws.getT("c5#w", packed.size(), &dw));
        API_HIP(e, hipMemcpy(dw, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
        API_TRY(e, e->ws.getT("conv#partial", (size_t)16 * 1024 * 1024, &partial));
        ConvArgs a;
        a.src.a = dxa; a.src.ca = ca; a.src.b = cb ? dxb : nullptr; a.src.cb = cb; a.src.Hs = H; a.src.Ws = W; a.src.mode = 0;
        a.src.prm = has_prm ? dprm : nullptr;
        a.w = dw; a.bias = dbias; a.out = dout; a.res = res ? dres : nullptr; a.res_mode = 0;
        a.B = B; a.Cin = C; a.Cout = Cout; a.CoutP = coutp; a.H = H; a.W = W; a.ks = 1;
        a.partial = partial; a.partial_capacity = (size_t)16 * 1024 * 1024;
        *path_out = 0;
        st = launch_conv(e->stream, a);
    }
    API_TRY(e, st);
    API_HIP(e, hipStreamSynchronize(e->stream));
    API_HIP(e, hipMemcpy(out, dout, no * 4, hipMemcpyDeviceToHost));
    return DPIR_OK;
}

// One 3x3 layer on caller-supplied host operands (include/diffpir_debug.h dpir_debug_conv3_desc): the prologue the forward would run
// (none / act_split or the fp32 kernel's own table prologue / gn_act_small), then the kernel plan_conv3 (conv_plan.h) names with conv9 and
// conv11 switched off (they have probes of their own) and conv8 by request only.  Which kernel ran, the split-K factor and the statistics
// kind are the plan launch_conv6 executed.
int dpir_debug_conv3_layer(dpir_engine* e, dpir_debug_conv3_desc* d) {
    if (!e || !d) return DPIR_ERR_INVALID;
    d->path_out = -1; d->ksplit_out = 0; d->stat_kind_out = 0;
    const int B = d->B, ca = d->ca, cb = d->cb, Cout = d->Cout, H = d->H, W = d->W, mode = d->mode, C = ca + cb;
    if (!d->xa || !d->w || !d->bias || !d->out || B <= 0 || ca <= 0 || cb < 0 || (cb > 0 && !d->xb) || Cout <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 2 ||
        d->res_mode < -1 || d->res_mode > 2 || (d->res_mode >= 0 && !d->res) || d->prologue < 0 || d->prologue > 2 ||
        (d->route != 0 && d->route != 6 && d->route != 7 && d->route != 8))
        return fail(e, invalid("conv3 layer: bad descriptor"));
    if (d->prologue == 1 && !d->prm) return fail(e, invalid("conv3 layer: prologue 1 needs the table"));
    if (d->prologue == 2 && (!d->gamma || !d->beta)) return fail(e, invalid("conv3 layer: prologue 2 needs gamma and beta"));
    if (mode == 1 && ((H | W) & 1)) return fail(e, invalid("conv3 layer: a nearest-up source needs an even output size"));
    if (d->res_mode == 1 && ((H | W) & 1)) return fail(e, invalid("conv3 layer: a half-resolution residual needs an even output size"));
    if (d->defer && (!d->split || (d->route != 0 && d->route != 7) || !d->gamma2 || !d->beta2 || !d->w2 || !d->bias2 || !d->out2 || d->Cout2 <= 0))
        return fail(e, invalid("conv3 layer: defer needs split, route 0 or 7 and the second stage's operands"));
    (void)hipSetDevice(e->device);
    const int Hs = mode == 1 ? H / 2 : (mode == 2 ? H * 2 : H), Ws = mode == 1 ? W / 2 : (mode == 2 ? W * 2 : W);
    const size_t HWs = (size_t)Hs * Ws, HW = (size_t)H * W;
    const size_t na = (size_t)B * ca * HWs, nb = (size_t)B * cb * HWs, no = (size_t)B * Cout * HW;
    const size_t nres = d->res_mode == 1 ? no / 4 : (d->res_mode == 2 ? no * 4 : no);
    const int coutp = round_up(Cout, 64);
    float *dxa = nullptr, *dxb = nullptr, *dbias = nullptr, *dout = nullptr, *dres = nullptr, *scale = nullptr; float4* dprm = nullptr;
    API_TRY(e, e->ws.getT("c3#xa", na, &dxa));
    API_TRY(e, e->ws.getT("c3#xb", nb + 1, &dxb));
    API_TRY(e, e->ws.getT("c3#b", (size_t)coutp, &dbias));
    API_TRY(e, e->ws.getT("c3#o", no, &dout));
    API_TRY(e, e->ws.getT("c3#res", nres, &dres));
    API_TRY(e, e->ws.getT("c3#prm", (size_t)B * C, &dprm));
    API_TRY(e, e->ws.getT("c3#scale", (size_t)4, &scale));
    API_HIP(e, hipMemcpy(dxa, d->xa, na * 4, hipMemcpyHostToDevice));
    if (cb) API_HIP(e, hipMemcpy(dxb, d->xb, nb * 4, hipMemcpyHostToDevice));
    API_HIP(e, hipMemset(dbias, 0, (size_t)coutp * 4));
    API_HIP(e, hipMemcpy(dbias, d->bias, (size_t)Cout * 4, hipMemcpyHostToDevice));
    if (d->prologue == 1) API_HIP(e, hipMemcpy(dprm, d->prm, (size_t)B * C * 16, hipMemcpyHostToDevice));
    if (d->res_mode >= 0) API_HIP(e, hipMemcpy(dres, d->res, nres * 4, hipMemcpyHostToDevice));
    const float quarter = 0.25f;
    API_HIP(e, hipMemcpy(scale, &quarter, 4, hipMemcpyHostToDevice));
    API_HIP(e, hipMemset(dout, 0xFF, no * 4));
    const float* res = d->res_mode >= 0 ? dres : nullptr;
    const int res_mode = d->res_mode >= 0 ? d->res_mode : 0;
    const CatSrc src{dxa, ca, cb ? dxb : nullptr, cb};
    const bool x1 = e->precision == 2;
    const size_t pcap = (size_t)16 * no;                       // room for 16 slabs
    ConvKnobs knobs = ConvKnobs::from_env();
    knobs.conv8 = knobs.conv9 = knobs.conv11 = false;
    Conv3Query q;
    q.B = B; q.Cin = C; q.Cout = Cout; q.H = H; q.W = W; q.precision = e->precision; q.w16 = e->precision != 0;
    q.slab = d->split != 0; q.slab_floats = pcap; q.defer = d->defer != 0; q.has_res = res != nullptr; q.out_scale_dev = d->scaled != 0;
    const bool f16path = plan_conv3(q, knobs, DeviceCaps{}).kernel != CK_FP32;
    float* partial = nullptr;
    if (d->split) {
        API_TRY(e, e->ws.getT("c3#partial", pcap, &partial));
        API_HIP(e, hipMemset(partial, 0xFF, pcap * 4));
    }
    // hipMemset of device memory returns before the fill has run, and it runs on the null stream, which the engine's non-blocking stream does not
    // wait for: without this the poison can land AFTER a kernel below has written (seen once: conv7's whole output NaN, operand planes poisoned late)
    API_HIP(e, hipDeviceSynchronize());

    if (d->route == 8) {        // Fwd::conv's output-layer route
        if (e->precision == 0) return fail(e, invalid("conv3 layer: conv8 needs an f16 engine"));
        if (d->prologue != 1 || cb || mode != 0 || res || d->scaled || d->split) return fail(e, invalid("conv3 layer: conv8 takes a table prologue, one source, no resampling, no residual"));
        if (!conv8_supported(B, C, Cout, H, W)) return fail(e, invalid("conv8: shape not supported"));
        std::vector<uint16_t> w8;
        const float w8_scale = pack_weights_conv8(d->w, Cout, C, w8);
        void* wp = nullptr;
        API_TRY(e, e->ws.get("c3#w8", w8.size() * 2, &wp));
        API_HIP(e, hipMemcpy(wp, w8.data(), w8.size() * 2, hipMemcpyHostToDevice));
        Conv8Args a8;
        a8.x = dxa; a8.prm = dprm; a8.w = wp; a8.w_scale = w8_scale; a8.bias = dbias; a8.out = dout;
        a8.B = B; a8.C = C; a8.Cout = Cout; a8.H = H; a8.W = W; a8.range_ctr = e->range_ctr; a8.x1 = x1;
        a8.silu = d->prm[3] != 0.f;
        API_TRY(e, launch_conv8(e->stream, a8));
        API_HIP(e, hipStreamSynchronize(e->stream));
        API_HIP(e, hipMemcpy(d->out, dout, no * 4, hipMemcpyDeviceToHost));
        d->path_out = 8;
        return DPIR_OK;
    }

    if (!f16path) {             // the fp32 kernel: everything the f16 path refuses, and the whole f32 engine
        if (d->route != 0) return fail(e, invalid("conv3 layer: conv6 / conv7 cannot be forced here (f32 engine or a shape the f16 path refuses)"));
        if (d->prologue == 2) return fail(e, Status{DPIR_ERR_UNSUPPORTED, "conv3 layer: gn_act_small only feeds the f16 path"});
        if (d->scaled || d->defer) return fail(e, invalid("conv3 layer: the fp32 kernel has no device output scale and no deferred combine"));
        // load_conv's packing of the fp32 operand: [CinP][taps][CoutP]
        const int cinp = round_up(C, 16);
        std::vector<float> packed((size_t)cinp * 9 * coutp, 0.f);
        for (int co = 0; co < Cout; ++co)
            for (int ci = 0; ci < C; ++ci)
                for (int t = 0; t < 9; ++t) packed[((size_t)ci * 9 + t) * coutp + co] = d->w[((size_t)co * C + ci) * 9 + t];
        float* dw = nullptr;
        API_TRY(e, e->ws.getT("c3#w", packed.size(), &dw));
        API_HIP(e, hipMemcpy(dw, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
        ConvArgs a;
        a.src.a = dxa; a.src.ca = ca; a.src.b = cb ? dxb : nullptr; a.src.cb = cb; a.src.Hs = Hs; a.src.Ws = Ws; a.src.mode = mode;
        a.src.prm = d->prologue == 1 ? dprm : nullptr;
        a.w = dw; a.bias = dbias; a.out = dout; a.res = res; a.res_mode = res_mode;
        a.B = B; a.Cin = C; a.Cout = Cout; a.CoutP = coutp; a.H = H; a.W = W; a.ks = 3;
        a.partial = partial; a.partial_capacity = partial ? pcap : 0;
        API_TRY(e, launch_conv(e->stream, a));
        API_HIP(e, hipStreamSynchronize(e->stream));
        API_HIP(e, hipMemcpy(d->out, dout, no * 4, hipMemcpyDeviceToHost));
        d->path_out = 0;
        return DPIR_OK;
    }

    // ---- the f16 path: operand planes, then launch_conv6
    const int C8 = 2 * ((C + 15) / 16);
    const size_t plane = (size_t)B * C8 * HW * 16;
    char* s16 = nullptr;
    API_TRY(e, e->ws.getT("c3#s16", 2 * plane, &s16));
    API_HIP(e, hipMemset(s16, 0xFF, 2 * plane));
    API_HIP(e, hipDeviceSynchronize());        // the poison is in place before the prologue writes the planes (see above)
    if (d->prologue == 2) {     // Fwd::gn_conv's fused low-resolution prologue
        if (C % 16 || !gn_act_small_supported(C, Hs, Ws, mode)) return fail(e, Status{DPIR_ERR_UNSUPPORTED, "conv3 layer: gn_act_small refuses this shape"});
        float *dg = nullptr, *db = nullptr, *df = nullptr;
        API_TRY(e, e->ws.getT("c3#gamma", (size_t)C, &dg));
        API_TRY(e, e->ws.getT("c3#beta", (size_t)C, &db));
        API_TRY(e, e->ws.getT("c3#film", (size_t)B * 2 * C, &df));
        API_HIP(e, hipMemcpy(dg, d->gamma, (size_t)C * 4, hipMemcpyHostToDevice));
        API_HIP(e, hipMemcpy(db, d->beta, (size_t)C * 4, hipMemcpyHostToDevice));
        if (d->film) API_HIP(e, hipMemcpy(df, d->film, (size_t)B * 2 * C * 4, hipMemcpyHostToDevice));
        GnActArgs ga;
        ga.src = src; ga.gamma = dg; ga.beta = db;
        ga.film = d->film ? df : nullptr; ga.film_stride = 2 * C; ga.film_off = 0; ga.fstep = nullptr; ga.frows = 2 * C;
        ga.silu = true; ga.mode = mode; ga.B = B; ga.Hs = Hs; ga.Ws = Ws;
        ga.hi = s16; ga.lo = x1 ? nullptr : s16 + plane; ga.range_ctr = e->range_ctr;
        API_TRY(e, launch_gn_act_small(e->stream, ga));
    } else {
        API_TRY(e, launch_act_split(e->stream, src, d->prologue == 1 ? dprm : nullptr, mode, B, H, W, s16, x1 ? nullptr : s16 + plane, e->range_ctr));
    }
    std::vector<uint16_t> w16v;
    const float w16_scale = pack_weights_conv6(d->w, Cout, C, w16v);
    void* wp = nullptr;
    API_TRY(e, e->ws.get("c3#w16", w16v.size() * 2, &wp));
    API_HIP(e, hipMemcpy(wp, w16v.data(), w16v.size() * 2, hipMemcpyHostToDevice));
    // Fwd::conv6_on_planes
    Conv6Args a6;
    a6.x1 = x1;
    a6.xhi = s16; a6.xlo = s16 + plane; a6.w16 = wp; a6.w16_scale = w16_scale;
    a6.bias = dbias; a6.out = dout; a6.res = res; a6.res_mode = res_mode;
    a6.B = B; a6.Cin = C; a6.Cout = Cout; a6.H = H; a6.W = W;
    a6.partial = partial; a6.partial_capacity = partial ? pcap : 0;
    a6.force_kernel = d->route;
    if (d->scaled) a6.out_scale_dev = scale;
    const int slots = conv6_stat_slots(H, W);
    float2* st = nullptr; double2* sp = nullptr;
    const size_t nst = (size_t)B * Cout * slots;
    if (slots > 0 && Cout % 32 == 0) {
        API_TRY(e, e->ws.getT("c3#st", nst, &st));
        API_TRY(e, e->ws.getT("c3#sp", (size_t)B * Cout, &sp));
        API_HIP(e, hipMemset(st, 0xFF, nst * 8));
        API_HIP(e, hipMemset(sp, 0xFF, (size_t)B * Cout * 16));
        API_HIP(e, hipDeviceSynchronize());
    }
    a6.stat = st; a6.stat_plane = sp;
    Conv3Plan ran;
    PendingConv pc;
    API_TRY(e, launch_conv6(e->stream, a6, &ran, d->defer ? &pc : nullptr));
    const int kind = ran.stat_kind;
    d->path_out = ran.kernel == CK_CONV6 ? 6 : 7; d->stat_kind_out = kind; d->ksplit_out = ran.ksplit;
    if (d->split && !d->defer) {     // the same launch again with the combine left pending and finished by launch_conv6_resolve
        PendingConv probe;
        Conv6Args b6 = a6;
        float* o2 = nullptr;
        API_TRY(e, e->ws.getT("c3#o_again", no, &o2));
        b6.out = o2;
        API_HIP(e, hipStreamSynchronize(e->stream));
        std::vector<float> first(no);
        API_HIP(e, hipMemcpy(first.data(), dout, no * 4, hipMemcpyDeviceToHost));
        API_TRY(e, launch_conv6(e->stream, b6, nullptr, &probe));
        if (probe.partial) API_TRY(e, launch_conv6_resolve(e->stream, probe));
        API_HIP(e, hipStreamSynchronize(e->stream));
        // both launches ran the same slabs in the same order: the output of the first one is what is returned, the second must equal it
        std::vector<float> again(no);
        API_HIP(e, hipMemcpy(again.data(), o2, no * 4, hipMemcpyDeviceToHost));
        if (memcmp(first.data(), again.data(), no * 4) != 0) return fail(e, Status{DPIR_ERR_STATE, "conv3 layer: two identical split-K launches disagree"});
    }
    if (d->defer) {
        if (kind != ST_PENDING) return fail(e, invalid("conv3 layer: defer was asked for but launch_conv6 did not split this launch"));
        // Fwd::gn_conv after a split-K conv1: the fused prologue of the next layer combines the slabs (and stores the finished tensor)
        const int Cn = Cout, Co2 = d->Cout2;
        if (Cn % 16 || !gn_act_small_supported(Cn, H, W, 0)) return fail(e, Status{DPIR_ERR_UNSUPPORTED, "conv3 layer: gn_act_small refuses the second stage"});
        const int C8b = 2 * ((Cn + 15) / 16);
        const size_t plane2 = (size_t)B * C8b * HW * 16, no2 = (size_t)B * Co2 * HW;
        char* s16b = nullptr; float *dg = nullptr, *db = nullptr, *dbias2 = nullptr, *dout2 = nullptr;
        API_TRY(e, e->ws.getT("c3#s16b", 2 * plane2, &s16b));
        API_TRY(e, e->ws.getT("c3#gamma2", (size_t)Cn, &dg));
        API_TRY(e, e->ws.getT("c3#beta2", (size_t)Cn, &db));
        API_TRY(e, e->ws.getT("c3#b2", (size_t)round_up(Co2, 64), &dbias2));
        API_TRY(e, e->ws.getT("c3#o2", no2, &dout2));
        API_HIP(e, hipMemset(s16b, 0xFF, 2 * plane2));
        API_HIP(e, hipMemcpy(dg, d->gamma2, (size_t)Cn * 4, hipMemcpyHostToDevice));
        API_HIP(e, hipMemcpy(db, d->beta2, (size_t)Cn * 4, hipMemcpyHostToDevice));
        API_HIP(e, hipMemset(dbias2, 0, (size_t)round_up(Co2, 64) * 4));
        API_HIP(e, hipMemcpy(dbias2, d->bias2, (size_t)Co2 * 4, hipMemcpyHostToDevice));
        API_HIP(e, hipMemset(dout2, 0xFF, no2 * 4));
        API_HIP(e, hipDeviceSynchronize());
        GnActArgs ga;
        ga.src = CatSrc{dout, Cn, nullptr, 0}; ga.pend = pc; ga.gamma = dg; ga.beta = db;
        ga.silu = true; ga.mode = 0; ga.B = B; ga.Hs = H; ga.Ws = W;
        ga.hi = s16b; ga.lo = x1 ? nullptr : s16b + plane2; ga.range_ctr = e->range_ctr;
        API_TRY(e, launch_gn_act_small(e->stream, ga));
        std::vector<uint16_t> w16b;
        const float w16b_scale = pack_weights_conv6(d->w2, Co2, Cn, w16b);
        void* wp2 = nullptr;
        API_TRY(e, e->ws.get("c3#w16b", w16b.size() * 2, &wp2));
        API_HIP(e, hipMemcpy(wp2, w16b.data(), w16b.size() * 2, hipMemcpyHostToDevice));
        Conv6Args c6;
        c6.x1 = x1; c6.xhi = s16b; c6.xlo = s16b + plane2; c6.w16 = wp2; c6.w16_scale = w16b_scale;
        c6.bias = dbias2; c6.out = dout2; c6.B = B; c6.Cin = Cn; c6.Cout = Co2; c6.H = H; c6.W = W;
        API_TRY(e, launch_conv6(e->stream, c6));
        API_HIP(e, hipStreamSynchronize(e->stream));
        API_HIP(e, hipMemcpy(d->out2, dout2, no2 * 4, hipMemcpyDeviceToHost));
    }
    API_HIP(e, hipStreamSynchronize(e->stream));
    API_HIP(e, hipMemcpy(d->out, dout, no * 4, hipMemcpyDeviceToHost));
    if (d->stat_out && (kind == 1 || kind == 2)) {
        if (kind == 1) {
            API_TRY(e, fold_slots(st, (size_t)B * Cout, slots, d->stat_out));
        } else {
            API_HIP(e, hipMemcpy(d->stat_out, sp, (size_t)B * Cout * 16, hipMemcpyDeviceToHost));
        }
    }
    return DPIR_OK;
}

// One 8 x 8 layer on caller-supplied host operands through conv9 (csrc/conv9.hip), as Fwd::conv6_on_planes / Fwd::resblock (unet.hip) launch it
// -- without their workgroup threshold, so that one image can be run alone.  Planes of the first layer: act_split (optionally with a table).
// hop: conv1's epilogue writes the second layer's planes (GroupNorm32(gamma2, beta2) + FiLM rows + SiLU), the second layer runs on conv9 too.
int dpir_debug_conv9_layer(dpir_engine* e, dpir_debug_conv9_desc* d) {
    if (!e || !d) return DPIR_ERR_INVALID;
    d->ran_out = 0;
    const int B = d->B, Cin = d->Cin, Cout = d->Cout, H = d->H, W = d->W;
    if (!d->x || !d->w || !d->bias || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || d->res_mode < -1 || d->res_mode > 2 ||
        (d->res_mode >= 0 && !d->res) || (!d->hop && !d->out) || (d->hop && (!d->gamma2 || !d->beta2 || !d->w2 || !d->bias2 || !d->out2 || d->Cout2 <= 0)))
        return fail(e, invalid("conv9 layer: bad descriptor"));
    if (e->grad_enabled) return fail(e, Status{DPIR_ERR_UNSUPPORTED, "conv9 layer: a gradient-mode engine keeps launch_conv6's route"});
    if (e->precision == 0) return fail(e, Status{DPIR_ERR_UNSUPPORTED, "conv9 layer: the f32 precision keeps the fp32 kernel"});
    if (d->hop && d->res_mode >= 0) return fail(e, invalid("conv9 layer: the hop's first layer takes no residual"));
    if ((d->res_mode == 1 && ((H | W) & 1))) return fail(e, invalid("conv9 layer: a half-resolution residual needs an even output size"));
    (void)hipSetDevice(e->device);
    const bool x1 = e->precision == 2;
    const size_t HW = (size_t)H * W, nx = (size_t)B * Cin * HW, no = (size_t)B * Cout * HW;
    const size_t nres = d->res_mode == 1 ? no / 4 : (d->res_mode == 2 ? no * 4 : no);
    const int chunks = (Cin + 15) / 16, C8 = 2 * chunks;
    const size_t plane = (size_t)B * C8 * HW * 16;
    float *dx = nullptr, *dbias = nullptr, *dout = nullptr, *dres = nullptr; float4* dprm = nullptr; double2* sp = nullptr; char* s16 = nullptr;
    API_TRY(e, e->ws.getT("c9#x", nx, &dx));
    API_TRY(e, e->ws.getT("c9#b", (size_t)round_up(Cout, 64), &dbias));
    API_TRY(e, e->ws.getT("c9#o", no, &dout));
    API_TRY(e, e->ws.getT("c9#res", nres, &dres));
    API_TRY(e, e->ws.getT("c9#prm", (size_t)B * Cin, &dprm));
    API_TRY(e, e->ws.getT("c9#sp", (size_t)B * Cout, &sp));
    API_TRY(e, e->ws.getT("c9#s16", 2 * plane, &s16));
    API_HIP(e, hipMemcpy(dx, d->x, nx * 4, hipMemcpyHostToDevice));
    API_HIP(e, hipMemset(dbias, 0, (size_t)round_up(Cout, 64) * 4));
    API_HIP(e, hipMemcpy(dbias, d->bias, (size_t)Cout * 4, hipMemcpyHostToDevice));
    if (d->prm) API_HIP(e, hipMemcpy(dprm, d->prm, (size_t)B * Cin * 16, hipMemcpyHostToDevice));
    if (d->res_mode >= 0) API_HIP(e, hipMemcpy(dres, d->res, nres * 4, hipMemcpyHostToDevice));
    // poison on the engine's stream (non-blocking: a null-stream memset is not ordered with the launches below)
    API_HIP(e, hipMemsetAsync(dout, 0xFF, no * 4, e->stream));
    API_HIP(e, hipMemsetAsync(sp, 0xFF, (size_t)B * Cout * 16, e->stream));
    API_HIP(e, hipMemsetAsync(s16, 0xFF, 2 * plane, e->stream));
    API_TRY(e, launch_act_split(e->stream, CatSrc{dx, Cin, nullptr, 0}, d->prm ? dprm : nullptr, 0, B, H, W, s16, x1 ? nullptr : s16 + plane, e->range_ctr));
    std::vector<uint16_t> w16v;
    const float w16_scale = pack_weights_conv6(d->w, Cout, Cin, w16v);
    void* wp = nullptr;
    API_TRY(e, e->ws.get("c9#w16", w16v.size() * 2, &wp));
    API_HIP(e, hipMemcpy(wp, w16v.data(), w16v.size() * 2, hipMemcpyHostToDevice));
    Conv9Args a9;
    a9.xhi = s16; a9.xlo = s16 + plane; a9.w16 = wp; a9.w16_scale = w16_scale; a9.bias = dbias; a9.out = dout;
    if (d->res_mode >= 0) { a9.res = dres; a9.res_mode = d->res_mode; }
    a9.B = B; a9.Cin = Cin; a9.Cout = Cout; a9.H = H; a9.W = W; a9.stat_plane = sp; a9.x1 = x1;
    d->ms_out = 0.0;
    if (!d->hop) {
        API_TRY(e, launch_conv9(e->stream, a9));
        API_TRY(e, time_repeats(e->stream, d->iters, [&]() { return launch_conv9(e->stream, a9); }, &d->ms_out));
        API_HIP(e, hipStreamSynchronize(e->stream));
        d->ran_out = 1;
        API_HIP(e, hipMemcpy(d->out, dout, no * 4, hipMemcpyDeviceToHost));
        if (d->stat_out) API_HIP(e, hipMemcpy(d->stat_out, sp, (size_t)B * Cout * 16, hipMemcpyDeviceToHost));
        return DPIR_OK;
    }
    HopStage h;
    API_TRY(e, hop_stage(e, "c9", d, B, Cout, HW, x1, 0, &h));
    a9.out = nullptr; a9.stat_plane = nullptr; a9.emit = &h.em;
    API_TRY(e, launch_conv9(e->stream, a9));
    Conv9Args b9;
    b9.xhi = h.s16b; b9.xlo = h.s16b + h.plane2; b9.w16 = h.wp2; b9.w16_scale = h.w2_scale; b9.bias = h.dbias2; b9.out = h.dout2;
    b9.B = B; b9.Cin = Cout; b9.Cout = d->Cout2; b9.H = H; b9.W = W; b9.x1 = x1;
    API_TRY(e, launch_conv9(e->stream, b9));
    API_TRY(e, time_repeats(e->stream, d->iters, [&]() -> Status { DPIR_TRY(launch_conv9(e->stream, a9)); return launch_conv9(e->stream, b9); }, &d->ms_out));
    API_HIP(e, hipStreamSynchronize(e->stream));
    d->ran_out = 1;
    API_HIP(e, hipMemcpy(d->out2, h.dout2, h.no2 * 4, hipMemcpyDeviceToHost));
    return DPIR_OK;
}

// One layer of the 8 x 32 geometry on caller-supplied host operands through conv11 (csrc/conv11.hip), or the same planes through launch_conv6
// with conv7 forced (route 7: the arm conv11 is timed against).  Planes: act_split (optionally with a table).  The timed repeats are the
// convolution launch alone.
int dpir_debug_conv11_layer(dpir_engine* e, dpir_debug_conv11_desc* d) {
    if (!e || !d) return DPIR_ERR_INVALID;
    d->ran_out = 0; d->ms_out = 0.0;
    const int B = d->B, Cin = d->Cin, Cout = d->Cout, H = d->H, W = d->W;
    if (!d->x || !d->w || !d->bias || (!d->hop && !d->out) || B <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || d->res_mode < -1 || d->res_mode > 2 ||
        (d->res_mode >= 0 && !d->res) || (d->route != 0 && d->route != 7) || (d->hop && d->route != 0) ||
        (d->hop && (!d->gamma2 || !d->beta2 || !d->w2 || !d->bias2 || !d->out2 || d->Cout2 <= 0)))
        return fail(e, invalid("conv11 layer: bad descriptor"));
    if (d->hop && d->res_mode >= 0) return fail(e, invalid("conv11 layer: the hop's first layer takes no residual"));
    if ((d->res_mode == 1 && ((H | W) & 1))) return fail(e, invalid("conv11 layer: a half-resolution residual needs an even output size"));
    (void)hipSetDevice(e->device);
    const size_t HW = (size_t)H * W, nx = (size_t)B * Cin * HW, no = (size_t)B * Cout * HW;
    const size_t nres = d->res_mode == 1 ? no / 4 : (d->res_mode == 2 ? no * 4 : no);
    const int chunks = (Cin + 15) / 16, C8 = 2 * chunks;
    const size_t plane = (size_t)B * C8 * HW * 16;
    Conv11Args a11;
    a11.B = B; a11.Cin = Cin; a11.Cout = Cout; a11.H = H; a11.W = W;
    a11.ksplit = d->ksplit; a11.precision = e->precision; a11.grad = e->grad_enabled;
    if (d->route == 0) {        // refusals before anything is allocated: dummy non-null operands, the checks that decide come first
        Conv11Args probe = a11;
        if (probe.grad || probe.precision != 1 || probe.ksplit != 1 || !conv11_supported(Cin, Cout, H, W)) {
            const Status st = launch_conv11(e->stream, probe);
            if (!st.ok()) return fail(e, st);
        }
        if (d->hop && !conv11_emit_supported(Cout, H, W))
            return fail(e, Status{DPIR_ERR_UNSUPPORTED, "conv11 layer: fused emission needs GroupNorm groups inside a wave's 64 channels and an image's tiles resident with room to spare"});
    } else if (e->grad_enabled || e->precision != 1) {
        return fail(e, Status{DPIR_ERR_UNSUPPORTED, "conv11 layer: the conv7 arm is timed on an f16x3 inference engine"});
    }
    const int slots = conv6_stat_slots(H, W);
    const size_t nst = (size_t)B * Cout * slots;
    float *dx = nullptr, *dbias = nullptr, *dout = nullptr, *dres = nullptr; float4* dprm = nullptr; float2* st = nullptr; char* s16 = nullptr;
    API_TRY(e, e->ws.getT("c11#x", nx, &dx));
    API_TRY(e, e->ws.getT("c11#b", (size_t)round_up(Cout, 64), &dbias));
    API_TRY(e, e->ws.getT("c11#o", no, &dout));
    API_TRY(e, e->ws.getT("c11#res", nres, &dres));
    API_TRY(e, e->ws.getT("c11#prm", (size_t)B * Cin, &dprm));
    API_TRY(e, e->ws.getT("c11#st", nst > 0 ? nst : 1, &st));
    API_TRY(e, e->ws.getT("c11#s16", 2 * plane, &s16));
    API_HIP(e, hipMemcpy(dx, d->x, nx * 4, hipMemcpyHostToDevice));
    API_HIP(e, hipMemset(dbias, 0, (size_t)round_up(Cout, 64) * 4));
    API_HIP(e, hipMemcpy(dbias, d->bias, (size_t)Cout * 4, hipMemcpyHostToDevice));
    if (d->prm) API_HIP(e, hipMemcpy(dprm, d->prm, (size_t)B * Cin * 16, hipMemcpyHostToDevice));
    if (d->res_mode >= 0) API_HIP(e, hipMemcpy(dres, d->res, nres * 4, hipMemcpyHostToDevice));
    API_HIP(e, hipMemsetAsync(dout, 0xFF, no * 4, e->stream));
    if (nst) API_HIP(e, hipMemsetAsync(st, 0xFF, nst * 8, e->stream));
    API_HIP(e, hipMemsetAsync(s16, 0xFF, 2 * plane, e->stream));
    API_TRY(e, launch_act_split(e->stream, CatSrc{dx, Cin, nullptr, 0}, d->prm ? dprm : nullptr, 0, B, H, W, s16, s16 + plane, e->range_ctr));
    std::vector<uint16_t> w16v, w11v;
    const float w16_scale = pack_weights_conv6(d->w, Cout, Cin, w16v);
    void* wp = nullptr;
    if (d->route == 0) {
        pack_weights_conv11(d->w, Cout, Cin, w16_scale, w11v);
        API_TRY(e, e->ws.get("c11#w11", w11v.size() * 2, &wp));
        API_HIP(e, hipMemcpy(wp, w11v.data(), w11v.size() * 2, hipMemcpyHostToDevice));
    } else {
        API_TRY(e, e->ws.get("c11#w16", w16v.size() * 2, &wp));
        API_HIP(e, hipMemcpy(wp, w16v.data(), w16v.size() * 2, hipMemcpyHostToDevice));
    }
    a11.xhi = s16; a11.xlo = s16 + plane; a11.w11 = wp; a11.w_scale = w16_scale; a11.bias = dbias; a11.out = dout;
    if (d->res_mode >= 0) { a11.res = dres; a11.res_mode = d->res_mode; }
    a11.stat = nst ? st : nullptr;
    Conv6Args a6;
    a6.xhi = s16; a6.xlo = s16 + plane; a6.w16 = wp; a6.w16_scale = w16_scale; a6.bias = dbias; a6.out = dout;
    if (d->res_mode >= 0) { a6.res = dres; a6.res_mode = d->res_mode; }
    a6.B = B; a6.Cin = Cin; a6.Cout = Cout; a6.H = H; a6.W = W; a6.stat = nst ? st : nullptr; a6.force_kernel = 7;
    HopStage h;
    Conv6Args c6;
    if (d->hop) {
        API_TRY(e, hop_stage(e, "c11", d, B, Cout, HW, false, (Cout + 63) / 64, &h));
        a11.out = nullptr; a11.stat = nullptr; a11.emit = &h.em;
        c6 = second_conv6(h, B, Cout, d->Cout2, H, W, false);
    }
    auto launch = [&]() -> Status {
        if (d->route != 0) return launch_conv6(e->stream, a6);
        if (!d->hop) return launch_conv11(e->stream, a11);
        DPIR_HIP(hipMemsetAsync(h.arena, 0, h.arena_words * 8, e->stream));
        DPIR_TRY(launch_conv11(e->stream, a11));
        return launch_conv6(e->stream, c6);
    };
    API_TRY(e, launch());
    API_TRY(e, time_repeats(e->stream, d->iters, launch, &d->ms_out));
    API_HIP(e, hipStreamSynchronize(e->stream));
    d->ran_out = d->route == 0 ? (d->hop ? 12 : 11) : 7;
    if (d->hop) {
        API_HIP(e, hipMemcpy(d->out2, h.dout2, h.no2 * 4, hipMemcpyDeviceToHost));
        return DPIR_OK;
    }
    API_HIP(e, hipMemcpy(d->out, dout, no * 4, hipMemcpyDeviceToHost));
    if (d->stat_out && nst) API_TRY(e, fold_slots(st, (size_t)B * Cout, slots, d->stat_out));
    return DPIR_OK;
}

// conv1 of an up-sampling ResBlock on caller-supplied host operands (include/diffpir_debug.h dpir_debug_conv_up_desc), as Fwd::resblock_up
// (unet.hip) launches it -- route 0: act_split at the SOURCE resolution + conv_up (csrc/conv_up.hip) -- or as the forward ran it before --
// route 1: act_split with the nearest-up source + launch_conv6.  hop: the first layer's epilogue writes the second layer's planes and the second
// layer runs through launch_conv6 in both routes.
int dpir_debug_conv_up_layer(dpir_engine* e, dpir_debug_conv_up_desc* d) {
    if (!e || !d) return DPIR_ERR_INVALID;
    d->ran_out = 0; d->ms_out = 0.0;
    const int B = d->B, Cin = d->Cin, Cout = d->Cout, Hs = d->Hs, Ws = d->Ws;
    if (!d->x || !d->w || !d->bias || B <= 0 || Cin <= 0 || Cout <= 0 || Hs <= 0 || Ws <= 0 || (!d->hop && !d->out) || d->route < 0 || d->route > 1 ||
        (d->hop && (!d->gamma2 || !d->beta2 || !d->w2 || !d->bias2 || !d->out2 || d->Cout2 <= 0)))
        return fail(e, invalid("conv_up layer: bad descriptor"));
    if (e->grad_enabled) return fail(e, Status{DPIR_ERR_UNSUPPORTED, "conv_up layer: a gradient-mode engine keeps launch_conv6's route"});
    if (e->precision == 0) return fail(e, Status{DPIR_ERR_UNSUPPORTED, "conv_up layer: the f32 precision keeps the fp32 kernel"});
    if (d->res) return fail(e, invalid("conv_up: conv1 of an up-sampling ResBlock takes no residual"));
    const int min_wg = d->force_hop ? 0 : kHopMinWg;
    if (d->route == 0) {
        if (const char* why = conv_up_supported(B, Cin, Cout, Hs, Ws, d->hop != 0, min_wg)) return fail(e, Status{DPIR_ERR_UNSUPPORTED, why});
    } else if (Cin % 16 || !conv6_supported(2 * Hs, 2 * Ws) || (d->hop && !conv7_emit_supported(B, Cout, 2 * Hs, 2 * Ws))) {
        return fail(e, Status{DPIR_ERR_UNSUPPORTED, "conv_up layer: launch_conv6's route refuses this shape"});
    }
    (void)hipSetDevice(e->device);
    const bool x1 = e->precision == 2;
    const int H = 2 * Hs, W = 2 * Ws;
    const size_t HWs = (size_t)Hs * Ws, HW = 4 * HWs, nx = (size_t)B * Cin * HWs, no = (size_t)B * Cout * HW;
    const int C8 = 2 * ((Cin + 15) / 16);
    const size_t plane_s = (size_t)B * C8 * HWs * 16, plane = 4 * plane_s;
    const int slots = conv_up_stat_slots(Hs, Ws);
    const size_t nst = (size_t)B * Cout * slots;
    float *dx = nullptr, *dbias = nullptr, *dout = nullptr; float4* dprm = nullptr; float2* st = nullptr; char* s16 = nullptr;
    API_TRY(e, e->ws.getT("cu#x", nx, &dx));
    API_TRY(e, e->ws.getT("cu#b", (size_t)round_up(Cout, 64), &dbias));
    API_TRY(e, e->ws.getT("cu#o", no, &dout));
    API_TRY(e, e->ws.getT("cu#prm", (size_t)B * Cin, &dprm));
    API_TRY(e, e->ws.getT("cu#st", nst, &st));
    API_TRY(e, e->ws.getT("cu#s16", 2 * plane, &s16));
    API_HIP(e, hipMemcpy(dx, d->x, nx * 4, hipMemcpyHostToDevice));
    API_HIP(e, hipMemset(dbias, 0, (size_t)round_up(Cout, 64) * 4));
    API_HIP(e, hipMemcpy(dbias, d->bias, (size_t)Cout * 4, hipMemcpyHostToDevice));
    if (d->prm) API_HIP(e, hipMemcpy(dprm, d->prm, (size_t)B * Cin * 16, hipMemcpyHostToDevice));
    API_HIP(e, hipMemsetAsync(dout, 0xFF, no * 4, e->stream));
    API_HIP(e, hipMemsetAsync(st, 0xFF, nst * 8, e->stream));
    API_HIP(e, hipMemsetAsync(s16, 0xFF, 2 * plane, e->stream));
    std::vector<uint16_t> wv;
    const float w_scale = d->route == 0 ? pack_weights_conv_up(d->w, Cout, Cin, wv) : pack_weights_conv6(d->w, Cout, Cin, wv);
    void* wp = nullptr;
    API_TRY(e, e->ws.get("cu#w", wv.size() * 2, &wp));
    API_HIP(e, hipMemcpy(wp, wv.data(), wv.size() * 2, hipMemcpyHostToDevice));
    const CatSrc src{dx, Cin, nullptr, 0};
    const float4* prm = d->prm ? dprm : nullptr;
    HopStage h;
    if (d->hop) API_TRY(e, hop_stage(e, "cu", d, B, Cout, HW, x1, (Cout + 63) / 64, &h));
    auto once = [&]() -> Status {
        if (d->hop) DPIR_HIP(hipMemsetAsync(h.arena, 0, h.arena_words * 8, e->stream));
        if (d->route == 0) {
            DPIR_TRY(launch_act_split(e->stream, src, prm, 0, B, Hs, Ws, s16, x1 ? nullptr : s16 + plane_s, e->range_ctr));
            ConvUpArgs a;
            a.xhi = s16; a.xlo = s16 + plane_s; a.wup = wp; a.wup_scale = w_scale; a.bias = dbias; a.out = d->hop ? nullptr : dout;
            a.B = B; a.Cin = Cin; a.Cout = Cout; a.Hs = Hs; a.Ws = Ws; a.stat = d->hop ? nullptr : st; a.x1 = x1;
            a.emit = d->hop ? &h.em : nullptr; a.min_wg_hop = min_wg;
            DPIR_TRY(launch_conv_up(e->stream, a));
        } else {
            DPIR_TRY(launch_act_split(e->stream, src, prm, 1, B, H, W, s16, x1 ? nullptr : s16 + plane, e->range_ctr));
            Conv6Args a6;
            a6.x1 = x1; a6.xhi = s16; a6.xlo = s16 + plane; a6.w16 = wp; a6.w16_scale = w_scale; a6.bias = dbias; a6.out = d->hop ? nullptr : dout;
            a6.B = B; a6.Cin = Cin; a6.Cout = Cout; a6.H = H; a6.W = W; a6.stat = d->hop ? nullptr : st;
            a6.emit = d->hop ? &h.em : nullptr;
            Conv3Plan ran;
            DPIR_TRY(launch_conv6(e->stream, a6, &ran));
            if (!d->hop && ran.stat_kind != ST_SLOTS) return invalid("conv_up layer: launch_conv6 produced no epilogue statistics here");
        }
        if (d->hop) DPIR_TRY(launch_conv6(e->stream, second_conv6(h, B, Cout, d->Cout2, H, W, x1)));
        return Status{};
    };
    API_TRY(e, once());
    API_TRY(e, time_repeats(e->stream, d->iters, once, &d->ms_out));       // the whole route again, back to back, averaged
    API_HIP(e, hipStreamSynchronize(e->stream));
    d->ran_out = d->route == 0 ? (d->hop ? 2 : 1) : 7;
    if (d->hop) {
        API_HIP(e, hipMemcpy(d->out2, h.dout2, h.no2 * 4, hipMemcpyDeviceToHost));
        return DPIR_OK;
    }
    API_HIP(e, hipMemcpy(d->out, dout, no * 4, hipMemcpyDeviceToHost));
    if (d->stat_out) API_TRY(e, fold_slots(st, (size_t)B * Cout, slots, d->stat_out));
    return DPIR_OK;
}

// The convolution launches of the engine's last forward with taps on (engine.h RouteRec): up to `cap` records into `recs`, the number there
// are into *n_out.
int dpir_debug_route_log(dpir_engine* e, dpir_debug_route_rec* recs, int cap, int* n_out) {
    if (!e || !n_out || (cap > 0 && !recs)) return DPIR_ERR_INVALID;
    *n_out = (int)e->route_log.size();
    for (int i = 0; i < *n_out && i < cap; ++i) {
        const RouteRec& r = e->route_log[i];
        snprintf(recs[i].layer, sizeof recs[i].layer, "%s", r.layer.c_str());
        recs[i].kernel = r.kernel; recs[i].ks = r.ks; recs[i].ksplit = r.ksplit; recs[i].hop = r.hop; recs[i].stat_kind = r.stat_kind;
        recs[i].workgroups = r.workgroups;
    }
    return DPIR_OK;
}

// The planner (csrc/conv_plan.h) without an engine or a GPU: capacities are arguments, knobs == null means the built-in defaults (not the
// environment).
static ConvKnobs knobs_of(const dpir_debug_conv_knobs* k) {
    ConvKnobs o;
    if (!k) return o;
    o.conv8 = k->conv8 != 0; o.conv9 = k->conv9 != 0; o.conv9_min_wg = k->conv9_min_wg; o.conv11 = k->conv11 != 0; o.conv_up = k->conv_up != 0;
    o.split_below = k->split_below; o.split_target = k->split_target; o.fuse_small = k->fuse_small != 0; o.fuse_h1 = k->fuse_h1 != 0;
    o.emit_skip = k->emit_skip;
    return o;
}
static dpir_debug_conv_plan plan_out(const Conv3Plan& p) {
    dpir_debug_conv_plan o;
    o.kernel = p.kernel; o.hop = p.hop; o.geo = p.geo; o.ksplit = p.ksplit; o.chunks_per_split = p.chunks_per_split;
    o.stat_kind = p.stat_kind; o.stat_slots = p.stat_slots; o.refused = p.refusal != nullptr; o.workgroups = p.workgroups;
    return o;
}
void dpir_debug_conv_knobs_default(dpir_debug_conv_knobs* k) {
    const ConvKnobs d;
    *k = dpir_debug_conv_knobs{d.conv8, d.conv9, d.conv9_min_wg, d.conv11, d.conv_up, d.split_below, d.split_target, d.fuse_small, d.fuse_h1, d.emit_skip};
}
int dpir_debug_conv3_plan(const dpir_debug_conv3_query* qs, int n, const dpir_debug_conv_knobs* knobs, int cap7, int cap11, int cap_up, dpir_debug_conv_plan* out) {
    if (!qs || !out || n < 0) return DPIR_ERR_INVALID;
    const ConvKnobs k = knobs_of(knobs);
    const DeviceCaps caps{cap7, cap11, cap_up};
    for (int i = 0; i < n; ++i) {
        const dpir_debug_conv3_query& d = qs[i];
        Conv3Query q;
        q.B = d.B; q.Cin = d.Cin; q.Cout = d.Cout; q.H = d.H; q.W = d.W; q.precision = d.precision; q.grad = d.grad != 0;
        q.w16 = d.w16 != 0; q.w8 = d.w8 != 0; q.w11 = d.w11 != 0; q.conv8_source = d.conv8_source != 0;
        q.slab = d.slab_floats > 0; q.slab_floats = (size_t)d.slab_floats; q.defer = d.defer != 0; q.hop = d.hop != 0; q.has_res = d.has_res != 0;
        q.stat_slots = q.stat_plane = d.stats != 0; q.force_kernel = d.force_kernel;
        out[i] = plan_out(plan_conv3(q, k, caps));
    }
    return DPIR_OK;
}
int dpir_debug_resblock_plan(const dpir_debug_resblock_query* d, const dpir_debug_conv_knobs* knobs, int cap7, int cap11, int cap_up, dpir_debug_resblock_plan_out* out) {
    if (!d || !out) return DPIR_ERR_INVALID;
    ResblockQuery q;
    q.B = d->B; q.Cin = d->Cin; q.Cout = d->Cout; q.H = d->H; q.W = d->W; q.mode = d->mode; q.concat = d->concat != 0; q.has_skip = d->Cin != d->Cout;
    q.gn1_c = d->Cin; q.gn2_c = d->Cout; q.precision = d->precision; q.grad = d->grad != 0;
    q.hop_allowed = d->hop_allowed != 0; q.arena_words_left = (size_t)d->arena_words_left;
    // the packs load_conv (unet.hip) makes for this precision and mode
    const bool f16 = d->precision != 0;
    q.conv1_w16 = q.conv2_w16 = f16; q.skip_w16 = f16 && q.has_skip;
    q.conv1_w11 = d->precision == 1 && conv11_supported(d->Cin, d->Cout, 8, 32); q.conv2_w11 = d->precision == 1 && conv11_supported(d->Cout, d->Cout, 8, 32);
    q.conv1_wup = f16 && d->mode == 1 && d->Cin % 16 == 0 && d->Cout % 32 == 0;
    const int Ho = d->mode == 1 ? d->H * 2 : (d->mode == 2 ? d->H / 2 : d->H), Wo = d->mode == 1 ? d->W * 2 : (d->mode == 2 ? d->W / 2 : d->W);
    q.small_prologue = gn_act_small_supported(d->Cin, d->H, d->W, 0); q.conv5_ok = conv5_supported(d->B, d->Cout, Ho, Wo);
    q.slab = d->slab_floats > 0; q.slab_floats = (size_t)d->slab_floats;
    const ResblockPlan rp = plan_resblock(q, knobs_of(knobs), DeviceCaps{cap7, cap11, cap_up});
    out->up = rp.up; out->skip_emit = rp.skip_emit; out->hop = rp.hop; out->arena_counters = rp.arena_counters;
    out->conv1 = plan_out(rp.conv1); out->conv2 = plan_out(rp.conv2);
    return DPIR_OK;
}

int dpir_debug_conv7_emit_supported(dpir_engine* e, int B, int Cout, int H, int W, int* capacity_out) {
    if (!e) return 0;
    (void)hipSetDevice(e->device);
    if (capacity_out) *capacity_out = device_caps().conv7;
    return conv7_emit_supported(B, Cout, H, W) ? 1 : 0;
}

}  // extern "C"
