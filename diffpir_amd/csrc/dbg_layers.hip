// Development-only: the attention core and one GroupNorm site, forward and backward, on caller-supplied host operands
// (include/diffpir_debug.h: dpir_debug_attention, dpir_debug_groupnorm).  Part of libdiffpir_dbg.so, which links against the product
// library: the entries upload the operands, call the product's launchers (launch_attention, launch_attention_bwd, launch_gn_stats,
// launch_gn_prm, launch_gn_bwd) as unet.hip / unet_bwd.hip call them, and download the results.  No kernel lives here.
// Also the two small entries of the operand-range tests: dpir_debug_range_counter and dpir_debug_grad_scale.
//
// Every buffer a kernel writes is allocated with GUARD floats of a fixed bit pattern on either side and is itself filled with the
// pattern (a NaN: an element the kernel left out shows as a non-finite output); the guard words that changed are counted.  Operands
// are allocated at their exact size.
#include "engine.h"
#include "grad.h"
#include "../../include/diffpir_debug.h"
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

namespace {
constexpr size_t GUARD = 256;                    // floats in front of and behind every output buffer
constexpr uint32_t PATTERN = 0x7FA5C3E1u;        // a NaN with a recognisable payload

struct Pool {                                    // frees what the entry allocated, on every return path
    hipStream_t s;
    std::vector<void*> all;
    struct G { uint32_t* base; size_t words; };
    std::vector<G> guarded;
    explicit Pool(hipStream_t st) : s(st) {}
    ~Pool() { for (void* p : all) (void)hipFree(p); }
    // an operand: exact size, uploaded
    template <class T> Status in(const T* host, size_t count, T** dev) {
        void* p = nullptr;
        if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) return Status{DPIR_ERR_NOMEM, "debug entry: hipMalloc of an operand failed"};
        all.push_back(p);
        DPIR_HIP(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, s));
        *dev = reinterpret_cast<T*>(p);
        return Status{};
    }
    // an output: guards on both sides, pattern everywhere; init != null: the buffer's prior contents
    template <class T> Status out(size_t count, T** dev, const T* init = nullptr) {
        static_assert(sizeof(T) % 4 == 0, "outputs are made of 32-bit words");
        const size_t words = count * (sizeof(T) / 4);
        void* p = nullptr;
        if (hipMalloc(&p, (words + 2 * GUARD) * 4) != hipSuccess) return Status{DPIR_ERR_NOMEM, "debug entry: hipMalloc of an output failed"};
        all.push_back(p);
        uint32_t* base = reinterpret_cast<uint32_t*>(p);
        DPIR_HIP(hipMemsetD32Async(p, (int)PATTERN, words + 2 * GUARD, s));
        if (init) DPIR_HIP(hipMemcpyAsync(base + GUARD, init, words * 4, hipMemcpyHostToDevice, s));
        guarded.push_back(G{base, words});
        *dev = reinterpret_cast<T*>(base + GUARD);
        return Status{};
    }
    // guard words that no longer hold the pattern, over every output buffer (after the stream was synchronised)
    Status count_bad(unsigned long long* bad) {
        std::vector<uint32_t> h(GUARD);
        unsigned long long n = 0;
        for (const G& g : guarded)
            for (int side = 0; side < 2; ++side) {
                DPIR_HIP(hipMemcpy(h.data(), g.base + (side ? GUARD + g.words : 0), GUARD * 4, hipMemcpyDeviceToHost));
                for (uint32_t v : h) n += v != PATTERN;
            }
        *bad = n;
        return Status{};
    }
};
}  // namespace

extern "C" {

int dpir_debug_attention(dpir_engine* e, dpir_debug_attention_desc* d) {
    if (!e || !d) return DPIR_ERR_INVALID;
    d->guard_bad_out = 0;
    const int B = d->B, C = d->C, T = d->T;
    if (B <= 0 || C <= 0 || T <= 0 || !d->qkv || !d->out || (d->dAtt && !d->dqkv)) return fail(e, invalid("attention probe: bad descriptor"));
    (void)hipSetDevice(e->device);
    Pool pool(e->stream);
    const size_t nq = (size_t)B * 3 * C * T, na = (size_t)B * C * T;
    float *qkv = nullptr, *out = nullptr;
    API_TRY(e, pool.in(d->qkv, nq, &qkv));
    API_TRY(e, pool.out(na, &out));
    API_TRY(e, launch_attention(e->stream, qkv, out, B, C, T, d->head_ch));
    float *dAtt = nullptr, *dqkv = nullptr, *P = nullptr, *dP = nullptr;
    if (d->dAtt) {
        API_TRY(e, pool.in(d->dAtt, na, &dAtt));
        API_TRY(e, pool.out(nq, &dqkv));
        // the scratch is T x T per (image, head): beyond the launcher's limit (grad.hip: its first statement refuses T > 1024 before any launch) nothing
        // of that size is allocated and the refusal is the launcher's own
        if (T <= 1024 && C % 64 == 0) {
            const size_t np = (size_t)B * (C / 64) * T * T;
            API_TRY(e, pool.out(np, &P));
            API_TRY(e, pool.out(np, &dP));
        }
        API_TRY(e, launch_attention_bwd(e->stream, qkv, dAtt, dqkv, P, dP, B, C, T));
        if (!P) return fail(e, Status{DPIR_ERR_STATE, "attention probe: launch_attention_bwd accepted a shape it documents as refused"});
    }
    API_HIP(e, hipStreamSynchronize(e->stream));
    API_HIP(e, hipMemcpy(d->out, out, na * 4, hipMemcpyDeviceToHost));
    if (dqkv) API_HIP(e, hipMemcpy(d->dqkv, dqkv, nq * 4, hipMemcpyDeviceToHost));
    unsigned long long bad = 0;
    API_TRY(e, pool.count_bad(&bad));
    d->guard_bad_out = bad;
    return DPIR_OK;
}

int dpir_debug_groupnorm(dpir_engine* e, dpir_debug_groupnorm_desc* d) {
    if (!e || !d) return DPIR_ERR_INVALID;
    d->guard_bad_out = 0; d->ns_out = 0;
    const int B = d->B, ca = d->ca, cb = d->cb, Hs = d->Hs, Ws = d->Ws, mode = d->mode, C = ca + cb;
    if (B <= 0 || ca <= 0 || cb < 0 || Hs <= 0 || Ws <= 0 || mode < 0 || mode > 2 || !d->xa || (cb > 0 && !d->xb) || !d->gamma || !d->beta ||
        !d->prm_out || !d->stats_out)
        return fail(e, invalid("groupnorm probe: bad descriptor"));
    if (d->dA && (!d->ga_out || (cb > 0 && !d->gb_out) || (d->acc_a && !d->ga_init) || (cb > 0 && d->acc_b && !d->gb_init)))
        return fail(e, invalid("groupnorm probe: the backward needs ga_out / gb_out, and the prior contents where it accumulates"));
    if (d->dA && d->extra && (mode != 0 || cb != 0)) return fail(e, invalid("groupnorm probe: extra belongs to a mode-0 single source (grad.h)"));
    (void)hipSetDevice(e->device);
    Pool pool(e->stream);
    const int HW = Hs * Ws;
    const size_t na = (size_t)B * ca * HW, nb = (size_t)B * cb * HW;
    float *xa = nullptr, *xb = nullptr, *gamma = nullptr, *beta = nullptr, *film = nullptr;
    API_TRY(e, pool.in(d->xa, na, &xa));
    if (cb) API_TRY(e, pool.in(d->xb, nb, &xb));
    API_TRY(e, pool.in(d->gamma, (size_t)C, &gamma));
    API_TRY(e, pool.in(d->beta, (size_t)C, &beta));
    if (d->film) API_TRY(e, pool.in(d->film, (size_t)B * 2 * C, &film));
    // Fwd::gn (unet.hip): one streaming statistics pass per source tensor, then the table
    GnStatSrc src[2];
    const float* tp[2] = {xa, xb};
    const int tc[2] = {ca, cb};
    for (int k = 0; k < 2; ++k) {
        src[k].c = tc[k];
        if (!tc[k]) continue;
        double2* part = nullptr;
        API_TRY(e, pool.out((size_t)B * tc[k], &part));
        API_TRY(e, launch_gn_stats(e->stream, CatSrc{tp[k], tc[k], nullptr, 0}, B, HW, part));
        src[k].part = part;
    }
    float4* prm = nullptr; float2* stats = nullptr;
    API_TRY(e, pool.out((size_t)B * C, &prm));
    API_TRY(e, pool.out((size_t)B * 32, &stats));
    API_TRY(e, launch_gn_prm(e->stream, src[0], src[1], HW, gamma, beta, film, 2 * C, 0, B, C, d->silu != 0, prm, nullptr, 0, stats));
    float *ga = nullptr, *gb = nullptr;
    if (d->dA) {
        const int Ho = mode == 1 ? Hs * 2 : (mode == 2 ? Hs >> 1 : Hs), Wo = mode == 1 ? Ws * 2 : (mode == 2 ? Ws >> 1 : Ws);
        float *dA = nullptr, *extra = nullptr; double2* sums = nullptr;
        API_TRY(e, pool.in(d->dA, (size_t)B * C * Ho * Wo, &dA));
        if (d->extra) API_TRY(e, pool.in(d->extra, na, &extra));
        const int ns = gn_bwd_parts(C, Hs, Ws);
        API_TRY(e, pool.out((size_t)B * 32 * ns, &sums));
        API_TRY(e, pool.out(na, &ga, d->acc_a ? d->ga_init : nullptr));
        if (cb) API_TRY(e, pool.out(nb, &gb, d->acc_b ? d->gb_init : nullptr));
        GnBwdArgs a;
        a.x = CatSrc{xa, ca, xb, cb}; a.prm = prm; a.stats = stats; a.dA = dA; a.mode = mode; a.Hs = Hs; a.Ws = Ws;
        a.sums = sums; a.ga = ga; a.gb = gb; a.acc_a = d->acc_a; a.acc_b = d->acc_b; a.extra = extra;
        API_TRY(e, launch_gn_bwd(e->stream, a, B));
        d->ns_out = ns;
    }
    API_HIP(e, hipStreamSynchronize(e->stream));
    API_HIP(e, hipMemcpy(d->prm_out, prm, (size_t)B * C * 16, hipMemcpyDeviceToHost));
    API_HIP(e, hipMemcpy(d->stats_out, stats, (size_t)B * 32 * 8, hipMemcpyDeviceToHost));
    if (ga) API_HIP(e, hipMemcpy(d->ga_out, ga, na * 4, hipMemcpyDeviceToHost));
    if (gb) API_HIP(e, hipMemcpy(d->gb_out, gb, nb * 4, hipMemcpyDeviceToHost));
    unsigned long long bad = 0;
    API_TRY(e, pool.count_bad(&bad));
    d->guard_bad_out = bad;
    return DPIR_OK;
}

// The engine's operand range guard word, read (and optionally zeroed) in stream order.  The layer probes synchronise without running the
// guard (only dpir_sync / dpir_d2h check it, only a forward or a loop clears it): this is how a test reads the word behind one probe.
int dpir_debug_range_counter(dpir_engine* e, unsigned long long* count, int clear) {
    if (!e || !count) return DPIR_ERR_INVALID;
    *count = 0;
    if (!e->range_ctr) return fail(e, Status{DPIR_ERR_STATE, "range counter probe: the engine has no guard word"});
    (void)hipSetDevice(e->device);
    API_HIP(e, hipMemcpyAsync(count, e->range_ctr, sizeof(*count), hipMemcpyDeviceToHost, e->stream));
    if (clear) API_HIP(e, hipMemsetAsync(e->range_ctr, 0, sizeof(*count), e->stream));
    API_HIP(e, hipStreamSynchronize(e->stream));
    return DPIR_OK;
}

// launch_grad_scale + launch_grad_unscale (grad.hip) on a host tensor, as unet_bwd.hip chains them around a dgrad convolution -- without the
// convolution, so that what comes back is x[n] * (s_min / s_n).
int dpir_debug_grad_scale(dpir_engine* e, dpir_debug_grad_scale_desc* d) {
    if (!e || !d) return DPIR_ERR_INVALID;
    d->guard_bad_out = 0; d->parts_out = 0;
    const int B = d->B, C = d->C;
    if (B <= 0 || C <= 0 || d->per_img <= 0 || !d->x || !d->sn_out || !d->scal_out || !d->prm_out || !d->x_out)
        return fail(e, invalid("grad scale probe: bad descriptor"));
    (void)hipSetDevice(e->device);
    Pool pool(e->stream);
    const size_t per = (size_t)d->per_img, n = (size_t)B * per;
    const int parts = grad_scale_parts(B);
    float *x = nullptr, *part = nullptr, *scal = nullptr, *sn = nullptr; float4* prm = nullptr;
    API_TRY(e, pool.out(n, &x, d->x));
    API_TRY(e, pool.out((size_t)B * parts, &part));
    API_TRY(e, pool.out((size_t)2, &scal));
    API_TRY(e, pool.out((size_t)2 * B, &sn));
    API_TRY(e, pool.out((size_t)B * C, &prm));
    API_TRY(e, launch_grad_scale(e->stream, x, B, per, part, scal, sn, prm, C));
    API_TRY(e, launch_grad_unscale(e->stream, x, B, per, sn + B));
    API_HIP(e, hipStreamSynchronize(e->stream));
    API_HIP(e, hipMemcpy(d->sn_out, sn, (size_t)2 * B * 4, hipMemcpyDeviceToHost));
    API_HIP(e, hipMemcpy(d->scal_out, scal, 8, hipMemcpyDeviceToHost));
    API_HIP(e, hipMemcpy(d->prm_out, prm, (size_t)B * C * 16, hipMemcpyDeviceToHost));
    API_HIP(e, hipMemcpy(d->x_out, x, n * 4, hipMemcpyDeviceToHost));
    d->parts_out = parts;
    unsigned long long bad = 0;
    API_TRY(e, pool.count_bad(&bad));
    d->guard_bad_out = bad;
    return DPIR_OK;
}

}  // extern "C"
