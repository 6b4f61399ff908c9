// FFT data step of the restoration (pre_calculate / data_solution, utils/utils_sisr.py:9-19, 65-95) above the kernel files: which layout the spectra
// of a (H, W, sf) problem are stored in (prox_layout -- the one place that asks fft2_supported / fft4_supported / the engine's prox mode), their
// allocation, the engine-owned tables, pre_calculate, the apply on each layout, the loop's fused step and the host reader.  The kernels live in
// fft.hip (FullBitrev), fft2.hip (HalfRows), fft4.hip (HalfCols) and fft_mixed.hip (FullDigitrev); what the two half layouts share beyond the passes
// (slot map, alias fold) is here.
//
// Shapes: 64^2, 256^2 and 512^2 at sf 1 / 2 / 4 take a half layout; every other power-of-two H in [16, 1024] x W in [16, 2048] at sf 1 / 2 / 4 / 8 /
// 16 takes FullBitrev; whatever those three refuse -- H or W no power of two, or another sf -- takes, under launch modes 2 and 3 (3 is the default;
// modes 0 and 1 keep refusing it with DPIR_ERR_UNSUPPORTED, dpir_set_prox_launch), FullDigitrev: H in [8, 1024], W in [8, 2048], no
// prime factor above 31, any sf in [1, 16] that divides both (fft_plan.h).  Every shape the first three served keeps its layout and its kernels.
#include "engine.h"
#include "fft4_body.h"
#include <math.h>
#include <string.h>

namespace dpir {

// ------------------------------------------------------------------------------------------ layout
static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
ProxLayout prox_layout_of(int prox_mode, int H, int W, int sf) {
    if (fft2_supported(H, W, sf)) return (prox_mode & 1) && fft4_supported(H, W, sf) ? ProxLayout::HalfCols : ProxLayout::HalfRows;
    const bool sf_pow2 = sf == 1 || sf == 2 || sf == 4 || sf == 8 || sf == 16;
    // bit 1 of the launch mode admits the mixed-radix layout; without it the generic power-of-two kernels are asked, and refuse, as before.
    // prox_check refuses a non-divisor on every layout
    return (pow2(H) && pow2(W) && sf_pow2) || !(prox_mode & 2) ? ProxLayout::FullBitrev : ProxLayout::FullDigitrev;
}
ProxLayout prox_layout(const dpir_engine* e, int H, int W, int sf) { return prox_layout_of(e->prox_mode, H, W, sf); }
int fft2_padded_width(int W) { const int cs = 16; return (W / 2 + 1 + cs - 1) / cs * cs; }   // multiple of the column strip
// ProxState::WP.  HalfCols: W/2 + 1 stored columns for sf = 1, sf * (W/sf/2 + 1) alias-grouped slots otherwise; the position of row u inside one: pos4(u) (fft4_body.h)
static int stored_width(ProxLayout L, int W, int sf) {
    if (L == ProxLayout::HalfCols) return sf == 1 ? W / 2 + 1 : sf * (W / sf / 2 + 1);
    return L == ProxLayout::HalfRows ? fft2_padded_width(W) : W;      // both full layouts store W columns
}

// sf > 1 on a half layout: slot -> (column | mirrored << 16) or -1 (padding), and column -> canonical slot, for `slots` stored columns
static void build_slot_map(int N, int sf, int slots, std::vector<int>& slot_col, std::vector<int>& col_slot) {
    const int Ws = N / sf;
    slot_col.assign(slots, -1);
    col_slot.assign(N / 2 + 1, -1);
    for (int q = 0; q <= Ws / 2; ++q)
        for (int b = 0; b < sf; ++b) {
            const int c = q + b * Ws;
            if (c >= N) continue;
            const int col = c <= N / 2 ? c : N - c, mir = c <= N / 2 ? 0 : 1;
            slot_col[sf * q + b] = col | (mir << 16);
            if (col_slot[col] < 0 || (!mir && (slot_col[col_slot[col]] >> 16))) col_slot[col] = sf * q + b;      // prefer the direct copy
        }
}

// invW[n, p, q] = mean over the sf x sf aliases of F2B (utils_sisr.py:71 `invW = mean(splits(F2B))`), from the alias-grouped half layout of NS slots
template <bool COLS>
__global__ void fold_f2b_kernel(const float* F2B, const int* slot_col, int N, int NS, int sf, float* invW, size_t total) {
    const int Hs = N / sf, QW = N / sf / 2 + 1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % QW);
        const int p = (int)((i / QW) % Hs);
        const size_t n = i / ((size_t)QW * Hs);
        const float* pl = F2B + n * (size_t)N * NS;
        // pairwise over the sf x sf aliases (sf 2 or 4), as the solve sums FB * FR (fft_regs.h, tree_sum)
        auto alias_col = [&](int b) -> float {
            const int slot = sf * q + b;
            const int cm = slot < NS ? slot_col[slot] : -1;
            if (cm < 0) return 0.f;
            const int base_row = (cm >> 16) ? (Hs - p) % Hs : p;          // |FB|^2 is real: the mirrored alias is just the mirrored row
            auto at = [&](int a) {
                const int u = base_row + a * Hs;
                return COLS ? pl[(size_t)slot * N + pos4(u)] : pl[(size_t)u * NS + slot];
            };
            return sf == 2 ? at(0) + at(1) : (at(0) + at(1)) + (at(2) + at(3));
        };
        const float acc = sf == 2 ? alias_col(0) + alias_col(1) : (alias_col(0) + alias_col(1)) + (alias_col(2) + alias_col(3));
        invW[i] = acc / (float)(sf * sf);
    }
}

// ------------------------------------------------------------------------------------------ engine-owned tables
static int ilog2u(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

template <class T> static Status upload(const std::vector<T>& h, T** dev) {
    DPIR_HIP(hipMalloc((void**)dev, h.size() * sizeof(T)));
    DPIR_HIP(hipMemcpy(*dev, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return Status{};
}

// W_N^m, m < N (fft.hip reads the first half), for N = 256 / 512 followed by fft4_wave.h's per-lane constants
Status ProxCache::table(int N, const float2** out) {
    auto it = tables.find(N);
    if (it == tables.end()) {
        std::vector<float2> tw(N);
        for (int m = 0; m < N; ++m) {
            double a = -2.0 * M_PI * (double)m / (double)N;
            tw[m] = make_float2((float)cos(a), (float)sin(a));
        }
        if (N == 256 || N == 512) { tw.resize(N + wave_tw_count(N)); wave_tw_fill(N, tw.data(), tw.data() + N); }
        float2* d = nullptr;
        DPIR_TRY(upload(tw, &d));
        it = tables.emplace(N, d).first;
    }
    *out = it->second;
    return Status{};
}
Status ProxCache::plan(int N, FftPlan* out) {
    if (N < 2 || (N & (N - 1))) return Status{DPIR_ERR_UNSUPPORTED, "FFT size must be a power of two"};
    const float2* tw = nullptr;
    DPIR_TRY(table(N, &tw));
    out->N = N; out->logN = ilog2u(N); out->tw = const_cast<float2*>(tw);
    return Status{};
}

Status ProxCache::mixed_plan(int N, int sf, MixedFft* out, const std::vector<int>** perm) {
    auto it = mixed.find({N, sf});
    if (it == mixed.end()) {
        Mixed m;
        if (!fft_plan_make(N, sf, &m.plan)) return Status{DPIR_ERR_UNSUPPORTED, "mixed fft: no plan for this length and sf"};
        fft_plan_perm(m.plan, m.perm);
        it = mixed.emplace(std::make_pair(N, sf), std::move(m)).first;
    }
    const float2* tw = nullptr;
    DPIR_TRY(table(N, &tw));
    out->plan = it->second.plan; out->tw = tw;
    if (perm) *perm = &it->second.perm;
    return Status{};
}

Status ProxCache::map(int N, int sf, ProxLayout layout, const SlotMap** out) {
    auto key = std::make_tuple(N, sf, layout);
    auto it = maps.find(key);
    if (it == maps.end()) {
        SlotMap m;
        build_slot_map(N, sf, stored_width(layout, N, sf), m.h_slot_col, m.h_col_slot);
        DPIR_TRY(upload(m.h_slot_col, &m.slot_col));
        DPIR_TRY(upload(m.h_col_slot, &m.col_slot));
        it = maps.emplace(key, std::move(m)).first;
    }
    *out = &it->second;
    return Status{};
}

void ProxCache::release() {
    for (auto& kv : tables) (void)hipFree(kv.second);
    for (auto& kv : maps) { (void)hipFree(kv.second.slot_col); (void)hipFree(kv.second.col_slot); }
}

// ------------------------------------------------------------------------------------------ shape checks, allocation
// The generic kernels (fft.hip) hold a 16-column strip of H + 1 rows in LDS: H <= 1024 (135 KB at 1024; 2048 would need 264 KB of the 160 KB per CU).
// The mixed-radix kernels (fft_mixed.hip) hold the same strip (at most 16 columns) and lift the power-of-two conditions: fft_mixed_refusal.
Status prox_check(ProxLayout layout, int sf, int B, int H, int W) {
    if (B < 1) return invalid("pre_calculate: B must be >= 1");
    if (sf < 1 || H % sf || W % sf) return invalid("pre_calculate: image size not divisible by sf");
    if (layout == ProxLayout::FullDigitrev) {
        char msg[192];
        bool unsupported = true;
        if (fft_mixed_refusal(H, W, sf, &unsupported, msg, sizeof msg)) return Status{unsupported ? DPIR_ERR_UNSUPPORTED : DPIR_ERR_INVALID, msg};
        return Status{};
    }
    if (layout != ProxLayout::FullBitrev) return Status{};
    if (sf != 1 && sf != 2 && sf != 4 && sf != 8 && sf != 16) return Status{DPIR_ERR_UNSUPPORTED, "fft prox: sf must be 1, 2, 4, 8 or 16"};
    if (!pow2(H) || !pow2(W) || H < 16 || W < 16 || H > 1024 || W > 2048)
        return Status{DPIR_ERR_UNSUPPORTED, "fft prox: H must be a power of two in [16, 1024] and W one in [16, 2048]"};
    return Status{};
}

static Status prox_check_psf(int kh, int kw, int H, int W) {
    if (kh < 1 || kw < 1) return invalid("pre_calculate: empty PSF");
    if (kh > H || kw > W) return invalid("PSF larger than the image");
    return Status{};
}

void prox_release(ProxState* st) {
    if (st->FB) (void)hipFree(st->FB);
    if (st->F2B) (void)hipFree(st->F2B);
    if (st->FBFy) (void)hipFree(st->FBFy);
    if (st->invW) (void)hipFree(st->invW);
    st->FB = nullptr; st->F2B = nullptr; st->FBFy = nullptr; st->invW = nullptr;
}

static Status prox_alloc(dpir_engine* e, ProxState* st) {
    const size_t hw = (size_t)st->H * st->WP, B = st->B;
    if (hipMalloc((void**)&st->FB, B * hw * sizeof(float2)) != hipSuccess ||
        hipMalloc((void**)&st->F2B, B * hw * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&st->FBFy, 3 * B * hw * sizeof(float2)) != hipSuccess)
        return Status{DPIR_ERR_NOMEM, "pre_calculate: hipMalloc failed"};
    if (st->layout == ProxLayout::FullDigitrev) {
        MixedFft f;
        DPIR_TRY(e->prox_cache.mixed_plan(st->H, st->sf, &f, &st->h_perm_h));
        DPIR_TRY(e->prox_cache.mixed_plan(st->W, st->sf, &f, &st->h_perm_w));
    }
    if (st->half() && st->sf > 1) {
        const ProxCache::SlotMap* m = nullptr;
        DPIR_TRY(e->prox_cache.map(st->W, st->sf, st->layout, &m));
        st->slot_col = m->slot_col; st->col_slot = m->col_slot; st->h_col_slot = &m->h_col_slot;
        if (hipMalloc((void**)&st->invW, B * (st->H / st->sf) * (st->W / st->sf / 2 + 1) * sizeof(float)) != hipSuccess)
            return Status{DPIR_ERR_NOMEM, "pre_calculate: hipMalloc failed"};
    }
    return Status{};
}

Status prox_ensure(dpir_engine* e, int sf, int B, int H, int W, ProxState* st, bool* reallocated) {
    if (reallocated) *reallocated = false;
    const ProxLayout layout = prox_layout(e, H, W, sf);       // sf and the launch mode decide the layout: a change of either re-allocates too
    DPIR_TRY(prox_check(layout, sf, B, H, W));
    if (st->FB && st->B == B && st->H == H && st->W == W && st->sf == sf && st->layout == layout) return Status{};
    if (reallocated) *reallocated = true;
    if (st->FB) DPIR_HIP(hipStreamSynchronize(e->stream));    // queued work may still read the spectra that go
    prox_release(st);
    *st = ProxState{};
    st->B = B; st->H = H; st->W = W; st->sf = sf; st->layout = layout; st->WP = stored_width(layout, W, sf);
    Status s = prox_alloc(e, st);
    if (!s.ok()) prox_release(st);
    return s;
}

// ------------------------------------------------------------------------------------------ the half-spectrum passes, whichever kernels run them
static Status half_rows_fwd(hipStream_t s, const ProxState& st, const float2* tw, const float* x, float pa, float pb, float pm, const StepDev* sp, float2* out,
                            int P, RowsFuse fu) {
    if (st.layout == ProxLayout::HalfCols) return launch_rfft4_rows(s, tw, st.W, x, pa, pb, pm, sp, out, P, st.WP, fu.eps6, fu.out_ch, st.slot_col, fu.pil);
    return launch_rfft_rows(s, tw, x, pa, pb, pm, sp, out, P, st.W, fu.eps6, fu.out_ch, st.slot_col, fu.pil);
}
// solve == null: plain forward column transforms (pre_calculate)
static Status half_cols(hipStream_t s, const ProxState& st, const float2* tw, float2* buf, const SolveArgs* solve, int P) {
    const SolveArgs a = solve ? *solve : SolveArgs{};
    if (st.layout == ProxLayout::HalfCols) return launch_cfft4_cols(s, tw, st.W, buf, a, solve != nullptr, P, st.WP);
    return launch_cfft_cols(s, tw, buf, a, solve != nullptr, P, st.H);
}
static Status half_rows_inv(hipStream_t s, const ProxState& st, const float2* tw, const float2* in, float* out, float scale, float oa, float ob,
                            const float* blend_base, float g, int P, const RenoiseFuse& rn) {
    if (st.layout == ProxLayout::HalfCols) return launch_irfft4_rows(s, tw, st.W, in, out, scale, oa, ob, blend_base, g, P, st.WP, rn, st.col_slot);
    return launch_irfft_rows(s, tw, in, out, scale, oa, ob, blend_base, g, P, st.W, rn, st.col_slot);
}
static Status half_fold(hipStream_t s, const ProxState& st) {
    if (st.sf != 2 && st.sf != 4) return invalid("fold_f2b: sf must be 2 or 4");
    const int N = st.W;
    const size_t total = (size_t)st.B * (N / st.sf) * (N / st.sf / 2 + 1);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    if (st.layout == ProxLayout::HalfCols) hipLaunchKernelGGL(fold_f2b_kernel<true>, grid, block, 0, s, st.F2B, st.slot_col, N, st.WP, st.sf, st.invW, total);
    else hipLaunchKernelGGL(fold_f2b_kernel<false>, grid, block, 0, s, st.F2B, st.slot_col, N, st.WP, st.sf, st.invW, total);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

// ------------------------------------------------------------------------------------------ pre_calculate
Status prox_precalc(dpir_engine* e, const float* y, const float* k, int kh, int kw, ProxState* st) {
    const int sf = st->sf, B = st->B, H = st->H, W = st->W;
    DPIR_TRY(prox_check_psf(kh, kw, H, W));
    hipStream_t s = e->stream;
    ProfScope ps(&e->prof, PC_FFT);
    if (st->half()) {
        // FB = rfft2(p2o-embedded PSF), FBFy = conj(FB) * rfft2(y)
        const float2* tw = nullptr;
        DPIR_TRY(e->prox_cache.table(W, &tw));
        float* psf = nullptr;
        DPIR_TRY(e->ws.getT("prox#psf", (size_t)B * H * W, &psf));
        DPIR_TRY(launch_psf_embed_real(s, k, kh, kw, psf, B, H, W));
        DPIR_TRY(half_rows_fwd(s, *st, tw, psf, 1.f, 0.f, 1.f, nullptr, st->FB, B, RowsFuse{}));
        DPIR_TRY(half_cols(s, *st, tw, st->FB, nullptr, B));
        const float* ysrc = y;
        if (sf > 1) {      // F(zero-stuffed y) (utils_sisr.py:84-85)
            float* yup = nullptr;
            DPIR_TRY(e->ws.getT("prox#yup", (size_t)B * 3 * H * W, &yup));
            DPIR_TRY(launch_upsample_real(s, y, sf, yup, B * 3, H / sf, W / sf));
            ysrc = yup;
        }
        DPIR_TRY(half_rows_fwd(s, *st, tw, ysrc, 1.f, 0.f, 1.f, nullptr, st->FBFy, B * 3, RowsFuse{}));
        DPIR_TRY(half_cols(s, *st, tw, st->FBFy, nullptr, B * 3));
        DPIR_TRY(launch_precalc_finish2(s, st->FB, st->FBFy, st->F2B, B, (size_t)H * st->WP));
        if (sf > 1) DPIR_TRY(half_fold(s, *st));
        return Status{};
    }
    if (st->layout == ProxLayout::FullDigitrev) {      // the same passes as below on the mixed-radix plans of H and W
        MixedFft mh, mw;
        DPIR_TRY(e->prox_cache.mixed_plan(H, sf, &mh));
        DPIR_TRY(e->prox_cache.mixed_plan(W, sf, &mw));
        DPIR_TRY(launch_psf_embed(s, k, kh, kw, st->FB, B, H, W));
        DPIR_TRY(launch_mixed_rows_fwd(s, mw, st->FB, nullptr, 1.f, 0.f, 1.f, B, H, W));
        DPIR_TRY(launch_mixed_cols(s, mh, st->FB, B, H, W, sf));
        DPIR_TRY(launch_upsample_embed(s, y, sf, st->FBFy, B * 3, H / sf, W / sf));
        DPIR_TRY(launch_mixed_rows_fwd(s, mw, st->FBFy, nullptr, 1.f, 0.f, 1.f, B * 3, H, W));
        DPIR_TRY(launch_mixed_cols(s, mh, st->FBFy, B * 3, H, W, sf));
        DPIR_TRY(launch_precalc_finish(s, st->FB, st->FBFy, st->F2B, B, H, W));
        return Status{};
    }
    FftPlan ph, pw;
    DPIR_TRY(e->prox_cache.plan(H, &ph));
    DPIR_TRY(e->prox_cache.plan(W, &pw));
    DPIR_TRY(launch_psf_embed(s, k, kh, kw, st->FB, B, H, W));
    DPIR_TRY(launch_fft_rows(s, pw, st->FB, nullptr, 1.f, 0.f, B, H, W, false));
    DPIR_TRY(launch_fft_cols(s, ph, st->FB, B, H, W, false));
    DPIR_TRY(launch_upsample_embed(s, y, sf, st->FBFy, B * 3, H / sf, W / sf));
    DPIR_TRY(launch_fft_rows(s, pw, st->FBFy, nullptr, 1.f, 0.f, B * 3, H, W, false));
    DPIR_TRY(launch_fft_cols(s, ph, st->FBFy, B * 3, H, W, false));
    DPIR_TRY(launch_precalc_finish(s, st->FB, st->FBFy, st->F2B, B, H, W));
    return Status{};
}

Status prox_create(dpir_engine* e, const float* y, const float* k, int kh, int kw, int sf, int B, int H, int W, ProxState* st) {
    DPIR_TRY(prox_check(prox_layout(e, H, W, sf), sf, B, H, W));      // every shape check before anything is allocated
    DPIR_TRY(prox_check_psf(kh, kw, H, W));
    Status s = prox_ensure(e, sf, B, H, W, st);
    if (s.ok()) s = prox_precalc(e, y, k, kh, kw, st);
    if (!s.ok()) prox_release(st);
    return s;
}

// ------------------------------------------------------------------------------------------ host reader
static unsigned brev(unsigned v, int bits) {
    unsigned r = 0;
    for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

// where element (u, v) of a natural-order plane is stored inside its H * WP plane, and whether the stored value is its conjugate
static size_t stored_index(const ProxState& st, int u, int v, bool* conj) {
    *conj = false;
    if (st.layout == ProxLayout::FullDigitrev)      // digit-reversed along both axes (fft_plan.h): natural[u][v] = stored[perm_H(u)][perm_W(v)]
        return (size_t)(*st.h_perm_h)[u] * st.W + (*st.h_perm_w)[v];
    if (!st.half())      // bit-reversed along both axes (fft.hip): natural[u][v] = stored[brev(u)][brev(v)]
        return (size_t)brev(u, ilog2u(st.H)) * st.W + brev(v, ilog2u(st.W));
    // natural[u][v] = stored[u][v] for v <= W/2, conj(stored[(H-u)%H][W-v]) beyond (Hermitian spectra of real signals)
    const bool mir = v > st.W / 2;
    const int su = mir ? (st.H - u) % st.H : u;
    int sv = mir ? st.W - v : v;
    if (st.h_col_slot) sv = (*st.h_col_slot)[sv];           // sf > 1: alias-grouped column order
    *conj = mir;
    return st.layout == ProxLayout::HalfCols ? (size_t)sv * st.H + pos4(su) : (size_t)su * st.WP + sv;
}

Status prox_read(dpir_engine* e, const ProxState& st, int which, void* host_dst, size_t cap_bytes) {
    if (which < 0 || which > 2) return invalid("dpir_prox_read: which must be 0, 1 or 2");
    const size_t hw = (size_t)st.H * st.W, shw = (size_t)st.H * st.WP;
    const size_t planes = which == 2 ? (size_t)3 * st.B : (size_t)st.B;
    const size_t esz = which == 1 ? sizeof(float) : sizeof(float2);
    if (cap_bytes < planes * hw * esz) return invalid("dpir_prox_read: destination too small");
    std::vector<char> tmp(planes * shw * esz);
    const void* src = which == 0 ? (const void*)st.FB : (which == 1 ? (const void*)st.F2B : (const void*)st.FBFy);
    if (int rc = dpir_d2h(e, tmp.data(), src, tmp.size())) return Status{rc, e->last_error};
    for (size_t pl = 0; pl < planes; ++pl)
        for (int u = 0; u < st.H; ++u)
            for (int v = 0; v < st.W; ++v) {
                bool conj = false;
                const size_t at = stored_index(st, u, v, &conj);
                char* dp = reinterpret_cast<char*>(host_dst) + (pl * hw + (size_t)u * st.W + v) * esz;
                memcpy(dp, tmp.data() + (pl * shw + at) * esz, esz);
                if (conj && which != 1) reinterpret_cast<float*>(dp)[1] = -reinterpret_cast<float*>(dp)[1];
            }
    return Status{};
}

// ------------------------------------------------------------------------------------------ data_solution
// What one apply on a half layout differs in from another; everything else (table, spectrum workspace, the state's spectra and slot maps, the
// 1 / (H W) of the inverse) prox_passes takes from the ProxState
struct ProxPassArgs {
    const float* x; float pa, pb, alpha; const StepDev* sp; RowsFuse fu;               // rows forward: v = (x*pa+pb)*alpha, or the fused eps -> x0 prologue; sp != null: alpha = sp->tau
    float* out; float oa, ob; const float* blend_base; float g; RenoiseFuse rn;        // rows inverse: out = (ifft)*oa+ob [blended with base by g], or the fused re-noise
};
// rows forward -> columns with the solve -> rows inverse
static Status prox_passes(dpir_engine* e, const ProxState& st, const ProxPassArgs& a) {
    const float2* tw = nullptr;
    DPIR_TRY(e->prox_cache.table(st.W, &tw));
    float2* hbuf = nullptr;
    DPIR_TRY(e->ws.getT("prox#hbuf", (size_t)st.B * 3 * st.H * st.WP, &hbuf));
    hipStream_t s = e->stream;
    ProfScope ps(&e->prof, PC_FFT);
    const int P = st.B * 3;
    SolveArgs solve{st.FB, st.F2B, st.FBFy, a.alpha, st.sf, a.sp, st.invW, st.slot_col};
    solve.pil = a.fu.pil;                   // both uses of tau (the row scale and the solve's alpha) take the same image's value
    DPIR_TRY(half_rows_fwd(s, st, tw, a.x, a.pa, a.pb, a.alpha, a.sp, hbuf, P, a.fu));
    DPIR_TRY(half_cols(s, st, tw, hbuf, &solve, P));
    return half_rows_inv(s, st, tw, hbuf, a.out, 1.0f / ((float)st.H * (float)st.W), a.oa, a.ob, a.blend_base, a.g, P, a.rn);
}

Status prox_data_solution(dpir_engine* e, const ProxState& st, const float* x, float pa, float pb, float alpha, float* out, float oa, float ob,
                          const float* blend_base, float g, const StepDev* sp, const LoopDev* pil) {
    if (!sp && !(alpha > 0.f)) return invalid("data_solution: alpha must be > 0");
    if (pil && !sp) return invalid("data_solution: the per-image form reads the device step block");
    if (st.half())
        return prox_passes(e, st, ProxPassArgs{x, pa, pb, alpha, sp, RowsFuse{nullptr, 0, pil}, out, oa, ob, (blend_base && g != 1.0f) ? blend_base : nullptr, g, RenoiseFuse{}});
    float2* buf = nullptr;
    DPIR_TRY(e->ws.getT("prox#buf", (size_t)st.B * 3 * st.H * st.W, &buf));
    hipStream_t s = e->stream;
    const float scale_hw = 1.0f / ((float)st.H * (float)st.W);
    if (st.layout == ProxLayout::FullDigitrev) {
        MixedFft mh, mw;
        DPIR_TRY(e->prox_cache.mixed_plan(st.H, st.sf, &mh));
        DPIR_TRY(e->prox_cache.mixed_plan(st.W, st.sf, &mw));
        ProfScope ps(&e->prof, PC_FFT);
        DPIR_TRY(launch_mixed_rows_fwd(s, mw, buf, x, pa, pb, alpha, st.B * 3, st.H, st.W, sp, pil));
        SolveArgs a{st.FB, st.F2B, st.FBFy, alpha, st.sf, sp};
        a.pil = pil;
        DPIR_TRY(launch_mixed_cols_solve(s, mh, buf, a, st.B, st.H, st.W));
        return launch_mixed_rows_inv(s, mw, buf, out, scale_hw, oa, ob, blend_base, g, st.B * 3, st.H, st.W);
    }
    FftPlan ph, pw;
    DPIR_TRY(e->prox_cache.plan(st.H, &ph));
    DPIR_TRY(e->prox_cache.plan(st.W, &pw));
    ProfScope ps(&e->prof, PC_FFT);
    DPIR_TRY(launch_fft_rows_real3(s, pw, buf, x, pa, pb, alpha, st.B * 3, st.H, st.W, sp, pil));
    SolveArgs a{st.FB, st.F2B, st.FBFy, alpha, st.sf, sp};
    a.pil = pil;
    DPIR_TRY(launch_fft_cols_solve(s, ph, buf, a, st.B, st.H, st.W));
    DPIR_TRY(launch_ifft_rows_real(s, pw, buf, out, scale_hw, oa, ob, blend_base, g, st.B * 3, st.H, st.W));
    return Status{};
}

Status prox_fused_step(dpir_engine* e, const ProxState& st, const dpir_loop_desc& d, bool last, bool with_n1, float* x, const float* out6, float* x0,
                       const StepDev* cur, const LoopDev* lp, bool* ran, bool per_image) {
    *ran = !last && d.generate_mode == 0 && !d.first_order && (d.task == DPIR_TASK_DEBLUR || d.task == DPIR_TASK_SR_BLUR) && st.half() && d.guidance == 1.0f;
    if (!*ran) return Status{};
    if (with_n1 && d.noise_n1_dev && !d.noise_n2_dev) return invalid("host n1 noise requires host n2 noise");
    const size_t total = (size_t)st.B * 3 * st.H * st.W;
    const RenoiseFuse rn{x, cur, lp, d.noise_n1_dev, d.noise_n2_dev, d.noise_n2_dev ? total : 0, with_n1 ? 1 : 0, per_image ? 1 : 0};
    DPIR_TRY(prox_passes(e, st, ProxPassArgs{x, 0.5f, 0.5f, 1.f, cur, RowsFuse{out6, e->net.desc.out_channels, per_image ? lp : nullptr}, x0, 2.f, -1.f, nullptr, 1.f, rn}));
    DPIR_HIP(hipGetLastError());
    return Status{};
}

// ------------------------------------------------------------------------------------------ measurement
// n back-to-back applies between two events on the engine stream, eagerly or as ONE captured graph (what the restoration loop replays: no host launch
// cost, no per-apply event records) -> device microseconds per apply, launch boundaries included
Status prox_apply_timed(dpir_engine* e, const ProxState& st, float* x0, float tau, float guidance, int n, bool use_graph, float* us_per_apply) {
    auto apply_n = [&](int reps) {
        Status s;
        for (int i = 0; i < reps && s.ok(); ++i) s = prox_data_solution(e, st, x0, 0.5f, 0.5f, tau, x0, 2.f, -1.f, x0, guidance);
        return s;
    };
    DPIR_TRY(apply_n(1));       // allocates the workspace, warms the code
    struct Scope {              // whatever the way out: events and graph destroyed, profiler back on
        dpir_engine* e; bool prof_on; hipEvent_t ev0 = nullptr, ev1 = nullptr; hipGraphExec_t exec = nullptr;
        ~Scope() {
            e->prof.on = prof_on;
            if (exec) (void)hipGraphExecDestroy(exec);
            if (ev0) (void)hipEventDestroy(ev0);
            if (ev1) (void)hipEventDestroy(ev1);
        }
    } sc{e, e->prof.on};
    DPIR_HIP(hipEventCreate(&sc.ev0));
    DPIR_HIP(hipEventCreate(&sc.ev1));
    e->prof.on = false;
    if (use_graph) {
        DPIR_TRY(capture_graph(e, [&] { return apply_n(n); }, &sc.exec));
        if (hipGraphLaunch(sc.exec, e->stream) != hipSuccess) return Status{DPIR_ERR_HIP, "hipGraphLaunch failed"};      // warm-up replay
    }
    Status s;
    (void)hipEventRecord(sc.ev0, e->stream);
    if (use_graph) { if (hipGraphLaunch(sc.exec, e->stream) != hipSuccess) s = Status{DPIR_ERR_HIP, "hipGraphLaunch failed"}; }
    else s = apply_n(n);
    (void)hipEventRecord(sc.ev1, e->stream);
    if (hipEventSynchronize(sc.ev1) != hipSuccess) s = Status{DPIR_ERR_HIP, "hipEventSynchronize failed"};
    float ms = 0.f;
    if (s.ok() && hipEventElapsedTime(&ms, sc.ev0, sc.ev1) == hipSuccess) *us_per_apply = ms * 1e3f / (float)n;
    return s;
}

}  // namespace dpir
