// FFT data step (pre_calculate / data_solution, utils/utils_sisr.py:9-19, 65-95): the spectra of a batch, the layout they are stored in and everything
// that depends on it (prox.hip).  The layout is decided in ONE place, prox_layout(); the C ABI, the restoration loop and the kernel files ask this module.
#pragma once
#include <functional>
#include <tuple>
#include "common.h"
#include "elem.h"

struct dpir_engine;

namespace dpir {

// How FB / F2B / FBFy of a ProxState are stored, i.e. which kernel family runs on them
enum class ProxLayout {
    FullBitrev,   // full c2c planes [H][W], bit-reversed along both axes (fft.hip: the general path)
    HalfRows,     // half spectrum, row-major [H][WP], WP = W/2 + 1 padded to the 16-column strip (fft2.hip)
    HalfCols,     // half spectrum, column-major [WP slots][H positions], no padding (fft4.hip: one wave per transform)
    FullDigitrev  // full c2c planes [H][W], digit-reversed along both axes by the mixed-radix plans of H and W (fft_mixed.hip: any size, any sf)
};
// the half layouts store the columns alias-grouped when sf > 1: slot sf q + b holds alias b of fold group q (fft2.hip)

struct ProxState {   // dpir_prox
    int B = 0, H = 0, W = 0, sf = 1;
    ProxLayout layout = ProxLayout::FullBitrev;
    int WP = 0;            // stored row length (complex elements); HalfCols: stored columns (slots) per plane.  A plane is H * WP elements in every layout
    float2* FB = nullptr; float* F2B = nullptr; float2* FBFy = nullptr;
    float* invW = nullptr; // half layouts, sf > 1: alias mean of F2B [B][H/sf][W/sf/2+1]
    const int* slot_col = nullptr; const int* col_slot = nullptr;     // half layouts, sf > 1: device slot maps (engine-owned, ProxCache)
    const std::vector<int>* h_col_slot = nullptr;                     // host copy (prox_read)
    const std::vector<int>* h_perm_h = nullptr; const std::vector<int>* h_perm_w = nullptr;   // FullDigitrev: stored position of frequency f (host, ProxCache)
    bool half() const { return layout == ProxLayout::HalfRows || layout == ProxLayout::HalfCols; }
};

// Engine-owned tables of the prox kernels, built on first use and freed with the engine
struct ProxCache {
    struct SlotMap { int* slot_col = nullptr; int* col_slot = nullptr; std::vector<int> h_slot_col, h_col_slot; };
    std::map<int, float2*> tables;                                // W_N^m (N entries) [+ fft4_wave.h's per-lane constants]; fft.hip's plans read the first half
    std::map<std::tuple<int, int, ProxLayout>, SlotMap> maps;     // (N, sf, layout) -> alias-grouped column permutation of a half layout
    struct Mixed { FftMixedPlan plan; std::vector<int> perm; };
    std::map<std::pair<int, int>, Mixed> mixed;                   // (N, sf) -> radix list and storage permutation (fft_plan.h)
    Status plan(int N, FftPlan* out);
    Status mixed_plan(int N, int sf, MixedFft* out, const std::vector<int>** perm = nullptr);
    Status table(int N, const float2** out);
    Status map(int N, int sf, ProxLayout layout, const SlotMap** out);
    void release();
};

int fft2_padded_width(int W);     // HalfRows: stored row length (fft2.hip's launchers derive it from N the same way)

// The layout a (H, W, sf) problem is stored in on this engine (dpir_set_prox_launch picks between the two half layouts where both exist)
ProxLayout prox_layout(const dpir_engine* e, int H, int W, int sf);
// the same decision from the launch mode alone (dpir_engine::prox_mode), and the shape check that goes with it: no engine, no GPU
ProxLayout prox_layout_of(int prox_mode, int H, int W, int sf);
Status prox_check(ProxLayout layout, int sf, int B, int H, int W);
// *st already fits (B, H, W, sf, layout), or it is released (after a stream synchronisation if it held spectra) and allocated anew; *reallocated tells which.
// The shape checks come first: an unsupported shape leaves *st as it was.  A failed allocation leaves it released.
Status prox_ensure(dpir_engine* e, int sf, int B, int H, int W, ProxState* st, bool* reallocated = nullptr);
void prox_release(ProxState* st);
// FB, F2B, FBFy (and invW) of *st from the measurement y [B,3,H/sf,W/sf] and the PSFs k [B,kh,kw]
Status prox_precalc(dpir_engine* e, const float* y, const float* k, int kh, int kw, ProxState* st);
// every shape check (PSF included), then prox_ensure + prox_precalc on a fresh *st; released again on failure
Status prox_create(dpir_engine* e, const float* y, const float* k, int kh, int kw, int sf, int B, int H, int W, ProxState* st);
// natural-order copy of FB (which 0), F2B (1) or FBFy (2) to the host
Status prox_read(dpir_engine* e, const ProxState& st, int which, void* host_dst, size_t cap_bytes);
// out = blend ? base + g*((ifft)*oa+ob - base) : (ifft)*oa+ob ; input pre-map v = (x*pa+pb)*alpha; sp != null: alpha = sp->tau;
// pil != null (with sp; dpir_run_loop_per_image): alpha = tau of each plane's image from the device loop block, the per-image kernels
Status prox_data_solution(dpir_engine* e, const ProxState& st, const float* x, float pa, float pb, float alpha, float* out, float oa, float ob,
                          const float* blend_base, float g, const StepDev* sp = nullptr, const LoopDev* pil = nullptr);
// The restoration loop's data step on a half layout, fused into three launches: eps -> clamped x0 in the row-FFT prologue, spectral solve between the
// column FFTs, re-noise (+ Philox) in the inverse row-FFT epilogue; x0 is never materialised.  *ran = false (nothing launched) when the step is not eligible.
Status prox_fused_step(dpir_engine* e, const ProxState& st, const dpir_loop_desc& d, bool last, bool with_n1, float* x, const float* out6, float* x0,
                       const StepDev* cur, const LoopDev* lp, bool* ran, bool per_image = false);
// measurement: n back-to-back applies between two events, eagerly or as one captured graph -> device microseconds per apply
Status prox_apply_timed(dpir_engine* e, const ProxState& st, float* x0, float tau, float guidance, int n, bool use_graph, float* us_per_apply);

// api.hip: `record` enqueued on the engine stream under capture (workspace frozen, profiler and taps off) -> an instantiated graph
Status capture_graph(dpir_engine* e, const std::function<Status()>& record, hipGraphExec_t* out);

}  // namespace dpir
