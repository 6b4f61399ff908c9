// fft4: the half-spectrum FFT prox at N = 256 and N = 512 (utils/utils_sisr.py:9-19, 65-95; the headline deblurring / SR configurations) with ONE WAVE PER
// TRANSFORM (fft4_wave.h) and a COLUMN-MAJOR half spectrum [plane][slot][position].  Same mathematics as fft2.hip (row-pair packing, half spectrum,
// closed-form solve between the column transforms), different mapping to the machine (bodies: fft4_body.h):
//   * rows    : a workgroup = 8 waves = 8 pairs of real rows (row r with r + 64): float4 loads, wave-private LDS re-distribution, 256-point FFT in the wave,
//               Hermitian un-packing into an LDS tile [slot][8 + 1] of 16-byte {A[k], B[k]} entries, then FULL 128-byte lines (16 positions of one slot) to memory;
//   * columns : a wave takes one column (2 KB contiguous; position order: two 1 KB wave loads): forward FFT -> closed-form solve on registers whose operands
//               (FBFy, FB, F2B, stored the same way by pre_calculate) are loaded with the column -> inverse FFT -> store.  No workgroup barrier (sf = 1), no strips,
//               no padding columns (129 stored columns instead of fft2's 144);
//   * rows inv: the workgroup loads its 16 positions of columns 0..128 as full lines into the tile, each wave re-packs its pair (Hermitian), inverse FFT, float4
//               epilogue (x*2-1, guidance blend, or the fused re-noise with Philox draws per float4 group exactly as fft2's).
// A batch-16 apply is 6 waves per SIMD in every pass (fft2: 1.5) at 40-57 VGPRs.  Measured 24.9 us per apply against fft2's 33.0.
// sf > 1 keeps fft2's alias-grouped SLOT order (slot sf q + b = alias b of fold group q): a workgroup's four column waves are four consecutive slots, i.e.
// one fold group at sf = 4 and two at sf = 2; the row aliases u + a N/sf of a column live in ONE lane (registers j, since N/sf is a multiple of 64).
#include "fft4_body.h"

namespace dpir {

// the three passes as one launch each (named kernels: they are what the rocprofv3 summaries under profiles/ list) (bodies: fft4_body.h)
template <int N, bool PI = false>
__global__ __launch_bounds__(RTHREADS) void rfft4_rows_kernel(const float* x, float pa, float pb, float pm, const StepDev* sp, float2* out, int NC,
                                                             const float2* tw, RowsFuse fu, const int* slot_col) {
    extern __shared__ __attribute__((aligned(16))) float2 sm4[];
    rows4_body<N, false, PI>(sm4, blockIdx.x, x, pa, pb, pm, sp, out, NC, tw, WaveTwN<N>{}, fu, slot_col);
}
template <int N, bool PI = false>
__global__ __launch_bounds__(RTHREADS) void irfft4_rows_kernel(const float2* in, float* out, float scale, float oa, float ob, const float* blend_base, float g,
                                                              int NC, const float2* tw, RenoiseFuse rn, const int* col_slot) {
    extern __shared__ __attribute__((aligned(16))) float2 sm4[];
    irows4_body<N, false, NoWait4, PI>(sm4, blockIdx.x, in, out, scale, oa, ob, blend_base, g, NC, tw, WaveTwN<N>{}, rn, col_slot, NoWait4{});
}
// grid: P * ceil(NC / 4) workgroups of four waves: one item each
template <int MODE, int SF, int N, bool PI = false>
__global__ __launch_bounds__(THREADS4) void cfft4_cols_kernel(float2* buf, SolveArgs a, int NC, const float2* tw) {
    extern __shared__ __attribute__((aligned(16))) float2 sm4[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = (NC + WAVES - 1) / WAVES;
    int plane, item;
    if (MODE >= 2) {
        // The solve's FB / F2B (/ invW) belong to the IMAGE: the three colour planes of an (image, item) pair read the same 3-6 KB per wave.  Workgroup b runs on
        // XCD b % 8 (own L2), so the pair's three workgroups are numbered 8 apart -- same XCD, dispatched back to back: the second and third hit that L2 instead of
        // fetching the spectra again over the fabric (counter traffic of the batch-16 column pass: 57.2 -> see profiles).  Grid: 3 x (pairs rounded up to 8).
        const int r = blockIdx.x & 7, t = blockIdx.x >> 3;
        const int c = t % 3, pair = 8 * (t / 3) + r;
        const int n = pair / groups;
        if (n >= a.images) return;                                     // padding workgroups (whole workgroup: no barrier is left waiting)
        item = pair - n * groups;
        plane = 3 * n + c;
    } else {
        plane = blockIdx.x / groups;
        item = blockIdx.x - plane * groups;
    }
    const WaveTwN<N> w = wave_tw_load<N>(tw, lane);
    cols4_item_body<MODE, SF, N, NoWait4, PI>(sm4 + wave * wlds(N), sm4 + WAVES * wlds(N), plane, item, wave, buf, a, NC, w, NoWait4{});
}

bool fft4_supported(int H, int W, int sf) { return H == W && (H == 256 || H == 512) && (sf == 1 || sf == 2 || sf == 4); }

static size_t lds4(int N, bool fold, int sf) { return ((size_t)WAVES * wlds(N) + (fold ? (size_t)WAVES * (N / sf) : 0)) * sizeof(float2); }
static size_t lds4_rows(int N, int NC) { return (size_t)RW * wlds(N) * sizeof(float2) + (size_t)NC * TST * sizeof(float4); }

template <int N, bool PI = false>
static Status rows_fwd(hipStream_t s, const float2* tw, const float* x, float pa, float pb, float pm, const StepDev* sp, float2* out, int P, int NC,
                       const float* eps6, int out_ch, const int* slot_col, const LoopDev* pil) {
    const size_t pairs = (size_t)P * N / 2;             // a multiple of RW: no partial workgroup
    static LdsAttrOnce attr;      // dynamic LDS above 64 KB (the 512-point row passes: 8 exchange tiles + the [slot][9] line tile = 74 KB) is allowed per kernel, once
    DPIR_HIP(attr.set(reinterpret_cast<const void*>(rfft4_rows_kernel<N, PI>), 160 * 1024));
    hipLaunchKernelGGL((rfft4_rows_kernel<N, PI>), dim3((unsigned)(pairs / RW)), dim3(RTHREADS), lds4_rows(N, NC), s, x, pa, pb, pm, sp, out, NC, tw,
                       RowsFuse{eps6, out_ch, pil}, slot_col);
    DPIR_HIP(hipGetLastError());
    return Status{};
}
Status launch_rfft4_rows(hipStream_t s, const float2* tw, int N, const float* x, float pa, float pb, float pm, const StepDev* sp, float2* out, int P, int NC,
                         const float* eps6, int out_ch, const int* slot_col, const LoopDev* pil) {
    if (eps6 && !sp) return invalid("rfft4_rows: the fused x0 prologue reads its coefficients from the device step block");
    if (pil && !sp) return invalid("rfft4_rows: the per-image form reads the device step block");
    if (pil && N == 256) return rows_fwd<256, true>(s, tw, x, pa, pb, pm, sp, out, P, NC, eps6, out_ch, slot_col, pil);
    if (pil && N == 512) return rows_fwd<512, true>(s, tw, x, pa, pb, pm, sp, out, P, NC, eps6, out_ch, slot_col, pil);
    if (N == 256) return rows_fwd<256>(s, tw, x, pa, pb, pm, sp, out, P, NC, eps6, out_ch, slot_col, pil);
    if (N == 512) return rows_fwd<512>(s, tw, x, pa, pb, pm, sp, out, P, NC, eps6, out_ch, slot_col, pil);
    return invalid("rfft4_rows: N must be 256 or 512");
}
template <int N, bool PI = false>
static Status rows_inv(hipStream_t s, const float2* tw, const float2* in, float* out, float scale, float oa, float ob, const float* blend, float g, int P,
                       int NC, RenoiseFuse rn, const int* col_slot) {
    const size_t pairs = (size_t)P * N / 2;
    static LdsAttrOnce attr;
    DPIR_HIP(attr.set(reinterpret_cast<const void*>(irfft4_rows_kernel<N, PI>), 160 * 1024));
    hipLaunchKernelGGL((irfft4_rows_kernel<N, PI>), dim3((unsigned)(pairs / RW)), dim3(RTHREADS), lds4_rows(N, N / 2 + 1), s, in, out, scale, oa, ob, blend, g, NC,
                       tw, rn, col_slot);
    DPIR_HIP(hipGetLastError());
    return Status{};
}
Status launch_irfft4_rows(hipStream_t s, const float2* tw, int N, const float2* in, float* out, float scale, float oa, float ob, const float* blend, float g,
                          int P, int NC, const RenoiseFuse& rn, const int* col_slot) {
    if (rn.per_image && !(rn.xt && rn.sp && rn.lp)) return invalid("irfft4_rows: the per-image form is the fused re-noise's");
    if (rn.per_image && N == 256) return rows_inv<256, true>(s, tw, in, out, scale, oa, ob, blend, g, P, NC, rn, col_slot);
    if (rn.per_image && N == 512) return rows_inv<512, true>(s, tw, in, out, scale, oa, ob, blend, g, P, NC, rn, col_slot);
    if (N == 256) return rows_inv<256>(s, tw, in, out, scale, oa, ob, blend, g, P, NC, rn, col_slot);
    if (N == 512) return rows_inv<512>(s, tw, in, out, scale, oa, ob, blend, g, P, NC, rn, col_slot);
    return invalid("irfft4_rows: N must be 256 or 512");
}
template <int N, bool PI = false>
static Status cols(hipStream_t s, const float2* tw, float2* buf, const SolveArgs& a_in, bool solve, int P, int NC) {
    const int groups = (NC + WAVES - 1) / WAVES;
    unsigned grid = (unsigned)(P * groups);
    SolveArgs a = a_in;
    if (solve) {
        if (P % 3) return invalid("cfft4_cols: the solve runs on the three colour planes of every image");
        a.images = P / 3;
        grid = 3u * (unsigned)(((size_t)(P / 3) * groups + 7) / 8 * 8);
    }
    if (!solve) hipLaunchKernelGGL((cfft4_cols_kernel<0, 1, N>), dim3(grid), dim3(THREADS4), lds4(N, false, 1), s, buf, a, NC, tw);
    else if (a.sf == 1) hipLaunchKernelGGL((cfft4_cols_kernel<2, 1, N, PI>), dim3(grid), dim3(THREADS4), lds4(N, false, 1), s, buf, a, NC, tw);
    else {
        if ((a.sf != 2 && a.sf != 4) || !a.invW || !a.slot_col || NC % a.sf) return invalid("cfft4_cols: bad sf > 1 arguments");
        if (a.sf == 2) hipLaunchKernelGGL((cfft4_cols_kernel<3, 2, N, PI>), dim3(grid), dim3(THREADS4), lds4(N, true, 2), s, buf, a, NC, tw);
        else hipLaunchKernelGGL((cfft4_cols_kernel<3, 4, N, PI>), dim3(grid), dim3(THREADS4), lds4(N, true, 4), s, buf, a, NC, tw);
    }
    DPIR_HIP(hipGetLastError());
    return Status{};
}
Status launch_cfft4_cols(hipStream_t s, const float2* tw, int N, float2* buf, const SolveArgs& a, bool solve, int P, int NC) {
    if (a.pil && !(solve && a.sp)) return invalid("cfft4_cols: the per-image form is the solve's and reads the device step block");
    if (a.pil && N == 256) return cols<256, true>(s, tw, buf, a, solve, P, NC);
    if (a.pil && N == 512) return cols<512, true>(s, tw, buf, a, solve, P, NC);
    if (N == 256) return cols<256>(s, tw, buf, a, solve, P, NC);
    if (N == 512) return cols<512>(s, tw, buf, a, solve, P, NC);
    return invalid("cfft4_cols: N must be 256 or 512");
}
}  // namespace dpir
