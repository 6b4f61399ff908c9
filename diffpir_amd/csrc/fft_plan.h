// The planner of the mixed-radix LDS transforms (fft_mixed.hip) and of the layout their spectra are stored in (ProxLayout::FullDigitrev): which
// lengths are served, the radix list of a length, the storage permutation, and the column strips of the solve.  The launchers, prox.hip's shape
// checks and host reader, and the probes (dpir_debug_fft_plan / dpir_debug_prox_layout) all ask here.  Plain C++: no HIP call, so the whole plan runs
// -- and is tested -- on a machine without a GPU.
//
// Forward transforms are decimation in frequency in place (natural in, digit-reversed out), inverse ones decimation in time (digit-reversed in,
// natural out), and spectra stay digit-reversed along both axes: fft.hip's bit-reversal trick with digits of any radix.  Stage s of the forward
// transform has radix r_s and works on blocks of L_s = N / (r_0 ... r_(s-1)) points; frequency f = k_0 + r_0 (k_1 + r_1 (k_2 + ...)) is stored at
// ((k_0 r_1 + k_1) r_2 + k_2) ... : the MOST significant frequency digit is the LEAST significant storage digit.  With the trailing radices
// multiplying to sf, the sf aliases f + a N / sf of one fold group are the sf consecutive stored positions [sf g, sf g + sf).
#pragma once
#include <cstddef>
#include <vector>
namespace dpir {

constexpr int kFftMaxStages = 12;       // 2048 = 4^5 * 2: six stages; 11 would be all-radix-2
constexpr int kFftMaxPrime = 31;        // the generic butterfly holds p points in registers
constexpr int kFftMinLen = 8, kFftMaxRows = 1024, kFftMaxCols = 2048;     // H in [8, 1024], W in [8, 2048]: the LDS of a column strip / of one row
constexpr int kFftMaxSf = 16;

struct FftMixedPlan {
    int N = 0, sf = 1, stages = 0;
    int radix[kFftMaxStages] = {};      // forward order; each 4, 2, 3, 5 or an odd prime <= 31; the trailing ones multiply to sf
};

// 0, or the smallest prime factor of N above kFftMaxPrime
int fft_unsupported_factor(int N);
// The radix list of an N-point transform whose aliases at stride N / sf are adjacent.  False (plan untouched) when N < 2, sf < 1, sf does not divide N
// or a prime factor is above kFftMaxPrime.
bool fft_plan_make(int N, int sf, FftMixedPlan* out);
// perm[f] = stored position of frequency f (a bijection of [0, N))
void fft_plan_perm(const FftMixedPlan& p, std::vector<int>& perm);

// Column strips of the solve: `width` columns each (a multiple of sf, at most 16, so that an sf x sf alias tile never straddles two strips and a
// strip of H + 1 rows fits the LDS), `count` of them over [0, W), the last one `last` columns wide (guarded in the kernel when last < width).
struct FftStrips { int width = 0, count = 0, last = 0; };
FftStrips fft_strips(int W, int sf);
// LDS bytes of the column kernel (the W_H table and one strip) and of the row kernels (the W_W table and `rows` rows)
size_t fft_cols_lds_bytes(int H, int strip_width);
int fft_rows_per_group(int W);
size_t fft_rows_lds_bytes(int W);

// Why the mixed-radix kernels refuse (H, W, sf), or null.  *unsupported tells DPIR_ERR_UNSUPPORTED from DPIR_ERR_INVALID; msg (>= 160 bytes) gets the text.
bool fft_mixed_refusal(int H, int W, int sf, bool* unsupported, char* msg, size_t cap);

}  // namespace dpir
