// Plan of the mixed-radix transforms (fft_plan.h): no HIP call in this file.
#include "fft_plan.h"
#include <stdio.h>

namespace dpir {

int fft_unsupported_factor(int N) {
    for (int p = 2; p <= kFftMaxPrime && N > 1; ++p)
        while (N % p == 0) N /= p;
    if (N <= 1) return 0;
    for (int p = kFftMaxPrime + 1; (long long)p * p <= N; ++p)
        if (N % p == 0) return p;
    return N;       // what is left has no factor up to its root: a prime
}

// radices of n appended to r[]: 4 while it divides, then 2, 3, 5, then the odd primes in ascending order
static int append_radices(int n, int* r, int at) {
    while (n % 4 == 0) { r[at++] = 4; n /= 4; }
    for (int p = 2; p <= kFftMaxPrime; ++p)
        while (n % p == 0) { r[at++] = p; n /= p; }
    return at;
}

bool fft_plan_make(int N, int sf, FftMixedPlan* out) {
    if (N < 2 || sf < 1 || N % sf || fft_unsupported_factor(N)) return false;
    FftMixedPlan p;
    p.N = N; p.sf = sf;
    p.stages = append_radices(N / sf, p.radix, 0);      // at most log2(2048) = 11 entries
    p.stages = append_radices(sf, p.radix, p.stages);
    *out = p;
    return true;
}

void fft_plan_perm(const FftMixedPlan& p, std::vector<int>& perm) {
    perm.assign(p.N, 0);
    for (int pos = 0; pos < p.N; ++pos) {
        int k[kFftMaxStages], rest = pos;
        for (int s = p.stages - 1; s >= 0; --s) { k[s] = rest % p.radix[s]; rest /= p.radix[s]; }
        int f = 0, weight = 1;
        for (int s = 0; s < p.stages; ++s) { f += k[s] * weight; weight *= p.radix[s]; }
        perm[f] = pos;
    }
}

FftStrips fft_strips(int W, int sf) {
    FftStrips s;
    s.width = sf * (16 / sf > 1 ? 16 / sf : 1);
    s.count = (W + s.width - 1) / s.width;
    s.last = W - (s.count - 1) * s.width;
    return s;
}

size_t fft_cols_lds_bytes(int H, int strip_width) { return ((size_t)H + (size_t)strip_width * (H + 1)) * 8; }
int fft_rows_per_group(int W) { return W >= 1024 ? 1 : 1024 / W; }
size_t fft_rows_lds_bytes(int W) { return ((size_t)W + (size_t)fft_rows_per_group(W) * W) * 8; }

bool fft_mixed_refusal(int H, int W, int sf, bool* unsupported, char* msg, size_t cap) {
    *unsupported = true;
    if (sf < 1 || H % sf || W % sf) {
        *unsupported = false;
        snprintf(msg, cap, "pre_calculate: image size not divisible by sf");
        return true;
    }
    if (sf > kFftMaxSf) { snprintf(msg, cap, "fft prox: sf must be in [1, %d] (got %d)", kFftMaxSf, sf); return true; }
    if (H < kFftMinLen || H > kFftMaxRows || W < kFftMinLen || W > kFftMaxCols) {
        snprintf(msg, cap, "fft prox: H must be in [%d, %d] and W in [%d, %d] (got %d x %d)", kFftMinLen, kFftMaxRows, kFftMinLen, kFftMaxCols, H, W);
        return true;
    }
    const int fh = fft_unsupported_factor(H), fw = fft_unsupported_factor(W);
    if (fh || fw) {
        snprintf(msg, cap, "fft prox: %s = %d has the prime factor %d; prime factors above %d are not supported", fh ? "H" : "W", fh ? H : W,
                 fh ? fh : fw, kFftMaxPrime);
        return true;
    }
    return false;
}

}  // namespace dpir
