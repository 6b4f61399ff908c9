// FFT data-fidelity prox at any image size and integer sf: fft.hip's three launches with mixed-radix transforms (ProxLayout::FullDigitrev).
//
// Same structure as fft.hip -- rows forward (real input, the (x*pa+pb)*pm prologue), columns forward + solve + columns inverse in one LDS strip,
// rows inverse (real output, scale, oa / ob, guided blend) -- and the same storage trick with digits in place of bits (fft_plan.h): forward
// transforms are decimation in frequency in place, inverse ones decimation in time, every spectrum stays digit-reversed along both axes, and
// because the plan ends in radices that multiply to sf, the sf x sf aliases (u + i H/sf, v + j W/sf) are one contiguous sf x sf tile of the stored
// plane.  Radices 2, 4, 3 and 5 have butterflies of their own; any other prime p <= 31 takes the generic one (p points in registers, p^2 complex
// multiply-adds).  Every twiddle, the p-th roots of the odd butterflies included, is ONE read of the engine's W_N^m table (computed in double,
// ProxCache::table) at an index reduced mod N in integers: no device sincosf, no product of twiddles.
#include "common.h"
#include "elem.h"
#include "fft_plan.h"
#include "fft_regs.h"

namespace dpir {

struct MixedStages { int N, stages; int radix[kFftMaxStages]; };

// One butterfly of a stage: the r points x[q m], q < r, of a block of L = r m points; j = the butterfly's offset in the block, ts = N / L.
// FWD: y_k = (sum_q x_q W_r^(q k)) W_L^(j k).  INV: y_q = sum_k (x_k conj W_L^(j k)) conj W_r^(q k), the exact inverse up to the factor r.
template <bool INV> __device__ __forceinline__ float2 twmul(float2 a, float2 w) { return INV ? cmulc2(a, w) : cmul2(a, w); }

template <bool INV> __device__ __forceinline__ void bfly2(float2* x, int m, int jt, const float2* tw) {
    float2 a = x[0], b = x[m];
    if (INV) b = cmulc2(b, tw[jt]);
    float2 s = cadd(a, b), d = csub(a, b);
    if (!INV) d = cmul2(d, tw[jt]);
    x[0] = s; x[m] = d;
}
template <bool INV> __device__ __forceinline__ void bfly4(float2* x, int m, int jt, const float2* tw) {
    float2 a0 = x[0], a1 = x[m], a2 = x[2 * m], a3 = x[3 * m];
    if (INV) { a1 = cmulc2(a1, tw[jt]); a2 = cmulc2(a2, tw[2 * jt]); a3 = cmulc2(a3, tw[3 * jt]); }
    fft4<INV>(a0, a1, a2, a3);
    if (!INV) { a1 = cmul2(a1, tw[jt]); a2 = cmul2(a2, tw[2 * jt]); a3 = cmul2(a3, tw[3 * jt]); }
    x[0] = a0; x[m] = a1; x[2 * m] = a2; x[3 * m] = a3;
}
// W_3 = (-1/2, -s): y_1 = (x_0 - t/2) -+ i s (x_1 - x_2), t = x_1 + x_2; s = -Im W_N^(N/3) from the table
template <bool INV> __device__ __forceinline__ void bfly3(float2* x, int m, int jt, const float2* tw, int N) {
    float2 a0 = x[0], a1 = x[m], a2 = x[2 * m];
    if (INV) { a1 = cmulc2(a1, tw[jt]); a2 = cmulc2(a2, tw[2 * jt]); }
    const float s = -tw[N / 3].y;
    const float2 t = cadd(a1, a2), d = csub(a1, a2);
    const float2 c = make_float2(a0.x - 0.5f * t.x, a0.y - 0.5f * t.y);
    const float2 e = mul_mi<INV>(make_float2(s * d.x, s * d.y));          // -+ i s d
    float2 y1 = cadd(c, e), y2 = csub(c, e);
    a0 = cadd(a0, t);
    if (!INV) { y1 = cmul2(y1, tw[jt]); y2 = cmul2(y2, tw[2 * jt]); }
    x[0] = a0; x[m] = y1; x[2 * m] = y2;
}
// W_5^1 = (c1, -s1), W_5^2 = (c2, -s2) from the table; the conjugate pairs (x_1, x_4) and (x_2, x_3) share their products
template <bool INV> __device__ __forceinline__ void bfly5(float2* x, int m, int jt, const float2* tw, int N) {
    float2 a0 = x[0], a1 = x[m], a2 = x[2 * m], a3 = x[3 * m], a4 = x[4 * m];
    if (INV) { a1 = cmulc2(a1, tw[jt]); a2 = cmulc2(a2, tw[2 * jt]); a3 = cmulc2(a3, tw[3 * jt]); a4 = cmulc2(a4, tw[4 * jt]); }
    const float2 w1 = tw[N / 5], w2 = tw[2 * (N / 5)];
    const float c1 = w1.x, s1 = -w1.y, c2 = w2.x, s2 = -w2.y;
    const float2 p1 = cadd(a1, a4), m1 = csub(a1, a4), p2 = cadd(a2, a3), m2 = csub(a2, a3);
    const float2 r1 = make_float2(a0.x + (c1 * p1.x + c2 * p2.x), a0.y + (c1 * p1.y + c2 * p2.y));
    const float2 r2 = make_float2(a0.x + (c2 * p1.x + c1 * p2.x), a0.y + (c2 * p1.y + c1 * p2.y));
    const float2 i1 = mul_mi<INV>(make_float2(s1 * m1.x + s2 * m2.x, s1 * m1.y + s2 * m2.y));
    const float2 i2 = mul_mi<INV>(make_float2(s2 * m1.x - s1 * m2.x, s2 * m1.y - s1 * m2.y));
    float2 y1 = cadd(r1, i1), y4 = csub(r1, i1), y2 = cadd(r2, i2), y3 = csub(r2, i2);
    a0 = cadd(a0, cadd(p1, p2));
    if (!INV) { y1 = cmul2(y1, tw[jt]); y2 = cmul2(y2, tw[2 * jt]); y3 = cmul2(y3, tw[3 * jt]); y4 = cmul2(y4, tw[4 * jt]); }
    x[0] = a0; x[m] = y1; x[2 * m] = y2; x[3 * m] = y3; x[4 * m] = y4;
}
// Any odd prime P <= 31: the P inputs in registers, one output at a time; W_P^(q k) = tw[((q k) mod P) N / P], the index stepped in integers
template <int P, bool INV> __device__ __forceinline__ void bflyp(float2* x, int m, int jt, const float2* tw, int N) {
    float2 v[P];
#pragma unroll
    for (int q = 0; q < P; ++q) v[q] = x[q * m];
    if (INV) {
#pragma unroll
        for (int q = 1; q < P; ++q) v[q] = cmulc2(v[q], tw[q * jt]);
    }
    const int step = N / P;
#pragma unroll 1
    for (int k = 0; k < P; ++k) {
        float2 acc = v[0];
        int e = 0;                      // (q k) mod P
#pragma unroll
        for (int q = 1; q < P; ++q) {
            e += k;
            if (e >= P) e -= P;
            const float2 t = twmul<INV>(v[q], tw[e * step]);
            acc = cadd(acc, t);
        }
        if (!INV && k) acc = cmul2(acc, tw[k * jt]);
        x[k * m] = acc;
    }
}

template <bool INV> __device__ __forceinline__ void butterfly(float2* x, int r, int m, int jt, const float2* tw, int N) {
    switch (r) {
        case 2: bfly2<INV>(x, m, jt, tw); break;
        case 4: bfly4<INV>(x, m, jt, tw); break;
        case 3: bfly3<INV>(x, m, jt, tw, N); break;
        case 5: bfly5<INV>(x, m, jt, tw, N); break;
        case 7: bflyp<7, INV>(x, m, jt, tw, N); break;
        case 11: bflyp<11, INV>(x, m, jt, tw, N); break;
        case 13: bflyp<13, INV>(x, m, jt, tw, N); break;
        case 17: bflyp<17, INV>(x, m, jt, tw, N); break;
        case 19: bflyp<19, INV>(x, m, jt, tw, N); break;
        case 23: bflyp<23, INV>(x, m, jt, tw, N); break;
        case 29: bflyp<29, INV>(x, m, jt, tw, N); break;
        default: bflyp<31, INV>(x, m, jt, tw, N); break;
    }
}

// `batch` transforms of p.N points living in LDS at d[b * stride + i]; all 256 threads call.  tw: the whole W_N^m table (N entries, LDS).
// FWD: DIF, natural -> digit-reversed.  INV: DIT, digit-reversed -> natural (unnormalised).  A butterfly's twiddle index j k (N / L) is below N.
template <bool INV>
__device__ __forceinline__ void mixed_fft_lds(float2* d, int batch, int stride, const MixedStages& p, const float2* tw) {
    const int N = p.N;
    int L = N;
    if (INV) { L = 1; }
    for (int st = 0; st < p.stages; ++st) {
        const int r = p.radix[INV ? p.stages - 1 - st : st];
        if (INV) L *= r;
        const int m = L / r, per = N / r, ts = N / L;
        for (int t = threadIdx.x; t < batch * per; t += blockDim.x) {
            const int b = t / per, u = t - b * per;
            const int blk = u / m, j = u - blk * m;
            butterfly<INV>(d + b * stride + blk * L + j, r, m, j * ts, tw, N);
        }
        if (!INV) L = m;
        __syncthreads();
    }
}

__device__ __forceinline__ void load_table(float2* lds_tw, const float2* tw, int N) {
    for (int i = threadIdx.x; i < N; i += blockDim.x) lds_tw[i] = tw[i];
}

// ---------------------------------------------------------------- rows, forward (real input, or the buffer's own rows)
// grid: total_rows / R blocks; block: 256 threads; R rows of W points.  PI: pm = tau of the ROW's image (fft.hip)
template <bool PI>
__global__ __launch_bounds__(256) void mixed_rows_fwd_kernel(float2* buf, const float* real_in, float pa, float pb, float pm, MixedStages pw, int R,
                                                              size_t total_rows, const float2* tw, const StepDev* sp, const LoopDev* lp) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int W = pw.N;
    float2* lds_tw = sm;
    float2* d = sm + W;
    if (sp) pm = sp->tau;
    load_table(lds_tw, tw, W);
    const size_t row0 = (size_t)blockIdx.x * R;
    const size_t rows_per_image = PI ? total_rows / lp->B : 1;
    for (int i = threadIdx.x; i < R * W; i += 256) {
        const int rr = i / W, c = i - rr * W;
        const size_t row = row0 + rr;
        float2 v = make_float2(0.f, 0.f);
        if (row < total_rows) {
            const size_t g = row * W + c;
            if (PI) pm = image_row(sp, lp, row / rows_per_image).x;
            if (real_in) v.x = (real_in[g] * pa + pb) * pm;
            else v = buf[g];
        }
        d[i] = v;
    }
    __syncthreads();
    mixed_fft_lds<false>(d, R, W, pw, lds_tw);
    for (int i = threadIdx.x; i < R * W; i += 256) {
        const size_t row = row0 + i / W;
        if (row < total_rows) buf[row0 * W + i] = d[i];
    }
}

// ---------------------------------------------------------------- rows, inverse, real output
__global__ __launch_bounds__(256) void mixed_rows_inv_kernel(const float2* buf, float* out, float scale, float oa, float ob, const float* blend_base, float g,
                                                              MixedStages pw, int R, size_t total_rows, const float2* tw) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int W = pw.N;
    float2* lds_tw = sm;
    float2* d = sm + W;
    load_table(lds_tw, tw, W);
    const size_t row0 = (size_t)blockIdx.x * R;
    for (int i = threadIdx.x; i < R * W; i += 256) {
        const size_t row = row0 + i / W;
        d[i] = row < total_rows ? buf[row0 * W + i] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    mixed_fft_lds<true>(d, R, W, pw, lds_tw);
    for (int i = threadIdx.x; i < R * W; i += 256) {
        const size_t row = row0 + i / W;
        if (row < total_rows) {
            const size_t gi = row0 * W + i;
            float v = (d[i].x * scale) * oa + ob;
            if (blend_base) { float b0 = blend_base[gi]; v = b0 + g * (v - b0); }
            out[gi] = v;
        }
    }
}

// ---------------------------------------------------------------- columns: FFT -> (solve) -> inverse FFT
// One workgroup per (plane, strip of cw columns); the last strip of a plane holds wv <= cw of them (both multiples of sf)
template <int MODE, bool PI = false>   // 0: forward only, 1: inverse only, 2: forward + solve + inverse; PI: alpha = tau of the plane's image (a.pil)
__global__ __launch_bounds__(256) void mixed_cols_kernel(float2* buf, SolveArgs a, MixedStages ph, int W, int cw, int strips, const float2* tw) {
    extern __shared__ __attribute__((aligned(16))) float2 sm[];
    const int H = ph.N;
    float2* lds_tw = sm;
    float2* d = sm + H;
    const int HS = H + 1;                   // padded column stride
    load_table(lds_tw, tw, H);
    const int plane = blockIdx.x / strips;
    const int m0 = (blockIdx.x - plane * strips) * cw;
    const int wv = min(cw, W - m0);
    float2* base = buf + (size_t)plane * H * W + m0;
    for (int i = threadIdx.x; i < wv * H; i += 256) {
        const int r = i / wv, c = i - r * wv;
        d[c * HS + r] = base[(size_t)r * W + c];
    }
    __syncthreads();
    if (MODE != 1) mixed_fft_lds<false>(d, wv, HS, ph, lds_tw);
    if (MODE == 2) {
        if (a.sp) a.alpha = a.sp->tau;
        if (PI) a.alpha = image_row(a.sp, a.pil, plane / 3).x;
        // one work item per sf x sf alias tile (rows and columns are in digit-reversed storage order)
        const int sf = a.sf;
        const int n_img = plane / 3;
        const float2* FB = a.FB + (size_t)n_img * H * W + m0;
        const float* F2B = a.F2B + (size_t)n_img * H * W + m0;
        const float2* FBFy = a.FBFy + (size_t)plane * H * W + m0;
        const int tc = wv / sf, tr = H / sf;
        const float inv_n = 1.0f / (float)(sf * sf);
        for (int it = threadIdx.x; it < tc * tr; it += 256) {
            const int rb = it / tc, cb = it - rb * tc;
            PairSum<float2, 9> sx;               // the sf^2 <= 256 aliases summed pairwise (fft_regs.h): the mean is cancelled against FR / alpha
            PairSum<float, 9> sw;
            for (int i = 0; i < sf; ++i)
                for (int j = 0; j < sf; ++j) {
                    const int r = rb * sf + i, c = cb * sf + j;
                    const size_t gi = (size_t)r * W + c;
                    float2 fr = d[c * HS + r];
                    const float2 y = FBFy[gi];
                    fr.x += y.x; fr.y += y.y;
                    d[c * HS + r] = fr;
                    sx.add(cmul2(FB[gi], fr));
                    sw.add(F2B[gi]);
                }
            float2 fbr = sx.sum();
            float invw = sw.sum();
            fbr.x *= inv_n; fbr.y *= inv_n; invw *= inv_n;
            const float den = invw + a.alpha;
            const float2 q = make_float2(fbr.x / den, fbr.y / den);
            for (int i = 0; i < sf; ++i)
                for (int j = 0; j < sf; ++j) {
                    const int r = rb * sf + i, c = cb * sf + j;
                    const size_t gi = (size_t)r * W + c;
                    const float2 fr = d[c * HS + r];
                    const float2 t = cmulc2(q, FB[gi]);        // conj(FB) * q
                    d[c * HS + r] = make_float2((fr.x - t.x) / a.alpha, (fr.y - t.y) / a.alpha);
                }
        }
        __syncthreads();
    }
    if (MODE != 0) mixed_fft_lds<true>(d, wv, HS, ph, lds_tw);
    for (int i = threadIdx.x; i < wv * H; i += 256) {
        const int r = i / wv, c = i - r * wv;
        base[(size_t)r * W + c] = d[c * HS + r];
    }
}

// ---------------------------------------------------------------- launchers
static MixedStages stages_of(const FftMixedPlan& p) {
    MixedStages s{};
    s.N = p.N; s.stages = p.stages;
    for (int i = 0; i < p.stages; ++i) s.radix[i] = p.radix[i];
    return s;
}
static Status check_mixed(const MixedFft& f, int N, int H, int W) {
    char msg[192];
    bool unsupported = true;
    if (fft_mixed_refusal(H, W, 1, &unsupported, msg, sizeof msg)) return Status{unsupported ? DPIR_ERR_UNSUPPORTED : DPIR_ERR_INVALID, msg};
    if (f.plan.N != N || !f.tw) return invalid("mixed fft: plan size mismatch");
    return Status{};
}

Status launch_mixed_rows_fwd(hipStream_t s, const MixedFft& pw, float2* buf, const float* real_in, float pa, float pb, float pm, int P, int H, int W,
                             const StepDev* sp, const LoopDev* pil) {
    DPIR_TRY(check_mixed(pw, W, H, W));
    if (pil && !sp) return invalid("fft rows: the per-image form reads the device step block");
    const int R = fft_rows_per_group(W);
    const size_t rows = (size_t)P * H, lds = fft_rows_lds_bytes(W);
    const dim3 grid((unsigned)((rows + R - 1) / R));
    if (pil) hipLaunchKernelGGL(mixed_rows_fwd_kernel<true>, grid, dim3(256), lds, s, buf, real_in, pa, pb, pm, stages_of(pw.plan), R, rows, pw.tw, sp, pil);
    else hipLaunchKernelGGL(mixed_rows_fwd_kernel<false>, grid, dim3(256), lds, s, buf, real_in, pa, pb, pm, stages_of(pw.plan), R, rows, pw.tw, sp, pil);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

Status launch_mixed_rows_inv(hipStream_t s, const MixedFft& pw, const float2* buf, float* out, float scale, float oa, float ob, const float* blend_base,
                             float g, int P, int H, int W) {
    DPIR_TRY(check_mixed(pw, W, H, W));
    const int R = fft_rows_per_group(W);
    const size_t rows = (size_t)P * H, lds = fft_rows_lds_bytes(W);
    hipLaunchKernelGGL(mixed_rows_inv_kernel, dim3((unsigned)((rows + R - 1) / R)), dim3(256), lds, s, buf, out, scale, oa, ob, blend_base, g,
                       stages_of(pw.plan), R, rows, pw.tw);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

template <int MODE, bool PI = false>
static Status launch_mixed_cols_mode(hipStream_t s, const MixedFft& ph, float2* buf, const SolveArgs& a, int P, int H, int W, int sf) {
    DPIR_TRY(check_mixed(ph, H, H, W));
    if (sf < 1 || sf > kFftMaxSf || H % sf || W % sf) return invalid("mixed fft cols: sf must divide H and W");
    const FftStrips st = fft_strips(W, sf);
    const size_t lds = fft_cols_lds_bytes(H, st.width);
    if (lds > 160 * 1024) return Status{DPIR_ERR_UNSUPPORTED, "mixed fft cols: the strip does not fit the LDS"};
    auto fn = mixed_cols_kernel<MODE, PI>;
    static LdsAttrOnce attr;
    DPIR_HIP(attr.set(reinterpret_cast<const void*>(fn), 160 * 1024));
    hipLaunchKernelGGL(fn, dim3((unsigned)(P * st.count)), dim3(256), lds, s, buf, a, stages_of(ph.plan), W, st.width, st.count, ph.tw);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

Status launch_mixed_cols(hipStream_t s, const MixedFft& ph, float2* buf, int P, int H, int W, int sf) {
    SolveArgs a{};
    a.sp = nullptr;
    return launch_mixed_cols_mode<0>(s, ph, buf, a, P, H, W, sf);
}

Status launch_mixed_cols_solve(hipStream_t s, const MixedFft& ph, float2* buf, const SolveArgs& a, int B, int H, int W) {
    if (ph.plan.sf != a.sf) return invalid("mixed fft cols: the plan's trailing radices do not multiply to sf");
    if (a.pil && !a.sp) return invalid("fft cols: the per-image form reads the device step block");
    return a.pil ? launch_mixed_cols_mode<2, true>(s, ph, buf, a, B * 3, H, W, a.sf) : launch_mixed_cols_mode<2>(s, ph, buf, a, B * 3, H, W, a.sf);
}

}  // namespace dpir
