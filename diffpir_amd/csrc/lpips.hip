// LPIPS v0.1 (net = 'vgg') on the engine: replaces loss_fn_vgg(x_0*2-1, img_H/255*2-1) of main_ddpir.py:489-493.
//
//   lpips_prep      x0 (f32 NCHW, un-clamped) and the ground truth (u8 NHWC or f32 NCHW in [0,1]) -> ONE scaled tensor of 2P rows, rows [0,P)
//                   the estimate and [P,2P) the ground truth: v*2-1, then (v - shift_c) / scale_c.  The scaling is applied here, ahead of the
//                   first convolution's zero padding (folded into the first bias the border pixels would differ).
//   trunk           13 x (3x3 pad 1 convolution + bias + ReLU), a 2x2 stride-2 max-pool (floor) behind convolutions 2, 4, 7, 10.
//                   The convolution is launch_conv, the exact-fp32 MFMA kernel of conv2.hip (CoutP % 64 == 0), whatever dpir_set_precision
//                   says.  That kernel adds the Cin * 9 products of an output into ONE fp32 accumulator in sequence; at Cin 512 the chain was
//                   25 - 80 x further from float64 than a blocked float32 convolution at relu4_3 / relu5_3, and its distance grows about
//                   linearly with the length of that sequence (measured; with 64-channel pieces it was still 14 - 38 x).  So a layer is run as
//                   Cin / 16 launches, one per 16-channel slab of the input (144 products per accumulator), each into its own partial tensor,
//                   and lpips_combine adds the slabs and the bias in float64 in slab order, applies the ReLU and rounds once.  Activations
//                   therefore live in SLAB layout [C/16][rows][16][H W] (a slab is a contiguous NCHW tensor launch_conv can read).  The split depends on the layer alone,
//                   never on the batch (no split-K inside launch_conv: partial = null), so a pixel's sum has one order whatever the batch.
//   lpips_head      per tap and pixel, in float64 from the float32 features: n = f / (sqrt(sum_c f^2) + 1e-10) for both halves,
//                   d = sum_c w_c (n0 - n1)^2 -- on the NORMALISED values, never the expanded sum w a^2 - 2 w a b + w b^2, which cancels to
//                   noise for near-identical images.  Reduction: wave shuffles -> LDS -> one double per workgroup -> a second kernel adds the
//                   workgroups of an image in index order and the five taps in tap order.  No atomics: an image's score has the same bits
//                   wherever it sits in the batch, for every B and chunk size, on every repeat.
// The 2B rows are processed in chunks of P pairs (kLpipsChunkPixels; DPIR_LPIPS_CHUNK = rows forces a smaller one), so the arena is bounded.
#include "engine.h"
#include "lpips.h"
#include <stdlib.h>

namespace dpir {

namespace {
struct VggLayer { int feat, cin, cout; bool tap, pool; };
const VggLayer kVgg[kLpipsConvs] = {
    {0, 3, 64, false, false},    {2, 64, 64, true, true},
    {5, 64, 128, false, false},  {7, 128, 128, true, true},
    {10, 128, 256, false, false}, {12, 256, 256, false, false}, {14, 256, 256, true, true},
    {17, 256, 512, false, false}, {19, 512, 512, false, false}, {21, 512, 512, true, true},
    {24, 512, 512, false, false}, {26, 512, 512, false, false}, {28, 512, 512, true, false},
};
const int kTapC[kLpipsTaps] = {64, 128, 256, 512, 512};
constexpr int kSlab = 16;       // input channels per launch_conv launch (divides every channel count of the trunk but the image's 3)

// ------------------------------------------------------------------------------------------ kernels
// one thread per (pair, channel, pixel): writes the estimate's row and the ground truth's row
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* x0, const uint8_t* gt_u8, const float* gt_f32, int P, int HW, float* out) {
    const size_t total = (size_t)P * 3 * HW;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t n = i / ((size_t)3 * HW), r = i - n * 3 * HW;
    const int c = (int)(r / HW);
    const size_t p = r - (size_t)c * HW;
    const float shift = c == 0 ? -0.030f : (c == 1 ? -0.088f : -0.188f);
    const float scale = c == 0 ? 0.458f : (c == 1 ? 0.448f : 0.450f);
    const float a = x0[i];
    const float g = gt_u8 ? (float)gt_u8[(n * HW + p) * 3 + c] / 255.0f : gt_f32[i];      // util.uint2single, as dpir_metrics forms it
    out[i] = ((a * 2.0f - 1.0f) - shift) / scale;
    out[total + i] = ((g * 2.0f - 1.0f) - shift) / scale;
}

// out (slab layout [Cout/kSlab][R][kSlab][HW]) = relu(bias + sum_i part[i]), part[i] = [R][Cout][HW] (the convolution of input slab i), added in float64
// in slab order and rounded once.  VEC: HW % 4 == 0, 16 bytes per lane; else one element per lane.
template <bool VEC>
__global__ __launch_bounds__(256) void lpips_combine_kernel(const float* part, int n_part, const float* bias, float* out, int R, int Cout, int HW) {
    constexpr int V = VEC ? 4 : 1;
    const int hwv = HW / V;
    const size_t total = (size_t)R * Cout * hwv, slab = (size_t)R * Cout * HW;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t plane = i / hwv;                 // r * Cout + co
    const int q = (int)(i - plane * hwv);
    const int r = (int)(plane / Cout), co = (int)(plane - (size_t)r * Cout);
    const float* src = part + plane * HW + (size_t)q * V;
    float* dst = out + (((size_t)(co / kSlab) * R + r) * kSlab + (co % kSlab)) * HW + (size_t)q * V;
    const double b = (double)bias[co];
    if (VEC) {
        double a0 = b, a1 = b, a2 = b, a3 = b;
        for (int k = 0; k < n_part; ++k) {
            const float4 v = *reinterpret_cast<const float4*>(src + k * slab);
            a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
        }
        float4 o;
        o.x = fmaxf((float)a0, 0.f); o.y = fmaxf((float)a1, 0.f); o.z = fmaxf((float)a2, 0.f); o.w = fmaxf((float)a3, 0.f);
        *reinterpret_cast<float4*>(dst) = o;
    } else {
        double a0 = b;
        for (int k = 0; k < n_part; ++k) a0 += (double)src[k * slab];
        *dst = fmaxf((float)a0, 0.f);
    }
}

// 2x2 stride-2 max-pool of post-ReLU planes, floor for odd sizes: out[., yo, xo] = max(0, the four inputs) (the max with 0 keeps it a ReLU + pool).  VEC: W % 4 == 0, a lane reads two float4 and
// writes one float2 (two outputs); else one output per lane from four scalar loads.  planes = rows * channels.
template <bool VEC>
__global__ __launch_bounds__(256) void lpips_pool_kernel(const float* x, float* out, size_t planes, int H, int W) {
    const int Ho = H >> 1, Wo = W >> 1;
    const int wq = VEC ? Wo >> 1 : Wo;                       // lanes per output row
    const size_t total = planes * Ho * wq;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t pl = i / ((size_t)Ho * wq);
    const int r = (int)(i - pl * Ho * wq);
    const int yo = r / wq, xq = r - yo * wq;
    const float* src = x + pl * H * W + (size_t)(2 * yo) * W;
    float* dst = out + pl * Ho * Wo + (size_t)yo * Wo;
    if (VEC) {
        const float4 a = *reinterpret_cast<const float4*>(src + 4 * xq);
        const float4 b = *reinterpret_cast<const float4*>(src + W + 4 * xq);
        float2 o;
        o.x = fmaxf(fmaxf(fmaxf(a.x, a.y), fmaxf(b.x, b.y)), 0.f);
        o.y = fmaxf(fmaxf(fmaxf(a.z, a.w), fmaxf(b.z, b.w)), 0.f);
        *reinterpret_cast<float2*>(dst + 2 * xq) = o;
    } else {
        const float* s = src + 2 * xq;
        dst[xq] = fmaxf(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[W], s[W + 1])), 0.f);
    }
}

// feat: slab layout [C/kSlab][2P][kSlab][HW], post-ReLU features of one tap, rows [0,P) the estimate and [P,2P) the ground truth.  One lane per pixel,
// grid (blocks, P).
// partial[p * gridDim.x + block] = sum over the block's pixels of sum_c w_c (n0 - n1)^2.
__global__ __launch_bounds__(256) void lpips_head_kernel(const float* feat, const float* w, int P, int C, int HW, double* partial) {
    const int p = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    double d = 0.0;
    if (pix < HW) {
        const int R = 2 * P;
        auto at = [&](int r, int c) { return feat + (((size_t)(c / kSlab) * R + r) * kSlab + (c % kSlab)) * HW + pix; };
        double s0 = 0.0, s1 = 0.0;
        for (int c = 0; c < C; ++c) {
            const double a = (double)*at(p, c), b = (double)*at(P + p, c);
            s0 += a * a; s1 += b * b;
        }
        const double i0 = 1.0 / (sqrt(s0) + 1e-10), i1 = 1.0 / (sqrt(s1) + 1e-10);
        for (int c = 0; c < C; ++c) {
            // two rounded products, then their difference (the file is built with contraction off: fused, identical images would leave the
            // rounding error of one product instead of 0)
            const double n0 = (double)*at(p, c) * i0, n1 = (double)*at(P + p, c) * i1;
            const double t = n0 - n1;
            d += (double)w[c] * (t * t);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o, 64);
    __shared__ double wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)p * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// second stage, one lane per pair: the workgroups of the image in index order, / HW, added to the running score of image pair0 + p in tap
// order (tap 0 starts it); the last tap rounds the sum of the five means to float once
__global__ void lpips_score_kernel(const double* partial, int P, int blocks, int HW, int tap, int pair0, double* score_d, float* score_f) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partial[(size_t)p * blocks + b];
    const double acc = (tap == 0 ? 0.0 : score_d[pair0 + p]) + s / (double)HW;
    score_d[pair0 + p] = acc;
    if (tap == kLpipsTaps - 1) score_f[pair0 + p] = (float)acc;
}

// ------------------------------------------------------------------------------------------ host
Status grow(void** p, size_t* cap, size_t need, size_t elem, const char* what) {
    if (*cap >= need) return Status{};
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc(p, need * elem) != hipSuccess) { (void)hipGetLastError(); return Status{DPIR_ERR_NOMEM, std::string("lpips: hipMalloc for ") + what + " failed"}; }
    *cap = need;
    return Status{};
}
template <class T> Status growT(T** p, size_t* cap, size_t need, const char* what) { return grow(reinterpret_cast<void**>(p), cap, need, sizeof(T), what); }

Status upload(LpipsState* st, const float* host, size_t n, float** dev) {
    void* p = nullptr;
    if (hipMalloc(&p, n * sizeof(float)) != hipSuccess) return Status{DPIR_ERR_NOMEM, "lpips: hipMalloc for weights failed"};
    st->weight_allocs.push_back(p);
    DPIR_HIP(hipMemcpy(p, host, n * sizeof(float), hipMemcpyHostToDevice));
    *dev = reinterpret_cast<float*>(p);
    return Status{};
}

const dpir_tensor* find(const dpir_tensor* w, int n, const std::string& key) {
    for (int i = 0; i < n; ++i) if (w[i].name && key == w[i].name) return &w[i];
    return nullptr;
}
}  // namespace

void lpips_free(dpir_engine* e) {
    LpipsState* st = e->lpips;
    if (!st) return;
    for (void* p : st->weight_allocs) (void)hipFree(p);
    void* bufs[] = {st->in, st->act[0], st->act[1], st->slabs, st->partial, st->score_d, st->score_f};
    for (void* p : bufs) if (p) (void)hipFree(p);
    for (float* p : st->tap) if (p) (void)hipFree(p);
    delete st;
    e->lpips = nullptr;
}

Status lpips_load(dpir_engine* e, const dpir_tensor* weights, int n) {
    DPIR_HIP(hipStreamSynchronize(e->stream));
    lpips_free(e);
    std::unique_ptr<LpipsState> st(new LpipsState());
    struct Guard { LpipsState* s; ~Guard() { if (s) for (void* p : s->weight_allocs) (void)hipFree(p); } } guard{st.get()};
    for (int l = 0; l < kLpipsConvs; ++l) {
        const VggLayer& v = kVgg[l];
        const std::string base = "features." + std::to_string(v.feat);
        const dpir_tensor* tw = find(weights, n, base + ".weight");
        if (!tw) return invalid("lpips state-dict key missing: " + base + ".weight");
        if (tw->ndim != 4 || tw->shape[0] != v.cout || tw->shape[1] != v.cin || tw->shape[2] != 3 || tw->shape[3] != 3)
            return invalid("lpips state-dict key " + base + ".weight: wrong shape");
        const dpir_tensor* tb = find(weights, n, base + ".bias");
        if (!tb) return invalid("lpips state-dict key missing: " + base + ".bias");
        if (tb->ndim != 1 || tb->shape[0] != v.cout) return invalid("lpips state-dict key " + base + ".bias: wrong shape");
        if (!tw->data || !tb->data) return invalid("lpips state-dict key " + base + ": null data");
        // OIHW -> [CinP][9][CoutP], zero padded, CinP % 16 == 0 and CoutP % 64 == 0: the packing of unet.hip's load_conv for launch_conv
        const int coutp = round_up(v.cout, 64), cinp = round_up(v.cin, 16);
        std::vector<float> packed((size_t)cinp * 9 * coutp, 0.f);
        for (int co = 0; co < v.cout; ++co)
            for (int ci = 0; ci < v.cin; ++ci)
                for (int t = 0; t < 9; ++t)
                    packed[((size_t)ci * 9 + t) * coutp + co] = tw->data[((size_t)co * v.cin + ci) * 9 + t];
        LpipsConv& c = st->conv[l];
        c.cin = v.cin; c.cout = v.cout; c.coutp = coutp;
        DPIR_TRY(upload(st.get(), packed.data(), packed.size(), &c.w));
        DPIR_TRY(upload(st.get(), tb->data, v.cout, &c.bias));
    }
    {
        const std::vector<float> z(512, 0.f);          // the slab launches add no bias: lpips_combine adds it in float64
        DPIR_TRY(upload(st.get(), z.data(), z.size(), &st->zero_bias));
    }
    for (int k = 0; k < kLpipsTaps; ++k) {
        const std::string key = "lin" + std::to_string(k) + ".weight";
        const dpir_tensor* t = find(weights, n, key);
        if (!t) return invalid("lpips state-dict key missing: " + key);
        long long numel = 1;
        if (t->ndim < 1 || t->ndim > 4) return invalid("lpips state-dict key " + key + ": wrong rank");
        for (int d = 0; d < t->ndim; ++d) numel *= t->shape[d];
        if (numel != kTapC[k]) return invalid("lpips state-dict key " + key + ": wrong shape");
        if (!t->data) return invalid("lpips state-dict key " + key + ": null data");
        DPIR_TRY(upload(st.get(), t->data, kTapC[k], &st->lin[k]));
    }
    guard.s = nullptr;
    st->loaded = true;
    e->lpips = st.release();
    return Status{};
}

Status lpips_run(dpir_engine* e, const float* x0, const uint8_t* gt_u8, const float* gt_f32, int B, int H, int W) {
    LpipsState* st = e->lpips;
    hipStream_t s = e->stream;
    const int HW = H * W;
    long long pairs = kLpipsChunkPixels / HW;
    if (const char* ev = getenv("DPIR_LPIPS_CHUNK")) { const long long rows = atoll(ev); if (rows >= 2 && rows / 2 < pairs) pairs = rows / 2; }
    const int Pmax = (int)std::min<long long>(std::max<long long>(pairs, 1), B);

    DPIR_TRY(growT(&st->in, &st->in_cap, (size_t)2 * Pmax * 3 * HW, "the scaled input"));
    size_t act_need = (size_t)2 * Pmax * 64 * HW;
    if (act_need > st->act_cap) {
        size_t c0 = st->act_cap, c1 = st->act_cap, c2 = st->act_cap;
        DPIR_TRY(growT(&st->act[0], &c0, act_need, "the activations"));
        DPIR_TRY(growT(&st->act[1], &c1, act_need, "the activations"));
        c2 *= 64 / kSlab;
        DPIR_TRY(growT(&st->slabs, &c2, act_need * (64 / kSlab), "the slab sums"));      // (Cin / kSlab) Cout h w <= (64 / kSlab) 64 H W at every layer
        st->act_cap = act_need;
    }
    DPIR_TRY(growT(&st->partial, &st->partial_cap, (size_t)Pmax * ((HW + 255) / 256), "the head sums"));
    if ((size_t)B > st->score_cap) {
        size_t c0 = st->score_cap, c1 = st->score_cap;
        DPIR_TRY(growT(&st->score_d, &c0, (size_t)B, "the scores"));
        DPIR_TRY(growT(&st->score_f, &c1, (size_t)B, "the scores"));
        st->score_cap = B;
    }
    for (int k = 0; k < kLpipsTaps; ++k) st->tap_numel[k] = 0;
    if (e->lpips_keep_taps) {
        int h = H, w = W;
        for (int k = 0; k < kLpipsTaps; ++k) {
            const size_t numel = (size_t)2 * B * kTapC[k] * h * w;
            DPIR_TRY(growT(&st->tap[k], &st->tap_cap[k], numel, "a feature tap"));
            h >>= 1; w >>= 1;
        }
    }

    for (int pair0 = 0; pair0 < B; pair0 += Pmax) {
        const int P = std::min(Pmax, B - pair0), R = 2 * P;
        const size_t off = (size_t)pair0 * 3 * HW;
        {
            const size_t total = (size_t)P * 3 * HW;
            hipLaunchKernelGGL(lpips_prep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x0 + off, gt_u8 ? gt_u8 + off : nullptr,
                               gt_f32 ? gt_f32 + off : nullptr, P, HW, st->in);
            DPIR_HIP(hipGetLastError());
        }
        const float* cur = st->in;
        int nxt = 0, h = H, w = W, tap = 0;
        for (int l = 0; l < kLpipsConvs; ++l) {
            const VggLayer& v = kVgg[l];
            const LpipsConv& c = st->conv[l];
            float* out = st->act[nxt];
            const int n_part = (c.cin + kSlab - 1) / kSlab, hw_l = h * w;
            for (int i = 0; i < n_part; ++i) {
                ConvArgs a;
                a.src.a = cur + (size_t)i * R * kSlab * hw_l; a.src.ca = std::min(c.cin, kSlab); a.src.Hs = h; a.src.Ws = w; a.src.mode = 0;
                a.w = c.w + (size_t)i * kSlab * 9 * c.coutp; a.bias = st->zero_bias; a.out = st->slabs + (size_t)i * R * c.cout * hw_l;
                a.B = R; a.Cin = a.src.ca; a.Cout = c.cout; a.CoutP = c.coutp; a.H = h; a.W = w; a.ks = 3;
                DPIR_TRY(launch_conv(s, a));
            }
            if (hw_l % 4 == 0) {
                const size_t total = (size_t)R * c.cout * (hw_l / 4);
                hipLaunchKernelGGL(lpips_combine_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, st->slabs, n_part, c.bias, out, R,
                                   c.cout, hw_l);
            } else {
                const size_t total = (size_t)R * c.cout * hw_l;
                hipLaunchKernelGGL(lpips_combine_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, st->slabs, n_part, c.bias, out, R,
                                   c.cout, hw_l);
            }
            DPIR_HIP(hipGetLastError());
            cur = out; nxt ^= 1;
            if (v.tap) {
                const int hw = h * w, blocks = (hw + 255) / 256;
                if (e->lpips_keep_taps) {
                    // slab layout -> [2B][C][hw]: per slab and half, P rows of kSlab hw contiguous floats, destination pitch one image
                    const size_t row = (size_t)c.cout * hw, piece = (size_t)kSlab * hw;
                    for (int sl = 0; sl < c.cout / kSlab; ++sl)
                        for (int half = 0; half < 2; ++half)
                            DPIR_HIP(hipMemcpy2DAsync(st->tap[tap] + ((size_t)half * B + pair0) * row + sl * piece, row * sizeof(float),
                                                      cur + ((size_t)sl * R + (size_t)half * P) * piece, piece * sizeof(float), piece * sizeof(float), P,
                                                      hipMemcpyDeviceToDevice, s));
                    st->tap_numel[tap] = (size_t)2 * B * row;
                }
                hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)blocks, (unsigned)P), dim3(256), 0, s, cur, st->lin[tap], P, c.cout, hw, st->partial);
                hipLaunchKernelGGL(lpips_score_kernel, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, s, st->partial, P, blocks, hw, tap, pair0,
                                   st->score_d, st->score_f);
                DPIR_HIP(hipGetLastError());
                ++tap;
            }
            if (v.pool) {
                float* po = st->act[nxt];
                const size_t planes = (size_t)R * c.cout;
                const int ho = h >> 1, wo = w >> 1;
                if (w % 4 == 0) {
                    const size_t total = planes * ho * (wo >> 1);
                    hipLaunchKernelGGL(lpips_pool_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cur, po, planes, h, w);
                } else {
                    const size_t total = planes * ho * wo;
                    hipLaunchKernelGGL(lpips_pool_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cur, po, planes, h, w);
                }
                DPIR_HIP(hipGetLastError());
                cur = po; nxt ^= 1; h = ho; w = wo;
            }
        }
    }
    return Status{};
}

}  // namespace dpir
