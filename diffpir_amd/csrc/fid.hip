// FID on the engine: the Inception-v3 `pool3` features of pytorch-fid (the middle column of the paper's tables, reference README.md:119-141).
//
//   fid_prep        uint8 NHWC or float32 NCHW in [0,1] -> float32 NCHW at 299 x 299: v = u8 / 255, bilinear resize (align_corners = False, no
//                   antialias: src = (dst + 0.5) in / out - 0.5 clamped below at 0, upper neighbour clamped to in - 1), then 2 v - 1.
//   fid_conv        one implicit-GEMM kernel for all 94 BasicConv layers: D[co][pixel] = sum_k W[k][co] X[k][pixel], k = (ci KH + kh) KW + kw, on the
//                   exact-fp32 MFMA (32x32x2), whatever dpir_set_precision says.  General (KH, KW), stride 1 or 2, padding (PH, PW); reads a channel
//                   range of an NCHW tensor and writes a channel range of the block's concat destination (a Mixed block never copies); bias + ReLU in
//                   the epilogue.  Weights are packed K-major [Kp][CoutP], zero padded; a per-layer table gives every k its input offset and (kh, kw).
//                   The pixels of the whole chunk are one flat GEMM dimension (1225 / 289 / 64 per image fit no tile): a tile may span images, but
//                   every output is its own sum over k in k order, so an image's values do not depend on where it sits.  No atomics, no split-K.
//                   Accumulation: an MFMA accumulator takes kFidFlush products, then it is added to a float64 running sum per output and cleared;
//                   bias is added in float64 and the sum is rounded to float once (profiles/fid/README.md has the measurements).
//   pools           max 3x3 s2 (valid, floor), avg 3x3 s1 p1 that does not count the padding, max 3x3 s1 p1; the last two write a temporary the
//                   branch_pool convolution reads.
//   fid_mean        the 8 x 8 mean in float64, positions in index order, rounded once.
// The executor runs the op list that fid_load builds from the block structure (stem, A x3, B, C x4, D, E x2), kFidChunk images at a time
// (DPIR_FID_CHUNK = images forces a smaller chunk), through five engine-owned buffers.
#include "engine.h"
#include "fid.h"
#include <stdlib.h>

namespace dpir {

namespace {
typedef float floatx16 __attribute__((ext_vector_type(16)));
constexpr int BCO = 64, BPX = 64, KC = 32, LR = KC / 4, LDS_LD = 96;      // block tile, rows of it per loader thread; LDS row pitch 96 floats: lanes l and l + 32 (rows k, k + 1) fall in different banks

struct FidConvArgs {
    const float* in; const float* w; const float* bias; const int2* ktab; float* out;
    long long NP;                   // images * Ho * Wo
    int Hin, Win, in_ct, in_c0;
    int Ho, Wo, out_ct, out_c0, Cout, CoutP;
    int stride, ph, pw, Kp, flush;  // flush: K chunks between two flushes of the accumulator (0: never)
};

// ------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void fid_prep_kernel(const uint8_t* u8, const float* f32, int B, int H, int W, float sy, float sx, float* out) {
    const size_t total = (size_t)B * 3 * kFidSide * kFidSide;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % kFidSide), oy = (int)((i / kFidSide) % kFidSide);
    const int c = (int)((i / ((size_t)kFidSide * kFidSide)) % 3);
    const size_t n = i / ((size_t)3 * kFidSide * kFidSide);
    const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1);
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    auto at = [&](int y, int x) {
        return u8 ? (float)u8[((n * H + y) * W + x) * 3 + c] / 255.0f : f32[((n * 3 + c) * H + y) * (size_t)W + x];
    };
    const float top = (1.f - lx) * at(y0, x0) + lx * at(y0, x1), bot = (1.f - lx) * at(y1, x0) + lx * at(y1, x1);
    out[i] = 2.f * ((1.f - ly) * top + ly * bot) - 1.f;
}

__global__ __launch_bounds__(256) void fid_conv_kernel(FidConvArgs p) {
    __shared__ float As[KC * LDS_LD], Bs[KC * LDS_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int wco = wave >> 1, wpx = wave & 1;
    const int co0 = blockIdx.y * BCO;
    const long long px0 = (long long)blockIdx.x * BPX;
    const int HoWo = p.Ho * p.Wo, HinWin = p.Hin * p.Win;
    // loader role: column lp of both tiles, rows lk + 4 r (r < LR)
    const int lp = t & 63, lk = t >> 6;
    const long long gp = px0 + lp;
    const bool pv = gp < p.NP;
    const long long n = pv ? gp / HoWo : 0;
    const int rem = pv ? (int)(gp - n * HoWo) : 0;
    const int oh = rem / p.Wo, ow = rem - oh * p.Wo;
    const int ih0 = oh * p.stride - p.ph, iw0 = ow * p.stride - p.pw;
    const long long base = (n * p.in_ct + p.in_c0) * HinWin + (long long)ih0 * p.Win + iw0;
    // Loads are unconditional (a lane outside the image reads element 0 and discards it) and the table row of chunk c + 2 is fetched while the
    // operands of chunk c + 1 are: the wave waits for memory once per chunk, not once per element.
    float ra[LR], rb[LR];
    int2 kt[LR];
    auto kload = [&](int k0) {
#pragma unroll
        for (int r = 0; r < LR; ++r) kt[r] = p.ktab[k0 + lk + 4 * r];        // < Kp: both tables are padded to it
    };
    auto gload = [&](int k0) {
#pragma unroll
        for (int r = 0; r < LR; ++r) {
            ra[r] = p.w[(size_t)(k0 + lk + 4 * r) * p.CoutP + co0 + lp];
            const int ih = ih0 + (kt[r].y >> 16), iw = iw0 + (kt[r].y & 0xffff);     // a padding row of the table carries kh = 0x4000: never inside
            const bool ok = pv && (unsigned)ih < (unsigned)p.Hin && (unsigned)iw < (unsigned)p.Win;
            const float v = p.in[ok ? base + kt[r].x : 0];
            rb[r] = ok ? v : 0.f;
        }
    };
    floatx16 acc;
    double sum[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.f; sum[r] = 0.0; }
    const int nch = p.Kp / KC;
    int since = 0;
    kload(0);
    gload(0);
    if (nch > 1) kload(KC);
    for (int c = 0; c < nch; ++c) {
#pragma unroll
        for (int r = 0; r < LR; ++r) {
            As[(lk + 4 * r) * LDS_LD + lp] = ra[r];
            Bs[(lk + 4 * r) * LDS_LD + lp] = rb[r];
        }
        __syncthreads();
        if (c + 1 < nch) {
            gload((c + 1) * KC);
            if (c + 2 < nch) kload((c + 2) * KC);
        }
#pragma unroll
        for (int q = 0; q < KC / 2; ++q)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * q + half) * LDS_LD + wco * 32 + l31], Bs[(2 * q + half) * LDS_LD + wpx * 32 + l31], acc, 0, 0, 0);
        __syncthreads();
        if (++since == p.flush) {
            since = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sum[r] += (double)acc[r]; acc[r] = 0.f; }
        }
    }
    const long long op = px0 + wpx * 32 + l31;
    if (op >= p.NP) return;
    const long long on = op / HoWo;
    const int orem = (int)(op - on * HoWo);
    float* dst = p.out + (on * p.out_ct + p.out_c0) * HoWo + orem;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + wco * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (co < p.Cout) dst[(size_t)co * HoWo] = fmaxf((float)((sum[r] + (double)acc[r]) + (double)p.bias[co]), 0.f);
    }
}

// MODE 0: max 3x3 stride 2, valid (floor).  MODE 1: avg 3x3 stride 1 pad 1, the divisor counts the taps inside the image.  MODE 2: max 3x3 stride 1 pad 1.
// One thread per output; src / dst are channel ranges [c0, c0 + C) of NCHW tensors with sct / dct channels.
template <int MODE>
__global__ __launch_bounds__(256) void fid_pool_kernel(const float* src, int sct, int sc0, float* dst, int dct, int dc0, long long N, int C, int Hin, int Win,
                                                       int Ho, int Wo) {
    const long long total = N * C * Ho * Wo;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
    const int c = (int)((i / ((long long)Wo * Ho)) % C);
    const long long n = i / ((long long)Wo * Ho * C);
    const float* s = src + (n * sct + sc0 + c) * Hin * Win;
    const int st = MODE == 0 ? 2 : 1, pad = MODE == 0 ? 0 : 1;
    float m = -INFINITY, a = 0.f;
    int cnt = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int y = oy * st - pad + dy, x = ox * st - pad + dx;
            if ((unsigned)y < (unsigned)Hin && (unsigned)x < (unsigned)Win) {
                const float v = s[y * Win + x];
                m = fmaxf(m, v); a += v; ++cnt;
            }
        }
    dst[((n * dct + dc0 + c) * Ho + oy) * Wo + ox] = MODE == 1 ? a / (float)cnt : m;
}

// feat[n][c] = mean over the hw positions of x[n][c], float64, index order, rounded once
__global__ __launch_bounds__(256) void fid_mean_kernel(const float* x, long long planes, int hw, float* feat) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= planes) return;
    const float* s = x + i * hw;
    double a = 0.0;
    for (int q = 0; q < hw; ++q) a += (double)s[q];
    feat[i] = (float)(a / (double)hw);
}

// ------------------------------------------------------------------------------------------ host: the network as a table
struct Tensor { int buf, c, h, w; };

struct Builder {
    FidState* st;
    int n_taps = 0;
    void use(int buf, int ct, int h, int w) { st->buf_floats[buf] = std::max(st->buf_floats[buf], (size_t)ct * h * w); }
    // BasicConv `name` on channels [0, cin) of src -> channels [dc0, dc0 + cout) of the dct-channel tensor in buffer dst
    Tensor conv(const std::string& name, Tensor src, int cout, int kh, int kw, int stride, int ph, int pw, int dst, int dc0, int dct) {
        FidLayer l{name, src.c, cout, kh, kw, stride, ph, pw};
        l.hin = src.h; l.win = src.w;
        l.ho = (src.h + 2 * ph - kh) / stride + 1; l.wo = (src.w + 2 * pw - kw) / stride + 1;
        l.kp = round_up(src.c * kh * kw, KC); l.coutp = round_up(cout, BCO);
        st->ops.push_back(FidOp{FID_CONV, (int)st->layers.size(), src.buf, 0, src.c, dst, dc0, dct, src.c, src.h, src.w, l.ho, l.wo, -1});
        st->layers.push_back(l);
        use(dst, dct, l.ho, l.wo);
        return Tensor{dst, cout, l.ho, l.wo};
    }
    Tensor conv1(const std::string& name, Tensor src, int cout, int dst, int dc0, int dct) { return conv(name, src, cout, 1, 1, 1, 0, 0, dst, dc0, dct); }
    Tensor pool(int kind, Tensor src, int dst, int dc0, int dct) {
        const int ho = kind == FID_MAXPOOL_S2 ? (src.h - 3) / 2 + 1 : src.h, wo = kind == FID_MAXPOOL_S2 ? (src.w - 3) / 2 + 1 : src.w;
        st->ops.push_back(FidOp{kind, -1, src.buf, 0, src.c, dst, dc0, dct, src.c, src.h, src.w, ho, wo, -1});
        use(dst, dct, ho, wo);
        return Tensor{dst, src.c, ho, wo};
    }
    void tap(Tensor t) {
        st->tap_c[n_taps] = t.c; st->tap_hw[n_taps] = t.h * t.w;
        st->ops.push_back(FidOp{FID_TAP, -1, t.buf, 0, t.c, t.buf, 0, t.c, t.c, t.h, t.w, t.h, t.w, n_taps++});
    }
};
constexpr int T0 = 2, T1 = 3, T2 = 4;

Tensor block_a(Builder& b, const std::string& n, Tensor in, int pf) {
    const int o = in.buf ^ 1, ct = 224 + pf;
    b.conv1(n + ".branch1x1", in, 64, o, 0, ct);
    Tensor t = b.conv1(n + ".branch5x5_1", in, 48, T0, 0, 48);
    b.conv(n + ".branch5x5_2", t, 64, 5, 5, 1, 2, 2, o, 64, ct);
    t = b.conv1(n + ".branch3x3dbl_1", in, 64, T0, 0, 64);
    t = b.conv(n + ".branch3x3dbl_2", t, 96, 3, 3, 1, 1, 1, T1, 0, 96);
    b.conv(n + ".branch3x3dbl_3", t, 96, 3, 3, 1, 1, 1, o, 128, ct);
    t = b.pool(FID_AVG3, in, T2, 0, in.c);
    b.conv1(n + ".branch_pool", t, pf, o, 224, ct);
    return Tensor{o, ct, in.h, in.w};
}
Tensor block_b(Builder& b, const std::string& n, Tensor in) {
    const int o = in.buf ^ 1, ct = 384 + 96 + in.c;
    Tensor r = b.conv(n + ".branch3x3", in, 384, 3, 3, 2, 0, 0, o, 0, ct);
    Tensor t = b.conv1(n + ".branch3x3dbl_1", in, 64, T0, 0, 64);
    t = b.conv(n + ".branch3x3dbl_2", t, 96, 3, 3, 1, 1, 1, T1, 0, 96);
    b.conv(n + ".branch3x3dbl_3", t, 96, 3, 3, 2, 0, 0, o, 384, ct);
    b.pool(FID_MAXPOOL_S2, in, o, 480, ct);
    return Tensor{o, ct, r.h, r.w};
}
Tensor block_c(Builder& b, const std::string& n, Tensor in, int c7) {
    const int o = in.buf ^ 1, ct = 768;
    b.conv1(n + ".branch1x1", in, 192, o, 0, ct);
    Tensor t = b.conv1(n + ".branch7x7_1", in, c7, T0, 0, c7);
    t = b.conv(n + ".branch7x7_2", t, c7, 1, 7, 1, 0, 3, T1, 0, c7);
    b.conv(n + ".branch7x7_3", t, 192, 7, 1, 1, 3, 0, o, 192, ct);
    t = b.conv1(n + ".branch7x7dbl_1", in, c7, T0, 0, c7);
    t = b.conv(n + ".branch7x7dbl_2", t, c7, 7, 1, 1, 3, 0, T1, 0, c7);
    t = b.conv(n + ".branch7x7dbl_3", t, c7, 1, 7, 1, 0, 3, T0, 0, c7);
    t = b.conv(n + ".branch7x7dbl_4", t, c7, 7, 1, 1, 3, 0, T1, 0, c7);
    b.conv(n + ".branch7x7dbl_5", t, 192, 1, 7, 1, 0, 3, o, 384, ct);
    t = b.pool(FID_AVG3, in, T2, 0, in.c);
    b.conv1(n + ".branch_pool", t, 192, o, 576, ct);
    return Tensor{o, ct, in.h, in.w};
}
Tensor block_d(Builder& b, const std::string& n, Tensor in) {
    const int o = in.buf ^ 1, ct = 320 + 192 + in.c;
    Tensor t = b.conv1(n + ".branch3x3_1", in, 192, T0, 0, 192);
    Tensor r = b.conv(n + ".branch3x3_2", t, 320, 3, 3, 2, 0, 0, o, 0, ct);
    t = b.conv1(n + ".branch7x7x3_1", in, 192, T0, 0, 192);
    t = b.conv(n + ".branch7x7x3_2", t, 192, 1, 7, 1, 0, 3, T1, 0, 192);
    t = b.conv(n + ".branch7x7x3_3", t, 192, 7, 1, 1, 3, 0, T0, 0, 192);
    b.conv(n + ".branch7x7x3_4", t, 192, 3, 3, 2, 0, 0, o, 320, ct);
    b.pool(FID_MAXPOOL_S2, in, o, 512, ct);
    return Tensor{o, ct, r.h, r.w};
}
Tensor block_e(Builder& b, const std::string& n, Tensor in, int pool_kind) {
    const int o = in.buf ^ 1, ct = 2048;
    b.conv1(n + ".branch1x1", in, 320, o, 0, ct);
    Tensor t = b.conv1(n + ".branch3x3_1", in, 384, T0, 0, 384);
    b.conv(n + ".branch3x3_2a", t, 384, 1, 3, 1, 0, 1, o, 320, ct);
    b.conv(n + ".branch3x3_2b", t, 384, 3, 1, 1, 1, 0, o, 704, ct);
    t = b.conv1(n + ".branch3x3dbl_1", in, 448, T0, 0, 448);
    t = b.conv(n + ".branch3x3dbl_2", t, 384, 3, 3, 1, 1, 1, T1, 0, 384);
    b.conv(n + ".branch3x3dbl_3a", t, 384, 1, 3, 1, 0, 1, o, 1088, ct);
    b.conv(n + ".branch3x3dbl_3b", t, 384, 3, 1, 1, 1, 0, o, 1472, ct);
    t = b.pool(pool_kind, in, T2, 0, in.c);
    b.conv1(n + ".branch_pool", t, 192, o, 1856, ct);
    return Tensor{o, ct, in.h, in.w};
}

void build_network(FidState* st) {
    Builder b{st};
    Tensor x{0, 3, kFidSide, kFidSide};
    b.use(0, 3, kFidSide, kFidSide);
    x = b.conv("Conv2d_1a_3x3", x, 32, 3, 3, 2, 0, 0, 1, 0, 32);
    x = b.conv("Conv2d_2a_3x3", x, 32, 3, 3, 1, 0, 0, 0, 0, 32);
    x = b.conv("Conv2d_2b_3x3", x, 64, 3, 3, 1, 1, 1, 1, 0, 64);
    x = b.pool(FID_MAXPOOL_S2, x, 0, 0, 64);
    b.tap(x);
    x = b.conv1("Conv2d_3b_1x1", x, 80, 1, 0, 80);
    x = b.conv("Conv2d_4a_3x3", x, 192, 3, 3, 1, 0, 0, 0, 0, 192);
    x = b.pool(FID_MAXPOOL_S2, x, 1, 0, 192);
    b.tap(x);
    x = block_a(b, "Mixed_5b", x, 32); b.tap(x);
    x = block_a(b, "Mixed_5c", x, 64); b.tap(x);
    x = block_a(b, "Mixed_5d", x, 64); b.tap(x);
    x = block_b(b, "Mixed_6a", x); b.tap(x);
    x = block_c(b, "Mixed_6b", x, 128); b.tap(x);
    x = block_c(b, "Mixed_6c", x, 160); b.tap(x);
    x = block_c(b, "Mixed_6d", x, 160); b.tap(x);
    x = block_c(b, "Mixed_6e", x, 192); b.tap(x);
    x = block_d(b, "Mixed_7a", x); b.tap(x);
    x = block_e(b, "Mixed_7b", x, FID_AVG3); b.tap(x);
    x = block_e(b, "Mixed_7c", x, FID_MAX3); b.tap(x);
    st->out_buf = x.buf;
}

Status grow(void** p, size_t* cap, size_t need, size_t elem, const char* what) {
    if (*cap >= need) return Status{};
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc(p, need * elem) != hipSuccess) { (void)hipGetLastError(); return Status{DPIR_ERR_NOMEM, std::string("fid: hipMalloc for ") + what + " failed"}; }
    *cap = need;
    return Status{};
}

Status upload(FidState* st, const void* host, size_t bytes, void** dev) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return Status{DPIR_ERR_NOMEM, "fid: hipMalloc for weights failed"}; }
    st->weight_allocs.push_back(p);
    DPIR_HIP(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    *dev = p;
    return Status{};
}

const dpir_tensor* find(const dpir_tensor* w, int n, const std::string& key) {
    for (int i = 0; i < n; ++i) if (w[i].name && key == w[i].name) return &w[i];
    return nullptr;
}

template <int MODE>
void launch_pool(hipStream_t s, const FidOp& o, const float* src, float* dst, long long N) {
    const long long total = N * o.c * o.ho * o.wo;
    hipLaunchKernelGGL(fid_pool_kernel<MODE>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, o.src_ct, o.src_c0, dst, o.dst_ct, o.dst_c0, N, o.c,
                       o.hin, o.win, o.ho, o.wo);
}
}  // namespace

void fid_free(dpir_engine* e) {
    FidState* st = e->fid;
    if (!st) return;
    for (void* p : st->weight_allocs) (void)hipFree(p);
    for (float* p : st->buf) if (p) (void)hipFree(p);
    for (float* p : st->tap) if (p) (void)hipFree(p);
    if (st->feat) (void)hipFree(st->feat);
    delete st;
    e->fid = nullptr;
}

Status fid_load(dpir_engine* e, const dpir_tensor* weights, int n) {
    DPIR_HIP(hipStreamSynchronize(e->stream));
    fid_free(e);
    std::unique_ptr<FidState> st(new FidState());
    struct Guard { FidState* s; ~Guard() { if (s) for (void* p : s->weight_allocs) (void)hipFree(p); } } guard{st.get()};
    build_network(st.get());
    if ((int)st->layers.size() != kFidConvs) return Status{DPIR_ERR_STATE, "fid: the network table does not have 94 convolutions"};
    for (FidLayer& l : st->layers) {
        const dpir_tensor* tw = find(weights, n, l.name + ".weight");
        if (!tw) return invalid("fid state-dict key missing: " + l.name + ".weight");
        if (tw->ndim != 4 || tw->shape[0] != l.cout || tw->shape[1] != l.cin || tw->shape[2] != l.kh || tw->shape[3] != l.kw)
            return invalid("fid state-dict key " + l.name + ".weight: wrong shape");
        const dpir_tensor* tb = find(weights, n, l.name + ".bias");
        if (!tb) return invalid("fid state-dict key missing: " + l.name + ".bias");
        if (tb->ndim != 1 || tb->shape[0] != l.cout) return invalid("fid state-dict key " + l.name + ".bias: wrong shape");
        if (!tw->data || !tb->data) return invalid("fid state-dict key " + l.name + ": null data");
        // OIHW -> [Kp][CoutP], k = (ci KH + kh) KW + kw, zero padded; the table gives k its offset inside an input image and (kh, kw)
        const int K = l.cin * l.kh * l.kw;
        std::vector<float> packed((size_t)l.kp * l.coutp, 0.f);
        std::vector<int2> ktab(l.kp);
        for (int k = 0; k < l.kp; ++k) {
            if (k >= K) { ktab[k] = int2{0, 0x4000 << 16}; continue; }
            const int ci = k / (l.kh * l.kw), kh = (k / l.kw) % l.kh, kw = k % l.kw;
            ktab[k] = int2{(ci * l.hin + kh) * l.win + kw, (kh << 16) | kw};
            for (int co = 0; co < l.cout; ++co) packed[(size_t)k * l.coutp + co] = tw->data[(size_t)co * K + k];
        }
        void* p = nullptr;
        DPIR_TRY(upload(st.get(), packed.data(), packed.size() * sizeof(float), &p)); l.w = reinterpret_cast<float*>(p);
        DPIR_TRY(upload(st.get(), tb->data, l.cout * sizeof(float), &p)); l.bias = reinterpret_cast<float*>(p);
        DPIR_TRY(upload(st.get(), ktab.data(), ktab.size() * sizeof(int2), &p)); l.ktab = reinterpret_cast<int2*>(p);
    }
    guard.s = nullptr;
    st->loaded = true;
    e->fid = st.release();
    return Status{};
}

Status fid_run(dpir_engine* e, const uint8_t* img_u8, const float* img_f32, int B, int H, int W) {
    FidState* st = e->fid;
    hipStream_t s = e->stream;
    int chunk = kFidChunk;
    if (const char* ev = getenv("DPIR_FID_CHUNK")) { const int v = atoi(ev); if (v >= 1 && v < chunk) chunk = v; }
    chunk = std::min(chunk, B);
    int flush = kFidFlush / KC;
    if (const char* ev = getenv("DPIR_FID_FLUSH")) { const int v = atoi(ev); if (v >= 0) flush = v == 0 ? 0 : std::max(1, v / KC); }     // probe of profiles/fid: products per flush, 0 = never

    if (chunk > st->buf_imgs) {
        for (int i = 0; i < kFidBufs; ++i) {
            size_t cap = st->buf_floats[i] * st->buf_imgs;
            void* p = st->buf[i];
            const Status g = grow(&p, &cap, st->buf_floats[i] * chunk, sizeof(float), "the activations");
            st->buf[i] = reinterpret_cast<float*>(p);
            if (!g.ok()) { st->buf_imgs = 0; return g; }
        }
        st->buf_imgs = chunk;
    }
    {
        void* p = st->feat;
        const Status g = grow(&p, &st->feat_cap, (size_t)B * kFidFeat, sizeof(float), "the features");
        st->feat = reinterpret_cast<float*>(p);
        DPIR_TRY(g);
    }
    for (int k = 0; k < kFidTaps; ++k) st->tap_numel[k] = 0;
    if (e->fid_keep_taps)
        for (int k = 0; k < kFidTaps - 1; ++k) {
            void* p = st->tap[k];
            const Status g = grow(&p, &st->tap_cap[k], (size_t)B * st->tap_c[k] * st->tap_hw[k], sizeof(float), "a feature tap");
            st->tap[k] = reinterpret_cast<float*>(p);
            DPIR_TRY(g);
        }

    const float sy = (float)H / (float)kFidSide, sx = (float)W / (float)kFidSide;
    for (int i0 = 0; i0 < B; i0 += chunk) {
        const long long P = std::min(chunk, B - i0);
        {
            const size_t total = (size_t)P * 3 * kFidSide * kFidSide, off = (size_t)i0 * 3 * H * W;
            hipLaunchKernelGGL(fid_prep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, img_u8 ? img_u8 + off : nullptr,
                               img_f32 ? img_f32 + off : nullptr, (int)P, H, W, sy, sx, st->buf[0]);
            DPIR_HIP(hipGetLastError());
        }
        for (const FidOp& o : st->ops) {
            const float* src = st->buf[o.src];
            float* dst = st->buf[o.dst];
            switch (o.kind) {
            case FID_CONV: {
                const FidLayer& l = st->layers[o.layer];
                FidConvArgs a;
                a.in = src; a.w = l.w; a.bias = l.bias; a.ktab = l.ktab; a.out = dst;
                a.NP = P * l.ho * l.wo;
                a.Hin = l.hin; a.Win = l.win; a.in_ct = o.src_ct; a.in_c0 = o.src_c0;
                a.Ho = l.ho; a.Wo = l.wo; a.out_ct = o.dst_ct; a.out_c0 = o.dst_c0; a.Cout = l.cout; a.CoutP = l.coutp;
                a.stride = l.stride; a.ph = l.ph; a.pw = l.pw; a.Kp = l.kp; a.flush = flush;
                hipLaunchKernelGGL(fid_conv_kernel, dim3((unsigned)((a.NP + BPX - 1) / BPX), (unsigned)(l.coutp / BCO)), dim3(256), 0, s, a);
                break;
            }
            case FID_MAXPOOL_S2: launch_pool<0>(s, o, src, dst, P); break;
            case FID_AVG3: launch_pool<1>(s, o, src, dst, P); break;
            case FID_MAX3: launch_pool<2>(s, o, src, dst, P); break;
            case FID_TAP:
                if (e->fid_keep_taps) {
                    const size_t row = (size_t)o.c * o.hin * o.win;
                    DPIR_HIP(hipMemcpyAsync(st->tap[o.tap] + (size_t)i0 * row, src, (size_t)P * row * sizeof(float), hipMemcpyDeviceToDevice, s));
                    st->tap_numel[o.tap] = (size_t)B * row;
                }
                break;
            }
            DPIR_HIP(hipGetLastError());
        }
        {
            const long long planes = P * kFidFeat;
            hipLaunchKernelGGL(fid_mean_kernel, dim3((unsigned)((planes + 255) / 256)), dim3(256), 0, s, st->buf[st->out_buf], planes,
                               st->tap_hw[kFidTaps - 2], st->feat + (size_t)i0 * kFidFeat);
            DPIR_HIP(hipGetLastError());
        }
    }
    st->tap_numel[kFidTaps - 1] = (size_t)B * kFidFeat;
    return Status{};
}

}  // namespace dpir
