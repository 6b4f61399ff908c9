// The measurement operator of the standalone deblurring program and its adjoint (main_ddpir_deblur.py:307-311, 317-321):
//     Tx(x) = conv2d(ReflectionPad2d(K // 2)(x / 2 + 0.5), eye(3) (x) k)
// a dense K x K cross-correlation (taps not flipped) with one PSF per image shared by its three channels, and what torch.autograd
// makes of it in utils_model.grad_and_value (utils/utils_model.py:390-394): gx = 0.5 R^T C^T g.
//
// One kernel serves both directions.  A workgroup of 256 threads owns a 32 x 64 output tile of one (image, channel) plane and stages
// the (32 + K - 1) x (64 + K) source window in LDS once; the border rule is resolved while staging (forward: reflection, the edge sample
// not repeated; adjoint: zeros around g), so the tap loop has no index arithmetic.  A thread keeps 8 horizontally adjacent outputs in
// registers and slides a 16-wide register window over its LDS row: 8 new LDS words feed 64 fmaf.  The PSF index depends on the
// workgroup and the loop counters only, so the taps travel the scalar path.  Every output accumulates its K * K taps with fmaf in
// ascending (a, b) order whatever the tile, plane or batch: image n of a batch is bit-identical to the same image run alone.
// The adjoint is the same correlation with the PSF read back to front over the zero-padded gradient (C^T g on the (H + 2p) x (W + 2p)
// grid), then a gather that folds the reflected border onto the interior: each pixel sums the at most 3 x 3 padded positions that
// ReflectionPad2d read it from, in a fixed order.  No atomics anywhere.
#include "blur.h"

namespace dpir {

namespace {
constexpr int TH = 32, TW = 64, PER = 8;        // output tile, outputs per thread (256 threads = 32 rows x 8 column groups)

__host__ __device__ inline int blur_kp(int K) { return (K + PER - 1) & ~(PER - 1); }      // taps per row, padded with zeros to the window step
__host__ __device__ inline int blur_stride(int K) { return TW + blur_kp(K) + 4; }         // (stride / 4) odd: rows 4 banks apart for the 16-byte reads

template <bool ADJ>
__global__ __launch_bounds__(256) void blur_tile_kernel(const float* __restrict__ src, const float* __restrict__ k, int K, float xa, float xb,
                                                        float* __restrict__ out, int Hs, int Ws, int Ho, int Wo, int off, BlurResidual res,
                                                        bool with_res) {
#pragma clang fp contract(off)
    extern __shared__ float tile[];
    const int pl = blockIdx.z, n = pl / 3;
    const int i0 = blockIdx.y * TH, j0 = blockIdx.x * TW;
    const int Kp = blur_kp(K), ncols = TW + Kp, stride = ncols + 4, rows = TH + K - 1;
    const float* sp = src + (size_t)pl * Hs * Ws;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int u = wave; u < rows; u += 4) {
        int si = i0 + u - off;
        bool rin = si >= 0 && si < Hs;
        if (!ADJ) { si = si < 0 ? -si : si; si = si > Hs - 1 ? 2 * (Hs - 1) - si : si; }
        si = si < 0 ? 0 : (si > Hs - 1 ? Hs - 1 : si);              // rows that only feed outputs outside the plane: any finite value
        // ncols <= 64 + 80 (BLUR_MAX_K): at most three columns per lane.  The loads are unconditional on clamped indices so that all three are in flight together
        float vals[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            int sj = j0 + lane + 64 * q - off;
            const bool cin = sj >= 0 && sj < Ws;
            if (!ADJ) { sj = sj < 0 ? -sj : sj; sj = sj > Ws - 1 ? 2 * (Ws - 1) - sj : sj; }
            sj = sj < 0 ? 0 : (sj > Ws - 1 ? Ws - 1 : sj);
            const float val = sp[(size_t)si * Ws + sj];
            vals[q] = ADJ ? ((rin && cin) ? val : 0.f) : val * xa + xb;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (lane + 64 * q < ncols) tile[u * stride + lane + 64 * q] = vals[q];
    }
    __syncthreads();
    const int ty = threadIdx.x >> 3, tx = threadIdx.x & 7;
    const float* kp = k + (size_t)n * K * K;
    float acc[PER];
#pragma unroll
    for (int o = 0; o < PER; ++o) acc[o] = 0.f;
    for (int a = 0; a < K; ++a) {
        const float* trow = tile + (ty + a) * stride + tx * PER;
        const int krow = (ADJ ? K - 1 - a : a) * K;
        float w[2 * PER];
        {
            const float4 l0 = *reinterpret_cast<const float4*>(trow), l1 = *reinterpret_cast<const float4*>(trow + 4);
            w[0] = l0.x; w[1] = l0.y; w[2] = l0.z; w[3] = l0.w; w[4] = l1.x; w[5] = l1.y; w[6] = l1.z; w[7] = l1.w;
        }
        for (int b0 = 0; b0 < Kp; b0 += PER) {
            const float4 h0 = *reinterpret_cast<const float4*>(trow + b0 + PER), h1 = *reinterpret_cast<const float4*>(trow + b0 + PER + 4);
            w[8] = h0.x; w[9] = h0.y; w[10] = h0.z; w[11] = h0.w; w[12] = h1.x; w[13] = h1.y; w[14] = h1.z; w[15] = h1.w;
            float kv[PER];
#pragma unroll
            for (int bb = 0; bb < PER; ++bb) {              // uniform per workgroup: scalar loads; taps past the row end are zeros
                const int b = b0 + bb, bc = b < K ? b : K - 1;
                const float t = kp[krow + (ADJ ? K - 1 - bc : bc)];
                kv[bb] = b < K ? t : 0.f;
            }
#pragma unroll
            for (int bb = 0; bb < PER; ++bb)
#pragma unroll
                for (int o = 0; o < PER; ++o) acc[o] = fmaf(kv[bb], w[bb + o], acc[o]);
#pragma unroll
            for (int o = 0; o < PER; ++o) w[o] = w[PER + o];
        }
    }
    const int i = i0 + ty, jb = j0 + tx * PER;
    const size_t base = ((size_t)pl * Ho + i) * Wo + jb;
    double ssq = 0.0;
    if (i < Ho) {
        if (out) {
            if ((Wo & 3) == 0 && jb + PER <= Wo) {
                *reinterpret_cast<float4*>(out + base) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                *reinterpret_cast<float4*>(out + base + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
            } else {
#pragma unroll
                for (int o = 0; o < PER; ++o) if (jb + o < Wo) out[base + o] = acc[o];
            }
        }
        if (with_res) {
#pragma unroll
            for (int o = 0; o < PER; ++o) {
                if (jb + o >= Wo) continue;
                float m = res.y[base + o] * res.ma + res.mb;
                if (res.noise) m = res.sa * m + res.s1m * res.noise[base + o];
                m = m * res.qa + res.qb;
                const float d = m - acc[o];
                res.diff[base + o] = d;
                ssq += (double)d * (double)d;
            }
        }
    }
    if (with_res) {
        __shared__ double red[4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ssq += __shfl_xor(ssq, o, 64);
        if (lane == 0) red[wave] = ssq;
        __syncthreads();
        if (threadIdx.x == 0)
            res.part[((size_t)pl * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// gx[i, j] = xa * sum over the padded positions (u, v) with r_H(u - p) = i, r_W(v - p) = j of pad[u, v]: u = i + p always, p - i when
// 1 <= i <= p (the top reflection), 2 (H - 1) - i + p when H - 1 - p <= i <= H - 2 (the bottom one); both can hold when p is close to H.
__global__ __launch_bounds__(256) void blur_fold_kernel(const float* __restrict__ pad, float xa, float* __restrict__ gx, int H, int W, int p) {
#pragma clang fp contract(off)
    const int pl = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= H * W) return;
    const int i = e / W, j = e - i * W;
    const int Wp = W + 2 * p;
    const float* pp = pad + (size_t)pl * (H + 2 * p) * Wp;
    int us[3], vs[3], nu = 0, nv = 0;
    us[nu++] = i + p;
    if (i >= 1 && i <= p) us[nu++] = p - i;
    if (i <= H - 2 && i >= H - 1 - p) us[nu++] = 2 * (H - 1) - i + p;
    vs[nv++] = j + p;
    if (j >= 1 && j <= p) vs[nv++] = p - j;
    if (j <= W - 2 && j >= W - 1 - p) vs[nv++] = 2 * (W - 1) - j + p;
    float acc = 0.f;
    for (int a = 0; a < nu; ++a)
        for (int b = 0; b < nv; ++b) acc += pp[(size_t)us[a] * Wp + vs[b]];
    gx[(size_t)pl * H * W + e] = acc * xa;
}

__global__ void norm_fold_per_image_kernel(const double* part, int per_img, int B, float* norm) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= B) return;
    double s = 0.0;
    for (int i = 0; i < per_img; ++i) s += part[(size_t)n * per_img + i];
    norm[n] = (float)sqrt(s);
}
}  // namespace

int blur_tiles(int H, int W) { return ((H + TH - 1) / TH) * ((W + TW - 1) / TW); }

Status blur_check(const char* entry, int kh, int kw, int B, int H, int W) {
    const std::string en(entry);
    if (B < 1 || H < 1 || W < 1) return invalid(en + ": B, H, W must be >= 1");
    if ((long long)H * W > 0x1fffffffLL) return invalid(en + ": H * W is out of range");
    if (kh < 1 || kh != kw) return invalid(en + ": the PSF must be square (kh == kw)");
    if ((kh & 1) == 0) return invalid(en + ": the PSF size must be odd (an even K gives an output that is not y's size)");
    if (kh / 2 >= H || kh / 2 >= W) return invalid(en + ": K / 2 must be smaller than H and W (ReflectionPad2d refuses a pad >= the size)");
    if ((long long)B * 3 > 65535) return invalid(en + ": B * 3 exceeds the grid limit");
    if (kh > BLUR_MAX_K) return Status{DPIR_ERR_UNSUPPORTED, en + ": PSFs larger than 79 x 79 are not implemented (the staged tile has to fit 64 KB of LDS)"};
    return Status{};
}

template <bool ADJ>
static Status launch_tile(hipStream_t s, const float* src, const float* k, int K, float xa, float xb, float* out, int B, int Hs, int Ws, int Ho, int Wo,
                          int off, const BlurResidual* res) {
    const dim3 grid((Wo + TW - 1) / TW, (Ho + TH - 1) / TH, B * 3);
    const size_t lds = (size_t)(TH + K - 1) * blur_stride(K) * sizeof(float);
    hipLaunchKernelGGL((blur_tile_kernel<ADJ>), grid, dim3(256), lds, s, src, k, K, xa, xb, out, Hs, Ws, Ho, Wo, off, res ? *res : BlurResidual{},
                       res != nullptr);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

Status launch_blur_reflect(hipStream_t s, const float* x, const float* k, int K, float xa, float xb, float* out, int B, int H, int W,
                           const BlurResidual* res) {
    if (res && (!res->y || !res->diff || !res->part)) return invalid("blur_reflect: the residual needs y, diff and part");
    return launch_tile<false>(s, x, k, K, xa, xb, out, B, H, W, H, W, K / 2, res);
}

Status launch_blur_reflect_adjoint(hipStream_t s, const float* g, const float* k, int K, float xa, float* pad, float* gx, int B, int H, int W) {
    const int p = K / 2;
    DPIR_TRY(launch_tile<true>(s, g, k, K, 1.f, 0.f, pad, B, H, W, H + 2 * p, W + 2 * p, 2 * p, nullptr));
    hipLaunchKernelGGL(blur_fold_kernel, dim3((H * W + 255) / 256, B * 3), dim3(256), 0, s, pad, xa, gx, H, W, p);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

Status launch_norm_fold_per_image(hipStream_t s, const double* part, int per_img, int B, float* norm) {
    hipLaunchKernelGGL(norm_fold_per_image_kernel, dim3((B + 63) / 64), dim3(64), 0, s, part, per_img, B, norm);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

}  // namespace dpir
