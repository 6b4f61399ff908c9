// The 8-bit evaluation protocol on the device: util.calculate_psnr and util.calculate_ssim (utils_image.py:586-599, 616-661) on tensor2uint
// bytes, for the RGB image and for the Y byte of rgb2ycbcr(only_y=True) (utils_image.py:446-467), after cropping `border` pixels from all four
// sides (main_ddpir_deblur.py:380, main_ddpir_inpainting.py:325, main_ddpir_sisr.py:406, 459).
//
// One workgroup owns a 32 x 16 tile of SSIM outputs of one image.  It stages the tile and its 10-pixel halo of both images into LDS as bytes
// (42 x 26 x {R, G, B, Y} x 2 = 8.7 KB; a float32 estimate is quantised on the way in exactly as finalize_kernel does, and Y is derived there),
// then runs the separable 11-tap filter in float64 one plane at a time: the five row-pass maps (x, y, x^2, y^2, xy) of one plane are
// 5 x 26 x 32 doubles = 33 KB, so a workgroup holds 42 KB and three of them fit a CU.  Every pixel of the cropped image belongs to exactly one
// tile for the squared-difference sums (the last tile row / column also owns its halo), which are exact 64-bit integers.
//
// Order: a thread adds its outputs in a fixed order, the workgroup adds its threads by a fixed shuffle tree, and metrics8_reduce_kernel adds an
// image's tiles in a fixed order -- no floating-point atomics, so an image's numbers do not depend on its place in the batch, on B or on the run.
// Built with -ffp-contract=off: the only fused multiply-adds are the two written out in y_byte.
#include "metrics8.h"
#include <math.h>

namespace dpir {

namespace {

constexpr int TW = kM8TileW, TH = kM8TileH, RW = TW + kM8Halo, RH = TH + kM8Halo;
constexpr int kThreads = 256;

struct M8Window { double g[kM8Taps]; };

// rgb2ycbcr(uint8, only_y=True): np.dot(img, [65.481, 128.553, 24.966]) / 255.0 + 16.0, .round() (half to even).  This FMA chain is the one
// summation order that reproduces numpy's dot on all 194 byte triplets whose value is an exact .5 tie ("8-bit metrics").
__device__ __forceinline__ uint8_t y_byte(uint8_t r, uint8_t g, uint8_t b) {
    return (uint8_t)rint(fma((double)b, 24.966, fma((double)g, 128.553, (double)r * 65.481)) / 255.0 + 16.0);
}

__device__ __forceinline__ void block_sum(double& a, double& b, unsigned long long& u, unsigned long long& v, Metrics8Sums* dst) {
    __shared__ double red_d[2][kThreads / 64];
    __shared__ unsigned long long red_u[2][kThreads / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64);
        u += __shfl_xor(u, o, 64); v += __shfl_xor(v, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red_d[0][threadIdx.x >> 6] = a; red_d[1][threadIdx.x >> 6] = b;
        red_u[0][threadIdx.x >> 6] = u; red_u[1][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        dst->ssim = (red_d[0][0] + red_d[0][1]) + (red_d[0][2] + red_d[0][3]);
        dst->ssim_y = (red_d[1][0] + red_d[1][1]) + (red_d[1][2] + red_d[1][3]);
        dst->sse = red_u[0][0] + red_u[0][1] + red_u[0][2] + red_u[0][3];
        dst->sse_y = red_u[1][0] + red_u[1][1] + red_u[1][2] + red_u[1][3];
    }
}

__global__ __launch_bounds__(kThreads) void metrics8_tile_kernel(const uint8_t* __restrict__ est_u8, const float* __restrict__ est_f32,
                                                                 const uint8_t* __restrict__ gt, int H, int W, int border, int tiles_x,
                                                                 int tiles_y, M8Window win, Metrics8Sums* __restrict__ partial) {
    __shared__ uint8_t px[2][4][RH][RW];            // [0 estimate, 1 ground truth][R, G, B, Y]
    __shared__ double rowm[5][RH][TW];              // row pass of one plane: x, y, x^2, y^2, xy
    const int tiles = tiles_x * tiles_y;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int Hc = H - 2 * border, Wc = W - 2 * border, vh = Hc - kM8Halo, vw = Wc - kM8Halo;
    const int r0 = ty * TH, c0 = tx * TW;
    const bool last_y = ty == tiles_y - 1, last_x = tx == tiles_x - 1;
    const size_t plane = (size_t)H * W;

    unsigned long long sse = 0, sse_y = 0;
    for (int i = threadIdx.x; i < RH * RW; i += kThreads) {
        const int lr = i / RW, lc = i - lr * RW;
        const int r = r0 + lr, c = c0 + lc;
        const bool in = r < Hc && c < Wc;
        uint8_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
        if (in) {
            const size_t pix = (size_t)(border + r) * W + (border + c);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                b[ch] = gt[((size_t)n * plane + pix) * 3 + ch];
                if (est_u8) a[ch] = est_u8[((size_t)n * plane + pix) * 3 + ch];
                else {
                    // tensor2uint, as finalize_kernel (elem.hip) forms it: clamp, x 255 in float32, round half to even
                    const float q = fminf(fmaxf(est_f32[((size_t)n * 3 + ch) * plane + pix], 0.0f), 1.0f) * 255.0f;
                    a[ch] = (uint8_t)rintf(q);
                }
            }
        }
        const uint8_t ya = y_byte(a[0], a[1], a[2]), yb = y_byte(b[0], b[1], b[2]);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { px[0][ch][lr][lc] = a[ch]; px[1][ch][lr][lc] = b[ch]; }
        px[0][3][lr][lc] = ya; px[1][3][lr][lc] = yb;
        if (in && (lr < TH || last_y) && (lc < TW || last_x)) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { const int d = (int)a[ch] - (int)b[ch]; sse += (unsigned long long)(d * d); }
            const int dy = (int)ya - (int)yb;
            sse_y += (unsigned long long)(dy * dy);
        }
    }

    constexpr double C1 = (0.01 * 255) * (0.01 * 255), C2 = (0.03 * 255) * (0.03 * 255);
    double ssim = 0.0, ssim_y = 0.0;
    for (int p = 0; p < 4; ++p) {
        __syncthreads();                            // px is staged (p = 0) / the column pass of the plane before is done with rowm
        for (int i = threadIdx.x; i < RH * TW; i += kThreads) {
            const int lr = i / TW, oc = i - lr * TW;
            double sa = 0.0, sb = 0.0, saa = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll
            for (int k = 0; k < kM8Taps; ++k) {
                const double a = (double)px[0][p][lr][oc + k], b = (double)px[1][p][lr][oc + k], w = win.g[k];
                sa += w * a; sb += w * b; saa += w * (a * a); sbb += w * (b * b); sab += w * (a * b);
            }
            rowm[0][lr][oc] = sa; rowm[1][lr][oc] = sb; rowm[2][lr][oc] = saa; rowm[3][lr][oc] = sbb; rowm[4][lr][oc] = sab;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < TH * TW; i += kThreads) {
            const int orow = i / TW, oc = i - orow * TW;
            if (r0 + orow >= vh || c0 + oc >= vw) continue;
            double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < kM8Taps; ++k) {
                const double w = win.g[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] += w * rowm[q][orow + k][oc];
            }
            const double mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu1_mu2 = m[0] * m[1];
            const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu1_mu2;
            const double v = ((2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
            if (p < 3) ssim += v; else ssim_y += v;
        }
    }
    block_sum(ssim, ssim_y, sse, sse_y, partial + blockIdx.x);
}

// one workgroup per image: thread t adds tiles t, t + 256, ... in that order, then the same tree as above
__global__ __launch_bounds__(kThreads) void metrics8_reduce_kernel(const Metrics8Sums* __restrict__ partial, int tiles, Metrics8Sums* __restrict__ out) {
    const Metrics8Sums* p = partial + (size_t)blockIdx.x * tiles;
    double a = 0.0, b = 0.0;
    unsigned long long u = 0, v = 0;
    for (int t = threadIdx.x; t < tiles; t += kThreads) { a += p[t].ssim; b += p[t].ssim_y; u += p[t].sse; v += p[t].sse_y; }
    block_sum(a, b, u, v, out + blockIdx.x);
}

}  // namespace

Status launch_metrics8(hipStream_t s, const uint8_t* est_u8, const float* est_f32, const uint8_t* gt, int B, int H, int W, int border,
                       Metrics8Sums* partial, Metrics8Sums* out) {
    const int vh = H - 2 * border - kM8Halo, vw = W - 2 * border - kM8Halo;
    if (B < 1 || border < 0 || vh < 1 || vw < 1 || (est_u8 != nullptr) == (est_f32 != nullptr)) return invalid("metrics8: bad arguments");
    const int tiles_x = (vw + TW - 1) / TW, tiles_y = (vh + TH - 1) / TH;
    if ((long long)tiles_x * tiles_y * B > 0x7fffffffLL) return invalid("metrics8: B * tiles is out of range");
    // cv2.getGaussianKernel(11, 1.5) in float64: exp(-(i - 5)^2 / (2 sigma^2)), normalised to sum 1
    M8Window win;
    double sum = 0.0;
    for (int i = 0; i < kM8Taps; ++i) { const double d = i - (kM8Taps - 1) / 2; win.g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5)); sum += win.g[i]; }
    for (int i = 0; i < kM8Taps; ++i) win.g[i] /= sum;
    hipLaunchKernelGGL(metrics8_tile_kernel, dim3((unsigned)(tiles_x * tiles_y * B)), dim3(kThreads), 0, s, est_u8, est_f32, gt, H, W, border,
                       tiles_x, tiles_y, win, partial);
    DPIR_HIP(hipGetLastError());
    hipLaunchKernelGGL(metrics8_reduce_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, (const Metrics8Sums*)partial, tiles_x * tiles_y, out);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

}  // namespace dpir
