// Declarations for blur.hip: the deblurring program's measurement operator and its adjoint (main_ddpir_deblur.py:307-311, 317-321).
#pragma once
#include "common.h"

namespace dpir {

// Fused residual of the forward operator: diff = m - out with m = (sa (ma y + mb) + s1m noise) qa + qb (noise may be null: m = (ma y + mb) qa + qb),
// and fp64 partial sums of diff^2, one per workgroup, laid out [B][3 * blur_tiles(H, W)] so that an image's partials are contiguous.
struct BlurResidual {
    const float* y = nullptr; const float* noise = nullptr;
    float ma = 1.f, mb = 0.f, sa = 1.f, s1m = 0.f, qa = 1.f, qb = 0.f;
    float* diff = nullptr; double* part = nullptr;
};
constexpr int BLUR_MAX_K = 79;      // the staged tile (32 + K - 1 rows of 64 + K columns) has to fit 64 KB of LDS
int blur_tiles(int H, int W);       // workgroups per (image, channel) plane
// kh == kw, K odd, K / 2 < H and W, B >= 1 (DPIR_ERR_INVALID); K <= BLUR_MAX_K (DPIR_ERR_UNSUPPORTED).  Nothing is launched on a violation.
Status blur_check(const char* entry, int kh, int kw, int B, int H, int W);
// out[n, c, i, j] = sum_{a, b} k[n, a, b] v[n, c, r_H(i + a - p), r_W(j + b - p)], v = x xa + xb, p = K / 2, r_L = ReflectionPad2d's index map.
// Taps are accumulated with fmaf in ascending (a, b) order.  out may be null when res is given (only the residual is wanted).
Status launch_blur_reflect(hipStream_t s, const float* x, const float* k, int K, float xa, float xb, float* out, int B, int H, int W,
                           const BlurResidual* res = nullptr);
// gx = xa R^T C^T g.  pad: scratch of B * 3 * (H + K - 1) * (W + K - 1) floats (C^T g on the padded grid).
Status launch_blur_reflect_adjoint(hipStream_t s, const float* g, const float* k, int K, float xa, float* pad, float* gx, int B, int H, int W);
// norm[n] = sqrt(sum of image n's per_img partials), folded in index order
Status launch_norm_fold_per_image(hipStream_t s, const double* part, int per_img, int B, float* norm);

}  // namespace dpir
