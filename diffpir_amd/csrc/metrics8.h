// Declarations for metrics8.hip: the 8-bit evaluation protocol of the reference's standalone programs (calculate_psnr / calculate_ssim on
// tensor2uint bytes, RGB and the Y byte of rgb2ycbcr, with a cropped border) in one pass per batch.
#pragma once
#include "common.h"

namespace dpir {

// What one image reduces to on the device: the SSIM sums over all valid positions (three channels for RGB) and the exact integer sums of
// squared byte differences over the cropped image.  The means and the logarithm are the host's (dpir_metrics_u8).
struct Metrics8Sums {
    double ssim, ssim_y;
    unsigned long long sse, sse_y;
};

constexpr int kM8TileW = 32, kM8TileH = 16;     // SSIM outputs per workgroup
constexpr int kM8Taps = 11, kM8Halo = kM8Taps - 1;

inline int metrics8_tiles(int H, int W, int border) {
    const int vh = H - 2 * border - kM8Halo, vw = W - 2 * border - kM8Halo;
    return ((vh + kM8TileH - 1) / kM8TileH) * ((vw + kM8TileW - 1) / kM8TileW);
}

// Exactly one of est_u8 [B,H,W,3] and est_f32 [B,3,H,W]; gt uint8 [B,H,W,3]; H - 2 border >= 11 and W - 2 border >= 11 (the caller checks).
// partial: workspace of B * metrics8_tiles(H, W, border) entries; out: B entries.  Enqueues two kernels on s.
Status launch_metrics8(hipStream_t s, const uint8_t* est_u8, const float* est_f32, const uint8_t* gt, int B, int H, int W, int border,
                       Metrics8Sums* partial, Metrics8Sums* out);

}  // namespace dpir
