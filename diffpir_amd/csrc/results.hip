// The saved measurement and the L / E / H comparison strip of one batch in ONE pass (HBM-bound).  Compiled with -ffp-contract=off: the byte
// conversion is to_u8 of progress.hip / finalize_kernel (elem.hip), clamp to [0, 1], x 255 in float32, round half to even.
//
// The measurement bytes are util.single2uint (utils_image.py) applied to the ENGINE's own float32 y, the array dpir_degrade returned: bit for bit
// np.uint8((y.clip(0, 1) * 255.).round()) of that array.  They are NOT single2uint of the reference's float64 img_L, which the engine never holds.
//
// Replaces main_ddpir.py:508-511, main_ddpir_deblur.py:423-424 and main_ddpir_inpainting.py:343-344 (single2uint(img_L), the saved measurement),
// main_ddpir_deblur.py:412-421 = main_ddpir_sisr.py:440-451 (img_I: cv2.INTER_NEAREST zoom x sf of the L bytes, the x 3 zoom of the kernel bytes
// written at img_I[:3kh, -3kw:], THEN img_L pasted at img_I[:h, :w]; np.concatenate([img_I, img_E, img_H], axis=1)) and
// main_ddpir_inpainting.py:346-347 (np.concatenate([single2uint(img_L), img_E, img_H], axis=1): the same strip at sf = 1 without an inset).
// The three writes of panel 0 are one per-pixel priority here -- native L over the inset over the zoom -- so no ordering between passes is
// needed.  INTER_NEAREST at an integer factor f reads source pixel floor(destination / f).
#include "common.h"
#include "results.h"

namespace dpir {

__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }

// One thread per group of PIX consecutive pixels of one row, all three channels: the NHWC bytes of a group are contiguous.  An image's groups
// are those of L ([0, qL): h w / PIX) followed by those of the strip ([qL, q): H 3W / PIX); a null output has no groups.
// VEC: w % 4 == 0 (hence W % 4 == 0: a group lies inside one panel, and inside or outside the pasted L) and every pointer aligned -> one
// 16-byte load per channel plane of y, 4-byte loads of est / gt and three 4-byte stores of the 12 interleaved bytes.  Otherwise one pixel per
// thread, scalar accesses.  Images along blockIdx.y, an image's groups along x by grid stride (q < 2^31: H W < 2^29 by check_shape).
template <bool VEC>
__global__ __launch_bounds__(256) void result_panels_kernel(ResultArgs a, unsigned qL, unsigned q) {
    constexpr int PIX = VEC ? 4 : 1;
    const unsigned H = (unsigned)a.H, W = (unsigned)a.W, sf = (unsigned)a.sf, h = H / sf, w = W / sf, hw = h * w, W3 = 3 * W;
    const unsigned ih = a.kv ? 3 * (unsigned)a.kh : 0, iw = a.kv ? 3 * (unsigned)a.kw : 0;      // the inset: rows [0, ih), columns [W - iw, W)
    for (unsigned n = blockIdx.y; n < (unsigned)a.B; n += gridDim.y) {
        const float* yn = a.y + (size_t)n * 3 * hw;
        for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < q; j += gridDim.x * blockDim.x) {
            uint8_t b[PIX * 3];
            uint8_t* dst;
            bool from_y = false;
            unsigned ysrc = 0;
            if (j < qL) {                                                       // the measurement at its own h x w
                ysrc = j * PIX;
                from_y = true;
                dst = a.L_u8 + ((size_t)n * hw + ysrc) * 3;
            } else {
                const unsigned g = (j - qL) * PIX, Y = g / W3, Xs = g - Y * W3, panel = Xs / W, X = Xs - panel * W;
                dst = a.leh_u8 + (((size_t)n * H + Y) * W3 + Xs) * 3;
                if (panel == 0) {
                    if (Y < h && X < w) {                                       // native L on top (VEC: w % 4 == 0, the whole group)
                        ysrc = Y * w + X;
                        from_y = true;
                    } else {
#pragma unroll
                        for (int e = 0; e < PIX; ++e) {
                            const unsigned Xe = X + e;
                            if (Y < ih && Xe >= W - iw) {                       // kernel bytes zoomed x 3, grey on three channels
                                const uint8_t v = a.kv[((size_t)n * a.kh + Y / 3) * a.kw + (Xe - (W - iw)) / 3];
                                b[e * 3] = v; b[e * 3 + 1] = v; b[e * 3 + 2] = v;
                            } else {                                            // L bytes zoomed x sf
                                const unsigned src = (Y / sf) * w + Xe / sf;
#pragma unroll
                                for (int c = 0; c < 3; ++c) b[e * 3 + c] = to_u8(yn[(size_t)c * hw + src]);
                            }
                        }
                    }
                } else {                                                        // est | gt, byte for byte
                    const uint8_t* src = (panel == 1 ? a.est : a.gt) + (((size_t)n * H + Y) * W + X) * 3;
                    if constexpr (VEC) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const uchar4 v = *reinterpret_cast<const uchar4*>(src + 4 * k);
                            b[4 * k] = v.x; b[4 * k + 1] = v.y; b[4 * k + 2] = v.z; b[4 * k + 3] = v.w;
                        }
                    } else {
                        for (int k = 0; k < 3; ++k) b[k] = src[k];
                    }
                }
            }
            if (from_y) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if constexpr (VEC) {
                        const float4 v = *reinterpret_cast<const float4*>(yn + (size_t)c * hw + ysrc);
                        b[c] = to_u8(v.x); b[3 + c] = to_u8(v.y); b[6 + c] = to_u8(v.z); b[9 + c] = to_u8(v.w);
                    } else {
                        b[c] = to_u8(yn[(size_t)c * hw + ysrc]);
                    }
                }
            }
            if constexpr (VEC) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    *reinterpret_cast<uchar4*>(dst + 4 * k) = make_uchar4(b[(4 * k)], b[(4 * k + 1)], b[(4 * k + 2)], b[(4 * k + 3)]);
            } else {
                for (int k = 0; k < 3; ++k) dst[k] = b[k];
            }
        }
    }
}

static bool aligned_to(const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) == 0; }

Status launch_result_panels(hipStream_t s, const ResultArgs& a) {
    if (!a.L_u8 && !a.leh_u8) return Status{};
    const size_t hw = (size_t)(a.H / a.sf) * (a.W / a.sf);
    const bool vec = (a.W / a.sf) % 4 == 0 && aligned_to(a.y, 15) && aligned_to(a.est, 3) && aligned_to(a.gt, 3) && aligned_to(a.L_u8, 3) &&
                     aligned_to(a.leh_u8, 3);
    const size_t pix = vec ? 4 : 1;
    const size_t qL = a.L_u8 ? hw / pix : 0, q = qL + (a.leh_u8 ? (size_t)a.H * a.W * 3 / pix : 0);
    // memory-bound: no more workgroups than the device keeps resident (8 x 256 threads per CU), the rest by grid stride
    const size_t cap = (size_t)(a.cus > 0 ? a.cus : 256) * 8;
    const unsigned gy = (unsigned)(a.B < 65535 ? a.B : 65535);
    size_t gx = (q + 255) / 256, per_image = cap / gy ? cap / gy : 1;
    if (gx > per_image) gx = per_image;
    const dim3 grid((unsigned)gx, gy);
    if (vec) hipLaunchKernelGGL(result_panels_kernel<true>, grid, dim3(256), 0, s, a, (unsigned)qL, (unsigned)q);
    else hipLaunchKernelGGL(result_panels_kernel<false>, grid, dim3(256), 0, s, a, (unsigned)qL, (unsigned)q);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

}  // namespace dpir
