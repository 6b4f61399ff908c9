// One panel of the progressive "process" strip in ONE pass over x (HBM-bound).  Compiled with -ffp-contract=off: x/2+.5 and the uint8
// conversion are finalize_kernel's expressions (elem.hip), operation for operation, so that the last panel equals the loop's own output
// bit for bit.
//
// Replaces main_ddpir_deblur.py:359-371 / main_ddpir_sisr.py:386-398 / main_ddpir_inpainting.py:302-313 (x_show = x/2+.5 kept at the steps of
// progress_seq, np.max / np.min for log_process), :400-406 / :356 (cv2.hconcat of the panels: here each panel is written at its column offset
// of the strip) and main_ddpir_inpainting.py:361-366 (the strip with the known pixels pasted back: y_t mask + (1 - mask) x_show).
#include "common.h"
#include "progress.h"

namespace dpir {

// max / min of floats by integer atomics on the float's own bit image: among non-negative floats the signed integer order is the float order,
// among negative floats the unsigned integer order is the reversed float order, and a slot that holds a float of the other sign is on the
// right side of both comparisons.  Exact and order-independent (no NaN in a panel: a NaN is ignored by fmaxf / fminf before it gets here).
__device__ __forceinline__ void atomic_max_f32(float* addr, float v) {
    if (!(__float_as_uint(v) >> 31)) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_min_f32(float* addr, float v) {
    if (!(__float_as_uint(v) >> 31)) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}

__global__ void progress_minmax_init_kernel(float* mm, int B) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < B) { mm[2 * n] = -INFINITY; mm[2 * n + 1] = INFINITY; }
}

__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }

// One thread per group of PIX consecutive pixels of one image row, all three channels: the NHWC bytes of a group are contiguous.
// VEC: W % 4 == 0 and every pointer aligned -> one 16-byte access per channel plane and three 4-byte stores of the 12 interleaved bytes;
// the strip's row pitch n_panels W and the column offset panel W are then multiples of 4 as well.  Otherwise one pixel per thread, scalar accesses.
// Images along blockIdx.y, an image's groups along x by grid stride (q < 2^29 by check_shape).
template <bool VEC>
__global__ __launch_bounds__(256) void progress_snapshot_kernel(ProgressArgs a, unsigned q) {
    constexpr int PIX = VEC ? 4 : 1;
    __shared__ float smax[4], smin[4];
    const unsigned HW = (unsigned)a.H * (unsigned)a.W, W = (unsigned)a.W;
    const size_t pitch = (size_t)a.n_panels * W, col0 = (size_t)a.panel * W;
    const bool masked = a.masked_f32 || a.masked_u8;
    for (unsigned n = blockIdx.y; n < (unsigned)a.B; n += gridDim.y) {
        float vmax = -INFINITY, vmin = INFINITY;
        for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < q; j += gridDim.x * blockDim.x) {
            const unsigned pix = j * PIX, h = pix / W, w = pix - h * W;
            float v[3][PIX], mv[3][PIX];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t src = ((size_t)n * 3 + c) * HW + pix;
                const size_t dst = (((size_t)n * 3 + c) * a.H + h) * pitch + col0 + w;
                float xv[PIX], yv[PIX] = {}, m[PIX] = {};
                if constexpr (VEC) {
                    const float4 X = *reinterpret_cast<const float4*>(a.x + src);
                    xv[0] = X.x; xv[1] = X.y; xv[2] = X.z; xv[3] = X.w;
                    if (masked) {
                        const float4 Y = *reinterpret_cast<const float4*>(a.y + src);
                        const uchar4 M = *reinterpret_cast<const uchar4*>(a.mask + src);
                        yv[0] = Y.x; yv[1] = Y.y; yv[2] = Y.z; yv[3] = Y.w;
                        m[0] = (float)M.x; m[1] = (float)M.y; m[2] = (float)M.z; m[3] = (float)M.w;
                    }
                } else {
                    xv[0] = a.x[src];
                    if (masked) { yv[0] = a.y[src]; m[0] = (float)a.mask[src]; }
                }
#pragma unroll
                for (int e = 0; e < PIX; ++e) {
                    v[c][e] = xv[e] / 2.0f + 0.5f;                                  // finalize_kernel
                    vmax = fmaxf(vmax, v[c][e]); vmin = fminf(vmin, v[c][e]);
                    mv[c][e] = yv[e] * m[e] + (1.0f - m[e]) * v[c][e];            // main_ddpir_inpainting.py:366
                }
                if constexpr (VEC) {
                    if (a.strip_f32) *reinterpret_cast<float4*>(a.strip_f32 + dst) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
                    if (a.masked_f32) *reinterpret_cast<float4*>(a.masked_f32 + dst) = make_float4(mv[c][0], mv[c][1], mv[c][2], mv[c][3]);
                } else {
                    if (a.strip_f32) a.strip_f32[dst] = v[c][0];
                    if (a.masked_f32) a.masked_f32[dst] = mv[c][0];
                }
            }
            const size_t ub = (((size_t)n * a.H + h) * pitch + col0 + w) * 3;      // NHWC bytes of the group: PIX * 3, contiguous
            if (a.strip_u8) {
                uint8_t b[PIX * 3];
#pragma unroll
                for (int e = 0; e < PIX; ++e)
#pragma unroll
                    for (int c = 0; c < 3; ++c) b[e * 3 + c] = to_u8(v[c][e]);
                if constexpr (VEC) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        *reinterpret_cast<uchar4*>(a.strip_u8 + ub + 4 * k) = make_uchar4(b[(4 * k)], b[(4 * k + 1)], b[(4 * k + 2)], b[(4 * k + 3)]);
                } else {
                    for (int k = 0; k < 3; ++k) a.strip_u8[ub + k] = b[k];
                }
            }
            if (a.masked_u8) {
                uint8_t b[PIX * 3];
#pragma unroll
                for (int e = 0; e < PIX; ++e)
#pragma unroll
                    for (int c = 0; c < 3; ++c) b[e * 3 + c] = to_u8(mv[c][e]);
                if constexpr (VEC) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        *reinterpret_cast<uchar4*>(a.masked_u8 + ub + 4 * k) = make_uchar4(b[(4 * k)], b[(4 * k + 1)], b[(4 * k + 2)], b[(4 * k + 3)]);
                } else {
                    for (int k = 0; k < 3; ++k) a.masked_u8[ub + k] = b[k];
                }
            }
        }
        if (!a.minmax) continue;
        // wave shuffle reduction -> the four waves of the block through LDS -> one pair of memory-side atomics per block
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            vmax = fmaxf(vmax, __shfl_xor(vmax, o));
            vmin = fminf(vmin, __shfl_xor(vmin, o));
        }
        if ((threadIdx.x & 63) == 0) { smax[threadIdx.x >> 6] = vmax; smin[threadIdx.x >> 6] = vmin; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float* mm = a.minmax + ((size_t)a.panel * a.B + n) * 2;
            atomic_max_f32(mm, fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3])));
            atomic_min_f32(mm + 1, fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3])));
        }
        __syncthreads();        // smax / smin are reused by the block's next image
    }
}

static bool aligned_to(const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) == 0; }

Status launch_progress_snapshot(hipStream_t s, const ProgressArgs& a) {
    const bool vec = a.W % 4 == 0 && aligned_to(a.x, 15) && aligned_to(a.strip_f32, 15) && aligned_to(a.masked_f32, 15) && aligned_to(a.y, 15) &&
                     aligned_to(a.mask, 3) && aligned_to(a.strip_u8, 3) && aligned_to(a.masked_u8, 3);
    if (a.minmax) {
        hipLaunchKernelGGL(progress_minmax_init_kernel, dim3((a.B + 255) / 256), dim3(256), 0, s, a.minmax + (size_t)a.panel * a.B * 2, a.B);
        DPIR_HIP(hipGetLastError());
    }
    const size_t q = (size_t)a.H * a.W / (vec ? 4 : 1);
    // memory-bound: no more workgroups than the device keeps resident (8 x 256 threads per CU), the rest by grid stride
    const size_t cap = (size_t)(a.cus > 0 ? a.cus : 256) * 8;
    const unsigned gy = (unsigned)(a.B < 65535 ? a.B : 65535);
    size_t gx = (q + 255) / 256, per_image = cap / gy ? cap / gy : 1;
    if (gx > per_image) gx = per_image;
    const dim3 grid((unsigned)gx, gy);
    if (vec) hipLaunchKernelGGL(progress_snapshot_kernel<true>, grid, dim3(256), 0, s, a, (unsigned)q);
    else hipLaunchKernelGGL(progress_snapshot_kernel<false>, grid, dim3(256), 0, s, a, (unsigned)q);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

}  // namespace dpir
