// The data side of one inpainting sub-step in ONE pass over x (HBM-bound): eps -> clamped x0, masked prox, re-noise to t_{i-1}, set-back to
// t_i (resampling, iter_num_U > 1) and the next sub-step's repaint mix.  Compiled with -ffp-contract=off: every expression below is the
// expression of xstart_kernel / prox_mask_kernel / renoise_kernel / ewise_kernel / repaint_mix_kernel (elem.hip), operation for operation,
// so that the pass equals the chain of those launches bit for bit.
//
// Replaces main_ddpir_inpainting.py:249-300 behind model_fn's network call: gaussian_diffusion.py:297,328-333 (x0), :267-268 (prox),
// :288-293 (re-noise), :296-300 (set-back), :244-246 of the NEXT sub-step (repaint), and the torch.randn_like draws inside them.
#include "common.h"
#include "inpaint.h"
#include "philox.h"

namespace dpir {

// one element of the pass; all flags are uniform over the grid
struct InpaintFlags { bool last, prox, with_n1, back, mix; };

__device__ __forceinline__ float inpaint_elem(float x, float eps, float yv, float m, float n1, float n2, float nb, float nr, const InpaintRowDev& r,
                                              float g, const InpaintFlags& f, float* x0_out, float* premix) {
    if (!f.last) {
        const StepDev& c = r.st;
        float v = c.c1 * x - c.c2 * eps;                         // xstart_kernel
        float a = fminf(fmaxf(v, -1.0f), 1.0f);
        if (x0_out) *x0_out = a;
        if (f.prox) {                                            // prox_mask_kernel
            float num = m * (2.0f * yv - 1.0f) + c.tau * a;
            float xp = num / (m + c.tau);
            a = a + g * (xp - a);
        }
        float e = (x - c.sa_t * a) / c.s1m_t;                    // renoise_kernel
        float inner = c.q * e;
        if (f.with_n1) inner = inner + c.es * n1;
        float w = c.sa_p * a + c.k1 * inner;
        w = w + c.k2 * n2;
        x = w;
        if (f.back) {                                            // set-back: ewise mul, mul, add
            float p = x * r.sae;
            float s = nb * r.sb;
            x = p + s;
        }
    }
    *premix = x;
    if (f.mix) {                                                 // repaint_mix_kernel with the next sub-step's coefficients
        float known = r.sa_n * (2.0f * yv - 1.0f) + r.s1m_n * nr;
        x = known * m + (1.0f - m) * x;
    }
    return x;
}

// One thread per group of 4 consecutive elements of one image (group j of image n <-> Philox counter j, as randn_kernel).  VEC: H*W % 4 == 0 and
// every pointer 16-byte aligned -> one 16-byte access per operand and lane, consecutive lanes on consecutive groups; otherwise the same
// groups with scalar accesses and a bounds check on the image's last, partial group.
template <bool VEC>
__global__ __launch_bounds__(256) void inpaint_step_kernel(InpaintStepArgs a, size_t P, unsigned q) {
    const InpaintRowDev r = a.row ? *a.row : a.row_val;
    const float* y = a.y; const uint8_t* mask = a.mask;
    const float *n1 = a.n1, *n2 = a.n2, *nb = a.nback, *nr = a.nrp_next;
    unsigned long long seed = a.seed; long long image_offset = a.image_offset;
    float* pm = a.premix_out;
    if (a.lp) {
        const InpaintLoopDev l = *a.lp;
        pm = r.emit ? l.premix : nullptr;
        y = l.y; mask = l.mask; seed = l.seed; image_offset = l.image_offset;
        if (!a.device_noise) {
            const size_t slice = (size_t)r.s * a.B * P;
            n1 = l.n1 ? l.n1 + slice : nullptr; n2 = l.n2 ? l.n2 + slice : nullptr; nb = l.nback ? l.nback + slice : nullptr;
            nr = l.nrp ? l.nrp + slice + (size_t)a.B * P : nullptr;
        }
    }
    InpaintFlags f;
    f.last = r.st.last != 0;
    f.prox = a.mode == 0;
    f.with_n1 = !f.last && r.st.es != 0.f;
    f.back = !f.last && r.back != 0;
    f.mix = a.mode == 1 && r.mix_next != 0;
    if (f.last && !f.mix) return;
    if (!f.mix) pm = nullptr;       // nothing is mixed in: x itself is what the panel shows
    const bool dev = a.device_noise != 0;
    const uint64_t s4 = 4ull * (uint64_t)r.s;
    // images along blockIdx.y, an image's groups along x by grid stride: no integer division per group (q < 2^29 by check_shape)
    for (unsigned n = blockIdx.y; n < (unsigned)a.B; n += gridDim.y)
    for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < q; j += gridDim.x * blockDim.x) {
        const size_t base = (size_t)n * P + (size_t)j * 4;
        const size_t ebase = (size_t)n * (P / 3) * a.eps_ch + (size_t)j * 4;
        const int cnt = VEC ? 4 : (int)((P - (size_t)j * 4) < 4 ? (P - (size_t)j * 4) : 4);
        float xv[4], ev[4] = {0.f, 0.f, 0.f, 0.f}, yv[4], mv[4], z1[4] = {0.f, 0.f, 0.f, 0.f}, z2[4] = {0.f, 0.f, 0.f, 0.f},
              zb[4] = {0.f, 0.f, 0.f, 0.f}, zr[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            const float4 X = *reinterpret_cast<const float4*>(a.x + base);
            const float4 Y = *reinterpret_cast<const float4*>(y + base);
            const uchar4 M = *reinterpret_cast<const uchar4*>(mask + base);
            float4 E = make_float4(0.f, 0.f, 0.f, 0.f), A1 = E, A2 = E, AB = E, AR = E;
            if (!f.last) E = *reinterpret_cast<const float4*>(a.eps + ebase);
            if (!dev) {
                if (f.with_n1) A1 = *reinterpret_cast<const float4*>(n1 + base);
                if (!f.last) A2 = *reinterpret_cast<const float4*>(n2 + base);
                if (f.back) AB = *reinterpret_cast<const float4*>(nb + base);
                if (f.mix) AR = *reinterpret_cast<const float4*>(nr + base);
            }
            xv[0] = X.x; xv[1] = X.y; xv[2] = X.z; xv[3] = X.w;
            yv[0] = Y.x; yv[1] = Y.y; yv[2] = Y.z; yv[3] = Y.w;
            mv[0] = (float)M.x; mv[1] = (float)M.y; mv[2] = (float)M.z; mv[3] = (float)M.w;
            ev[0] = E.x; ev[1] = E.y; ev[2] = E.z; ev[3] = E.w;
            if (!dev) {
                z1[0] = A1.x; z1[1] = A1.y; z1[2] = A1.z; z1[3] = A1.w;
                z2[0] = A2.x; z2[1] = A2.y; z2[2] = A2.z; z2[3] = A2.w;
                zb[0] = AB.x; zb[1] = AB.y; zb[2] = AB.z; zb[3] = AB.w;
                zr[0] = AR.x; zr[1] = AR.y; zr[2] = AR.z; zr[3] = AR.w;
            }
        } else {
            for (int e = 0; e < 4; ++e) {
                const bool in = e < cnt;
                xv[e] = in ? a.x[base + e] : 0.f;
                yv[e] = in ? y[base + e] : 0.f;
                mv[e] = in ? (float)mask[base + e] : 0.f;
                if (in && !f.last) ev[e] = a.eps[ebase + e];
                if (in && !dev) {
                    if (f.with_n1) z1[e] = n1[base + e];
                    if (!f.last) z2[e] = n2[base + e];
                    if (f.back) zb[e] = nb[base + e];
                    if (f.mix) zr[e] = nr[base + e];
                }
            }
        }
        if (dev) {      // the draws randn_kernel would make for these elements: streams draw + 4 s (1 eta, 2 zeta, 3 repaint), set-back 2^32 + s
            const uint64_t img = (uint64_t)(image_offset + (long long)n);
            if (f.with_n1) philox_normal4(seed, 1ull + s4, img, j, z1);
            if (!f.last) philox_normal4(seed, 2ull + s4, img, j, z2);
            if (f.back) philox_normal4(seed, (1ull << 32) + (uint64_t)r.s, img, j, zb);
            if (f.mix) philox_normal4(seed, 3ull + s4 + 4ull, img, j, zr);
        }
        float ov[4], x0v[4], pv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = inpaint_elem(xv[e], ev[e], yv[e], mv[e], z1[e], z2[e], zb[e], zr[e], r, a.guidance, f, &x0v[e], &pv[e]);
        if (VEC) {
            *reinterpret_cast<float4*>(a.x + base) = make_float4(ov[0], ov[1], ov[2], ov[3]);
            if (pm) *reinterpret_cast<float4*>(pm + base) = make_float4(pv[0], pv[1], pv[2], pv[3]);
            if (a.x0_out && !f.last) *reinterpret_cast<float4*>(a.x0_out + base) = make_float4(x0v[0], x0v[1], x0v[2], x0v[3]);
        } else {
            for (int e = 0; e < cnt; ++e) {
                a.x[base + e] = ov[e];
                if (pm) pm[base + e] = pv[e];
                if (a.x0_out && !f.last) a.x0_out[base + e] = x0v[e];
            }
        }
    }
}

Status launch_inpaint_step(hipStream_t s, const InpaintStepArgs& a) {
    const size_t P = (size_t)3 * a.HW, q = (P + 3) / 4;
    bool vec = !a.scalar_only && a.HW % 4 == 0 && aligned16(a.x) && aligned16(a.eps) && aligned16(a.x0_out) && aligned16(a.premix_out);
    if (!a.lp) vec = vec && aligned16(a.y) && aligned4(a.mask) && aligned16(a.n1) && aligned16(a.n2) && aligned16(a.nback) && aligned16(a.nrp_next);
    const dim3 grid = resident_grid(q, a.B, a.cus);
    if (vec) hipLaunchKernelGGL(inpaint_step_kernel<true>, grid, dim3(256), 0, s, a, P, (unsigned)q);
    else hipLaunchKernelGGL(inpaint_step_kernel<false>, grid, dim3(256), 0, s, a, P, (unsigned)q);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

}  // namespace dpir
