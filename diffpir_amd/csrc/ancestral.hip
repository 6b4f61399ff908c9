// The data side of one ancestral inpainting step in ONE pass over x (HBM-bound): eps -> clamped x0, the posterior mean, the learned-range
// variance, the sample x_{t-1} (or ddim_sample's, eta = 0) and the next step's repaint mix.  Compiled with -ffp-contract=off: every expression
// below is the expression of psample_kernel (grad.hip) / repaint_mix_kernel (elem.hip), operation for operation, so that the pass equals
// dpir_p_sample's arithmetic followed by dpir_repaint_mix bit for bit.
//
// Replaces main_ddpir.py:365-366 behind model_fn's network call -- utils_model.py:219-246 'pred_x_prev' = GaussianDiffusion.p_sample
// (gaussian_diffusion.py:232-333, 395-439) or ddim_sample (:537-585) -- and :356-358 of the NEXT step (repaint), with the torch.randn_like
// draws inside them.
#include "common.h"
#include "ancestral.h"
#include "philox.h"

namespace dpir {

// one element of the pass; ddim and mix are uniform over the grid
__device__ __forceinline__ float ancestral_elem(float x, float eps, float vv, float yv, float m, float n, float nr, const AncestralRowDev& r, float nonzero,
                                                bool ddim, bool mix, float* x0_out, float* premix) {
    const StepDev& c = r.st;
    const float u = c.c1 * x - c.c2 * eps;                          // psample_kernel
    const float xs = fminf(fmaxf(u, -1.0f), 1.0f);
    *x0_out = xs;
    float o;
    if (ddim) {         // eta = 0: eps re-derived from the clamped x0 (gaussian_diffusion.py:345-349, 566), sigma * noise == 0
        const float e2 = (c.c1 * x - xs) / c.c2;
        o = xs * r.sa_prev + r.s1m_prev * e2;
    } else {
        const float frac = (vv + 1.0f) / 2.0f;
        const float lv = frac * r.max_log + (1.0f - frac) * r.min_log;
        const float mean = r.pc1 * xs + r.pc2 * x;
        o = mean + nonzero * expf(0.5f * lv) * n;
    }
    *premix = o;
    if (mix) {                                                      // repaint_mix_kernel with the next step's coefficients
        const float known = r.sa_n * (2.0f * yv - 1.0f) + r.s1m_n * nr;
        o = known * m + (1.0f - m) * o;
    }
    return o;
}

// One thread per group of 4 consecutive elements of one image (group j of image n <-> Philox counter j, as randn_kernel).  VEC: H*W % 4 == 0 and
// every pointer 16-byte aligned -> one 16-byte access per operand and lane, consecutive lanes on consecutive groups; otherwise the same
// groups with scalar accesses and a bounds check on the image's last, partial group.
// x, y, mask and the noise have the image stride P = 3 H W; the network output has 6 H W: element i of image n reads eps at n 6HW + i and v at
// n 6HW + 3HW + i (channel c of x <-> channels c and 3 + c).
template <bool VEC>
__global__ __launch_bounds__(256) void ancestral_step_kernel(AncestralStepArgs a, size_t P, unsigned q) {
    const AncestralRowDev r = a.row ? *a.row : a.row_val;
    const float* y = a.y; const uint8_t* mask = a.mask;
    const float *nps = a.nps, *nr = a.nrp_next;
    unsigned long long seed = a.seed; long long image_offset = a.image_offset;
    float* pm = a.premix_out;
    if (a.lp) {
        const AncestralLoopDev l = *a.lp;
        pm = r.emit ? l.premix : nullptr;
        y = l.y; mask = l.mask; seed = l.seed; image_offset = l.image_offset;
        if (!a.device_noise) {
            const size_t slice = (size_t)r.s * a.B * P;
            nps = l.nps ? l.nps + slice : nullptr;
            nr = l.nrp ? l.nrp + slice + (size_t)a.B * P : nullptr;
        }
    }
    const bool ddim = a.ddim != 0;
    const bool mix = a.mode == 1 && r.mix_next != 0;
    const bool draw = !ddim && r.nonzero != 0;      // the sampler's draw is read: otherwise it is multiplied by 0 (the value used is 0)
    const float nonzero = r.nonzero ? 1.0f : 0.0f;
    if (!mix) pm = nullptr;         // nothing is mixed in: x itself is what the panel shows
    const bool dev = a.device_noise != 0;
    const uint64_t s4 = 4ull * ((uint64_t)r.s + 1ull);
    // images along blockIdx.y, an image's groups along x by grid stride: no integer division per group (q < 2^29 by check_shape)
    for (unsigned n = blockIdx.y; n < (unsigned)a.B; n += gridDim.y)
    for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < q; j += gridDim.x * blockDim.x) {
        const size_t base = (size_t)n * P + (size_t)j * 4;
        const size_t ebase = (size_t)n * 2 * P + (size_t)j * 4;     // eps; v is P further on
        const int cnt = VEC ? 4 : (int)((P - (size_t)j * 4) < 4 ? (P - (size_t)j * 4) : 4);
        float xv[4], ev[4], vv[4], yv[4] = {0.f, 0.f, 0.f, 0.f}, mv[4] = {0.f, 0.f, 0.f, 0.f}, zs[4] = {0.f, 0.f, 0.f, 0.f}, zr[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            const float4 X = *reinterpret_cast<const float4*>(a.x + base);
            const float4 E = *reinterpret_cast<const float4*>(a.out6 + ebase);
            const float4 V = *reinterpret_cast<const float4*>(a.out6 + ebase + P);
            xv[0] = X.x; xv[1] = X.y; xv[2] = X.z; xv[3] = X.w;
            ev[0] = E.x; ev[1] = E.y; ev[2] = E.z; ev[3] = E.w;
            vv[0] = V.x; vv[1] = V.y; vv[2] = V.z; vv[3] = V.w;
            if (mix) {
                const float4 Y = *reinterpret_cast<const float4*>(y + base);
                const uchar4 M = *reinterpret_cast<const uchar4*>(mask + base);
                yv[0] = Y.x; yv[1] = Y.y; yv[2] = Y.z; yv[3] = Y.w;
                mv[0] = (float)M.x; mv[1] = (float)M.y; mv[2] = (float)M.z; mv[3] = (float)M.w;
            }
            if (!dev) {
                if (draw) { const float4 A = *reinterpret_cast<const float4*>(nps + base); zs[0] = A.x; zs[1] = A.y; zs[2] = A.z; zs[3] = A.w; }
                if (mix) { const float4 A = *reinterpret_cast<const float4*>(nr + base); zr[0] = A.x; zr[1] = A.y; zr[2] = A.z; zr[3] = A.w; }
            }
        } else {
            for (int e = 0; e < 4; ++e) {
                const bool in = e < cnt;
                xv[e] = in ? a.x[base + e] : 0.f;
                ev[e] = in ? a.out6[ebase + e] : 0.f;
                vv[e] = in ? a.out6[ebase + P + e] : 0.f;
                if (in && mix) { yv[e] = y[base + e]; mv[e] = (float)mask[base + e]; }
                if (in && !dev) {
                    if (draw) zs[e] = nps[base + e];
                    if (mix) zr[e] = nr[base + e];
                }
            }
        }
        if (dev) {      // the draws randn_kernel would make for these elements: sampler 4 (s + 1), the next step's repaint mix 3 + 4 (s + 1)
            const uint64_t img = (uint64_t)(image_offset + (long long)n);
            if (draw) philox_normal4(seed, s4, img, j, zs);
            if (mix) philox_normal4(seed, 3ull + s4, img, j, zr);
        }
        float ov[4], x0v[4], pv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = ancestral_elem(xv[e], ev[e], vv[e], yv[e], mv[e], zs[e], zr[e], r, nonzero, ddim, mix, &x0v[e], &pv[e]);
        if (VEC) {
            *reinterpret_cast<float4*>(a.x + base) = make_float4(ov[0], ov[1], ov[2], ov[3]);
            if (pm) *reinterpret_cast<float4*>(pm + base) = make_float4(pv[0], pv[1], pv[2], pv[3]);
            if (a.x0_out) *reinterpret_cast<float4*>(a.x0_out + base) = make_float4(x0v[0], x0v[1], x0v[2], x0v[3]);
        } else {
            for (int e = 0; e < cnt; ++e) {
                a.x[base + e] = ov[e];
                if (pm) pm[base + e] = pv[e];
                if (a.x0_out) a.x0_out[base + e] = x0v[e];
            }
        }
    }
}

Status launch_ancestral_step(hipStream_t s, const AncestralStepArgs& a) {
    const size_t P = (size_t)3 * a.HW, q = (P + 3) / 4;
    // H*W % 4 == 0 keeps every image's base (n P, n 2P) and the v planes (+ P) on a 16-byte boundary
    bool vec = !a.scalar_only && a.HW % 4 == 0 && aligned16(a.x) && aligned16(a.out6) && aligned16(a.x0_out) && aligned16(a.premix_out);
    if (!a.lp) vec = vec && aligned16(a.y) && aligned4(a.mask) && aligned16(a.nps) && aligned16(a.nrp_next);
    const dim3 grid = resident_grid(q, a.B, a.cus);
    if (vec) hipLaunchKernelGGL(ancestral_step_kernel<true>, grid, dim3(256), 0, s, a, P, (unsigned)q);
    else hipLaunchKernelGGL(ancestral_step_kernel<false>, grid, dim3(256), 0, s, a, P, (unsigned)q);
    DPIR_HIP(hipGetLastError());
    return Status{};
}

}  // namespace dpir
