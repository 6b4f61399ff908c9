// What the 3x3 f16 MFMA kernels share behind their main loops.  conv7.hip, conv11.hip, conv_up.hip: the fused-hop rendezvous and the operand
// split with its range guard.  All of them, and conv8.hip, conv9.hip, act.hip: the tile geometries, the vector types and the small
// helpers.  A kernel keeps what follows its own MFMA's C/D layout, and its plain epilogue (residual loader, store pass).
// The rendezvous exists in the device pass only, as the kernel bodies that call it (lds_dma.h).
#pragma once
#include "conv6_params.h"
#include "elem.h"      // StepDev (the FiLM row of the step, read by hop_rendezvous)
#include "lds_dma.h"
#include <type_traits>
namespace dpir {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Workgroup tile of 256 pixels: TI images x 2^LTH rows x 2^LTW columns, staged with a one-pixel halo in 16-byte entries (8 channels).
template <int LTW_, int LTH_, int TI_>
struct TileGeoOf {
    static constexpr int LTW = LTW_, LTH = LTH_, TI = TI_, TW = 1 << LTW_, TH = 1 << LTH_, LW = TW + 2, LH = TH + 2;
    static constexpr int PATCH = TI * LH * LW;             // entries per k-half
    static constexpr int NPIECE = (2 * PATCH + 63) / 64;   // one-KiB DMA pieces per plane (hi or lo)
    static constexpr int XB = NPIECE * 1024;               // bytes per plane and buffer
    static constexpr size_t LDS = (size_t)4 * XB;          // two buffers x (hi, lo); the epilogue slabs and the hop scratch alias them
    static_assert(LDS >= 4 * 32 * 68 * 4 && LDS >= 4 * 512 * 4 + 2 * 2 * 16 * 2 * 8, "epilogue slabs / hop scratch");
};
template <int GEO> struct TileGeo;
template <> struct TileGeo<0> : TileGeoOf<5, 3, 1> {};     // 8 rows x 32 columns
template <> struct TileGeo<1> : TileGeoOf<4, 4, 1> {};     // 16 x 16
template <> struct TileGeo<2> : TileGeoOf<3, 3, 4> {};     // 4 images x 8 x 8

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

template <int CTRL>
__device__ __forceinline__ float dpp_row_shr(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

__device__ __forceinline__ float silu(float v) {
    float e = __builtin_amdgcn_exp2f(v * -1.4426950408889634f);
    return v * __builtin_amdgcn_rcpf(1.0f + e);
}

// f16 operand range guard.  The split clamps to +-65000 so that hi stays finite; a value that needed the clamp (or a NaN)
// makes the result wrong, so it is COUNTED: one atomic per wave that saw one (none in the normal case), read back by
// dpir_sync / dpir_d2h, which then fail with DPIR_ERR_RANGE instead of returning a silently saturated image.  ctr may be null: no guard.
__device__ __forceinline__ void range_report(bool bad, unsigned long long* ctr) {
    const unsigned long long m = __ballot(bad);
    if (m != 0ull && ctr && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) atomicAdd(ctr, (unsigned long long)__builtin_popcountll(m));
}

// One value of an emitted operand plane: GroupNorm + FiLM from the table entry m = {mean, a, b}, SiLU, range flag, clamp, f16 hi / lo split
__device__ __forceinline__ void norm_split(float x, const float4& m, bool& bad, _Float16& h, _Float16& l) {
    float v = (x - m.x) * m.y + m.z;
    v = silu(v);
    bad |= !(fabsf(v) <= 65000.f);
    v = fminf(fmaxf(v, -65000.f), 65000.f);
    h = (_Float16)v;
    l = (_Float16)(v - (float)h);
}

#if defined(__HIP_DEVICE_COMPILE__)
// ---- The fused-hop rendezvous (Conv6Emit) of a wave that owns WAVE_CH output channels (64: conv7, conv11; 32: conv_up) of a workgroup
// of 2 co-halves (cw) x 2 pixel halves (pw).  In: the wave's per-channel {sum, sum of squares} over its pixels in wl[64 ..] / wl[128 ..],
// where wl = lds + wave * 512 floats is the wave's scratch, written by the caller with a wave barrier behind it.  Out: the wave's
// {mean, a, b, 0} GroupNorm + FiLM table in wl + 192.  `arrivals` workgroups -- the tiles of one (image n0, channel block co_blk),
// consecutive ids -- meet here; npix = pixels of the normalised plane.
//
// GroupNorm needs GROUP sums only, and with integer accumulation the order of the additions is immaterial: the channels of a group and
// the two pixel halves of the workgroup are folded here, so that ONE atomic instruction per workgroup (<= 32 groups x {S, SS}) is left.
// (Per-channel atomics from every wave -- 512 per workgroup, 2 M per launch -- cost 0.8 ms per forward: profiles/r04.)  The atomic is a
// memory-side one that RETURNS: once the result is back it has been performed (an agent-scope release fence instead writes back the XCD's
// dirty L2 lines, i.e. everybody's plane stores: +1.5 ms per forward, profiles/r04).
//
// Why the wait ends.  A workgroup waits only for the workgroups of its own (image, channel block): consecutive ids (image-major order, no
// XCD renumbering), at most half of the workgroups the device holds at once (conv_plan.cpp, DeviceCaps).  The dispatcher hands out ids in
// increasing order, and nobody waits before having arrived.  Take the lowest set with a workgroup that has not arrived: every workgroup
// of a lower set has arrived and leaves without waiting for anything else; a member of the set that is not resident yet is preceded only
// by ids of that set or lower ones, and the resident members of the set occupy at most half of the slots, so it is dispatched as soon as
// a lower workgroup leaves (or at once) and arrives after a bounded amount of MFMA work.  Should the assumption fail all the same, the
// spin is bounded and reports through the range guard (2^40), never a hang.
template <int WAVE_CH>
__device__ __forceinline__ void hop_rendezvous(const Conv6K& p, float* lds, float* wl, int wave, int cw, int pw, int lane, int n0, int co_blk, int co_wave, int arrivals, int npix) {
    static_assert(WAVE_CH == 64 || WAVE_CH == 32, "a wave owns 64 or 32 channels");
    constexpr int GS = WAVE_CH / 4;                       // gsum stride: the most groups a wave can own (4 channels per group)
    const int cg = p.Cout >> 5;                           // channels per group: 4, 8, 16 (or 32)
    const int gpw = WAVE_CH / cg;                         // groups per wave
    double* gsum = reinterpret_cast<double*>(lds + 4 * 512);      // [cw 2][pw 2][GS groups][2] behind the per-wave areas
    if (lane < gpw) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < cg; ++k) { s1 += (double)wl[64 + lane * cg + k]; s2 += (double)wl[128 + lane * cg + k]; }
        gsum[((cw * 2 + pw) * GS + lane) * 2] = s1;
        gsum[((cw * 2 + pw) * GS + lane) * 2 + 1] = s2;
    }
    __syncthreads();
    const int gpb = 2 * gpw;                              // groups of this workgroup's channel block
    long long* const accb = p.em.acc + ((size_t)n0 * 32 + (size_t)co_blk * gpb) * 2;
    if (wave == 0) {
        const int gl = lane >> 1, t = lane & 1;           // lane = (group of the block, S | SS)
        long long r = 0;
        if (gl < gpb) {
            const int c2 = gl / gpw, g = gl - c2 * gpw;
            const double v = gsum[((c2 * 2 + 0) * GS + g) * 2 + t] + gsum[((c2 * 2 + 1) * GS + g) * 2 + t];
            r = __hip_atomic_fetch_add(accb + gl * 2 + t, __double2ll_rn(v * (t ? 4096.0 : 1048576.0)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        asm volatile("s_waitcnt vmcnt(0)" : : "v"((int)r) : "memory");
        if (lane == 0) {
            unsigned* cp = p.em.cnt + (size_t)n0 * p.n_co_blocks + co_blk;
            const unsigned old = __hip_atomic_fetch_add(cp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            asm volatile("" : : "v"(old));
            int spins = 0;
            while (__hip_atomic_load(cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < (unsigned)(arrivals + p.em.expect_extra)) {
                switch (p.em.sleep_sel) {          // the argument of s_sleep is an immediate
                    case 0: __builtin_amdgcn_s_sleep(2); break;
                    case 1: __builtin_amdgcn_s_sleep(8); break;
                    case 3: __builtin_amdgcn_s_sleep(32); break;
                    case 4: __builtin_amdgcn_s_sleep(64); break;
                    case 6: __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); break;
                    case 7: __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); break;
                    case 2: __builtin_amdgcn_s_sleep(16); break;
                    default: __builtin_amdgcn_s_sleep(127); break;
                }
                if (++spins > p.em.spin_limit) { atomicAdd(p.em.range_ctr, 1ull << 40); break; }      // never hang the GPU: report through the range guard
            }
        }
    }
    __syncthreads();
    if (WAVE_CH == 64 || lane < WAVE_CH) {
        const int c = co_wave + lane;
        const long long* ap = accb + (size_t)((cw * gpw) + lane / cg) * 2;
        const double S = (double)__hip_atomic_load(ap, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) * (1.0 / 1048576.0);
        const double SS = (double)__hip_atomic_load(ap + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) * (1.0 / 4096.0);
        const double cntd = (double)cg * npix;
        const double mean = S / cntd;
        double var = SS / cntd - mean * mean;
        if (var < 0) var = 0;
        const float rstd = (float)(1.0 / sqrt(var + 1e-5));
        float a = rstd * p.em.gamma[c];
        float b = p.em.beta[c];
        if (p.em.film) {   // h = GN(h) * (1 + scale) + shift   (unet.py:250-251), gn_prm_kernel's arithmetic
            const float* f = p.em.film + (p.em.fstep ? (size_t)p.em.fstep->i * p.em.frows : 0) + (size_t)n0 * p.em.film_stride + p.em.film_off;
            const float sc = 1.0f + f[c];
            const float sh = f[p.Cout + c];
            a = a * sc;
            b = b * sc + sh;
        }
        reinterpret_cast<float4*>(wl + 192)[lane] = make_float4((float)mean, a, b, 0.f);
    }
    __builtin_amdgcn_wave_barrier();
}

#endif
}  // namespace dpir
