// conv9: the 3x3 convolution of the f16x3 / f16x1 modes for 8 x 8 layers, one workgroup per (image, 32 output channels).
//
// Same arithmetic, operand planes and weight pack as conv6 / conv7 (f16x3: al*bh, ah*bl, ah*bh per product, in that order per
// accumulator), but the workgroup owns the WHOLE image and the WHOLE K for its 32 output channels:
//   * no split-K: launch_conv6 gives a 512 -> 512 @ 8 x 8 layer at B = 16 sixteen workgroups (128 co x 4 images) and therefore sixteen
//     K slices, each writing a full fp32 slab (32 MB for a 2 MB tensor) that gn_act_small / conv6_reduce read back.  Here the grid is
//     B x Cout / 32 workgroups (256 for that layer) and nothing but the result is written;
//   * inside the workgroup the four waves split K: wave w takes the 16-channel chunks w, w + 4, ... and both 32-pixel tiles of the
//     image (two 32 x 32 accumulators).  The partial accumulators are summed through LDS in wave order ((w0 + w1) + w2) + w3, so the
//     result does not depend on the launch, the batch or the dispatch order: a replay is bitwise reproducible, image n of a batch
//     equals the same image alone;
//   * per-(image, channel) fp64 {sum, sum of squares} records are final when the workgroup stores its planes (the record format of
//     the split-K combine, conv6_reduce_kernel), and -- EMIT -- a GroupNorm group of the output (Cout / 32 channels, a divisor of 32)
//     is complete inside the workgroup: the hop conv1 -> GroupNorm + FiLM + SiLU -> conv2 of a ResBlock writes conv2's operand
//     planes from the epilogue without conv7-EMIT's atomics, arrival counters or waiting.
// Each wave stages the 10 x 10 halo patch of ITS chunk by LDS-DMA (out-of-image positions are out-of-range offsets = zeros, as conv6)
// into a private double buffer and loads the 9 taps' A fragments straight into registers one whole chunk ahead (18 b128 loads per
// lane in flight in f16x3): at one wave per SIMD the kernel lives on L2 -> CU latency, not on the matrix pipe.
#include "common.h"
#include "elem.h"
#include "conv_epilogue.h"
#include "conv9.h"

namespace dpir {

constexpr int kC9WaveLds = 16384;                    // per wave: [2 buffers][hi | lo][4 KiB]
constexpr int kC9RedStride = 68;                     // floats per channel row of the cross-wave sum
constexpr int kC9RedBytes = 4 * 32 * kC9RedStride * 4;
constexpr int kC9Lds = 4 * kC9WaveLds;               // the epilogue areas alias the staging buffers
static_assert(kC9RedBytes + 512 + 2 * 4096 <= kC9Lds, "epilogue areas");

template <int HW, bool X1, bool EMIT>
__global__ __launch_bounds__(256, 1) void conv9_image_kernel(Conv9K p) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(HW == 64, "the 8 x 8 image is the one built");
    constexpr int W = 8, H = 8, LW = W + 2, LH = H + 2;
    constexpr int PATCH = LH * LW;                      // entries per k-half
    constexpr int NPIECE = (2 * PATCH + 63) / 64;       // one-KiB DMA pieces per plane
    constexpr int XB = NPIECE * 1024;
    constexpr int NPL = X1 ? 1 : 2;                     // operand planes (hi [, lo])
    constexpr int NACT = NPL * NPIECE;                  // activation DMA instructions per wave and chunk
    constexpr int TAPS = 9;
    static_assert(2 * 2 * XB == kC9WaveLds, "per-wave staging");
    extern __shared__ __attribute__((aligned(16))) char smem9[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int half = lane >> 5;

    // Workgroup b runs on XCD b % 8: the B workgroups that share a weight tile get one XCD and consecutive dispatch slots, so an XCD's
    // L2 keeps at most two weight tiles at a time instead of streaming the whole pack.
    const int tiles = p.Cout >> 5;
    const int bid = blockIdx.x;
    int cot, n;
    if ((tiles & 7) == 0) { cot = (bid & 7) + 8 * (bid / (8 * p.B)); n = (bid >> 3) % p.B; }
    else { cot = bid % tiles; n = bid / tiles; }
    const int co_blk = cot >> 2, ct = cot & 3;

    // ---- activation DMA: every wave stages the patch of its own chunk (out-of-image positions out of range = zeros)
    unsigned x_off[NPIECE];
#pragma unroll
    for (int u = 0; u < NPIECE; ++u) {
        const int f = u * 64 + lane;
        const int kg = f / PATCH;
        const int e = f - kg * PATCH;
        const int hy = e / LW, hx = e - hy * LW;
        const int gy = hy - 1, gx = hx - 1;
        const bool ok = kg < 2 && gy >= 0 && gy < H && gx >= 0 && gx < W;
        x_off[u] = ok ? ((unsigned)((n * p.C8 + kg) * HW + gy * W + gx) << 4) : kOutOfRange;
    }
    const size_t xplane_bytes = (size_t)p.B * p.C8 * HW * 16;
    char* const wlds = smem9 + wave * kC9WaveLds;
    auto dma_x = [&](int chunk, int buf, int q) __attribute__((always_inline)) {
        const int u = X1 ? q : q >> 1, plane = X1 ? 0 : q & 1;
        const size_t coff = (size_t)chunk * 2 * HW * 16;
        const __amdgpu_buffer_rsrc_t rx = rsrc_uniform((plane ? p.xlo : p.xhi) + coff, (unsigned)(xplane_bytes - coff));
        BLDS6(rx, wlds + buf * 2 * XB + plane * XB + u * 1024, x_off[u], 0);
    };

    // ---- B fragments: pixel tile j = rows 4 j .. 4 j + 3 of the image (pixel 32 j + l31), k-half = lane >> 5
    const int lane_b = (l31 >> 3) * LW + (l31 & 7) + half * PATCH;
    const half8* xbase = reinterpret_cast<const half8*>(wlds) + lane_b;

    // ---- A fragments straight from the weight pack: record (chunk, co_blk, co-tile, tap) = 2 KiB [hi | lo], 16 B per lane
    const unsigned lane16 = (unsigned)lane * 16u;
    half8 a_h[TAPS], a_l[TAPS];
    auto load_a = [&](int chunk, auto tap_c) __attribute__((always_inline)) {
        constexpr int tap = decltype(tap_c)::value;
        const char* base = p.w16 + (((size_t)chunk * p.n_co_blocks + co_blk) * 4 + ct) * (TAPS * 2048);
        const __amdgpu_buffer_rsrc_t rw = rsrc_uniform(base, TAPS * 2048);
        a_h[tap] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rw, lane16, tap * 2048u, 0));
        if (!X1) a_l[tap] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rw, lane16, tap * 2048u + 1024u, 0));
    };

    floatx16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    // B fragment sets: tap t >= 1 uses set t & 1, tap 0 the third one (9 taps: tap 8 and the next chunk's tap 0 are both in flight)
    half8 b_h[3][2], b_l[3][2];
    auto read_b = [&](int buf, auto tap_c, auto set_c) __attribute__((always_inline)) {
        constexpr int tap = decltype(tap_c)::value, set = decltype(set_c)::value;
        constexpr int toff = (tap / 3) * LW + (tap % 3);
        const half8* xh = xbase + buf * (2 * XB / 16);
        const half8* xl = xh + XB / 16;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            b_h[set][j] = xh[j * 4 * LW + toff];
            if (!X1) b_l[set][j] = xl[j * 4 * LW + toff];
        }
    };

    // One K chunk of this wave: the next chunk's patch is requested first (NACT DMA instructions into the other buffer); then per tap
    // the B fragments of the NEXT tap are read, the tap's MFMAs issued, and the SAME tap of the next chunk loaded into the A registers
    // just used (one whole chunk ahead: 9 * NPL b128 loads per lane in flight).  The DMA pieces are older than the register loads of
    // taps 0 .. 7, so "at most 8 * NPL outstanding" at tap 8 proves that the patch has landed.  One barrier per round and wave.
    auto chunk_body = [&](auto more_c, int chunk, int cur) __attribute__((always_inline)) {
        constexpr bool MORE = decltype(more_c)::value;
        if (MORE) {
#pragma unroll
            for (int q = 0; q < NACT; ++q) dma_x(chunk + 4, cur ^ 1, q);
        }
        static_for<0, TAPS>([&](auto tap_c) __attribute__((always_inline)) {
            constexpr int tap = decltype(tap_c)::value;
            constexpr int set = tap == 0 ? 2 : (tap & 1);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (tap + 1 < TAPS) {
                read_b(cur, std::integral_constant<int, tap + 1>{}, std::integral_constant<int, (tap + 1) & 1>{});
            } else if (MORE) {
                wait_vmcnt<(TAPS - 1) * NPL>();
                barrier_lds_only();
                read_b(cur ^ 1, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
            }
            __builtin_amdgcn_sched_barrier(0);
            // per accumulator: al * bh, ah * bl, ah * bh -- conv6's order
            if (!X1) {
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_l[tap], b_h[set][j], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_h[tap], b_l[set][j], acc[j], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_h[tap], b_h[set][j], acc[j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (MORE) load_a(chunk + 4, tap_c);
        });
        __builtin_amdgcn_sched_barrier(0);
    };

    // Every wave runs the same number of rounds with one barrier each (inside the chunk body when another chunk follows); a wave whose
    // share of K is used up -- or empty: fewer than four chunks -- only keeps the barrier count.
    const int rounds = (p.n_chunks + 3) >> 2;
    int chunk = wave;
    if (chunk < p.n_chunks) {
#pragma unroll
        for (int q = 0; q < NACT; ++q) dma_x(chunk, 0, q);
        static_for<0, TAPS>([&](auto tap_c) __attribute__((always_inline)) { load_a(chunk, tap_c); });
    }
    wait_vmcnt<0>();
    __syncthreads();
    if (chunk < p.n_chunks) read_b(0, std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{});
    for (int it = 0; it < rounds; ++it, chunk += 4) {
        if (chunk + 4 < p.n_chunks) {
            chunk_body(std::true_type{}, chunk, it & 1);
        } else {
            if (chunk < p.n_chunks) chunk_body(std::false_type{}, chunk, it & 1);
            barrier_lds_only();
        }
    }

    // ---- cross-wave sum in wave order.  acc[j][r] of lane (l31, half) = channel 8 (r >> 2) + 4 half + (r & 3), pixel 32 j + l31.
    float* const red = reinterpret_cast<float*>(smem9);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            red[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * kC9RedStride + j * 32 + l31] = acc[j][r];
    __syncthreads();
    const int ch = tid >> 3, seg = tid & 7;             // this thread: channel ch of the tile, image row seg (8 pixels)
    const int co = cot * 32 + ch;
    float v[8];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float4 lo4 = *reinterpret_cast<const float4*>(red + (w * 32 + ch) * kC9RedStride + seg * 8);
        const float4 hi4 = *reinterpret_cast<const float4*>(red + (w * 32 + ch) * kC9RedStride + seg * 8 + 4);
        const float t[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = w == 0 ? t[i] : v[i] + t[i];
    }
    {
        const float osc = p.out_scale, bv = p.bias[co];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = v[i] * osc + bv;
    }
    const size_t plane = (size_t)n * p.Cout + co;

    if constexpr (!EMIT) {
        if (p.res) {
            float r[8];
            if (p.res_mode == 0) {                          // same shape
                const float4 a = *reinterpret_cast<const float4*>(p.res + plane * HW + seg * 8), b = *reinterpret_cast<const float4*>(p.res + plane * HW + seg * 8 + 4);
                r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
            } else if (p.res_mode == 1) {                   // half resolution, nearest up-sampling
                const float4 a = *reinterpret_cast<const float4*>(p.res + plane * (HW / 4) + (seg >> 1) * (W / 2));
                r[0] = a.x; r[1] = a.x; r[2] = a.y; r[3] = a.y; r[4] = a.z; r[5] = a.z; r[6] = a.w; r[7] = a.w;
            } else {                                        // double resolution, 2 x 2 mean (conv6_reduce_kernel's formula)
                const float* rp = p.res + plane * (4 * HW) + (size_t)(2 * seg) * (2 * W);
#pragma unroll
                for (int h4 = 0; h4 < 4; ++h4) {
                    const float4 a = *reinterpret_cast<const float4*>(rp + h4 * 4), b = *reinterpret_cast<const float4*>(rp + 2 * W + h4 * 4);
                    r[2 * h4] = ((a.x + a.y) + (b.x + b.y)) * 0.25f;
                    r[2 * h4 + 1] = ((a.z + a.w) + (b.z + b.w)) * 0.25f;
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = r[i] + v[i];
        }
        float* op = p.out + plane * HW + seg * 8;
        *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(op + 4) = make_float4(v[4], v[5], v[6], v[7]);
        if (p.stat) {                                       // the split-K combine's record: fp64 sums of the stored plane
            double s = (((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3])) + (((double)v[4] + (double)v[5]) + ((double)v[6] + (double)v[7]));
            double ss = (((double)v[0] * v[0] + (double)v[1] * v[1]) + ((double)v[2] * v[2] + (double)v[3] * v[3])) +
                        (((double)v[4] * v[4] + (double)v[5] * v[5]) + ((double)v[6] * v[6] + (double)v[7] * v[7]));
#pragma unroll
            for (int o = 4; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); ss += __shfl_xor(ss, o, 64); }
            if (seg == 0) p.stat[plane] = make_double2(s, ss);
        }
    } else {
        // ---- fused emission (Conv6Emit without its accumulators / counters): GroupNorm groups are whole inside the 32-channel tile
        double2* const chs = reinterpret_cast<double2*>(smem9 + kC9RedBytes);                 // [32] per-channel {sum, sum of squares}
        _Float16* const th = reinterpret_cast<_Float16*>(smem9 + kC9RedBytes + 512);          // [hi | lo][64 px][32 ch]
        {
            double s = 0.0, ss = 0.0;
#pragma unroll
            for (int i = 0; i < 8; ++i) { s += (double)v[i]; ss += (double)v[i] * v[i]; }
#pragma unroll
            for (int o = 4; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); ss += __shfl_xor(ss, o, 64); }
            if (seg == 0) chs[ch] = make_double2(s, ss);
        }
        __syncthreads();
        const int cg = p.Cout >> 5;                        // channels per group: divides 32 (conv9_supported)
        const int g0 = (ch / cg) * cg;
        double S = 0.0, SS = 0.0;
        for (int k = 0; k < cg; ++k) { S += chs[g0 + k].x; SS += chs[g0 + k].y; }
        const double cntd = (double)cg * HW;
        const double mean = S / cntd;
        double var = SS / cntd - mean * mean;
        if (var < 0) var = 0;
        const float rstd = (float)(1.0 / sqrt(var + 1e-5));
        float a = rstd * p.em.gamma[co];
        float b = p.em.beta[co];
        if (p.em.film) {   // h = GN(h) * (1 + scale) + shift, gn_prm_kernel's arithmetic
            const float* f = p.em.film + (p.em.fstep ? (size_t)p.em.fstep->i * p.em.frows : 0) + (size_t)n * p.em.film_stride + p.em.film_off;
            const float sc = 1.0f + f[co];
            const float sh = f[p.Cout + co];
            a = a * sc;
            b = b * sc + sh;
        }
        const float meanf = (float)mean;
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float x = (v[i] - meanf) * a + b;
            x = silu(x);
            bad |= !(fabsf(x) <= 65000.f);
            x = fminf(fmaxf(x, -65000.f), 65000.f);
            const _Float16 h = (_Float16)x;
            th[(seg * 8 + i) * 32 + ch] = h;
            if (!X1) th[2048 + (seg * 8 + i) * 32 + ch] = (_Float16)(x - (float)h);
        }
        __syncthreads();
        {
            const int c8l = tid >> 6, px = tid & 63;          // one 16-byte plane entry (8 channels of one pixel) per thread
            const size_t eo = (((size_t)n * p.em.C8 + (cot * 4 + c8l)) * HW + px) << 4;
            *reinterpret_cast<u32x4*>(p.em.hi + eo) = *reinterpret_cast<const u32x4*>(th + px * 32 + c8l * 8);
            if (!X1) *reinterpret_cast<u32x4*>(p.em.lo + eo) = *reinterpret_cast<const u32x4*>(th + 2048 + px * 32 + c8l * 8);
        }
        range_report(bad, p.em.range_ctr);
    }
#endif
}

template <bool X1, bool EMIT>
static Status launch9(hipStream_t s, const Conv9K& k, int blocks) {
    auto fn = conv9_image_kernel<64, X1, EMIT>;
    static LdsAttrOnce attr_set;                  // once per kernel pointer (and device)
    DPIR_HIP(attr_set.set(reinterpret_cast<const void*>(fn), kC9Lds));
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(256), kC9Lds, s, k);
    return Status{};
}

bool conv9_supported(int B, int Cin, int Cout, int H, int W, bool emit) { return conv9_refusal(B, Cin, Cout, H, W, emit) == nullptr; }

Status launch_conv9(hipStream_t s, const Conv9Args& a) {
    const bool emit = a.emit != nullptr;
    if (const char* why = conv9_refusal(a.B, a.Cin, a.Cout, a.H, a.W, emit)) return Status{DPIR_ERR_UNSUPPORTED, why};
    if (!a.xhi || (!a.x1 && !a.xlo) || !a.w16 || !a.bias) return invalid("conv9: operand planes, f16 weight pack and bias are required");
    if (a.res && (a.res_mode < 0 || a.res_mode > 2)) return invalid("conv9: bad residual mode");
    Conv9K k{};
    k.xhi = reinterpret_cast<const char*>(a.xhi); k.xlo = reinterpret_cast<const char*>(a.xlo); k.C8 = a.Cin / 8;
    k.w16 = reinterpret_cast<const char*>(a.w16); k.bias = a.bias; k.out = a.out; k.res = a.res; k.res_mode = a.res_mode;
    k.B = a.B; k.Cout = a.Cout; k.n_chunks = a.Cin / 16; k.n_co_blocks = (a.Cout + 127) / 128;
    k.out_scale = 1.0f / a.w16_scale;
    k.stat = a.stat_plane;
    const int blocks = a.B * (a.Cout / 32);
    if (emit) {
        if (a.res || !a.emit->hi || (!a.x1 && !a.emit->lo) || !a.emit->gamma || !a.emit->beta || !a.emit->range_ctr || a.emit->C8 != a.Cout / 8)
            return invalid("conv9: fused emission takes no residual and needs the next convolution's planes, gamma, beta and the range guard");
        k.em = *a.emit;
        DPIR_TRY(a.x1 ? (launch9<true, true>(s, k, blocks)) : (launch9<false, true>(s, k, blocks)));
    } else {
        if (!a.out) return invalid("conv9: no output");
        DPIR_TRY(a.x1 ? (launch9<true, false>(s, k, blocks)) : (launch9<false, false>(s, k, blocks)));
    }
    DPIR_HIP(hipGetLastError());
    return Status{};
}

}  // namespace dpir
