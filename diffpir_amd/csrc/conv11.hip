// conv11: conv7's 8 x 32 geometry with v_mfma_f32_16x16x32_f16 in the main loop (conv7: 32x32x16).  Same workgroup tile (128 output
// channels x 8 rows x 32 columns, 256 threads), same wave tile (64 co x 128 px = 4 M-tiles x 8 N-tiles = 32 accumulators of 4 registers,
// 128 in all as conv7's 8 of 16), same operand planes by LDS-DMA, weights straight into registers from a host pack in lane order, f16x3
// products per accumulator in conv6's order (al*bh, ah*bl, ah*bh), same weight scale and out_scale, same epilogue.  Every individual
// product equals conv7's; the fp32 accumulation order inside K differs, so outputs agree to rounding, not bit for bit.
//
// K = 32 per instruction, planes in 16-channel chunks: the flattened (chunk, tap) sequence is walked in consecutive PAIRS -- lanes 0-31
// carry the first (chunk, tap) of a pair, lanes 32-63 the second, (lane >> 4) & 1 is the 8-channel half of the chunk.  Over a period of two
// chunks (18 entries, 9 pair steps):  even chunk (0,1) (2,3) (4,5) (6,7), then (8, odd chunk's 0), odd chunk (1,2) (3,4) (5,6) (7,8).
// Only step 4 reads both patch buffers, so conv7's double buffer (44 KiB, two workgroups per CU) is enough.  (Pairing two chunks of the
// same tap needs four resident patches, 87 KiB: one workgroup per CU.)  Per period three barriers instead of conv7's two: before step 4
// (the odd chunk has landed), after step 4's reads (buffer 0 may be refilled), at the end (the next even chunk has landed, buffer 1 is free).
//
// A step = 4 groups (one pixel row of the wave's four, two N-tiles) of 4 M-tiles x 2 N-tiles x 3 = 24 MFMAs; the B fragments of the next
// group are read while a group runs (two register sets), the 8 A fragments of the next step (4 M-tiles x hi / lo, 8 KiB per wave) are
// requested at the start of a step into the other of two register slots.  9 steps per period is odd, so the slot parity alternates from
// period to period: the period body is instantiated for both parities.
//
// Measured back to back against conv7 on one box, random planes, B = 16 (profiles/conv11/README.md): x0.92-0.94 of conv7's time on every
// routed shape of the FFHQ forward (128 -> 128 @256^2 762 -> 714 us, 256 -> 128 @256^2 1376 -> 1281, 256 -> 256 @128^2 706 -> 657); forward,
// DPIR_CONV11=1/0 interleaved in one call: 16.92 vs 17.71 ms.  f16x3 only; f16x1, split-K launches, the 16 x 16 and 8 x 8 geometries, partial
// co-blocks and gradient mode stay on launch_conv6 (plan_conv3, conv_plan.cpp).
#include "common.h"
#include "elem.h"
#include "conv_epilogue.h"
#include "conv11.h"
#include <atomic>

namespace dpir {

namespace c11 {
using G = TileGeo<0>;                               // conv7's 8 x 32 tile
constexpr int LW = G::LW, NPIECE = G::NPIECE, XB = G::XB;
constexpr int NXT = (NPIECE + 3) / 4;               // per wave and plane
constexpr int NACT = 2 * NXT;                       // activation DMA instructions per wave and chunk (hi, lo)
constexpr int TAPS = 9;
[[maybe_unused]] constexpr int STEPS = 9;            // pair steps per period of two chunks
constexpr size_t LDS = G::LDS;
[[maybe_unused]] constexpr int AREC = 8 * 1024;                     // weight bytes per (pair step, co-block, wave co-half): 4 M-tiles x (hi, lo) x 1 KiB
static_assert(NACT == 6, "two pieces per step in the first three steps of a window");
// entry q of a period (0 .. 17): chunk parity q / 9 = patch buffer, tap q % 9 -> offset of the fragment read, in 16-byte entries
constexpr int frag_off(int q) { return (q / TAPS) * (2 * XB / 16) + ((q % TAPS) / 3) * LW + (q % TAPS) % 3; }
}  // namespace c11

// EMIT: the fused hop to the next convolution of a ResBlock (Conv6Emit, conv7's contract).  Everything up to the epilogue is the same kernel;
// workgroups keep their natural order (image-major, the co-block outside the tiles of an image), so that the workgroups that wait for one
// another -- the tiles of one (image, co-block) -- are consecutive ids.
template <bool EMIT>
__global__ __launch_bounds__(256, 2) void conv11_mfma_kernel(Conv6K p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using namespace c11;
    constexpr int TW = G::TW, TH = G::TH, PATCH = G::PATCH;
    extern __shared__ __attribute__((aligned(16))) char smem11[];      // [2 buffers][hi|lo][XB]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cw = wave & 1, pw = wave >> 1;       // co half (64 channels), pixel half (rows 4 pw .. 4 pw + 3)
    const int l15 = lane & 15;
    const int khalf = (lane >> 4) & 1;             // 8-channel half of the 16-channel chunk
    const bool second = lane >= 32;                // which (chunk, tap) of the pair

    int bid = blockIdx.x;
    if (!EMIT && (gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);      // XCD-contiguous tiles, as conv6 / conv7
    const int tiles_per_img = p.tiles_x * p.tiles_y;
    const int per_img = tiles_per_img * p.n_co_blocks;
    const int co_blk = EMIT ? (bid % per_img) / tiles_per_img : bid % p.n_co_blocks;
    const int ptile = EMIT ? (bid / per_img) * tiles_per_img + (bid % per_img) % tiles_per_img : bid / p.n_co_blocks;
    const int n0 = ptile / tiles_per_img;
    const int trem = ptile - n0 * tiles_per_img;
    const int co_wave = co_blk * 128 + cw * 64;              // this wave's first output channel
    const int ty0 = (trem / p.tiles_x) * TH;
    const int tx0 = (trem % p.tiles_x) * TW;
    const int HW = p.H * p.W;
    const int nper = p.n_chunks_total >> 1;

    // ---- activation DMA: conv7's (pieces dealt to the 4 waves, out-of-image positions out of range = zeros)
    unsigned x_off[NXT];
#pragma unroll
    for (int u = 0; u < NXT; ++u) {
        int piece = wave + u * 4;
        if (piece > NPIECE - 1) piece = NPIECE - 1;
        const int f = piece * 64 + lane;
        const int kg = f / PATCH;
        const int e = f - kg * PATCH;
        const int hy = e / LW, hx = e - hy * LW;
        const int gy = ty0 + hy - 1, gx = tx0 + hx - 1;
        const bool ok = kg < 2 && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
        x_off[u] = ok ? ((unsigned)((n0 * p.C8 + kg) * HW + gy * p.W + gx) << 4) : kOutOfRange;
    }
    const size_t xplane_bytes = (size_t)p.B * p.C8 * HW * 16;
    auto dma_x = [&](int chunk, int buf, int q) __attribute__((always_inline)) {
        const int u = q >> 1, plane = q & 1;
        int piece = wave + u * 4;
        if (piece > NPIECE - 1) piece = NPIECE - 1;
        const size_t coff = (size_t)chunk * 2 * HW * 16;
        const __amdgpu_buffer_rsrc_t rx = rsrc_uniform((plane ? p.xlo : p.xhi) + coff, (unsigned)(xplane_bytes - coff));
        BLDS6(rx, smem11 + buf * 2 * XB + plane * XB + piece * 1024, x_off[u], 0);
    };

    // ---- B fragments: N-tile (row j of the wave's four, column half cb) = 16 pixels; a lane reads the entry of its pixel, its k-half
    // and its (chunk, tap) of the pair.  The second entry of a pair lies 1 (next tap, same row), LW - 2 (next tap row) or -- step 4 -- one
    // buffer minus two rows and two columns behind the first: three lane pointers, everything else is an immediate offset.
    const half8* const xlane = reinterpret_cast<const half8*>(smem11) + l15 + khalf * PATCH + 4 * pw * LW;
    const half8* const xb_next = xlane + (second ? 1 : 0);
    const half8* const xb_row = xlane + (second ? LW - 2 : 0);
    const half8* const xb_buf = xlane + (second ? frag_off(TAPS) - frag_off(TAPS - 1) : 0);
    auto xstep = [&](int s) __attribute__((always_inline)) -> const half8* {       // s is a compile-time constant after unrolling
        const int d = frag_off(2 * s + 1) - frag_off(2 * s);
        return (d == 1 ? xb_next : (d == LW - 2 ? xb_row : xb_buf)) + frag_off(2 * s);
    };

    // ---- A fragments straight from the pack: 8 KiB per (pair step, co-block, co-half) = [M-tile][hi | lo] 1 KiB records, 16 B per lane
    const unsigned lane16 = (unsigned)lane * 16u;
    half8 a_h[2][4], a_l[2][4];
    auto load_a = [&](int step, int slot) __attribute__((always_inline)) {
        const char* base = p.w16 + (((size_t)step * p.n_co_blocks + co_blk) * 2 + cw) * AREC;
        const __amdgpu_buffer_rsrc_t rw = rsrc_uniform(base, (unsigned)AREC);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            a_h[slot][m] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rw, lane16, (unsigned)(m * 2048), 0));
            a_l[slot][m] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rw, lane16, (unsigned)(m * 2048 + 1024), 0));
        }
    };

    floatx4 acc[4][8];                             // [M-tile][N-tile = 2 j + cb]
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 8; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[m][n][r] = 0.f;

    half8 b_h[2][2], b_l[2][2];                    // two sets (one in use, one being filled) of two N-tiles
    auto read_b = [&](const half8* xp, int j, int set) __attribute__((always_inline)) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int o = j * LW + cb * 16;
            b_h[set][cb] = xp[o];
            b_l[set][cb] = xp[XB / 16 + o];
        }
    };
    auto mfma_group = [&](int j, int set, int slot) __attribute__((always_inline)) {
        // per accumulator: al * bh, ah * bl, ah * bh -- conv6's order
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[m][2 * j + cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_l[slot][m], b_h[set][cb], acc[m][2 * j + cb], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[m][2 * j + cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_h[slot][m], b_l[set][cb], acc[m][2 * j + cb], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[m][2 * j + cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_h[slot][m], b_h[set][cb], acc[m][2 * j + cb], 0, 0, 0);
    };

    // ---- prologue: first patch, weights of step 0
#pragma unroll
    for (int q = 0; q < NACT; ++q) dma_x(0, 0, q);
    load_a(0, 0);
    wait_vmcnt<0>();
    __syncthreads();
    read_b(xstep(0), 0, 0);

    // One period: steps 0-3 read buffer 0 (even chunk), step 4 both, steps 5-8 buffer 1 (odd chunk).  Steps 0-2 request the odd chunk into
    // buffer 1, steps 5-7 the next even chunk into buffer 0 (two pieces each, in front of the step's weight request): where a landed
    // patch is needed (end of steps 3 and 8) the only younger loads are the 8 weight fragments of the next step.
    // In the last period the prefetches past the end fetch the last chunk / the last step again (L2 hits, never read): the instruction stream
    // -- and the counted waits -- are the same in every period.
    const int last_chunk = p.n_chunks_total - 1, last_step = nper * STEPS - 1;
    auto period = [&](auto par_c, int per) __attribute__((always_inline)) {
        constexpr int PAR = decltype(par_c)::value;
        const int even_next = min(2 * per + 2, last_chunk);
        static_for<0, STEPS>([&](auto s_c) __attribute__((always_inline)) {
            constexpr int s = decltype(s_c)::value;
            constexpr int slot = (s + PAR) & 1;
            constexpr int sn = (s + 1) % STEPS;
            const half8* xp = xstep(s);
            static_for<0, 4>([&](auto j_c) __attribute__((always_inline)) {
                constexpr int j = decltype(j_c)::value;
                if (j < 3) {
                    read_b(xp, j + 1, (j + 1) & 1);
                } else {
                    if (s == 3 || s == 8) {
                        wait_vmcnt<8>();           // the weights of the next step may still be in flight
                        barrier_lds_only();
                    } else if (s == 4) {
                        barrier_lds_only();        // every wave has read the even chunk's last tap: buffer 0 may be refilled
                    }
                    read_b(xstep(sn), 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (j == 0) {
                    if (s < 3) { dma_x(2 * per + 1, 1, 2 * s); dma_x(2 * per + 1, 1, 2 * s + 1); }
                    if (s >= 5 && s < 8) { dma_x(even_next, 0, 2 * (s - 5)); dma_x(even_next, 0, 2 * (s - 5) + 1); }
                    load_a(min(per * STEPS + s + 1, last_step), slot ^ 1);
                }
                __builtin_amdgcn_sched_barrier(0);
                mfma_group(j, j & 1, slot);
                __builtin_amdgcn_sched_barrier(0);
            });
        });
    };
    {
        // Two shapes of the same loop.  The register allocator is at the limit of 256 in both variants and the shape of the control flow around
        // the loop decides whether an accumulator is spilled on the way out: the emitting variant is spill-free with the mid-loop exit, the
        // plain one with a separate last period (the compiler report in profiles/conv11/README.md is the check).
        if constexpr (EMIT) {
            for (int per = 0; per < nper; per += 2) {       // an odd period count leaves in the middle
                period(std::integral_constant<int, 0>{}, per);
                if (per + 1 >= nper) break;
                period(std::integral_constant<int, 1>{}, per + 1);
            }
        } else {
            int per = 0;
            for (; per + 1 < nper; per += 2) {
                period(std::integral_constant<int, 0>{}, per);
                period(std::integral_constant<int, 1>{}, per + 1);
            }
            if (per < nper) period(std::integral_constant<int, 0>{}, per);
        }
    }

    if constexpr (EMIT) {
        // ---- fused emission (Conv6Emit), conv7's step by step.  Accumulator layout: acc[m][2 j + cb][r] of lane l = channel 16 m + 4 (l >> 4) + r
        // of the wave's 64, pixel (row 4 pw + j, column 16 cb + (l & 15)) of the tile.
        __syncthreads();
        const int rsub = lane >> 4;
        float* wl = reinterpret_cast<float*>(smem11) + wave * 512;      // per-wave scratch: [0,64) bias, [64,128) S, [128,192) SS, [192,448) table
        const float osc = p.out_scale;
        wl[lane] = p.bias[co_wave + lane];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = m * 16 + 4 * rsub + r;
                const float b = wl[ch];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    const float v = acc[m][n][r] * osc + b;
                    acc[m][n][r] = v;
                    s1 += v; s2 += v * v;
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }      // the 16 lanes of this channel
                if (l15 == 0) { wl[64 + ch] = s1; wl[128 + ch] = s2; }
            }
        __builtin_amdgcn_wave_barrier();
        hop_rendezvous<64>(p, reinterpret_cast<float*>(smem11), wl, wave, cw, pw, lane, n0, co_blk, co_wave, tiles_per_img, HW);
        const float4* tab = reinterpret_cast<const float4*>(wl + 192);
        bool bad = false;
        // A 16-byte plane entry = 8 channels of one pixel; this lane holds 4 of them (r = 0 .. 3 at 4 (l >> 4)), lane ^ 16 the other 4.  For a
        // pair of pixel rows (j, j + 1) v_permlane16_swap hands the even 16-lane rows both halves of row j and the odd ones both halves of
        // row j + 1: one 16-byte store per lane.
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            float4 t4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) t4[q] = tab[m * 16 + 4 * rsub + q];
            const int c8 = (co_wave + m * 16 + 8 * (rsub >> 1)) >> 3;
#pragma unroll
            for (int jp = 0; jp < 2; ++jp)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    half4v h0, l0, h1, l1;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        _Float16 th, tl;
                        norm_split(acc[m][2 * (2 * jp) + cb][q], t4[q], bad, th, tl); h0[q] = th; l0[q] = tl;
                        norm_split(acc[m][2 * (2 * jp + 1) + cb][q], t4[q], bad, th, tl); h1[q] = th; l1[q] = tl;
                    }
                    const u32x2 a_hh = __builtin_bit_cast(u32x2, h0), b_hh = __builtin_bit_cast(u32x2, h1);
                    const u32x2 a_ll = __builtin_bit_cast(u32x2, l0), b_ll = __builtin_bit_cast(u32x2, l1);
                    u32x4 eh, el;
                    {
                        const auto s0 = __builtin_amdgcn_permlane16_swap(a_hh.x, b_hh.x, false, false), s1 = __builtin_amdgcn_permlane16_swap(a_hh.y, b_hh.y, false, false);
                        eh.x = s0[0]; eh.y = s1[0]; eh.z = s0[1]; eh.w = s1[1];
                    }
                    const size_t eo = (((size_t)n0 * p.em.C8 + c8) * HW + (size_t)(ty0 + 4 * pw + 2 * jp + (rsub & 1)) * p.W + (tx0 + 16 * cb + l15)) << 4;
                    *reinterpret_cast<u32x4*>(p.em.hi + eo) = eh;
                    {
                        const auto s0 = __builtin_amdgcn_permlane16_swap(a_ll.x, b_ll.x, false, false), s1 = __builtin_amdgcn_permlane16_swap(a_ll.y, b_ll.y, false, false);
                        el.x = s0[0]; el.y = s1[0]; el.z = s0[1]; el.w = s1[1];
                        *reinterpret_cast<u32x4*>(p.em.lo + eo) = el;
                    }
                }
        }
        range_report(bad, p.em.range_ctr);
        return;
    }

    // ---- epilogue: conv7's, four passes q = (32-channel pair of M-tiles i, pixel-row pair jp) of 32 co x 64 px: bias, un-scaling, residual in
    // its three forms, GroupNorm partial sums (slot = the 64-pixel group of the tile).  Only the accumulator -> slab scatter differs:
    // acc[m][2 j + cb][r] of lane l = channel 16 m + 4 (l >> 4) + r of the wave's 64, pixel (row 4 pw + j, column 16 cb + (l & 15)).
    __syncthreads();
    constexpr int TS = 68;
    constexpr int GPI = (TW * TH) / 64;                      // 64-pixel groups per image inside one tile
    float* tr = reinterpret_cast<float*>(smem11) + wave * (32 * TS);
    const int q4 = lane & 15, rsub = lane >> 4;
    const float osc = p.out_scale;
    const bool do_stat = p.stat != nullptr;
    const int res_mode = p.res ? p.res_mode : -1;
    const size_t img0 = (size_t)n0 * p.Cout;
    const size_t res_plane = res_mode == 1 ? (size_t)(HW >> 2) : (res_mode == 2 ? (size_t)HW * 4 : (size_t)HW);
    float* const out_base = p.out + img0 * HW;
    const float* const res_base = res_mode >= 0 ? p.res + img0 * res_plane : p.bias;
    const unsigned res_bytes = res_mode >= 0 ? 0xFFFFFFFFu : 0u;
    const void* const stat_base = do_stat ? (const void*)(p.stat + img0 * p.stat_slots) : (const void*)p.bias;
    const unsigned stat_bytes = do_stat ? 0xFFFFFFFFu : 0u;
    auto f4 = [](u32x4 v) { return make_float4(as_f32(v.x), as_f32(v.y), as_f32(v.z), as_f32(v.w)); };

    const __amdgpu_buffer_rsrc_t r_bias = rsrc_uniform(p.bias, (unsigned)p.Cout * 4u);
    struct PassGeo { int y, x; unsigned pix; };      // tiles lie inside the image and co-blocks are full: no bounds to check
    auto geo = [&](int q) {
        const int pp = (pw * 2 + (q & 1)) * 64 + q4 * 4;
        PassGeo g;
        g.y = ty0 + ((pp >> 5) & (TH - 1));
        g.x = tx0 + (pp & (TW - 1));
        g.pix = (unsigned)(g.y * p.W + g.x);
        return g;
    };
    auto load_res = [&](int q, float4 (&rv)[8]) __attribute__((always_inline)) {
        const PassGeo g = geo(q);
        const int co0 = co_wave + (q >> 1) * 32;
        const __amdgpu_buffer_rsrc_t r_res = rsrc_uniform(res_base, res_bytes);
        if (res_mode <= 0) {                               // same shape as the output (or none: zero-sized descriptor)
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int co = co0 + it * 4 + rsub;
                const unsigned off = ((unsigned)co * (unsigned)HW + g.pix) * 4u;
                rv[it] = f4(__builtin_amdgcn_raw_buffer_load_b128(r_res, off, 0, 0));
            }
        } else if (res_mode == 1) {                        // residual at half resolution, nearest up-sampling (unet.py:107)
            const unsigned Wr = (unsigned)(p.W >> 1), HWr = (unsigned)(HW >> 2);
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int co = co0 + it * 4 + rsub;
                const unsigned off = ((unsigned)co * HWr + (unsigned)(g.y >> 1) * Wr + (unsigned)(g.x >> 1)) * 4u;
                const u32x2 r2 = __builtin_amdgcn_raw_buffer_load_b64(r_res, off, 0, 0);
                const float a = as_f32(r2.x), b = as_f32(r2.y);
                rv[it] = make_float4(a, a, b, b);
            }
        } else {                                           // residual at double resolution, 2x2 average pooling (unet.py:136)
            const unsigned Wr = (unsigned)p.W * 2u, HWr = (unsigned)HW * 4u;
#pragma unroll
            for (int h = 0; h < 4; ++h) {                  // two channel rows (8 loads) at a time: register pressure
                float4 a0[2], a1[2], b0[2], b1[2];
#pragma unroll
                for (int i2 = 0; i2 < 2; ++i2) {
                    const int co = co0 + (h * 2 + i2) * 4 + rsub;
                    const unsigned off = ((unsigned)co * HWr + (unsigned)(2 * g.y) * Wr + (unsigned)(2 * g.x)) * 4u;
                    a0[i2] = f4(__builtin_amdgcn_raw_buffer_load_b128(r_res, off, 0, 0));
                    a1[i2] = f4(__builtin_amdgcn_raw_buffer_load_b128(r_res, off + 16u, 0, 0));
                    b0[i2] = f4(__builtin_amdgcn_raw_buffer_load_b128(r_res, off + Wr * 4u, 0, 0));
                    b1[i2] = f4(__builtin_amdgcn_raw_buffer_load_b128(r_res, off + Wr * 4u + 16u, 0, 0));
                }
#pragma unroll
                for (int i2 = 0; i2 < 2; ++i2)
                    rv[h * 2 + i2] = make_float4(((a0[i2].x + a0[i2].y) + (b0[i2].x + b0[i2].y)) * 0.25f, ((a0[i2].z + a0[i2].w) + (b0[i2].z + b0[i2].w)) * 0.25f,
                                                 ((a1[i2].x + a1[i2].y) + (b1[i2].x + b1[i2].y)) * 0.25f, ((a1[i2].z + a1[i2].w) + (b1[i2].z + b1[i2].w)) * 0.25f);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    float4 rv[2][8];
    load_res(0, rv[0]);
    static_for<0, 4>([&](auto q_c) __attribute__((always_inline)) {
        constexpr int q = decltype(q_c)::value;
        constexpr int i = q >> 1, jp = q & 1;
        const PassGeo g = geo(q);
        const int co0 = co_wave + i * 32;
        float bv[8];                                         // per pass (conv7 holds both co-tiles' from the start): registers
#pragma unroll
        for (int it = 0; it < 8; ++it) bv[it] = as_f32(__builtin_amdgcn_raw_buffer_load_b32(r_bias, (unsigned)(co0 + it * 4 + rsub) * 4u, 0, 0));
#pragma unroll
        for (int mm = 0; mm < 2; ++mm)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        tr[(mm * 16 + 4 * rsub + r) * TS + jj * 32 + cb * 16 + l15] = acc[2 * i + mm][2 * (2 * jp + jj) + cb][r] * osc;
        __builtin_amdgcn_sched_barrier(0);
        if (q + 1 < 4) load_res(q + 1, rv[(q + 1) & 1]);   // requested before this pass's stores
        __builtin_amdgcn_sched_barrier(0);
        const int slot = trem * GPI + ((pw * 2 + jp) % GPI);
        const __amdgpu_buffer_rsrc_t r_out = rsrc_uniform(out_base, 0xFFFFFFFFu);
        const __amdgpu_buffer_rsrc_t r_stat = rsrc_uniform(stat_base, stat_bytes);
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int co_l = it * 4 + rsub;
            const int co = co0 + co_l;
            float4 v = *reinterpret_cast<const float4*>(tr + co_l * TS + q4 * 4);
            {
                v.x += bv[it]; v.y += bv[it]; v.z += bv[it]; v.w += bv[it];
                const float4 r4 = rv[q & 1][it];
                v.x = r4.x + v.x; v.y = r4.y + v.y; v.z = r4.z + v.z; v.w = r4.w + v.w;
            }
            u32x4 sv;
            sv.x = as_u32(v.x); sv.y = as_u32(v.y); sv.z = as_u32(v.z); sv.w = as_u32(v.w);
            const unsigned plane_l = (unsigned)co;
            __builtin_amdgcn_raw_buffer_store_b128(sv, r_out, (plane_l * (unsigned)HW + g.pix) * 4u, 0, 0);
            if (do_stat) {
                float s1 = (v.x + v.y) + (v.z + v.w);
                float s2 = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
                s1 += dpp_row_shr<0x111>(s1); s2 += dpp_row_shr<0x111>(s2);
                s1 += dpp_row_shr<0x112>(s1); s2 += dpp_row_shr<0x112>(s2);
                s1 += dpp_row_shr<0x114>(s1); s2 += dpp_row_shr<0x114>(s2);
                s1 += dpp_row_shr<0x118>(s1); s2 += dpp_row_shr<0x118>(s2);
                u32x2 st;
                st.x = as_u32(s1); st.y = as_u32(s2);
                const bool wr = q4 == 15;
                __builtin_amdgcn_raw_buffer_store_b64(st, r_stat, wr ? (plane_l * (unsigned)p.stat_slots + (unsigned)slot) * 8u : kOutOfRange, 0, 0);
            }
        }
    });
#endif
}

bool conv11_supported(int Cin, int Cout, int H, int W) { return conv11_shape_ok(Cin, Cout, H, W); }
KernelRef conv11_emit_kernel() { return KernelRef{reinterpret_cast<const void*>(conv11_mfma_kernel<true>), c11::LDS}; }
bool conv11_emit_supported(int Cout, int H, int W) { return conv11_hop_ok(Cout, H, W, device_caps().conv11); }

Status launch_conv11(hipStream_t s, const Conv11Args& a) {
    if (a.grad) return Status{DPIR_ERR_UNSUPPORTED, "conv11: a gradient-mode forward keeps launch_conv6's route"};
    if (a.precision == 0) return Status{DPIR_ERR_UNSUPPORTED, "conv11: the f32 precision keeps the fp32 kernel"};
    if (a.precision != 1) return Status{DPIR_ERR_UNSUPPORTED, "conv11: built for f16x3 only, f16x1 keeps conv7"};
    if (a.ksplit != 1) return Status{DPIR_ERR_UNSUPPORTED, "conv11: whole K only, split-K launches keep conv6"};
    if (a.Cin <= 0 || a.Cin % 32) return Status{DPIR_ERR_UNSUPPORTED, "conv11: Cin must be a multiple of 32 (an even number of 16-channel chunks)"};
    if (a.Cout <= 0 || a.Cout % 128) return Status{DPIR_ERR_UNSUPPORTED, "conv11: Cout must be a multiple of 128 (full co-blocks)"};
    if (a.W <= 0 || a.W % 32 || a.H <= 0 || a.H % 8) return Status{DPIR_ERR_UNSUPPORTED, "conv11: 8 x 32 tiles inside the image only (W % 32 == 0, H % 8 == 0)"};
    if (!a.xhi || !a.xlo || !a.w11 || !a.bias || a.B <= 0) return invalid("conv11: bad arguments");
    Conv6K k{};
    k.xhi = reinterpret_cast<const char*>(a.xhi); k.xlo = reinterpret_cast<const char*>(a.xlo);
    k.w16 = reinterpret_cast<const char*>(a.w11); k.bias = a.bias; k.out = a.out; k.res = a.res; k.res_mode = a.res_mode;
    k.B = a.B; k.Cout = a.Cout; k.H = a.H; k.W = a.W;
    k.n_chunks_total = a.Cin / 16;
    k.C8 = 2 * k.n_chunks_total;
    k.tiles_x = a.W / 32; k.tiles_y = a.H / 8; k.n_co_blocks = a.Cout / 128;
    k.ksplit = 1; k.chunks_per_split = k.n_chunks_total;
    k.out_scale = 1.0f / a.w_scale;
    k.stat = a.stat; k.stat_slots = a.stat ? conv6_stat_slots(a.H, a.W) : 0;
    if ((size_t)a.B * k.C8 * a.H * a.W * 16 >= ((size_t)1 << 32) || (size_t)a.Cout * a.H * a.W * 16 >= ((size_t)1 << 32))
        return invalid("conv11: an operand plane or an image's output exceeds the 4 GiB buffer-descriptor range");
    const long long blocks = (long long)k.tiles_x * k.tiles_y * a.B * k.n_co_blocks;
    if (blocks > 0x7FFFFFFFll) return invalid("conv11: too many workgroups");
    if (a.emit) {
        if (a.res || !a.emit->hi || !a.emit->lo || !a.emit->acc || !a.emit->cnt || !a.emit->range_ctr || !a.emit->gamma || !a.emit->beta)
            return invalid("conv11: fused emission takes no residual and needs both planes, the accumulators, the counters and the range guard");
        if (!conv11_emit_supported(a.Cout, a.H, a.W))
            return Status{DPIR_ERR_UNSUPPORTED, "conv11: fused emission needs GroupNorm groups inside a wave's 64 channels and an image's tiles resident with room to spare"};
        k.em = *a.emit;
        k.out = nullptr; k.stat = nullptr; k.stat_slots = 0;
        auto fn = conv11_mfma_kernel<true>;
        static LdsAttrOnce attr_emit;
        DPIR_HIP(attr_emit.set(reinterpret_cast<const void*>(fn), (int)c11::LDS));
        hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(256), c11::LDS, s, k);
    } else {
        if (!a.out) return invalid("conv11: bad arguments");
        auto fn = conv11_mfma_kernel<false>;
        static LdsAttrOnce attr_set;
        DPIR_HIP(attr_set.set(reinterpret_cast<const void*>(fn), (int)c11::LDS));
        hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(256), c11::LDS, s, k);
    }
    DPIR_HIP(hipGetLastError());
    return Status{};
}

void pack_weights_conv11(const float* w, int cout, int cin, float scale, std::vector<uint16_t>& out) {
    const int taps = 9;
    const int steps = (cin / 16) * taps / 2, cblocks = cout / 128;
    out.assign((size_t)steps * cblocks * 2 * 4 * 2 * 512, 0);        // 512 halves = 1 KiB per record
    for (int st = 0; st < steps; ++st)
        for (int cbk = 0; cbk < cblocks; ++cbk)
            for (int cwv = 0; cwv < 2; ++cwv)
                for (int m = 0; m < 4; ++m) {
                    uint16_t* hi = out.data() + (((((size_t)st * cblocks + cbk) * 2 + cwv) * 4 + m) * 2) * 512;
                    uint16_t* lo = hi + 512;
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const int q = 2 * st + (l >> 5), ch = q / taps, tap = q % taps;
                            const int co = cbk * 128 + cwv * 64 + m * 16 + (l & 15), ci = ch * 16 + ((l >> 4) & 1) * 8 + j;
                            const float v = w[((size_t)co * cin + ci) * taps + tap] * scale;
                            const _Float16 h = (_Float16)v;
                            const _Float16 lw = (_Float16)(v - (float)h);
                            __builtin_memcpy(&hi[(size_t)l * 8 + j], &h, 2);
                            __builtin_memcpy(&lo[(size_t)l * 8 + j], &lw, 2);
                        }
                }
}

}  // namespace dpir
