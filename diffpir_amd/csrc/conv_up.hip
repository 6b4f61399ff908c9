// conv_up: conv1 of an up-sampling ResBlock (3x3, zero padding 1, on a nearest-x2 up-sampled image) as FOUR 2x2 PHASE CONVOLUTIONS of the
// source image, one per output parity (a, b) = (y & 1, x & 1).  Output row 2i + a reads the up-sampled rows 2i + a - 1 .. 2i + a + 1, i.e.
//     a = 0: source rows i - 1, i      with row weights  w[0],        w[1] + w[2]
//     a = 1: source rows i, i + 1      with row weights  w[0] + w[1], w[2]
// and the columns combine the same way; the zero padding of the up-sampled image is the zero padding of the source image.  16 tap-products
// per source pixel instead of 36 (4/9 of conv7's MFMAs), operand planes at the source resolution (a quarter of the bytes, and act_split
// no longer stores every source pixel four times).  Same arithmetic as conv6 / conv7 otherwise: f16x3 = al*bh, ah*bl, ah*bh in that order
// per accumulator, fp32 accumulation, weights pre-scaled by a power of two and split into f16 hi / lo on the host (here from the float64
// sum of the contributing taps), 16 B per lane loaded straight into registers as the MFMA A fragment.
//
// Mapping.  A workgroup is (source tile of 8 rows x 32 columns, 64 real output channels, row parity a); its four waves are
// (cw = 32 of the 64 channels, pw = source rows 4 pw .. 4 pw + 3).  The two co-tiles of a wave are the two COLUMN parities b = 0, 1 of the
// same 32 channels: acc[b][j] is 32 channels x 32 source columns of source row 4 pw + j, i.e. output pixels (2 row + a, 2 column + b).  A
// lane therefore holds both x-neighbours of an output pixel pair -- the fp32 rows and the 16-byte plane entries it stores are contiguous --
// and the workgroup count equals conv7's on the up-sampled image (4 x fewer tiles, 2 x more channel blocks, 2 parities).
// A K chunk (16 input channels) is six UNITS (p, c): source row tap p = 0, 1 (patch row p + a) and patch column c = 0, 1, 2.  The B fragment
// at column c serves b = 0 with column tap q = c and b = 1 with q = c - 1: units c = 0 / 2 feed one co-tile (12 MFMAs per wave in f16x3),
// unit c = 1 both (24): 96 MFMAs and 6 B positions per pixel tile and chunk (conv7: 216 and 9).  The eight weight records of a chunk
// ((p, b, q), order of use) run through a FOUR-slot register ring, requested two units ahead; 8 % 4 == 0 keeps the slot a compile-time
// constant of the unrolled chunk body.
#include "common.h"
#include <atomic>
#include "elem.h"
#include "conv_epilogue.h"
#include "conv_up.h"
#include <math.h>

namespace dpir {

// Conv6K as conv7 reads it, with H, W, tiles_x, tiles_y of the SOURCE image, n_co_blocks = 64-channel blocks and stat_slots of the output.
// EMIT: the fused hop to conv2 (Conv6Emit), see the epilogue.
template <bool X1, bool EMIT>
__global__ __launch_bounds__(256, 2) void conv_up_kernel(Conv6K p) {
#if defined(__HIP_DEVICE_COMPILE__)
    using G = TileGeo<0>;
    constexpr int TW = G::TW, TH = G::TH, LW = G::LW, PATCH = G::PATCH, NPIECE = G::NPIECE, XB = G::XB;
    constexpr int NXT = (NPIECE + 3) / 4;               // per wave and plane
    constexpr int NPL = X1 ? 1 : 2;                     // operand planes (hi [, lo])
    constexpr int NACT = NPL * NXT;                     // activation DMA instructions per wave and chunk
    static_assert(NACT <= 6, "two activation pieces per unit in units 0 .. 2: older than the weights requested in units 4 and 5");
    constexpr int UNITS = 6;
    extern __shared__ __attribute__((aligned(16))) char smem_u[];      // [2 buffers][hi|lo][XB]; the epilogue slabs alias it

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cw = wave & 1, pw = wave >> 1;            // 32 of the block's 64 channels; source rows 4 pw .. 4 pw + 3
    const int l31 = lane & 31;
    const int half = lane >> 5;

    int bid = blockIdx.x;
    if (!EMIT && (gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);      // XCD-contiguous tiles, as conv6
    const int tiles_per_img = p.tiles_x * p.tiles_y;
    // EMIT: inside an image the channel block is the OUTER index, so that the workgroups that wait for one another -- one (image, 64-channel
    // block): both row parities of every source tile -- are 2 x tiles_per_img CONSECUTIVE ids.  No XCD renumbering there.
    int cb, par, ptile;
    if (EMIT) {
        const int per_img = 2 * tiles_per_img * p.n_co_blocks;
        const int r = bid % per_img;
        cb = r / (2 * tiles_per_img);
        const int r2 = r - cb * (2 * tiles_per_img);
        par = r2 & 1;
        ptile = (bid / per_img) * tiles_per_img + (r2 >> 1);
    } else {
        const int nv = 2 * p.n_co_blocks;
        const int v = bid % nv;
        par = v & 1;
        cb = v >> 1;
        ptile = bid / nv;
    }
    const int n0 = ptile / tiles_per_img;
    const int trem = ptile - n0 * tiles_per_img;
    const int co_wave = cb * 64 + cw * 32;                   // this wave's first output channel
    const bool wave_live = co_wave < p.Cout;
    const int ty0 = (trem / p.tiles_x) * TH;
    const int tx0 = (trem % p.tiles_x) * TW;
    const int HW = p.H * p.W;                                // source
    const int Wo = 2 * p.W, HWo = 4 * HW;                    // output
    const int n_chunks = p.n_chunks_total;

    // ---- activation DMA: conv7's (pieces dealt to the 4 waves, out-of-image positions out of range = zeros), on the source planes
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
        const int u = X1 ? q : q >> 1, plane = X1 ? 0 : q & 1;
        int piece = wave + u * 4;
        if (piece > NPIECE - 1) piece = NPIECE - 1;
        const size_t coff = (size_t)chunk * 2 * HW * 16;
        const __amdgpu_buffer_rsrc_t rx = rsrc_uniform((plane ? p.xlo : p.xhi) + coff, (unsigned)(xplane_bytes - coff));
        BLDS6(rx, smem_u + buf * 2 * XB + plane * XB + piece * 1024, x_off[u], 0);
    };

    // ---- B fragments: patch row p + a, patch column c of the wave's four source rows (pixel tile j = source row 4 pw + j)
    const int lane_b = l31 + half * PATCH + (4 * pw + par) * LW;
    const half8* xbase = reinterpret_cast<const half8*>(smem_u) + lane_b;

    // ---- A fragments straight from the phase pack: (chunk, 64-channel block, a, cw) = 8 records (p, b, q) of 2 KiB [hi | lo], 16 B per lane
    const unsigned lane16 = (unsigned)lane * 16u;
    half8 a_h[4], a_l[4];
    auto load_a = [&](int chunk, int rec) __attribute__((always_inline)) {
        const char* base = p.w16 + ((((size_t)chunk * p.n_co_blocks + cb) * 2 + par) * 2 + cw) * (8 * 2048);
        const __amdgpu_buffer_rsrc_t rw = rsrc_uniform(base, 8 * 2048);
        const unsigned so = (unsigned)(rec * 2048);
        a_h[rec & 3] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rw, lane16, so, 0));
        if (!X1) a_l[rec & 3] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rw, lane16, so + 1024u, 0));
    };

    floatx16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    half8 b_h[2][2], b_l[2][2];      // two pixel tiles per set, two sets (one in use, one being filled)
    auto read_b = [&](int buf, int unit, int grp, int set) __attribute__((always_inline)) {      // pixel tiles 2 grp, 2 grp + 1
        const half8* xh = xbase + buf * (2 * XB / 16);
        const half8* xl = xh + XB / 16;
        const int uoff = (unit / 3) * LW + (unit % 3);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int o = (grp * 2 + j) * LW + uoff;
            b_h[set][j] = xh[o];
            if (!X1) b_l[set][j] = xl[o];
        }
    };
    // one record against the two pixel tiles of a group; per accumulator: al * bh, ah * bl, ah * bh -- conv6's order
    auto mfma_rec = [&](int b, int grp, int set, int slot) __attribute__((always_inline)) {
        if (!X1) {
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[b][grp * 2 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_l[slot], b_h[set][j], acc[b][grp * 2 + j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[b][grp * 2 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_h[slot], b_l[set][j], acc[b][grp * 2 + j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[b][grp * 2 + j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_h[slot], b_h[set][j], acc[b][grp * 2 + j], 0, 0, 0);
    };
    // unit (p, c): record p * 4 + b * 2 + q with c = q + b
    auto mfma_group = [&](int unit, int grp, int set) __attribute__((always_inline)) {
        const int pp = unit / 3, c = unit % 3;
        if (c == 0) mfma_rec(0, grp, set, (pp * 4 + 0) & 3);
        else if (c == 1) { mfma_rec(0, grp, set, (pp * 4 + 1) & 3); mfma_rec(1, grp, set, (pp * 4 + 2) & 3); }
        else mfma_rec(1, grp, set, (pp * 4 + 3) & 3);
    };

    // Waves whose 32 output channels lie beyond Cout only carry their share of the activation DMA and keep the barrier count
    // (prologue, one per chunk boundary, epilogue): no weights, no MFMAs.
    if (!wave_live) {
#pragma unroll
        for (int q = 0; q < NACT; ++q) dma_x(0, 0, q);
        wait_vmcnt<0>();
        __syncthreads();
        int it = 0;
        for (int chunk = 0; chunk + 1 < n_chunks; ++chunk, ++it) {
#pragma unroll
            for (int q = 0; q < NACT; ++q) dma_x(chunk + 1, (it & 1) ^ 1, q);
            wait_vmcnt<0>();
            __syncthreads();
        }
        __syncthreads();
        return;
    }

    // ---- prologue: first patch, the records of units 0 and 1
#pragma unroll
    for (int q = 0; q < NACT; ++q) dma_x(0, 0, q);
    load_a(0, 0);
    load_a(0, 1);
    load_a(0, 2);
    wait_vmcnt<0>();
    __syncthreads();
    read_b(0, 0, 0, 0);

    // One K chunk: 6 units x 2 groups.  Unit u requests the records of unit u + 2 (units 4 / 5: the next chunk's units 0 / 1) into the slots
    // that unit u - 1 has finished with, and, for u < 3, two activation pieces of the next chunk.  The compiler counts the register loads
    // itself; the activation pieces are older than the 3 records requested in units 4 and 5, so "at most those 3 x NPL loads outstanding"
    // at the chunk boundary proves that they have landed.
    auto chunk_body = [&](auto more_c, int chunk, int it) __attribute__((always_inline)) {
        constexpr bool MORE = decltype(more_c)::value;
        const int cur = it & 1;
        static_for<0, UNITS>([&](auto unit_c) __attribute__((always_inline)) {
            constexpr int u = decltype(unit_c)::value;
            read_b(cur, u, 1, 1);
            __builtin_amdgcn_sched_barrier(0);
            if (MORE && u < 3) {
                if (2 * u < NACT) dma_x(chunk + 1, cur ^ 1, 2 * u);
                if (2 * u + 1 < NACT) dma_x(chunk + 1, cur ^ 1, 2 * u + 1);
            }
            if (u == 0) load_a(chunk, 3);
            else if (u == 1) load_a(chunk, 4);
            else if (u == 2) { load_a(chunk, 5); load_a(chunk, 6); }
            else if (u == 3) load_a(chunk, 7);
            else if (MORE && u == 4) load_a(chunk + 1, 0);
            else if (MORE && u == 5) { load_a(chunk + 1, 1); load_a(chunk + 1, 2); }
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(u, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (u + 1 < UNITS) {
                read_b(cur, u + 1, 0, 0);
            } else if (MORE) {
                wait_vmcnt<3 * NPL>();             // the records of the next chunk's units 0 and 1 may still be in flight
                barrier_lds_only();
                read_b(cur ^ 1, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(u, 1, 1);
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    {
        int it = 0, chunk = 0;
        for (; chunk + 1 < n_chunks; ++chunk, ++it) chunk_body(std::true_type{}, chunk, it);
        chunk_body(std::false_type{}, chunk, it);
    }

    // Accumulator layout: acc[b][j][r] of lane (l31, half) = channel 8 * (r >> 2) + 4 * half + (r & 3) of the wave's 32, output pixel
    // (2 * (ty0 + 4 pw + j) + a, 2 * (tx0 + l31) + b).
    if constexpr (EMIT) {
        // ---- fused emission (Conv6Emit), conv7<EMIT>'s scheme: per-channel sums -> hop_rendezvous (one (image, 64-channel block): both row parities
        // of every source tile) -> GroupNorm + FiLM + SiLU + f16 split of the wave's own accumulators into conv2's planes.
        __syncthreads();
        float* wl = reinterpret_cast<float*>(smem_u) + wave * 512;      // per-wave scratch: [0,32) bias, [64,96) S, [128,160) SS, [192,320) table
        const float osc = p.out_scale;
        if (lane < 32) wl[lane] = p.bias[co_wave + lane];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = (r & 3) + 8 * (r >> 2) + 4 * half;
            const float b = wl[ch];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = acc[i][j][r] * osc + b;
                    acc[i][j][r] = v;
                    s1 += v; s2 += v * v;
                }
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }      // the 32 lanes of this half
            if (l31 == 0) { wl[64 + ch] = s1; wl[128 + ch] = s2; }
        }
        __builtin_amdgcn_wave_barrier();
        hop_rendezvous<32>(p, reinterpret_cast<float*>(smem_u), wl, wave, cw, pw, lane, n0, cb, co_wave, 2 * tiles_per_img, HWo);
        const float4* tab = reinterpret_cast<const float4*>(wl + 192);
        bool bad = false;
        // A 16-byte plane entry = 8 channels of one pixel; this lane holds 4 of them (4 half .. 4 half + 3), lane ^ 32 the other 4, for BOTH
        // x-neighbours 2 x + 0 / 2 x + 1.  v_permlane32_swap hands the lower lanes both halves of the even pixel and the upper lanes both
        // halves of the odd one: one 16-byte store per lane, 1 KiB of one output row per instruction.
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
            float4 m[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) m[q] = tab[8 * jb + 4 * half + q];
            const int c8 = (co_wave + 8 * jb) >> 3;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                half4v h0, l0, h1, l1;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    _Float16 th, tl;
                    norm_split(acc[0][j][jb * 4 + q], m[q], bad, th, tl); h0[q] = th; l0[q] = tl;
                    norm_split(acc[1][j][jb * 4 + q], m[q], bad, th, tl); h1[q] = th; l1[q] = tl;
                }
                const u32x2 e_h = __builtin_bit_cast(u32x2, h0), o_h = __builtin_bit_cast(u32x2, h1);
                const u32x2 e_l = __builtin_bit_cast(u32x2, l0), o_l = __builtin_bit_cast(u32x2, l1);
                u32x4 eh, el;
                {
                    const auto s0 = __builtin_amdgcn_permlane32_swap(e_h.x, o_h.x, false, false), s1 = __builtin_amdgcn_permlane32_swap(e_h.y, o_h.y, false, false);
                    eh.x = s0[0]; eh.y = s1[0]; eh.z = s0[1]; eh.w = s1[1];
                }
                const size_t eo = (((size_t)n0 * p.em.C8 + c8) * HWo + (size_t)(2 * (ty0 + 4 * pw + j) + par) * Wo + (2 * (tx0 + l31) + half)) << 4;
                *reinterpret_cast<u32x4*>(p.em.hi + eo) = eh;
                if (!X1) {
                    const auto s0 = __builtin_amdgcn_permlane32_swap(e_l.x, o_l.x, false, false), s1 = __builtin_amdgcn_permlane32_swap(e_l.y, o_l.y, false, false);
                    el.x = s0[0]; el.y = s1[0]; el.z = s0[1]; el.w = s1[1];
                    *reinterpret_cast<u32x4*>(p.em.lo + eo) = el;
                }
            }
        }
        range_report(bad, p.em.range_ctr);
        return;
    }

    // ---- plain epilogue: four passes j (source row 4 pw + j) of 32 co x 64 px -- one output-row segment of 64 pixels per channel, the two
    // column parities interleaved through the per-wave LDS slab: bias, un-scaling, GroupNorm partial sums (one slot per pass)
    __syncthreads();
    constexpr int TS = 68;
    float* tr = reinterpret_cast<float*>(smem_u) + wave * (32 * TS);
    const int q4 = lane & 15, rsub = lane >> 4;
    const float osc = p.out_scale;
    const bool do_stat = p.stat != nullptr;
    const size_t img0 = (size_t)n0 * p.Cout;
    float* const out_base = p.out + img0 * HWo;
    const void* const stat_base = do_stat ? (const void*)(p.stat + img0 * p.stat_slots) : (const void*)p.bias;
    const unsigned stat_bytes = do_stat ? 0xFFFFFFFFu : 0u;

    float bv[8];
    {
        const __amdgpu_buffer_rsrc_t r_bias = rsrc_uniform(p.bias, (unsigned)p.Cout * 4u);
#pragma unroll
        for (int it = 0; it < 8; ++it) bv[it] = as_f32(__builtin_amdgcn_raw_buffer_load_b32(r_bias, (unsigned)(co_wave + it * 4 + rsub) * 4u, 0, 0));
    }
    static_for<0, 4>([&](auto j_c) __attribute__((always_inline)) {
        constexpr int j = decltype(j_c)::value;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                tr[((r & 3) + 8 * (r >> 2) + 4 * half) * TS + 2 * l31 + b] = acc[b][j][r] * osc;
        const unsigned pix = (unsigned)((2 * (ty0 + 4 * pw + j) + par) * Wo + 2 * tx0 + q4 * 4);
        const int slot = (trem * 2 + par) * 8 + pw * 4 + j;
        const __amdgpu_buffer_rsrc_t r_out = rsrc_uniform(out_base, 0xFFFFFFFFu);
        const __amdgpu_buffer_rsrc_t r_stat = rsrc_uniform(stat_base, stat_bytes);
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int co_l = it * 4 + rsub;
            const int co = co_wave + co_l;
            const bool ok = co < p.Cout;
            float4 v = *reinterpret_cast<const float4*>(tr + co_l * TS + q4 * 4);
            v.x += bv[it]; v.y += bv[it]; v.z += bv[it]; v.w += bv[it];
            if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
            u32x4 sv;
            sv.x = as_u32(v.x); sv.y = as_u32(v.y); sv.z = as_u32(v.z); sv.w = as_u32(v.w);
            __builtin_amdgcn_raw_buffer_store_b128(sv, r_out, ok ? ((unsigned)co * (unsigned)HWo + pix) * 4u : kOutOfRange, 0, 0);
            if (do_stat) {
                float s1 = (v.x + v.y) + (v.z + v.w);
                float s2 = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
                s1 += dpp_row_shr<0x111>(s1); s2 += dpp_row_shr<0x111>(s2);
                s1 += dpp_row_shr<0x112>(s1); s2 += dpp_row_shr<0x112>(s2);
                s1 += dpp_row_shr<0x114>(s1); s2 += dpp_row_shr<0x114>(s2);
                s1 += dpp_row_shr<0x118>(s1); s2 += dpp_row_shr<0x118>(s2);
                u32x2 st;
                st.x = as_u32(s1); st.y = as_u32(s2);
                const bool wr = q4 == 15 && ok;
                __builtin_amdgcn_raw_buffer_store_b64(st, r_stat, wr ? ((unsigned)co * (unsigned)p.stat_slots + (unsigned)slot) * 8u : kOutOfRange, 0, 0);
            }
        }
    });
#endif
}

constexpr size_t kConvUpLds = TileGeo<0>::LDS;      // the source tile is conv7's 8 x 32 one
static_assert(2 * kConvUpLds <= 160 * 1024, "two workgroups per CU");

template <bool X1, bool EMIT>
static Status launch_up(hipStream_t s, const Conv6K& k, int blocks) {
    auto fn = conv_up_kernel<X1, EMIT>;
    static LdsAttrOnce attr_set;
    DPIR_HIP(attr_set.set(reinterpret_cast<const void*>(fn), (int)kConvUpLds));
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(256), kConvUpLds, s, k);
    return Status{};
}

KernelRef conv_up_emit_kernel() { return KernelRef{reinterpret_cast<const void*>(conv_up_kernel<false, true>), kConvUpLds}; }
int conv_up_stat_slots(int Hs, int Ws) { return geometry(2 * Hs, 2 * Ws).stat_slots; }
const char* conv_up_supported(int B, int Cin, int Cout, int Hs, int Ws, bool emit, int min_wg_hop) {
    return conv_up_refusal(B, Cin, Cout, Hs, Ws, emit, min_wg_hop, emit ? device_caps().conv_up : 0);
}

Status launch_conv_up(hipStream_t s, const ConvUpArgs& a) {
    if (a.res) return invalid("conv_up: conv1 of an up-sampling ResBlock takes no residual");
    if (const char* why = conv_up_supported(a.B, a.Cin, a.Cout, a.Hs, a.Ws, a.emit != nullptr, a.min_wg_hop)) return Status{DPIR_ERR_UNSUPPORTED, why};
    if (!a.xhi || (!a.x1 && !a.xlo) || !a.wup || !a.bias || (!a.emit && !a.out)) return invalid("conv_up: null operand");
    Conv6K k{};
    k.xhi = reinterpret_cast<const char*>(a.xhi); k.xlo = reinterpret_cast<const char*>(a.xlo);
    k.w16 = reinterpret_cast<const char*>(a.wup); k.bias = a.bias; k.out = a.out; k.res = nullptr; k.res_mode = 0;
    k.B = a.B; k.Cout = a.Cout; k.H = a.Hs; k.W = a.Ws;
    k.n_chunks_total = a.Cin / 16;
    k.C8 = 2 * k.n_chunks_total;
    k.tiles_x = a.Ws / 32; k.tiles_y = a.Hs / 8;
    k.n_co_blocks = (a.Cout + 63) / 64;
    k.ksplit = 1; k.chunks_per_split = k.n_chunks_total; k.partial = nullptr; k.zeros = nullptr;
    k.out_scale = 1.0f / a.wup_scale; k.out_scale_dev = nullptr;
    k.stat = a.emit ? nullptr : a.stat; k.stat_slots = conv_up_stat_slots(a.Hs, a.Ws);
    const int blocks = (int)conv_up_workgroups(a.B, a.Cout, a.Hs, a.Ws);
    if (a.emit) {
        if (!a.emit->hi || (!a.x1 && !a.emit->lo) || !a.emit->acc || !a.emit->cnt || !a.emit->range_ctr || !a.emit->gamma || !a.emit->beta)
            return invalid("conv_up: the hop needs planes, accumulators, counters, the range guard and the GroupNorm affine");
        k.em = *a.emit;
        DPIR_TRY((a.x1 ? launch_up<true, true>(s, k, blocks) : launch_up<false, true>(s, k, blocks)));
    } else {
        DPIR_TRY((a.x1 ? launch_up<true, false>(s, k, blocks) : launch_up<false, false>(s, k, blocks)));
    }
    DPIR_HIP(hipGetLastError());
    return Status{};
}

// Host: OIHW fp32 3x3 -> [chunk (16 ci)][64-channel block][a][cw (32 co)][record p * 4 + b * 2 + q][hi | lo][k-half][32 co][8 ci] f16: one 2 KiB
// record per (p, b, q), its two 1 KiB halves in MFMA A-fragment lane order (lane = k-half * 32 + co), as pack_weights_conv6's.  The
// contributing taps are summed in float64 (row parity a: p = 0 -> {w[0]} / {w[0], w[1]}, p = 1 -> {w[1], w[2]} / {w[2]}; columns alike), scaled
// by the power of two that puts the largest |combined weight| into [512, 1024) (pack_weights_conv6's rule; combined weights are up to 4 x
// larger) and split into hi = f16(v), lo = f16(v - hi) from the float64 value.
static _Float16 f16_nearest(double v) {      // float64 -> f16 in ONE rounding (through float32 a value can land on an f16 tie it was not on)
    _Float16 best = (_Float16)(float)v;
    uint16_t bits;
    __builtin_memcpy(&bits, &best, 2);
    for (int d = -1; d <= 1; d += 2) {
        const uint16_t nb = (uint16_t)(bits + d);
        if ((nb & 0x7C00) == 0x7C00 || ((nb ^ bits) & 0x8000)) continue;      // never into inf / nan or across the sign
        _Float16 c;
        __builtin_memcpy(&c, &nb, 2);
        const double eb = fabs(v - (double)best), ec = fabs(v - (double)c);
        if (ec < eb || (ec == eb && (nb & 1) == 0)) best = c;
    }
    return best;
}

float pack_weights_conv_up(const float* w, int cout, int cin, std::vector<uint16_t>& out) {
    const int chunks = (cin + 15) / 16, cblocks = (cout + 63) / 64;
    auto taps_of = [](int par, int t, int& k0, int& k1) {      // kernel rows (columns) k0 .. k1 of 2x2 tap t at parity par
        if (par == 0) { k0 = t == 0 ? 0 : 1; k1 = t == 0 ? 0 : 2; }
        else { k0 = t == 0 ? 0 : 2; k1 = t == 0 ? 1 : 2; }
    };
    auto combined = [&](int co, int ci, int a, int b, int pp, int q) -> double {
        int y0, y1, x0, x1;
        taps_of(a, pp, y0, y1);
        taps_of(b, q, x0, x1);
        double s = 0.0;
        for (int ky = y0; ky <= y1; ++ky)
            for (int kx = x0; kx <= x1; ++kx) s += (double)w[((size_t)co * cin + ci) * 9 + ky * 3 + kx];
        return s;
    };
    double mxd = 0.0;
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int v = 0; v < 16; ++v) mxd = fmax(mxd, fabs(combined(co, ci, v >> 3, (v >> 2) & 1, (v >> 1) & 1, v & 1)));
    const float mx = (float)mxd;
    float scale = 1.0f;
    if (mx > 0.f) scale = exp2f(floorf(log2f(1024.0f / mx)));
    while (mx * scale >= 1024.0f) scale *= 0.5f;
    out.assign((size_t)chunks * cblocks * 2 * 2 * 8 * 1024, 0);       // 1024 halves = 2 KiB per record
    for (int ch = 0; ch < chunks; ++ch)
        for (int cbk = 0; cbk < cblocks; ++cbk)
            for (int a = 0; a < 2; ++a)
                for (int wv = 0; wv < 2; ++wv)
                    for (int rec = 0; rec < 8; ++rec) {
                        const int pp = rec >> 2, b = (rec >> 1) & 1, q = rec & 1;
                        uint16_t* hi = out.data() + ((((((size_t)ch * cblocks + cbk) * 2 + a) * 2 + wv) * 8) + rec) * 1024;
                        uint16_t* lo = hi + 512;
                        for (int kh = 0; kh < 2; ++kh)
                            for (int col = 0; col < 32; ++col)
                                for (int j = 0; j < 8; ++j) {
                                    const int co = cbk * 64 + wv * 32 + col, ci = ch * 16 + kh * 8 + j;
                                    const double v = (co < cout && ci < cin) ? combined(co, ci, a, b, pp, q) * (double)scale : 0.0;
                                    const _Float16 h = f16_nearest(v);
                                    const _Float16 l = f16_nearest(v - (double)h);
                                    const size_t o = ((size_t)kh * 32 + col) * 8 + j;
                                    __builtin_memcpy(&hi[o], &h, 2);
                                    __builtin_memcpy(&lo[o], &l, 2);
                                }
                    }
    return scale;
}

}  // namespace dpir
