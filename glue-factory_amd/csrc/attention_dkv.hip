// bf16 attention backward, part 2 (dK and dV) at head_dim 64: the step's dominant kernel.  Own
// translation unit with its own compiler flags (csrc/Makefile).  The dQ kernel launched in front of it (attention_bwd3.hip,
// or attention_generic.hip without ATTN_PLAIN_STATS) leaves the two per-row vectors it starts from in `delta`.
#include "gf_common.h"
#include "gf_amd.h"
#include "attn_common.h"

using namespace gfattn;

namespace {

// dK / dV: one workgroup per 128 keys (32 per wave, K and V fragments in registers; K carries the exact power-of-two
// part p2 of scale * log2(e) = p2 * rr), Q / dO tiles of 64 query rows and the two per-row vectors the dQ kernel wrote
// (stat[0] = -lse * log2(e) / rr, stat[1] = -delta) streamed through the ring.  The vectors are the INITIAL VALUES of
// the S and dP accumulators -- they land there straight from LDS -- so P = exp2(rr * acc) and dS = P * acc.
constexpr int DKV_STATS = 2 * FT_TILE;                 // per wave: 16 lse | 16 delta | duplicates (256 B)
constexpr int DKV_STAGE = 2 * FT_TILE + 1024;
constexpr int DKV_NSTAGE = 3;

// Timing probes only (tools/probe/attn_stall_table.sh; the shipped library builds with 0): what does the dK/dV loop cost
// without ... 1 the exponentials, 2 the two output products (dV += P^T dO, dK += dS^T Q: 8 of the 16 MFMAs of a half tile),
// 4 the DMA of the next tiles, 8 the hardware-transposed LDS reads of the output products' operands, 16 the row-major LDS
// reads + statistics.  Results are wrong by construction.
#ifndef GF_DKV_ABL
#define GF_DKV_ABL 0
#endif
#if GF_DKV_ABL & 2
#define GF_DKV_OUT_MMA(acc, a, b) do { const auto a_ = (a); const auto b_ = (b); asm volatile("" ::"v"(a_), "v"(b_)); } while (0)
#else
#define GF_DKV_OUT_MMA(acc, a, b) mma16(acc, a, b)
#endif
template <int QB, bool PRE, bool SPLIT, typename Mid>      // SPLIT: P and dS as hi + lo bf16 pairs (attention_fwd3.hip)
__device__ __forceinline__ void dkv_half_tile(f32x16 (&dk)[2], f32x16 (&dv)[2], const bf16x8 (&kf)[4],
                                              const bf16x8 (&vf)[4], const unsigned (&aR)[4],
                                              const unsigned (&aT)[4], unsigned aS, float c,
                                              int hi, int nvalid, Mid&& mid) {
    f32x4 l4[4], d4[4];
#define GF_ST(g) l4[g] = __builtin_bit_cast(f32x4, lds_rd128<(2 * QB + (g >> 1)) * 256 + 32 * (g & 1)>(aS)); \
                 d4[g] = __builtin_bit_cast(f32x4, lds_rd128<(2 * QB + (g >> 1)) * 256 + 32 * (g & 1) + 64>(aS));
    if (!(GF_DKV_ABL & 16)) { GF_ST(0) GF_ST(1) GF_ST(2) GF_ST(3) }
    else {
#pragma unroll
        for (int g = 0; g < 4; ++g) { l4[g] = f32x4{0.f, 0.f, 0.f, 0.f}; d4[g] = l4[g]; }
    }
#undef GF_ST
    u32x4 qa[4], da[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qa[s] = (GF_DKV_ABL & 16) ? u32x4{0u, 0u, 0u, 0u} : lds_rd128<QB * 4096>(aR[s]);
    wait_lgkm<4>();
    f32x16 sa, dp;
#pragma unroll
    for (int g = 0; g < 4; ++g) {                                   // the per-row vectors ARE the initial values (stored
        tie(l4[g]);                                                 // negated and in the exponent's units by the dQ kernel)
        tie(d4[g]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sa[4 * g + e] = l4[g][e];
            dp[4 * g + e] = d4[g][e];
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) da[s] = (GF_DKV_ABL & 16) ? u32x4{0u, 0u, 0u, 0u} : lds_rd128<FT_TILE + QB * 4096>(aR[s]);
    wait_lgkm<4>();
#pragma unroll
    for (int s = 0; s < 4; ++s) {                               // k-steps chained on ONE accumulator: switching
        tie(qa[s]);                                             // accumulators between MFMAs measured 9 % slower
        mma16(sa, as_frag(qa[s]), kf[s]);                       // S[q][key] - lse/scale
    }
    // transposed operands: [t][db] -> rows 16t + 4hi + {0..3} (lo) and + 8 (hi half), columns db*32 + l31
    u32x2 dot[2][2][2], qt[2][2][2];
#define GF_TR(dst, base, t, db) dst[t][db][0] = (GF_DKV_ABL & 8) ? u32x2{0u, 0u} : lds_rdtr<base + QB * 4096 + t * 2048>(aT[db]); \
                                dst[t][db][1] = (GF_DKV_ABL & 8) ? u32x2{0u, 0u} : lds_rdtr<base + QB * 4096 + t * 2048 + 1024>(aT[2 + db]);
    GF_TR(dot, FT_TILE, 0, 0) GF_TR(dot, FT_TILE, 0, 1) GF_TR(dot, FT_TILE, 1, 0) GF_TR(dot, FT_TILE, 1, 1)
    wait_lgkm<8>();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        tie(da[s]);
        mma16(dp, as_frag(da[s]), vf[s]);                       // dP[q][key] - delta
    }
    GF_TR(qt, 0, 0, 0) GF_TR(qt, 0, 0, 1) GF_TR(qt, 0, 1, 0) GF_TR(qt, 0, 1, 1)
#undef GF_TR
    if (!(GF_DKV_ABL & 4)) mid();                               // DMA issue rides in the VALU gap
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float pr = (GF_DKV_ABL & 1) ? sa[r] : fast_exp2(PRE ? sa[r] : sa[r] * c);
        sa[r] = pr;
        dp[r] = pr * dp[r];                                     // dS overwrites dP
    }
    if (nvalid < 64) {                                          // ragged last tile: rows past Nq contribute 0
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (QB * 32 + crow(r, hi) >= nvalid) { sa[r] = 0.f; dp[r] = 0.f; }
    }
    wait_lgkm<8>();
    {
        const bf16x8 pf0 = cvt_frag(sa, 0), pf1 = cvt_frag(sa, 1);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            tie(dot[0][db][0]); tie(dot[0][db][1]); tie(dot[1][db][0]); tie(dot[1][db][1]);
            GF_DKV_OUT_MMA(dv[db], as_frag(dot[0][db][0], dot[0][db][1]), pf0);
            GF_DKV_OUT_MMA(dv[db], as_frag(dot[1][db][0], dot[1][db][1]), pf1);
        }
        if (SPLIT) {
            const bf16x8 pl0 = cvt_frag_lo(sa, 0, pf0), pl1 = cvt_frag_lo(sa, 1, pf1);
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                GF_DKV_OUT_MMA(dv[db], as_frag(dot[0][db][0], dot[0][db][1]), pl0);
                GF_DKV_OUT_MMA(dv[db], as_frag(dot[1][db][0], dot[1][db][1]), pl1);
            }
        }
    }
    wait_lgkm<0>();
    {
        const bf16x8 pf0 = cvt_frag(dp, 0), pf1 = cvt_frag(dp, 1);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            tie(qt[0][db][0]); tie(qt[0][db][1]); tie(qt[1][db][0]); tie(qt[1][db][1]);
            GF_DKV_OUT_MMA(dk[db], as_frag(qt[0][db][0], qt[0][db][1]), pf0);
            GF_DKV_OUT_MMA(dk[db], as_frag(qt[1][db][0], qt[1][db][1]), pf1);
        }
        if (SPLIT) {
            const bf16x8 pl0 = cvt_frag_lo(dp, 0, pf0), pl1 = cvt_frag_lo(dp, 1, pf1);
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                GF_DKV_OUT_MMA(dk[db], as_frag(qt[0][db][0], qt[0][db][1]), pl0);
                GF_DKV_OUT_MMA(dk[db], as_frag(qt[1][db][0], qt[1][db][1]), pl1);
            }
        }
    }
}

// NW waves per workgroup (32 keys each) share the Q/dO stream; PRE: rr == 1, no multiply per score; EVEN: Nq % 64 == 0 -- no
// ragged tile: unconditional re-fetching DMA (tiles past the end fetch the last one again), constant wait counts, no
// row masking: no tile-dependent branch in the loop (attention_fwd3.hip)
template <int NW, bool PRE, bool EVEN, bool SPLIT = false>
__global__ __launch_bounds__(64 * NW, 8 / NW) void attn_bwd_dkv_bf16_kernel(AttnParams p) {
    constexpr int KPB = 32 * NW, PPW = 8 / NW;    // keys per block, 1-KiB DMA pieces per wave and matrix
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned lds0 = (unsigned)(size_t)smem;

    const int nkb = (p.Nk + KPB - 1) / KPB;
    const int total = nkb * p.H * p.B;
    int lb = xcd_remap(blockIdx.x, total);
    const int kb_ = lb % nkb, h = (lb / nkb) % p.H, b = lb / (nkb * p.H);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5, s16 = lane & 15, half = (lane >> 4) & 1;
#ifdef GF_DKV_PRIO
    // static priority asymmetry between the waves that share a SIMD (probe knob; see DESIGN.md "convoy")
    if (NW == 8) { if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256) __builtin_amdgcn_s_setprio(GF_DKV_PRIO); }
    else if ((blockIdx.x >> 8) & 1) __builtin_amdgcn_s_setprio(GF_DKV_PRIO);
#endif
    const int krow = kb_ * KPB + wave * 32 + l31;
    const int kld = min(krow, p.Nk - 1);

    const bf16_t* qp = reinterpret_cast<const bf16_t*>(p.q) + b * p.sqb + h * p.sqh;
    const bf16_t* kp = reinterpret_cast<const bf16_t*>(p.k) + b * p.skb + h * p.skh;
    const bf16_t* vp = reinterpret_cast<const bf16_t*>(p.v) + b * p.svb + h * p.svh;
    const bf16_t* dop = reinterpret_cast<const bf16_t*>(p.dout) + b * p.sdob + h * p.sdoh;
    const float* lsep = p.delta + ((int64_t)b * p.H + h) * p.Nq;                       // stat[0]
    const float* delp = lsep + (int64_t)p.B * p.H * p.Nq;                               // stat[1]

    // ---- DMA descriptors: chunk (2 wave + i) * 64 + lane of a tile -> row, swizzled source column
    int drow[PPW], dcol[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        drow[i] = (PPW * wave + i) * 8 + (lane >> 3);
        dcol[i] = ((lane & 7) ^ fswz(drow[i])) * 8;
    }
    const float* statp = (lane & 16) ? delp : lsep;
    const int srow = 16 * wave + s16;
    const bool stat_wave = __builtin_amdgcn_readfirstlane(wave) < 4;
    // part 0: Q pieces + stats, part 1: dO pieces (issued in the VALU gaps of the two half tiles)
    const int64_t qstep = 64 * p.sqn, dostep = 64 * p.sdon;
    const bf16_t* gq[PPW];
    const bf16_t* gdo[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        gq[i] = qp + (int64_t)drow[i] * p.sqn + dcol[i];
        gdo[i] = dop + (int64_t)drow[i] * p.sdon + dcol[i];
    }
    auto issue_part = [&](int part, int t, int stage) {
        char* sb = smem + stage * DKV_STAGE;
        const int q0 = t * 64;
        if (EVEN || q0 + 64 <= p.Nq) {
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                if (part == 0) dma16(gq[i] + t * qstep, sb + (PPW * wave + i) * 1024);
                else dma16(gdo[i] + t * dostep, sb + FT_TILE + (PPW * wave + i) * 1024);
            }
        } else {                                                // ragged last tile: rows clamped to Nq - 1
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                const int64_t r = min(q0 + drow[i], p.Nq - 1);
                if (part == 0) dma16(qp + r * p.sqn + dcol[i], sb + (PPW * wave + i) * 1024);
                else dma16(dop + r * p.sdon + dcol[i], sb + FT_TILE + (PPW * wave + i) * 1024);
            }
        }
        if (part == 0 && stat_wave) dma4(statp + (EVEN ? q0 + srow : min(q0 + srow, p.Nq - 1)), sb + DKV_STATS + wave * 256);
    };
    auto issue_tile = [&](int t, int stage) { issue_part(0, t, stage); issue_part(1, t, stage); };

    const int nt = (p.Nq + 63) / 64;
    issue_tile(0, 0);
    if (EVEN) issue_tile(min(1, nt - 1), 1);
    else if (nt > 1) issue_tile(1, 1);

    const float p2 = p.p2, c = PRE ? 1.f : p.rr;                   // c: the non-power-of-two rest rr of scale * log2(e)
    bf16x8 kf[4], vf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        kf[s] = *reinterpret_cast<const bf16x8*>(kp + (int64_t)kld * p.skn + 16 * s + 8 * hi);
        if (p2 != 1.f) kf[s] = scale_frag(kf[s], p2);
        vf[s] = *reinterpret_cast<const bf16x8*>(vp + (int64_t)kld * p.svn + 16 * s + 8 * hi);
    }

    f32x16 dk[2], dv[2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[db][r] = 0.f; dv[db][r] = 0.f; }

    // ---- per-lane LDS read addresses (stage 0); see the layout note in attn_common.h.  The same values as fq_addresses()
    // returns, kept inline: through the helper the compiler assigns registers and orders the prologue differently (same
    // register and instruction counts), and this kernel's code is not to move without a measurement
    unsigned bR[4], bT[4];
    {
        const unsigned rb = l31 * 128 + 16 * (hi ^ fswz(l31));
#pragma unroll
        for (int s = 0; s < 4; ++s) bR[s] = lds0 + (rb ^ (32 * s));
        const int bq = s16 >> 3;
        const unsigned tb = (4 * hi + (s16 >> 2)) * 128 + 8 * (s16 & 1) +
                            16 * ((2 * half + ((s16 & 3) >> 1)) ^ (4 * bq + hi));
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int db = 0; db < 2; ++db) bT[2 * u + db] = lds0 + (tb ^ (32 * u) ^ (64 * db));
    }
    const unsigned bS = lds0 + DKV_STATS + 16 * hi;

    int stage = 0;
    for (int t = 0; t < nt; ++t) {
        if (!EVEN && t + 1 >= nt) wait_vm<0>();                   // tile t landed (this wave's share)
        else if (stat_wave) wait_vm<2 * PPW + 1>();
        else wait_vm<2 * PPW>();
        __builtin_amdgcn_s_barrier();                             // ... everyone's; stage of tile t-1 is free
        __builtin_amdgcn_sched_barrier(0);
        const unsigned so = stage * DKV_STAGE;
        unsigned aR[4], aT[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { aR[i] = bR[i] + so; aT[i] = bT[i] + so; }
        const int nvalid = EVEN ? 64 : p.Nq - t * 64;
        const int nstage = stage == 0 ? 2 : stage - 1;
        const bool more = EVEN || t + 2 < nt;
        const int tn = EVEN ? min(t + 2, nt - 1) : t + 2;
        dkv_half_tile<0, PRE, SPLIT>(dk, dv, kf, vf, aR, aT, bS + so, c, hi, nvalid,
                         [&] { if (more) issue_part(0, tn, nstage); });
        dkv_half_tile<1, PRE, SPLIT>(dk, dv, kf, vf, aR, aT, bS + so, c, hi, nvalid,
                         [&] { if (more) issue_part(1, tn, nstage); });
        stage = stage == 2 ? 0 : stage + 1;
    }
    if (EVEN) wait_vm<0>();                                       // the re-fetched tail tiles
    if (krow < p.Nk) {
        bf16_t* dkp = reinterpret_cast<bf16_t*>(p.dk) + b * p.sdkb + h * p.sdkh + (int64_t)krow * p.sdkn;
        bf16_t* dvp = reinterpret_cast<bf16_t*>(p.dv) + b * p.sdvb + h * p.sdvh + (int64_t)krow * p.sdvn;
        if (p.flags & GF_ATTN_ACC_DK) add_row<64>(dkp, dk, p.scale, hi); else store_row<bf16_t, 64>(dkp, dk, p.scale, hi);
        store_row<bf16_t, 64>(dvp, dv, 1.f, hi);
    }
}

}  // namespace

namespace gfattn {

int launch_dkv_bf16(const AttnParams& p, hipStream_t st) {
#ifdef GF_DKV_NW
    constexpr int NW = GF_DKV_NW;
#else
    constexpr int NW = 4;                       // 8 waves sharing one Q/dO stream measured 7 % slower
#endif
    const int total = ((p.Nk + 32 * NW - 1) / (32 * NW)) * p.H * p.B;
    const size_t lds = DKV_NSTAGE * DKV_STAGE;
    void (*const kern[8])(AttnParams) = {attn_bwd_dkv_bf16_kernel<NW, false, false>, attn_bwd_dkv_bf16_kernel<NW, false, true>,
                                         attn_bwd_dkv_bf16_kernel<NW, true, false>, attn_bwd_dkv_bf16_kernel<NW, true, true>,
                                         attn_bwd_dkv_bf16_kernel<NW, false, false, true>, attn_bwd_dkv_bf16_kernel<NW, false, true, true>,
                                         attn_bwd_dkv_bf16_kernel<NW, true, false, true>, attn_bwd_dkv_bf16_kernel<NW, true, true, true>};
    static unsigned long long attr_set = 0;     // function attributes are per DEVICE: one bit per device ordinal
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 64 || !((attr_set >> dev) & 1ull)) {
        for (auto k : kern)
            if (int e = set_lds(k, lds)) return e;
        if (dev < 64) attr_set |= 1ull << dev;
    }
    kern[((p.flags & GF_ATTN_SPLIT) ? 4 : 0) + (p.rr == 1.f ? 2 : 0) + (p.Nq % 64 == 0 ? 1 : 0)]<<<dim3(total), dim3(64 * NW), lds, st>>>(p);
    return gf_launched();
}

}  // namespace gfattn
