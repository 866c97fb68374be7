// Fused backward of the assignment head (gf_head_bwd).  Own translation unit with its own compiler flags (csrc/Makefile).
#include "gf_launch.h"
#include "attn_common.h"

using namespace gfattn;

namespace {

// ===========================================================================================
// Assignment-head backward, one side (lightglue.py:256-290 autograd; the "dual softmax" part):
//   S_so = oth_s . own_o,   dS_so = exp(S_so - ns_s) gs_s + exp(S_so - no_o) go_o,   dOwn_o = sum_s dS_so oth_s
// with (ns, gs) / (no, go) the log-sum-exp normaliser and incoming coefficient of the streamed row / of the owner.
// Called twice (owner = md1 rows -> d md1, owner = md0 rows -> d md0): no [B,N,N] dS tensor is written and no
// library GEMM follows.  It IS the attention forward's machinery (attn_common.h) with D = 256: the
// streamed [64 x 256] tile is four 64 x 64 sub-tiles in the forward's LDS-DMA ring layout, S^T comes from row
// fragments (ds_read_b128), dS goes from the accumulator registers straight into the second product, whose other
// operand oth^T is read with ds_read_b64_tr_b16 from the SAME tile.  One wave owns 32 owner rows and the whole
// 256-wide output row (8 accumulator tiles): one wave per SIMD, 512-register budget.
// ===========================================================================================
constexpr int HB_TILE = 4 * FT_TILE;                 // 64 rows x 256 channels
constexpr int HB_STAGE = HB_TILE + 1024;             // + ns | gs (64 floats each) | spare copies
constexpr int HB_NSTAGE = 3;

struct HeadBwdParams {
    const bf16_t* own; const bf16_t* oth;            // [B, No, 256], [B, Ns, 256]
    const float* no; const float* go;                // [B, No]
    const float* ns; const float* gs;                // [B, Ns]
    bf16_t* down;                                    // [B, No, 256]
    int B, No, Ns;
};

__global__ __launch_bounds__(256, 1) void head_bwd_bf16_kernel(HeadBwdParams p) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned lds0 = (unsigned)(size_t)smem;
    const int nob = (p.No + 127) / 128;
    const int lb = xcd_remap(blockIdx.x, nob * p.B);
    const int ob = lb % nob, b = lb / nob;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int orow = ob * 128 + wave * 32 + l31;
    const int old_ = min(orow, p.No - 1);
    const bf16_t* ownp = p.own + ((int64_t)b * p.No + old_) * 256;
    const bf16_t* othp = p.oth + (int64_t)b * p.Ns * 256;
    const float* nsp = p.ns + (int64_t)b * p.Ns;
    const float* gsp = p.gs + (int64_t)b * p.Ns;

    const int nt = (p.Ns + 63) / 64;
    // part i of tile t's DMA: i < 4 the two pieces of sub-tile i, i == 4 the per-row vectors (waves 0 / 1 bring ns / gs,
    // waves 2 / 3 the same into spare slots: equal vmcnt in every wave).  Tiles past the end re-fetch the last one.
    auto issue_part = [&](int t, int stage, int i) {
        char* sb = smem + stage * HB_STAGE;
        const int tc = min(t, nt - 1);
        if (i < 4) {
            fq_issue(othp + 64 * i, 256, tc * 64, p.Ns, sb + i * FT_TILE, wave, lane);
        } else {
            const float* src = (wave & 1) ? gsp : nsp;
            dma4(src + min(tc * 64 + lane, p.Ns - 1), sb + HB_TILE + (wave & 1) * 256 + (wave >> 1) * 512);
        }
    };
#pragma unroll
    for (int i = 0; i < 5; ++i) issue_part(0, 0, i);
#pragma unroll
    for (int i = 0; i < 5; ++i) issue_part(1, 1, i);

    bf16x8 of[16];                                     // owner row: B operand of S^T, k-step 4c + s
#pragma unroll
    for (int k = 0; k < 16; ++k) of[k] = *reinterpret_cast<const bf16x8*>(ownp + 16 * k + 8 * hi);
    const float no2 = p.no[(int64_t)b * p.No + old_] * GF_LOG2E;
    const float go = p.go[(int64_t)b * p.No + old_];

    f32x16 acc[8];                                     // dOwn^T[d][o]: d-tile 2c + db
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const FqAddr ad = fq_addresses(lds0, lane);

    int stage = 0;
    for (int t = 0; t < nt; ++t) {
        wait_vm<9>();                                             // tile t landed (this wave's pieces; t + 1 in flight)
        __builtin_amdgcn_s_barrier();                             // ... everyone's; the stage of tile t-1 is free
        __builtin_amdgcn_sched_barrier(0);
        const int nstage = stage == 0 ? 2 : stage - 1;            // tile t + 2 goes there, piece by piece between MFMAs
        const unsigned so = stage * HB_STAGE;
        unsigned aR[4], aT[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { aR[i] = ad.aR[i] + so; aT[i] = ad.aT[i] + so; }
        const unsigned aV = lds0 + so + HB_TILE + 16 * hi;        // ns of rows 8 g + 4 hi .. + 3 (gs: + 256 bytes)
        const int s0 = t * 64;
        if (s0 + 64 > p.Ns) {        // ragged last tile: the clamped duplicate rows become zero rows of oth (no contribution)
            const int lim = p.Ns - s0;
            for (int i = threadIdx.x; i < 4 * 64 * 8; i += 256) {
                const int row = (i >> 3) & 63;
                if (row >= lim) *reinterpret_cast<u32x4*>(smem + so + (i >> 9) * FT_TILE + row * 128 + (i & 7) * 16) = u32x4{0, 0, 0, 0};
            }
            __syncthreads();
        }

        // One wave per SIMD: the exponentials only overlap the matrix pipe if they sit BETWEEN MFMAs in program order.
        // Schedule per tile: S(rows 0-31) | S(rows 32-63) with dS(rows 0-31) one element per MFMA gap |
        // second product (rows 0-31) with dS(rows 32-63) in its gaps | second product (rows 32-63).
        u32x4 vn[2][4], vg[2][4];
        f32x16 sc0, sc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sc0[r] = 0.f; sc1[r] = 0.f; }
        auto elem = [&](f32x16& sc, const u32x4 (&n_)[4], const u32x4 (&g_)[4], int i) {
            const f32x4 n4 = __builtin_bit_cast(f32x4, n_[i >> 2]), g4 = __builtin_bit_cast(f32x4, g_[i >> 2]);
            const float x = sc[i];
            sc[i] = fast_exp2((x - n4[i & 3]) * GF_LOG2E) * g4[i & 3] + fast_exp2(fmaf(x, GF_LOG2E, -no2)) * go;
        };
        u32x4 ka[4], kc[4];
#define GF_HB_RD(dst, c, KB) _Pragma("unroll") for (int s = 0; s < 4; ++s) dst[s] = lds_rd128<(c) * FT_TILE + (KB) * 4096>(aR[s]);
#define GF_HB_S(sc, src, c, SIDE) _Pragma("unroll") for (int s = 0; s < 4; ++s) { tie(src[s]); mma16(sc, as_frag(src[s]), of[4 * (c) + s]); SIDE(4 * (c) + s) }
#define GF_HB_NONE(i)
#define GF_HB_DMA(i) if ((i) % 3 == 0 && (i) / 3 < 5) issue_part(t + 2, nstage, (i) / 3);
#define GF_HB_E0(i) elem(sc0, vn[0], vg[0], i);
#define GF_HB_E1(i) elem(sc1, vn[1], vg[1], i);
        // (never more than 12 LDS requests in flight: the counter holds 15)
#pragma unroll
        for (int g = 0; g < 4; ++g) { vn[0][g] = lds_rd128<0>(aV + 32 * g); vg[0][g] = lds_rd128<256>(aV + 32 * g); }
        GF_HB_RD(ka, 0, 0)
        wait_lgkm<4>();                                       // the row vectors of rows 0-31
        GF_HB_RD(kc, 1, 0)
        wait_lgkm<4>();
        GF_HB_S(sc0, ka, 0, GF_HB_DMA)
        GF_HB_RD(ka, 2, 0)
        wait_lgkm<4>();
        GF_HB_S(sc0, kc, 1, GF_HB_DMA)
        GF_HB_RD(kc, 3, 0)
        wait_lgkm<4>();
        GF_HB_S(sc0, ka, 2, GF_HB_DMA)
        GF_HB_RD(ka, 0, 1)
        wait_lgkm<4>();
        GF_HB_S(sc0, kc, 3, GF_HB_DMA)
#pragma unroll
        for (int g = 0; g < 4; ++g) { vn[1][g] = lds_rd128<128>(aV + 32 * g); vg[1][g] = lds_rd128<256 + 128>(aV + 32 * g); }
#pragma unroll
        for (int g = 0; g < 4; ++g) { tie(vn[0][g]); tie(vg[0][g]); }
        wait_lgkm<8>();                                       // ka (rows 32-63, sub-tile 0); the vectors still in flight
        GF_HB_RD(kc, 1, 1)
        GF_HB_S(sc1, ka, 0, GF_HB_E0)
        wait_lgkm<4>();                                       // the row vectors of rows 32-63
        GF_HB_RD(ka, 2, 1)
        wait_lgkm<4>();
        GF_HB_S(sc1, kc, 1, GF_HB_E0)
        GF_HB_RD(kc, 3, 1)
        wait_lgkm<4>();
        GF_HB_S(sc1, ka, 2, GF_HB_E0)
        // oth^T fragments of sub-tile 0, rows 0-31, requested under the last S block
        u32x2 va[2][2][2], vb[2][2][2];
#define GF_HB_TR(dst, c, KB) GF_FQ_TR(dst, (c) * FT_TILE, KB, 0, 0) GF_FQ_TR(dst, (c) * FT_TILE, KB, 0, 1) \
                             GF_FQ_TR(dst, (c) * FT_TILE, KB, 1, 0) GF_FQ_TR(dst, (c) * FT_TILE, KB, 1, 1)
        GF_HB_TR(va, 0, 0)
        wait_lgkm<8>();
        GF_HB_S(sc1, kc, 3, GF_HB_E0)
#pragma unroll
        for (int g = 0; g < 4; ++g) { tie(vn[1][g]); tie(vg[1][g]); }
        bf16x8 p0 = cvt_frag(sc0, 0), p1 = cvt_frag(sc0, 1);

        // ---- dOwn^T[d][o] += oth^T[d][s] dS[s][o]: sub-tile c feeds d-tiles 2c, 2c + 1 for both 16-row k-steps
#define GF_HB_MMA(src, c, SIDE)                                                                            \
        _Pragma("unroll") for (int db = 0; db < 2; ++db) {                                                 \
            tie(src[0][db][0]); tie(src[0][db][1]); tie(src[1][db][0]); tie(src[1][db][1]);                \
            mma16(acc[2 * (c) + db], as_frag(src[0][db][0], src[0][db][1]), p0); SIDE(4 * (c) + 2 * db)    \
            mma16(acc[2 * (c) + db], as_frag(src[1][db][0], src[1][db][1]), p1); SIDE(4 * (c) + 2 * db + 1) \
        }
        wait_lgkm<0>();
        GF_HB_TR(vb, 1, 0)
        GF_HB_MMA(va, 0, GF_HB_E1)
        wait_lgkm<0>();
        GF_HB_TR(va, 2, 0)
        GF_HB_MMA(vb, 1, GF_HB_E1)
        wait_lgkm<0>();
        GF_HB_TR(vb, 3, 0)
        GF_HB_MMA(va, 2, GF_HB_E1)
        wait_lgkm<0>();
        GF_HB_TR(va, 0, 1)
        GF_HB_MMA(vb, 3, GF_HB_E1)
        p0 = cvt_frag(sc1, 0); p1 = cvt_frag(sc1, 1);
        wait_lgkm<0>();
        GF_HB_TR(vb, 1, 1)
        GF_HB_MMA(va, 0, GF_HB_NONE)
        wait_lgkm<0>();
        GF_HB_TR(va, 2, 1)
        GF_HB_MMA(vb, 1, GF_HB_NONE)
        wait_lgkm<0>();
        GF_HB_TR(vb, 3, 1)
        GF_HB_MMA(va, 2, GF_HB_NONE)
        wait_lgkm<0>();
        GF_HB_MMA(vb, 3, GF_HB_NONE)
#undef GF_HB_MMA
#undef GF_HB_TR
#undef GF_HB_RD
#undef GF_HB_S
#undef GF_HB_NONE
#undef GF_HB_DMA
#undef GF_HB_E0
#undef GF_HB_E1
        stage = stage == 2 ? 0 : stage + 1;
    }
    wait_vm<0>();                                                 // the re-fetched tail tiles
    if (orow < p.No) {
        bf16_t* dst = p.down + ((int64_t)b * p.No + orow) * 256;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x16 pair[2] = {acc[2 * c], acc[2 * c + 1]};
            store_row<bf16_t, 64>(dst + 64 * c, pair, 1.f, hi);
        }
    }
}

}  // namespace

extern "C" int gf_head_bwd(const void* a, const void* b, const float* r, const float* c, const float* gr, const float* gc,
                           void* da, void* db, int B, int M, int N, int D, int dtype, void* stream) {
    if (B <= 0 || M <= 0 || N <= 0) return GF_ERR_SHAPE;
    if (dtype != GF_BF16 || D != 256) return GF_ERR_UNSUPPORTED;
    hipStream_t st = gf_stream(stream);
    const size_t lds = (size_t)HB_NSTAGE * HB_STAGE;
    if (int e = set_lds(head_bwd_bf16_kernel, lds)) return e;
    HeadBwdParams p;
    // d md1: owner = md1 rows (columns of S), streamed = md0 rows
    p.own = static_cast<const bf16_t*>(b); p.oth = static_cast<const bf16_t*>(a); p.no = c; p.go = gc; p.ns = r; p.gs = gr;
    p.down = static_cast<bf16_t*>(db); p.B = B; p.No = N; p.Ns = M;
    head_bwd_bf16_kernel<<<dim3(((N + 127) / 128) * B), dim3(256), lds, st>>>(p);
    if (int e = gf_launched()) return e;
    // d md0: owner = md0 rows, streamed = md1 rows
    p.own = static_cast<const bf16_t*>(a); p.oth = static_cast<const bf16_t*>(b); p.no = r; p.go = gr; p.ns = c; p.gs = gc;
    p.down = static_cast<bf16_t*>(da); p.No = M; p.Ns = N;
    head_bwd_bf16_kernel<<<dim3(((M + 127) / 128) * B), dim3(256), lds, st>>>(p);
    return gf_launched();
}
