// Weight / bias gradient of a linear layer over the token axis:
//     dW[n][k] = sum_m dY[m][n] X[m][k],   db[n] = sum_m dY[m][n]        (M = B*N tokens ~ 1.3e5)
// i.e. autograd's grad of F.linear (reference: every nn.Linear of lightglue.py:131-221, 271-290).
// The library GEMM handles this "tiny output, huge reduction" shape poorly (0.16-0.26 ms per
// call, 2/3 of all GEMM time of the step), so it is hand-written.
//
// One scheme, three kernels.  The scheme (split-M): a workgroup owns one 128x128 tile of dW and one
// slice of M (plan(): as many slices as fill one round of the chip; dw_tile(): which block gets
// which), streams that slice's dY / X rows through LDS into MFMAs with fp32 accumulation, and writes
// its partial tile to the workspace part[slice][Nout][K] (bias: bpart[slice][Nout]);
// linear_dw_reduce then sums the slices into fp32 dW / db -- deterministic, no atomics.
//
// The kernels differ in how the rows get from global memory into MFMA fragments; select_kernel() is
// the only place that chooses:
//   linear_dw_dma_kernel  bf16, Nout % 128 == 0 and K % 128 == 0: LDS-DMA ring.  Every linear of the
//                         benchmarked step, and the only tier that reads a two-source X (gf_linear_dw2).
//   linear_dw_tr_kernel   bf16, any other Nout, K (multiples of 8): register-staged row-major tiles,
//                         transposing LDS reads.
//   linear_dw_f32_kernel  fp32 (parity mode), Nout, K multiples of 4: register-staged, tiles
//                         transposed by the LDS stores.
// Each was the fast path until the next replaced it on the shapes that one can take (the section
// comments keep the measurements).  The two older ones stay as capability paths: the DMA tier's
// staging is unguarded, 128 columns wide and bf16-only, so ragged shapes and fp32 need them.
#include <cstdlib>
#include <type_traits>
#include "gf_launch.h"

#ifndef GF_DW_WG          // workgroup slots of one dW round (two per CU); probe builds override it
#define GF_DW_WG 512
#endif

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------
// Shared by the tiers: which tile and slice a block owns, the store of its partial tile, and the
// bias partial of the two register-staged tiers.
// ---------------------------------------------------------------------------------------------
struct DwTile { int tn, tk, slice, m_begin, m_end; };

// Grid: ntile * (nslice rounded up to 8) blocks; a block whose slice begins at or past M has no work.
// XCD-aware order: block b runs on XCD b % 8; all output tiles of one M-slice are given to the
// same XCD back to back, so the dY / X row slabs they share are served by that XCD's L2 instead of
// being re-read from HBM once per tile (4x the traffic at 512x512).  plan() counts on this order.
// RAGGED (here and below): Nout or K need not be a multiple of 128, so the last tile may hang over.
template <bool RAGGED>
__device__ __forceinline__ DwTile dw_tile(int Nout, int K, int rows_per_slice, int M) {
    const int ntk = RAGGED ? (K + 127) / 128 : K / 128;
    const int ntile = (RAGGED ? (Nout + 127) / 128 : Nout / 128) * ntk;
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int tile = j % ntile;
    DwTile t;
    t.slice = (j / ntile) * 8 + xcd;
    t.tn = tile / ntk;
    t.tk = tile % ntk;
    t.m_begin = t.slice * rows_per_slice;
    t.m_end = min(M, t.m_begin + rows_per_slice);
    return t;
}

// acc[i][j] of the 2 x 2 waves (each 64 (n) x 64 (k)) -> pp[n][k], this slice's [Nout][K] partial.
// C[n][k]: lane column = k (l31), rows n = crow(r, hi); wn, wk, l31, hi as the kernels compute them.
template <bool RAGGED>
__device__ __forceinline__ void store_partial(float* pp, const f32x16 (&acc)[2][2], int tn, int tk, int wn, int wk,
                                              int l31, int hi, int Nout, int K) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kk = tk * 128 + wk * 64 + j * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int nn = tn * 128 + wn * 64 + i * 32 + crow(r, hi);
                if (!RAGGED || (nn < Nout && kk < K)) pp[(int64_t)nn * K + kk] = acc[i][j][r];
            }
        }
}

// bpart[slice][tn's 128 columns] from per-thread column sums (tk == 0 blocks).  A thread's 16-byte chunk of the
// 128-wide row (CPR = 128 / VEC chunks) is the same for every M-chunk, but the rows of a chunk are spread over the whole
// workgroup: item it = tid + 256 i holds bsum[i][0 .. VEC) of chunk it % CPR, and the 256 ITEMS / CPR items of a chunk are
// combined through LDS (`red`: the tile buffers, reused after the main loop's last barrier).
template <int VEC, int ITEMS>
__device__ __forceinline__ void bias_through_lds(float* red, const float (&bsum)[ITEMS][VEC], float* bpart, int slice, int tn, int Nout) {
    constexpr int CPR = 128 / VEC;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        int it = threadIdx.x + 256 * i;
#pragma unroll
        for (int e = 0; e < VEC; ++e) red[it * VEC + e] = bsum[i][e];
    }
    __syncthreads();
    for (int col = threadIdx.x; col < 128; col += 256) {
        const int cc = col / VEC, e = col % VEC;
        float v = 0.f;
        for (int p = 0; p < 256 * ITEMS / CPR; ++p) v += red[(p * CPR + cc) * VEC + e];
        if (tn * 128 + col < Nout) bpart[(int64_t)slice * Nout + tn * 128 + col] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// fp32: dY / X row tiles (64 tokens x 128 columns) go through LDS TRANSPOSED (token axis contiguous,
// so MFMA fragments are 16-byte reads), double-buffered with register prefetch.  The transposition
// is done by the staging stores: 4-byte pairs of two rows.
// ---------------------------------------------------------------------------------------------
constexpr int F32_VEC = 4;                      // floats per 16-byte chunk
constexpr int F32_LDT = 64 + F32_VEC;           // transposed tile stride (16-byte aligned rows)
constexpr int F32_TILE = 128 * F32_LDT;         // elements: [128 cols][64 tokens]
constexpr int F32_CPR = 128 / F32_VEC;          // 16-byte chunks per 128-wide row slice
constexpr int F32_ITEMS = 32 * F32_CPR / 256;   // (row pair, chunk) items per thread
constexpr int F32_LDS = 4 * F32_TILE * 4;       // bytes: 2 buffers x (A^T tile | B^T tile)

struct F32Regs { u32x4 a[F32_ITEMS], b[F32_ITEMS]; };

// 8-element (16-byte) blocks of a transposed row are XOR-swizzled by the row's chunk index so that
// the coalesced staging order (consecutive lanes = consecutive 16-byte chunks of one source row)
// spreads its transposed 4-byte stores over the LDS banks; fragment reads stay 16-byte.
__device__ __forceinline__ int dswz(int d, int pos) { return pos ^ (((d >> 3) & 7) << 3); }

// rows [m0, m0+64) x cols [c0, c0+128) of a row-major [M, ld] matrix (zero beyond M / ncols)
__device__ __forceinline__ void f32_load(F32Regs& rg, const float* g, int64_t ld, int m0, int mend, int c0, int ncols) {
#pragma unroll
    for (int i = 0; i < F32_ITEMS; ++i) {
        int it = threadIdx.x + 256 * i;
        int cc = it % F32_CPR, p = it / F32_CPR;
        int r0 = m0 + 2 * p, r1 = r0 + 1, col = c0 + cc * F32_VEC;
        u32x4 z = {0, 0, 0, 0};
        bool okc = col < ncols;
        rg.a[i] = (okc && r0 < mend) ? *reinterpret_cast<const u32x4*>(g + (int64_t)r0 * ld + col) : z;
        rg.b[i] = (okc && r1 < mend) ? *reinterpret_cast<const u32x4*>(g + (int64_t)r1 * ld + col) : z;
    }
}
__device__ __forceinline__ void f32_store(const F32Regs& rg, float* ldsT) {
#pragma unroll
    for (int i = 0; i < F32_ITEMS; ++i) {
        int it = threadIdx.x + 256 * i;
        int cc = it % F32_CPR, p = it / F32_CPR;
        union { u32x4 u; float e[F32_VEC]; } x, y;
        x.u = rg.a[i];
        y.u = rg.b[i];
#pragma unroll
        for (int e = 0; e < F32_VEC; ++e) {
            f32x2 pr = {x.e[e], y.e[e]};
            const int d = cc * F32_VEC + e;
            *reinterpret_cast<f32x2*>(ldsT + d * F32_LDT + dswz(d, 2 * p)) = pr;
        }
    }
}

__global__ __launch_bounds__(256, 2) void linear_dw_f32_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                               float* __restrict__ part, float* __restrict__ bpart,
                                                               int M, int Nout, int K, int rows_per_slice) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lds = reinterpret_cast<float*>(smem);
    const DwTile t = dw_tile<true>(Nout, K, rows_per_slice, M);
    if (t.m_begin >= M) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int wn = wave >> 1, wk = wave & 1;       // 2 x 2 waves, each 64 (n) x 64 (k)

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float bsum[F32_ITEMS][F32_VEC];
#pragma unroll
    for (int i = 0; i < F32_ITEMS; ++i)
#pragma unroll
        for (int e = 0; e < F32_VEC; ++e) bsum[i][e] = 0.f;

    F32Regs ra, rb;
    auto add_bias = [&]() {
        if (t.tk == 0) {
#pragma unroll
            for (int i = 0; i < F32_ITEMS; ++i) {
                union { u32x4 u; float e[F32_VEC]; } x0, x1;
                x0.u = ra.a[i];
                x1.u = ra.b[i];
#pragma unroll
                for (int e = 0; e < F32_VEC; ++e) bsum[i][e] += x0.e[e] + x1.e[e];
            }
        }
    };
    const int nchunk = (t.m_end - t.m_begin + 63) / 64;
    if (nchunk > 0) {
        f32_load(ra, dy, Nout, t.m_begin, t.m_end, t.tn * 128, Nout);
        f32_load(rb, x, K, t.m_begin, t.m_end, t.tk * 128, K);
        add_bias();
        f32_store(ra, lds);
        f32_store(rb, lds + F32_TILE);
    }
    __syncthreads();
    for (int c = 0; c < nchunk; ++c) {
        const float* At = lds + (c & 1) * 2 * F32_TILE;
        const float* Bt = At + F32_TILE;
        if (c + 1 < nchunk) {
            f32_load(ra, dy, Nout, t.m_begin + (c + 1) * 64, t.m_end, t.tn * 128, Nout);
            f32_load(rb, x, K, t.m_begin + (c + 1) * 64, t.m_end, t.tk * 128, K);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {      // 64 tokens = 4 k-steps of 16
            Frag<float> af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int dn = wn * 64 + i * 32 + l31, dk = wk * 64 + i * 32 + l31;
                af[i] = ld_frag8(At + dn * F32_LDT + dswz(dn, 16 * s + 8 * hi));
                bf[i] = ld_frag8(Bt + dk * F32_LDT + dswz(dk, 16 * s + 8 * hi));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma32(acc[i][j], af[i], bf[j]);
        }
        if (c + 1 < nchunk) {
            add_bias();
            float* nb = lds + ((c + 1) & 1) * 2 * F32_TILE;
            f32_store(ra, nb);
            f32_store(rb, nb + F32_TILE);
        }
        __syncthreads();
    }
    store_partial<true>(part + (int64_t)t.slice * Nout * K, acc, t.tn, t.tk, wn, wk, l31, hi, Nout, K);
    if (t.tk == 0) bias_through_lds(lds, bsum, bpart, t.slice, t.tn, Nout);
}

// ---------------------------------------------------------------------------------------------
// bf16, any Nout / K: ROW-MAJOR LDS tiles (16-byte coalesced global loads -> conflict-free 16-byte LDS
// stores, no transposing stores at all) read back through gfx950's transposing LDS load
// ds_read_b64_tr_b16.  Semantics (probed on hardware, tools/probe/tr.hip): inside each group of 16
// lanes, lane s supplies the address of 4 consecutive bf16; output lane i receives, for j = 0..3,
// element (i & 3) of source lane (i >> 2) + 4 j.  With source lane s pointing at
// tile[m0 + (s >> 2)][c0 + 4 (s & 3)], output lane i holds column c0 + i at rows m0 .. m0 + 3:
// exactly the "4 consecutive tokens of my column" an MFMA fragment needs.
// ---------------------------------------------------------------------------------------------
constexpr int TR_LD = 128 + 32;                 // row stride (bf16): 320 B -> rows 16 banks apart (of 64)
constexpr int TR_TILE = 64 * TR_LD;
constexpr int TR_LDS = 4 * TR_TILE * 2;         // bytes: 2 buffers x (dY tile | X tile), row-major

__device__ __forceinline__ u32x2 ds_read_tr16(const bf16_t* p) {
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"((unsigned)(size_t)p) : "memory");
    return v;
}

struct TrRegs { u32x4 v[4]; unsigned ok; };     // 64 x 128 bf16 tile = 1024 chunks / 256 threads

// Loads are UNCONDITIONAL (indices clamped into the matrix, validity kept as bits and applied when
// the registers are stashed): predicated loads become exec-masked branches, which both serialise
// issue and make the compiler fall back to s_waitcnt vmcnt(0), i.e. no prefetch across iterations.
__device__ __forceinline__ void tr_load(TrRegs& rg, const bf16_t* g, int64_t ld, int m0, int mend, int c0, int ncols) {
    rg.ok = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int it = threadIdx.x + 256 * i;
        int cc = it & 15, r = it >> 4;
        int row = m0 + r, col = c0 + cc * 8;
        rg.ok |= (unsigned)(row < mend && col < ncols) << i;
        rg.v[i] = *reinterpret_cast<const u32x4*>(g + (int64_t)min(row, mend - 1) * ld + min(col, ncols - 8));
    }
}
__device__ __forceinline__ void tr_mask(TrRegs& rg) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned keep = (rg.ok >> i) & 1u ? 0xffffffffu : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) rg.v[i][e] &= keep;
    }
}
__device__ __forceinline__ void tr_store(const TrRegs& rg, bf16_t* tile) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int it = threadIdx.x + 256 * i;
        int cc = it & 15, r = it >> 4;
        *reinterpret_cast<u32x4*>(tile + r * TR_LD + cc * 8) = rg.v[i];
    }
}

__global__ __launch_bounds__(256, 2) void linear_dw_tr_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                              float* __restrict__ part, float* __restrict__ bpart,
                                                              int M, int Nout, int K, int rows_per_slice) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* lds = reinterpret_cast<bf16_t*>(smem);
    const DwTile t = dw_tile<true>(Nout, K, rows_per_slice, M);
    if (t.m_begin >= M) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int wn = wave >> 1, wk = wave & 1;
    // per-lane part of the transposing-read address: row (s >> 2) + 8 hi, column 16 (g & 1) + 4 (s & 3)
    const int s16 = lane & 15, g1 = (lane >> 4) & 1;
    const int lane_off = ((s16 >> 2) + 8 * hi) * TR_LD + 16 * g1 + 4 * (s16 & 3);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float bsum[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) bsum[i][e] = 0.f;

    // Global loads run TWO chunks ahead of the MFMAs (two register sets, statically indexed through an
    // unroll-by-2), the LDS image one chunk ahead.
    TrRegs ra0, rb0, ra1, rb1;
    auto load = [&](TrRegs& a_, TrRegs& b_, int c) {
        tr_load(a_, dy, Nout, t.m_begin + c * 64, t.m_end, t.tn * 128, Nout);
        tr_load(b_, x, K, t.m_begin + c * 64, t.m_end, t.tk * 128, K);
    };
    auto stash = [&](TrRegs& a_, TrRegs& b_, int c) {
        tr_mask(a_);
        tr_mask(b_);
        if (t.tk == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                union { u32x4 u; bf16_t e[8]; } v;
                v.u = a_.v[i];
#pragma unroll
                for (int e = 0; e < 8; ++e) bsum[i][e] += (float)v.e[e];
            }
        }
        bf16_t* nb = lds + (c & 1) * 2 * TR_TILE;
        tr_store(a_, nb);
        tr_store(b_, nb + TR_TILE);
    };
    // Fragment reads of k-step ks+1 are issued before the MFMAs of k-step ks (two register sets), so the
    // LDS latency of the (compiler-invisible) transposing reads hides behind 4 MFMAs instead of stalling.
    struct FragSet { u32x2 a[2][2], b[2][2]; };
    auto issue = [&](FragSet& f, const bf16_t* At, const bf16_t* Bt, int ks) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bf16_t* pa = At + (16 * ks) * TR_LD + wn * 64 + i * 32 + lane_off;
            const bf16_t* pb = Bt + (16 * ks) * TR_LD + wk * 64 + i * 32 + lane_off;
            f.a[i][0] = ds_read_tr16(pa);
            f.a[i][1] = ds_read_tr16(pa + 4 * TR_LD);
            f.b[i][0] = ds_read_tr16(pb);
            f.b[i][1] = ds_read_tr16(pb + 4 * TR_LD);
        }
    };
    auto wait_all = [&](FragSet& f) {
        // asm loads are invisible to the compiler's waitcnt bookkeeping: tie every destination to the wait
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(f.a[0][0]), "+v"(f.a[0][1]), "+v"(f.a[1][0]), "+v"(f.a[1][1]),
                       "+v"(f.b[0][0]), "+v"(f.b[0][1]), "+v"(f.b[1][0]), "+v"(f.b[1][1])
                     :: "memory");
        __builtin_amdgcn_sched_barrier(0);
    };
    auto mfmas = [&](const FragSet& f) {
        Frag<bf16_t> af[2], bf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            union { u32x2 u[2]; bf16x8 v; } ta, tb;
            ta.u[0] = f.a[i][0]; ta.u[1] = f.a[i][1];
            tb.u[0] = f.b[i][0]; tb.u[1] = f.b[i][1];
            af[i].v = ta.v;
            bf[i].v = tb.v;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) mma32(acc[i][j], af[i], bf[j]);
    };
    auto compute = [&](int c) {
        const bf16_t* At = lds + (c & 1) * 2 * TR_TILE;
        const bf16_t* Bt = At + TR_TILE;
        FragSet f0, f1;
        issue(f0, At, Bt, 0);
        wait_all(f0);
        issue(f1, At, Bt, 1);
        mfmas(f0);
        wait_all(f1);
        issue(f0, At, Bt, 2);
        mfmas(f1);
        wait_all(f0);
        issue(f1, At, Bt, 3);
        mfmas(f0);
        wait_all(f1);
        mfmas(f1);
    };
    const int nchunk = (t.m_end - t.m_begin + 63) / 64;
    if (nchunk > 0) {
        load(ra0, rb0, 0);
        if (nchunk > 1) load(ra1, rb1, 1);
        stash(ra0, rb0, 0);
    }
    __syncthreads();
    // top of iteration c: LDS[c&1] holds chunk c; register set (c+1)&1 holds chunk c+1 (maybe in flight)
    for (int c = 0; c < nchunk; c += 2) {
        if (c + 2 < nchunk) load(ra0, rb0, c + 2);
        compute(c);
        if (c + 1 < nchunk) stash(ra1, rb1, c + 1);
        __syncthreads();
        if (c + 1 < nchunk) {
            if (c + 3 < nchunk) load(ra1, rb1, c + 3);
            compute(c + 1);
            if (c + 2 < nchunk) stash(ra0, rb0, c + 2);
            __syncthreads();
        }
    }
    store_partial<true>(part + (int64_t)t.slice * Nout * K, acc, t.tn, t.tk, wn, wk, l31, hi, Nout, K);
    if (t.tk == 0) {
        float tot[1][8];                        // a thread's four items share one column chunk (tid & 15)
#pragma unroll
        for (int e = 0; e < 8; ++e) tot[0][e] = bsum[0][e] + bsum[1][e] + bsum[2][e] + bsum[3][e];
        bias_through_lds(reinterpret_cast<float*>(smem), tot, bpart, t.slice, t.tn, Nout);
    }
}

// ---------------------------------------------------------------------------------------------
// bf16, Nout % 128 == 0 and K % 128 == 0: LDS-DMA staging.  The register-staged kernel above spends more
// LDS-pipe time on its staging stores (8 ds_write_b128 per thread and chunk: ~415 cycles per workgroup-chunk
// at 79 B/clk) than on the transposing reads the MFMAs need (256 cycles), and the LDS pipe is what bounds it.
// Here `global_load_lds_dwordx4` writes the tiles (32 tokens x 128 channels of dY and of X per stage,
// unpadded rows, 16-byte chunks XOR-swizzled by (row & 3) << 2 so the 4-row transposing reads hit distinct
// bank groups) into a 4-stage ring, counted vmcnt, one raw barrier per chunk; the bias gradient is a third
// MFMA against a fragment of ones.
// ---------------------------------------------------------------------------------------------
constexpr int DM_ROWS = 32, DM_TILE = DM_ROWS * 256, DM_STAGE = 2 * DM_TILE, DM_NSTAGE = 4;
constexpr int DM_LDS = DM_NSTAGE * DM_STAGE;    // bytes
typedef __attribute__((address_space(3))) void dm_lds_void;
typedef const __attribute__((address_space(1))) void dm_glb_void;

template <int OFF> __device__ __forceinline__ u32x2 dm_rdtr(unsigned a) {
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(a), "n"(OFF) : "memory");
    return v;
}
template <int N> __device__ __forceinline__ void dm_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <typename V> __device__ __forceinline__ void dm_tie(V& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ bf16x8 dm_frag(u32x2 lo, u32x2 hi) {
    u32x4 v = {lo[0], lo[1], hi[0], hi[1]};
    return __builtin_bit_cast(bf16x8, v);
}

template <int SO, bool BIAS>
__device__ __forceinline__ void dm_chunk(f32x16 (&acc)[2][2], f32x16 (&bacc)[2], unsigned aA, unsigned aB) {
    // 32 tokens = 2 k-steps: [ks][i][half] for the dY^T (A) and X^T (B) fragments; i toggles address bit 6
    u32x2 fa[2][2][2], fb[2][2][2];
#define GF_RD(ks) \
    fa[ks][0][0] = dm_rdtr<SO + ks * 4096>(aA);            fa[ks][0][1] = dm_rdtr<SO + ks * 4096 + 1024>(aA); \
    fa[ks][1][0] = dm_rdtr<SO + ks * 4096>(aA ^ 64u);      fa[ks][1][1] = dm_rdtr<SO + ks * 4096 + 1024>(aA ^ 64u); \
    fb[ks][0][0] = dm_rdtr<SO + DM_TILE + ks * 4096>(aB);  fb[ks][0][1] = dm_rdtr<SO + DM_TILE + ks * 4096 + 1024>(aB); \
    fb[ks][1][0] = dm_rdtr<SO + DM_TILE + ks * 4096>(aB ^ 64u); fb[ks][1][1] = dm_rdtr<SO + DM_TILE + ks * 4096 + 1024>(aB ^ 64u);
    GF_RD(0)
    GF_RD(1)
#undef GF_RD
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (bf16_t)1.0f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        if (ks == 0) asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < 2; ++i) { dm_tie(fa[ks][i][0]); dm_tie(fa[ks][i][1]); dm_tie(fb[ks][i][0]); dm_tie(fb[ks][i][1]); }
        const bf16x8 a0 = dm_frag(fa[ks][0][0], fa[ks][0][1]), a1 = dm_frag(fa[ks][1][0], fa[ks][1][1]);
        const bf16x8 b0 = dm_frag(fb[ks][0][0], fb[ks][0][1]), b1 = dm_frag(fb[ks][1][0], fb[ks][1][1]);
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
        if (BIAS) {
            bacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, ones, bacc[0], 0, 0, 0);
            bacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, ones, bacc[1], 0, 0, 0);
        }
    }
}

// x: the X source of THIS k-tile, already offset to its first column; ldx: that source's row stride (two-source calls:
// tiles left of K1 read x1, the others x2 -- the virtual concatenation [x1 | x2] is never built)
template <bool BIAS>
__device__ __forceinline__ void dm_body(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, int ldx,
                                        float* __restrict__ pp, float* __restrict__ bp, int M, int Nout, int K, int m_begin,
                                        int m_end, int tn, int tk) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const unsigned lds0 = (unsigned)(size_t)smem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5, s16 = lane & 15, g1 = (lane >> 4) & 1;
    const int wn = wave >> 1, wk = wave & 1;

    // ---- DMA descriptors: pieces 2*wave, 2*wave+1 of each tile; a piece = 4 rows x 256 B
    const int prow = lane >> 4, pphys = lane & 15;
    const int plog = pphys ^ ((prow & 3) << 2);
    const bf16_t* gA = dy + (int64_t)tn * 128 + plog * 8;
    const bf16_t* gB = x + plog * 8;
    auto issue = [&](int c, int stage) {
        char* sb = smem + stage * DM_STAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int piece = 2 * wave + i;
            const int64_t row = min(m_begin + c * DM_ROWS + 4 * piece + prow, M - 1);
            __builtin_amdgcn_global_load_lds((dm_glb_void*)(gA + row * Nout), (dm_lds_void*)(sb + piece * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((dm_glb_void*)(gB + row * ldx), (dm_lds_void*)(sb + DM_TILE + piece * 1024), 16, 0, 0);
        }
    };
    const int nchunk = (m_end - m_begin + DM_ROWS - 1) / DM_ROWS;
#pragma unroll
    for (int c = 0; c < DM_NSTAGE - 1; ++c)
        if (c < nchunk) issue(c, c);

    f32x16 acc[2][2], bacc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) bacc[i][r] = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }
    // per-lane transposing-read addresses (stage 0, k-step 0, first half): row 8 hi + (s16 >> 2), 8-byte piece
    // (s16 & 1) of logical 16-byte chunk 8 w + 2 g1 + ((s16 & 3) >> 1), XOR-swizzled by (row & 3) << 2
    const int rr = (s16 >> 2) & 3;
    auto rd_addr = [&](int w) {
        const int chunk = (8 * w + 2 * g1 + ((s16 & 3) >> 1)) ^ (rr << 2);
        return lds0 + (unsigned)((8 * hi + (s16 >> 2)) * 256 + chunk * 16 + (s16 & 1) * 8);
    };
    const unsigned aA = rd_addr(wn), aB = rd_addr(wk);

    auto step = [&](int c, auto stage_c) {
        constexpr int ST = decltype(stage_c)::value;
        if (c + 1 >= nchunk) dm_wait_vm<0>();                     // chunk c landed (this wave's pieces)
        else if (c + 2 >= nchunk) dm_wait_vm<4>();
        else dm_wait_vm<8>();
        __builtin_amdgcn_s_barrier();                             // ... everyone's; the stage of chunk c-1 is free
        __builtin_amdgcn_sched_barrier(0);
        if (c + DM_NSTAGE - 1 < nchunk) issue(c + DM_NSTAGE - 1, (ST + DM_NSTAGE - 1) % DM_NSTAGE);
        const int valid = m_end - (m_begin + c * DM_ROWS);
        if (valid < DM_ROWS) {                                    // ragged last chunk: rows past m_end count as 0
            for (int i = threadIdx.x; i < 2 * DM_ROWS * 16; i += 256) {
                const int row = (i >> 4) & (DM_ROWS - 1);
                if (row >= valid) *reinterpret_cast<u32x4*>(smem + ST * DM_STAGE + (i >> 9) * DM_TILE + row * 256 + (i & 15) * 16) = u32x4{0, 0, 0, 0};
            }
            __syncthreads();
        }
        dm_chunk<ST * DM_STAGE, BIAS>(acc, bacc, aA, aB);
    };
    for (int c = 0; c < nchunk; c += DM_NSTAGE) {
        step(c, std::integral_constant<int, 0>{});
        if (c + 1 < nchunk) step(c + 1, std::integral_constant<int, 1>{});
        if (c + 2 < nchunk) step(c + 2, std::integral_constant<int, 2>{});
        if (c + 3 < nchunk) step(c + 3, std::integral_constant<int, 3>{});
    }
    store_partial<false>(pp, acc, tn, tk, wn, wk, l31, hi, Nout, K);
    if (BIAS && wk == 0 && l31 == 0) {          // every column of the ones-product holds the row sums
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) bp[tn * 128 + wn * 64 + i * 32 + crow(r, hi)] = bacc[i][r];
    }
}

__global__ __launch_bounds__(256, 2) void linear_dw_dma_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                               const bf16_t* __restrict__ x2, int K1,
                                                               float* __restrict__ part, float* __restrict__ bpart,
                                                               int M, int Nout, int K, int rows_per_slice) {
    const DwTile t = dw_tile<false>(Nout, K, rows_per_slice, M);
    if (t.m_begin >= M) return;
    float* pp = part + (int64_t)t.slice * Nout * K;
    float* bp = bpart + (int64_t)t.slice * Nout;
    const bf16_t* xs = x + (int64_t)t.tk * 128;
    int ldx = K;
    if (x2 != nullptr) {                         // x = [x1 (K1 columns) | x2 (K - K1 columns)], K1 % 128 == 0
        if (t.tk * 128 < K1) { ldx = K1; }
        else { xs = x2 + (int64_t)(t.tk * 128 - K1); ldx = K - K1; }
    }
    if (t.tk == 0) dm_body<true>(dy, xs, ldx, pp, bp, M, Nout, K, t.m_begin, t.m_end, t.tn, t.tk);
    else dm_body<false>(dy, xs, ldx, pp, bp, M, Nout, K, t.m_begin, t.m_end, t.tn, t.tk);
}

// ---------------------------------------------------------------------------------------------
// Sum of the per-slice partials.  A workgroup covers 64 float4 columns with FOUR slice groups (one per wave,
// slices k = g mod 4) that meet in LDS: a 256x256 output with 64 slices is 256 workgroups of 16-deep
// chains instead of 64 workgroups of 64-deep ones (the kernel is latency-, not bandwidth-bound).
// Blocks past the weight columns reduce the bias partials the same way.  Deterministic (no atomics).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linear_dw_reduce(const float* __restrict__ part, const float* __restrict__ bpart,
                                                        float* __restrict__ dw, float* __restrict__ db, int nslice,
                                                        int64_t nw, int Nout, int nwb) {
    __shared__ f32x4 red[3][64];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const bool is_bias = (int)blockIdx.x >= nwb;
    const int64_t ncol4 = is_bias ? Nout / 4 : nw / 4;
    const int64_t j = (int64_t)(is_bias ? blockIdx.x - nwb : blockIdx.x) * 64 + c;
    const float* src = is_bias ? bpart : part;
    const int64_t stride = is_bias ? Nout : nw;
    f32x4 a0 = {0, 0, 0, 0}, a1 = a0;
    if (j < ncol4) {
        int k = g;
        // eight slices in flight per thread (a loop of load pairs waits for every pair: nslice / 8 dependent round trips in a
        // kernel that is nothing but latency); same two chains, same order
        for (; k + 28 < nslice; k += 32) {
            f32x4 x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = *reinterpret_cast<const f32x4*>(src + (int64_t)(k + 4 * u) * stride + 4 * j);
#pragma unroll
            for (int u = 0; u < 8; u += 2) { a0 += x[u]; a1 += x[u + 1]; }
        }
        for (; k + 4 < nslice; k += 8) {
            a0 += *reinterpret_cast<const f32x4*>(src + (int64_t)k * stride + 4 * j);
            a1 += *reinterpret_cast<const f32x4*>(src + (int64_t)(k + 4) * stride + 4 * j);
        }
        if (k < nslice) a0 += *reinterpret_cast<const f32x4*>(src + (int64_t)k * stride + 4 * j);
    }
    a0 += a1;
    if (g > 0) red[g - 1][c] = a0;
    __syncthreads();
    if (g == 0 && j < ncol4) {
        a0 = (a0 + red[0][c]) + (red[1][c] + red[2][c]);
        *reinterpret_cast<f32x4*>((is_bias ? db : dw) + 4 * j) = a0;
    }
}

// ---------------------------------------------------------------------------------------------
// Host: slice plan, tier selection, the one launch sequence.
// ---------------------------------------------------------------------------------------------
struct DwPlan { int ntile, nslice, rows; };
DwPlan plan(int M, int Nout, int K) {
    DwPlan p;
    p.ntile = ((Nout + 127) / 128) * ((K + 127) / 128);
    // One full round of two workgroups per CU (512 slots): slices = floor(512 / tiles), so no workgroup is
    // left for a second, nearly empty round (12 tiles x 43 slices = 516 workgroups ran 27 % slower).
    // Measured on MI355X at M = 131072 with the 4-group reduce.  (-DGF_DW_WG=... in probe builds.)
    const int total_wg = GF_DW_WG;
    // slices are dealt to the 8 XCDs round-robin: keep (slices per XCD) x tiles within that XCD's 64 slots
    int per_xcd = (total_wg / 8) / p.ntile;
    if (per_xcd < 1) per_xcd = 1;
    int want = 8 * per_xcd;
    int rows = (M + want - 1) / want;
    rows = ((rows + 63) / 64) * 64;
    if (rows < 256) rows = 256;
    p.rows = rows;
    p.nslice = (M + rows - 1) / rows;
    return p;
}

enum DwTier { DW_F32, DW_TR, DW_DMA };

// The tier (>= 0) that serves a call, or the GF_ERR_* (< 0) that rejects it.
int select_kernel(int dtype, int Nout, int K, bool two_source) {
    const bool dma = dtype == GF_BF16 && Nout % 128 == 0 && K % 128 == 0;
    if (two_source) return dma ? DW_DMA : GF_ERR_UNSUPPORTED;     // only the DMA tier picks its X source per k-tile
    const int align = gf_vec_elems(dtype);                        // 16-byte rows
    if (Nout % align || K % align) return GF_ERR_ALIGN;
    if (dtype == GF_F32) return DW_F32;
    if (dtype != GF_BF16) return GF_ERR_DTYPE;
    return dma ? DW_DMA : DW_TR;
}

// Every tier asks for 64 KiB of dynamic LDS or more (64, 80 and 136 KiB).  The limit without this call is not 48 KiB:
// gf_ln_gelu_bwd at bf16 C = 2048 launches with exactly 65536 bytes and no attribute (tests/test_gpu_elementwise.py,
// test_ln_gelu[bfloat16-2048]).  Nothing above 64 KiB has been launched without the opt-in, so all three keep it
// (gf_allow_lds in launch()).

// plan -> carve the workspace -> tile kernel of `tier` -> slice reduction.  x2 / K1: the second source (DMA tier) or null / 0.
int launch(DwTier tier, const void* dy, const void* x, const void* x2, int K1, float* dw, float* db, void* ws,
           int M, int Nout, int K, hipStream_t st) {
    const DwPlan p = plan(M, Nout, K);
    const int64_t nw = (int64_t)Nout * K;
    float* part = reinterpret_cast<float*>(ws);                   // [nslice][Nout][K]
    float* bpart = part + p.nslice * nw;                          // [nslice][Nout]
    const dim3 grid(p.ntile * ((p.nslice + 7) / 8) * 8);          // slices padded to the 8 XCDs dw_tile() deals them to
    const bf16_t *dyh = reinterpret_cast<const bf16_t*>(dy), *xh = reinterpret_cast<const bf16_t*>(x);
    switch (tier) {
    case DW_F32:
        if (int e = gf_allow_lds(linear_dw_f32_kernel, F32_LDS)) return e;
        linear_dw_f32_kernel<<<grid, 256, F32_LDS, st>>>(reinterpret_cast<const float*>(dy), reinterpret_cast<const float*>(x),
                                                         part, bpart, M, Nout, K, p.rows);
        break;
    case DW_TR:
        if (int e = gf_allow_lds(linear_dw_tr_kernel, TR_LDS)) return e;
        linear_dw_tr_kernel<<<grid, 256, TR_LDS, st>>>(dyh, xh, part, bpart, M, Nout, K, p.rows);
        break;
    case DW_DMA:
        if (int e = gf_allow_lds(linear_dw_dma_kernel, DM_LDS)) return e;
        linear_dw_dma_kernel<<<grid, 256, DM_LDS, st>>>(dyh, xh, reinterpret_cast<const bf16_t*>(x2), K1, part, bpart, M, Nout, K,
                                                        p.rows);
        break;
    }
    if (int rc = gf_launched()) return rc;
    const int nwb = (int)((nw / 4 + 63) / 64), nbb = db ? (Nout / 4 + 63) / 64 : 0;   // 64 float4 columns per block
    linear_dw_reduce<<<dim3(nwb + nbb), 256, 0, st>>>(part, bpart, dw, db, p.nslice, nw, Nout, nwb);
    return gf_launched();
}

}  // namespace

extern "C" int64_t gf_linear_dw_ws_bytes(int M, int Nout, int K) {
    if (M <= 0 || Nout <= 0 || K <= 0) return GF_ERR_SHAPE;
    DwPlan p = plan(M, Nout, K);
    return ((int64_t)p.nslice * Nout * K + (int64_t)p.nslice * Nout) * 4 + 256;
}

extern "C" int gf_linear_dw2(const void* dy, const void* x1, const void* x2, int K1, float* dw, float* db, void* ws,
                             int M, int Nout, int K, int dtype, void* stream) {
    if (M <= 0 || Nout <= 0 || K <= 0 || K1 <= 0 || K1 >= K) return GF_ERR_SHAPE;
    if (K1 % 128 || x1 == nullptr || x2 == nullptr) return GF_ERR_UNSUPPORTED;      // a k-tile reads ONE source
    const int tier = select_kernel(dtype, Nout, K, true);
    if (tier < 0) return tier;
    return launch((DwTier)tier, dy, x1, x2, K1, dw, db, ws, M, Nout, K, gf_stream(stream));
}

extern "C" int gf_linear_dw(const void* dy, const void* x, float* dw, float* db, void* ws,
                            int M, int Nout, int K, int dtype, void* stream) {
    if (M <= 0 || Nout <= 0 || K <= 0) return GF_ERR_SHAPE;
    const int tier = select_kernel(dtype, Nout, K, false);
    if (tier < 0) return tier;
    return launch((DwTier)tier, dy, x, nullptr, 0, dw, db, ws, M, Nout, K, gf_stream(stream));
}
