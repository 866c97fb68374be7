// Sinkhorn, streaming tier (N + 1 <= 2304): rows live in REGISTERS, one read of Z per iteration, no LDS staging.  The maths is
// stated at the top of sinkhorn_common.h.
//
// The generic kernels (sinkhorn_generic.hip) spend their time moving every element global -> VGPR -> LDS (ds_write is the
// slowest LDS instruction) -> VGPR four times.  Here a wave owns SKF_RPW whole rows, one after the other: a
// row is NS float4 per lane (columns 4*(lane + 64 k) .. +3), loaded once with 16-byte coalesced loads from a
// padded, log2e-prescaled copy Zp [Bc, R, Cp] (Cp = C rounded up to 4, pad = -inf; the copy is made once per
// call, 1/T of the iteration traffic).  The next rows' loads are in flight while the current row is processed.
//
// One exponential per element and iteration: with ref_i = the previous u_i (log2 units, + SKF_SHIFT)
//     e_ij   = exp2(Zp_ij + v_j + ref_i)                 (<= nu_j 2^SHIFT: column-normalised by the last v)
//     rs_i   = sum_j e_ij          ->  u_i' = lmu_i - log2(rs_i) + ref_i           (the exact row update)
//     S_j   += e_ij * f_i,  f_i = 2^SHIFT mu_i / rs_i   (= exp2(Zp_ij + v_j + u_i' + SHIFT), <= mu_i 2^SHIFT)
//     v_j'   = v_j + lnu_j - log2(S_j) + SHIFT                                      (the exact column update)
// i.e. the row pass and the column pass share the exponential; no running maxima are needed because after a
// column (row) update every term is bounded by the column (row) marginal.  Only the very first row update
// (u = v = 0, nothing normalised yet) uses ref_i = -max_j Z_ij.  SKF_SHIFT = 64 moves the representable
// floor to a marginal of 2^-190; below that the sum is clamped (never NaN).
// Column sums are kept per lane in registers over the wave's rows, combined over the 4 waves of a workgroup
// through LDS once, and written as ONE partial row per 32 matrix rows (3 % of the Z traffic); a small second
// kernel finishes v.  The backward sweep has the same shape (see skf_bwd_iter).
#include "sinkhorn_common.h"

using namespace gfsk;

namespace {

#ifndef SKF_PF_V
#define SKF_PF_V 2
#endif
constexpr int SKF_PF = SKF_PF_V;               // rows in flight ahead of the one being processed
constexpr int SKF_NB = SKF_PF + 1;             // register row buffers (ring, statically indexed)

// Zp[b][i][4q..4q+3] = Z[b][i][..] * log2e, -inf past C.  One thread per float4 of Zp.
__global__ __launch_bounds__(256) void skf_prescale(const float* __restrict__ Z, float* __restrict__ Zp, Geo g, int rows_total) {
    const int nvec = g.Cp >> 2;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)rows_total * nvec) return;
    const size_t row = idx / nvec;
    const int q = (int)(idx - row * nvec);
    const float* src = Z + row * g.C + 4 * q;
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (4 * q + c < g.C) ? src[c] * GF_LOG2E : -INFINITY;
    *reinterpret_cast<f32x4*>(Zp + row * g.Cp + 4 * q) = o;
}

template <int NS>
__device__ __forceinline__ void skf_load_row(f32x4 (&z)[NS], const float* __restrict__ zrow, int lane, int nvec) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int q = lane + 64 * k;
        z[k] = q < nvec ? *reinterpret_cast<const f32x4*>(zrow + 4 * q) : splat4(-INFINITY);
    }
}

// workgroup-level sum of the per-wave column accumulators -> one partial row
template <int NS>
__device__ __forceinline__ void skf_store_partial(const f32x4 (&S)[NS], f32x4* red, float* __restrict__ prow, int lane,
                                                  int wave, int nvec) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int q = lane + 64 * k;
        if (q < nvec) red[wave * (NS * 64) + q] = S[k];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nvec; q += 256) {
        const f32x4 a = red[q], b = red[NS * 64 + q], c = red[2 * NS * 64 + q], d = red[3 * NS * 64 + q];
        *reinterpret_cast<f32x4*>(prow + 4 * q) = (a + b) + (c + d);
    }
}

// grid (nblk, Bc).  v2 [Bc, Cp] (log2 units), u2 [Bc, R] read (previous) and written (new) in place.
template <int NS, bool FIRST>
__global__ __launch_bounds__(256, 2) void skf_fwd_iter(const float* __restrict__ Zp, const float* __restrict__ v2,
                                                       float* __restrict__ u2, float* __restrict__ u_hist,
                                                       float* __restrict__ part, Geo g) {
    __shared__ f32x4 red[4 * NS * 64];
    const int blk = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nvec = g.Cp >> 2;
    const int row0 = blk * SKF_RPB + wave * SKF_RPW;
    const int nrows = min(SKF_RPW, g.R - row0);
    f32x4 vv[NS], S[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int q = lane + 64 * k;
        vv[k] = (!FIRST && q < nvec) ? *reinterpret_cast<const f32x4*>(v2 + (size_t)b * g.Cp + 4 * q) : splat4(0.f);
        S[k] = splat4(0.f);
    }
    if (nrows > 0) {
        const float* zrow = Zp + ((size_t)b * g.R + row0) * g.Cp;
        f32x4 zb[SKF_NB][NS];
#pragma unroll
        for (int p = 0; p < SKF_PF; ++p)
            if (p < nrows) skf_load_row<NS>(zb[p], zrow + (size_t)p * g.Cp, lane, nvec);
        for (int r0 = 0; r0 < nrows; r0 += SKF_NB) {
#pragma unroll
            for (int s_ = 0; s_ < SKF_NB; ++s_) {
                const int r = r0 + s_;
                if (r + SKF_PF < nrows)
                    skf_load_row<NS>(zb[(s_ + SKF_PF) % SKF_NB], zrow + (size_t)(r + SKF_PF) * g.Cp, lane, nvec);
                if (r >= nrows) continue;
                f32x4 (&e)[NS] = zb[s_];
                const int gi = row0 + r;
                float ref;
                if (FIRST) {
                    float mx = -INFINITY;
#pragma unroll
                    for (int k = 0; k < NS; ++k)
#pragma unroll
                        for (int c = 0; c < 4; ++c) mx = fmaxf(mx, e[k][c]);
                    ref = -wave_allmax(mx);
                } else {
                    ref = u2[(size_t)b * g.R + gi] + SKF_SHIFT;
                }
                float rs = 0.f;
#pragma unroll
                for (int k = 0; k < NS; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float x = fast_exp2(e[k][c] + vv[k][c] + ref);
                        e[k][c] = x;
                        rs += x;
                    }
                rs = fmaxf(wave_allsum(rs), 1.17549435e-38f);
                const float lmu2 = lmu(g, gi) * GF_LOG2E, l2 = fast_log2(rs);
                const float un = lmu2 - l2 + ref;
                const float f = fast_exp2(lmu2 - l2 + SKF_SHIFT);
#pragma unroll
                for (int k = 0; k < NS; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) S[k][c] = fmaf(e[k][c], f, S[k][c]);
                if (lane == 0) {
                    u2[(size_t)b * g.R + gi] = un;
                    u_hist[(size_t)b * g.R + gi] = un * GF_LN2;
                }
            }
        }
    }
    skf_store_partial<NS>(S, red, part + ((size_t)b * g.nblk + blk) * g.Cp, lane, wave, nvec);
}

// sum of the nblk partial rows of 64 columns: 4 groups of threads take every 4th partial row, LDS combines them
__device__ __forceinline__ float skf_colsum(const float* __restrict__ part, int b, int j, int cx, int grp, float (*ss)[64],
                                            const Geo& g) {
    const float* p = part + (size_t)b * g.nblk * g.Cp + j;
    float s0 = 0.f, s1 = 0.f;
    int k = grp;
    for (; k + 4 < g.nblk; k += 8) { s0 += p[(size_t)k * g.Cp]; s1 += p[(size_t)(k + 4) * g.Cp]; }
    if (k < g.nblk) s0 += p[(size_t)k * g.Cp];
    ss[grp][cx] = s0 + s1;
    __syncthreads();
    return (ss[0][cx] + ss[1][cx]) + (ss[2][cx] + ss[3][cx]);
}

// grid (Cp/64 rounded up, Bc), 256 threads: v2' = v2 + lnu - log2(sum of partials) + SHIFT
__global__ __launch_bounds__(256) void skf_cols_fwd(const float* __restrict__ part, float* __restrict__ v2,
                                                    float* __restrict__ v_hist, int first, Geo g) {
    __shared__ float ss[4][64];
    const int cx = threadIdx.x & 63, grp = threadIdx.x >> 6, b = blockIdx.y;
    const int j = blockIdx.x * 64 + cx, jc = min(j, g.Cp - 1);
    const float tot = skf_colsum(part, b, jc, cx, grp, ss, g);
    if (grp != 0 || j >= g.Cp) return;
    float vn = 0.f;                                   // pad columns: any finite value (Zp is -inf there)
    if (j < g.C) {
        const float S = fmaxf(tot, 1.17549435e-38f);
        vn = (first ? 0.f : v2[(size_t)b * g.Cp + j]) + lnu(g, j) * GF_LOG2E - fast_log2(S) + SKF_SHIFT;
        v_hist[(size_t)b * g.C + j] = vn * GF_LN2;
    }
    v2[(size_t)b * g.Cp + j] = vn;
}

// ---- backward iteration k: e_ij = exp(Z_ij + u^k_i + v^k_j - lnu_j) (<= 1, columns sum to 1) serves both sums:
//   ubar^k_i     = base_i - sum_j e_ij vbar^k_j
//   vbar^{k-1}_j = -c_j sum_i e_ij w_i,   w_i = ubar^k_i exp(-lmu_i),  c_j = exp(v^{k-1}_j - v^k_j + lnu_j)
// (exp(Z_ij + u^k_i - lmu_i + v^{k-1}_j) = e_ij exp(-lmu_i) c_j); c_j is applied by skf_cols_bwd.
template <int NS>
__global__ __launch_bounds__(256, 2) void skf_bwd_iter(const float* __restrict__ Zp, const float* __restrict__ uk,
                                                       const float* __restrict__ a2p, const float* __restrict__ vbp,
                                                       const float* __restrict__ base, float* __restrict__ ubar_out,
                                                       float* __restrict__ part, Geo g) {
    // a2p [Bc, Cp] = (v^k - lnu) log2e, vbp [Bc, Cp] = vbar^k, both zero in the pad columns (written by
    // skf_cols_bwd / skf_bwd_prep)
    __shared__ f32x4 red[4 * NS * 64];
    const int blk = blockIdx.x, b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nvec = g.Cp >> 2;
    const int row0 = blk * SKF_RPB + wave * SKF_RPW;
    const int nrows = min(SKF_RPW, g.R - row0);
    f32x4 a2[NS], vb[NS], S[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int q = lane + 64 * k;
        a2[k] = q < nvec ? *reinterpret_cast<const f32x4*>(a2p + (size_t)b * g.Cp + 4 * q) : splat4(0.f);
        vb[k] = q < nvec ? *reinterpret_cast<const f32x4*>(vbp + (size_t)b * g.Cp + 4 * q) : splat4(0.f);
        S[k] = splat4(0.f);
    }
    if (nrows > 0) {
        const float* zrow = Zp + ((size_t)b * g.R + row0) * g.Cp;
        f32x4 zb[SKF_NB][NS];
#pragma unroll
        for (int p = 0; p < SKF_PF; ++p)
            if (p < nrows) skf_load_row<NS>(zb[p], zrow + (size_t)p * g.Cp, lane, nvec);
        for (int r0 = 0; r0 < nrows; r0 += SKF_NB) {
#pragma unroll
            for (int s_ = 0; s_ < SKF_NB; ++s_) {
                const int r = r0 + s_;
                if (r + SKF_PF < nrows)
                    skf_load_row<NS>(zb[(s_ + SKF_PF) % SKF_NB], zrow + (size_t)(r + SKF_PF) * g.Cp, lane, nvec);
                if (r >= nrows) continue;
                f32x4 (&e)[NS] = zb[s_];
                const int gi = row0 + r;
                const float u2 = uk[(size_t)b * g.R + gi] * GF_LOG2E;
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < NS; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float x = fast_exp2(e[k][c] + a2[k][c] + u2);
                        e[k][c] = x;
                        acc = fmaf(x, vb[k][c], acc);
                    }
                acc = wave_allsum(acc);
                const float ub = (base ? base[(size_t)b * g.R + gi] : 0.f) - acc;
                const float w = ub * fast_exp2(-lmu(g, gi) * GF_LOG2E);
#pragma unroll
                for (int k = 0; k < NS; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) S[k][c] = fmaf(e[k][c], w, S[k][c]);
                if (lane == 0) ubar_out[(size_t)b * g.R + gi] = ub;
            }
        }
    }
    skf_store_partial<NS>(S, red, part + ((size_t)b * g.nblk + blk) * g.Cp, lane, wave, nvec);
}

// grid (Cp/64 rounded up, Bc): vbar^{k-1}_j = -exp(v^{k-1}_j - v^k_j + lnu_j) * sum of partials   (v^0 = 0);
// also the padded inputs of the NEXT reverse iteration (k-1): a2p = (v^{k-1} - lnu) log2e, vbp = vbar^{k-1}
__global__ __launch_bounds__(256) void skf_cols_bwd(const float* __restrict__ part, const float* __restrict__ vk,
                                                    const float* __restrict__ vprev, float* __restrict__ vbar_out,
                                                    float* __restrict__ a2p, float* __restrict__ vbp, Geo g) {
    __shared__ float ss[4][64];
    const int cx = threadIdx.x & 63, grp = threadIdx.x >> 6, b = blockIdx.y;
    const int j = blockIdx.x * 64 + cx, jc = min(j, g.Cp - 1);
    const float tot = skf_colsum(part, b, jc, cx, grp, ss, g);
    if (grp != 0 || j >= g.Cp) return;
    float vbn = 0.f, a2n = 0.f;
    if (j < g.C) {
        const float vp = vprev ? vprev[(size_t)b * g.C + j] : 0.f;
        vbn = -__expf(vp - vk[(size_t)b * g.C + j] + lnu(g, j)) * tot;
        a2n = (vp - lnu(g, j)) * GF_LOG2E;
        vbar_out[(size_t)b * g.C + j] = vbn;
    }
    a2p[(size_t)b * g.Cp + j] = a2n;
    vbp[(size_t)b * g.Cp + j] = vbn;
}

// first reverse iteration (k = T): a2p from v^T, vbp = colsum(G)
__global__ __launch_bounds__(256) void skf_bwd_prep(const float* __restrict__ vT, const float* __restrict__ gsum_col,
                                                    float* __restrict__ a2p, float* __restrict__ vbp, Geo g) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= g.Cp) return;
    const bool ok = j < g.C;
    a2p[(size_t)b * g.Cp + j] = ok ? (vT[(size_t)b * g.C + j] - lnu(g, j)) * GF_LOG2E : 0.f;
    vbp[(size_t)b * g.Cp + j] = ok ? gsum_col[(size_t)b * g.C + j] : 0.f;
}

// ---- final gradient: dZ = G - sum_k [ e1^k vbar^k_j + e2^k ubar^k_i ] as ONE rank-2T product on the matrix cores.
// With the last iterates as reference, E_ij = exp(Z_ij + u^T_i + v^T_j - lnu_j) (<= 1: its columns sum to 1),
//   e1^k_ij vbar^k_j = E_ij * exp(u^k_i - u^T_i)                   * [exp(v^k_j - v^T_j) vbar^k_j]
//   e2^k_ij ubar^k_i = E_ij * [exp(u^k_i - u^T_i - lmu_i) ubar^k_i] * exp(v^{k-1}_j - v^T_j + lnu_j)
// so dZ = G - E o (P Q^T) with P [R, 2T], Q [C, 2T].  The product runs on
// v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains); the differences of iterates are small (Sinkhorn contracts), the
// exponents are clamped to +-80 so that nothing can overflow.  2T is padded to a multiple of 16 with zeros.
// P/Q layout: [pairs, R or C, KP] row-major, k contiguous.
__device__ __forceinline__ float exp_clamped(float x) { return __expf(fminf(fmaxf(x, -80.f), 80.f)); }

// grid (ceil(max(R,C)/256), T, Bc): thread = one row (or column) of one iteration's two factor columns
__global__ __launch_bounds__(256) void skf_factors(const float* __restrict__ u_hist, const float* __restrict__ v_hist,
                                                   const float* __restrict__ ubar_hist, const float* __restrict__ vbar_hist,
                                                   float* __restrict__ P, float* __restrict__ Q, int T, int KP,
                                                   size_t ustride, size_t vstride, Geo g) {
    const int x = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y + 1, b = blockIdx.z;
    if (x < g.R) {
        const float uk = u_hist[(size_t)(k - 1) * ustride + (size_t)b * g.R + x];
        const float uT = u_hist[(size_t)(T - 1) * ustride + (size_t)b * g.R + x];
        const float ub = ubar_hist[(size_t)(k - 1) * ustride + (size_t)b * g.R + x];
        float* p = P + ((size_t)b * g.R + x) * KP + 2 * (k - 1);
        p[0] = exp_clamped(uk - uT);
        p[1] = exp_clamped(uk - uT - lmu(g, x)) * ub;
    }
    if (x < g.C) {
        const float vk = v_hist[(size_t)(k - 1) * vstride + (size_t)b * g.C + x];
        const float vT = v_hist[(size_t)(T - 1) * vstride + (size_t)b * g.C + x];
        const float vp = k >= 2 ? v_hist[(size_t)(k - 2) * vstride + (size_t)b * g.C + x] : 0.f;
        const float vb = vbar_hist[(size_t)k * vstride + (size_t)b * g.C + x];
        float* q = Q + ((size_t)b * g.C + x) * KP + 2 * (k - 1);
        q[0] = exp_clamped(vk - vT) * vb;
        q[1] = exp_clamped(vp - vT + lnu(g, x));
    }
    if (k == T) {                                   // zero the k padding once
        for (int c = 2 * T; c < KP; ++c) {
            if (x < g.R) P[((size_t)b * g.R + x) * KP + c] = 0.f;
            if (x < g.C) Q[((size_t)b * g.C + x) * KP + c] = 0.f;
        }
    }
}

// grid (ceil(C/128) * ceil(R/128), Bc), 256 threads: one wave = a 64 x 64 block (2 x 2 MFMA tiles) of the workgroup's 128 x 128,
// the factor fragments of the next k-step in flight under the current one's MFMAs.  (Round 6: was one 32 x 32 tile per wave with
// the loads in front of their MFMAs -- ablations of that form: 0.97 of its 1.46 ms per step were the product, against 0.34 ms at
// the exact-fp32 MFMA rate; prefetching took 0.15 ms off the call, sharing every fragment between two tiles another 0.12:
// 7.96 -> 7.71 ms backward at B = 32, T = 100, bit-identical -- the summation order over k is unchanged.)
__global__ __launch_bounds__(256) void skf_final_bwd(const float* __restrict__ Z, const float* __restrict__ G,
                                                     const float* __restrict__ P, const float* __restrict__ Q,
                                                     const float* __restrict__ uT, const float* __restrict__ vT,
                                                     float* __restrict__ gZ, int KP, Geo g) {
    const int ncb = (g.C + 127) / 128;
    const int b = blockIdx.y, rb = blockIdx.x / ncb, cb = blockIdx.x % ncb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int i0 = rb * 128 + (wave >> 1) * 64, j0 = cb * 128 + (wave & 1) * 64;
    if (i0 >= g.R || j0 >= g.C) return;
    const float* prow[2];
    const float* qrow[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        prow[t] = P + ((size_t)b * g.R + min(i0 + 32 * t + l31, g.R - 1)) * KP + 8 * hi;
        qrow[t] = Q + ((size_t)b * g.C + min(j0 + 32 * t + l31, g.C - 1)) * KP + 8 * hi;
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.f;
    Frag<float> p0 = ld_frag8(prow[0]), p1 = ld_frag8(prow[1]), q0 = ld_frag8(qrow[0]), q1 = ld_frag8(qrow[1]);
    for (int s_ = 0; s_ < KP; s_ += 16) {
        const int sn = min(s_ + 16, KP - 16);                       // (the last step re-fetches itself: no branch)
        const Frag<float> p0n = ld_frag8(prow[0] + sn), p1n = ld_frag8(prow[1] + sn);
        const Frag<float> q0n = ld_frag8(qrow[0] + sn), q1n = ld_frag8(qrow[1] + sn);
        mma32(acc[0][0], p0, q0);
        mma32(acc[0][1], p0, q1);
        mma32(acc[1][0], p1, q0);
        mma32(acc[1][1], p1, q1);
        p0 = p0n; p1 = p1n; q0 = q0n; q1 = q1n;
    }
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int j = j0 + 32 * tj + l31;
        if (j >= g.C) continue;
        const float cj = vT[(size_t)b * g.C + j] - lnu(g, j);
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + 32 * ti + crow(r, hi);
                if (i < g.R) {
                    const size_t idx = ((size_t)b * g.R + i) * g.C + j;
                    const float E = __expf(Z[idx] + uT[(size_t)b * g.R + i] + cj);
                    gZ[idx] = G[idx] - E * acc[ti][tj][r];
                }
            }
    }
}

// T iterations of one chunk; NS = float4 per lane and row.  All pointers are offset to the chunk's first pair; history strides
// are g.B * R (or C).
template <int NS> int skf_fwd_iters(const float* Zp, float* v2, float* u2, float* u_hist, float* v_hist, float* part,
                                    const Geo& g, int bc, int iters, hipStream_t st) {
    for (int it = 0; it < iters; ++it) {
        float* uh = u_hist + (size_t)it * g.B * g.R;
        if (it == 0) skf_fwd_iter<NS, true><<<dim3(g.nblk, bc), 256, 0, st>>>(Zp, v2, u2, uh, part, g);
        else skf_fwd_iter<NS, false><<<dim3(g.nblk, bc), 256, 0, st>>>(Zp, v2, u2, uh, part, g);
        skf_cols_fwd<<<dim3((g.Cp + 63) / 64, bc), 256, 0, st>>>(part, v2, v_hist + (size_t)it * g.B * g.C, it == 0, g);
    }
    return gf_launched();
}
// a2p / vbp: as skf_bwd_prep left them for k = T
template <int NS> int skf_bwd_iters(const float* Zp, const float* u_hist, const float* v_hist, const float* gsum_row,
                                    float* ubar_hist, float* vbar_hist, float* part, float* a2p, float* vbp, const Geo& g,
                                    int bc, int iters, hipStream_t st) {
    for (int k = iters; k >= 1; --k) {
        const float* uk = u_hist + (size_t)(k - 1) * g.B * g.R;
        const float* vk = v_hist + (size_t)(k - 1) * g.B * g.C;
        const float* vp = k >= 2 ? v_hist + (size_t)(k - 2) * g.B * g.C : nullptr;
        skf_bwd_iter<NS><<<dim3(g.nblk, bc), 256, 0, st>>>(Zp, uk, a2p, vbp, k == iters ? gsum_row : nullptr,
                                                           ubar_hist + (size_t)(k - 1) * g.B * g.R, part, g);
        skf_cols_bwd<<<dim3((g.Cp + 63) / 64, bc), 256, 0, st>>>(part, vk, vp, vbar_hist + (size_t)(k - 1) * g.B * g.C,
                                                                 a2p, vbp, g);
    }
    return gf_launched();
}

// index of the NS instantiation that holds a row of g (make_geo: g.fast <=> at most SKF_MAX_NS * 64 float4 per row)
int ns_index(const Geo& g) { return min(((g.Cp >> 2) + 63) / 64, SKF_MAX_NS) - 1; }

}  // namespace

namespace gfsk {

void skf_prescale_launch(const float* Z, float* Zp, const Geo& g, int bc, hipStream_t st) {
    const size_t nv4 = (size_t)bc * g.R * (g.Cp >> 2);
    skf_prescale<<<dim3((unsigned)((nv4 + 255) / 256)), 256, 0, st>>>(Z, Zp, g, bc * g.R);
}

int skf_fwd_launch(const float* Zp, float* v2, float* u2, float* u_hist, float* v_hist, float* part, const Geo& g, int bc,
                   int iters, hipStream_t st) {
    static constexpr decltype(&skf_fwd_iters<1>) by_ns[SKF_MAX_NS] = {
        skf_fwd_iters<1>, skf_fwd_iters<2>, skf_fwd_iters<3>, skf_fwd_iters<4>, skf_fwd_iters<5>,
        skf_fwd_iters<6>, skf_fwd_iters<7>, skf_fwd_iters<8>, skf_fwd_iters<9>};
    return by_ns[ns_index(g)](Zp, v2, u2, u_hist, v_hist, part, g, bc, iters, st);
}

// first reverse iteration (k = T): a2p from vT = v^T, vbp = colsum(G)
void skf_bwd_prep_launch(const float* vT, const float* gsum_col, float* a2p, float* vbp, const Geo& g, int bc, hipStream_t st) {
    skf_bwd_prep<<<dim3((g.Cp + 255) / 256, bc), 256, 0, st>>>(vT, gsum_col, a2p, vbp, g);
}

int skf_bwd_launch(const float* Zp, const float* u_hist, const float* v_hist, const float* gsum_row, float* ubar_hist,
                   float* vbar_hist, float* part, float* a2p, float* vbp, const Geo& g, int bc, int iters, hipStream_t st) {
    static constexpr decltype(&skf_bwd_iters<1>) by_ns[SKF_MAX_NS] = {
        skf_bwd_iters<1>, skf_bwd_iters<2>, skf_bwd_iters<3>, skf_bwd_iters<4>, skf_bwd_iters<5>,
        skf_bwd_iters<6>, skf_bwd_iters<7>, skf_bwd_iters<8>, skf_bwd_iters<9>};
    return by_ns[ns_index(g)](Zp, u_hist, v_hist, gsum_row, ubar_hist, vbar_hist, part, a2p, vbp, g, bc, iters, st);
}

// dZ of one chunk from the finished histories: the rank-2T factors P, Q [bc, R or C, KP] (scratch), then the product
void skf_final_bwd_launch(const float* Z, const float* G, const float* u_hist, const float* v_hist, const float* ubar_hist,
                          const float* vbar_hist, float* P, float* Q, int KP, float* gZ, const Geo& g, int bc, int iters,
                          hipStream_t st) {
    const size_t us = (size_t)g.B * g.R, vs = (size_t)g.B * g.C;
    skf_factors<<<dim3((max(g.R, g.C) + 255) / 256, iters, bc), 256, 0, st>>>(u_hist, v_hist, ubar_hist, vbar_hist, P, Q, iters,
                                                                              KP, us, vs, g);
    skf_final_bwd<<<dim3(((g.C + 127) / 128) * ((g.R + 127) / 128), bc), 256, 0, st>>>(
        Z, G, P, Q, u_hist + (iters - 1) * us, v_hist + (iters - 1) * vs, gZ, KP, g);
}

}  // namespace gfsk
