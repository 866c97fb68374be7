// Register-staged attention kernels, forward and backward, as templates over the element type and head_dim: fp32 at every
// head_dim, bf16 at head_dim 32 / 128, and bf16 at head_dim 64 where K / V rows lie outside what the LDS-DMA kernels'
// buffer descriptors address (kvdma_ok, attn_common.h).  A capability path, not a tuned one (at head_dim 128 the fragments
// of a row exceed the register budget and spill).
//
// One workgroup = 4 waves; a wave owns 64 query rows (forward, dQ) or 32 keys (dK/dV); K/V (resp. Q/dO) stream through
// LDS in 64-row tiles, staged through registers.  The score tile is produced transposed (keys on the MFMA i axis, the
// owning row on j = lane&31), so the softmax statistics, the rescale of O and the lse/delta factors are all lane-local; P
// is fed back to the second MFMA straight from the accumulator registers with a matching key-order on the V^T fragments
// (no LDS round trip, no permutes).
#include "gf_common.h"
#include "gf_amd.h"
#include "attn_common.h"

#include <type_traits>

using namespace gfattn;

namespace {

// Position of tile row r inside a transposed LDS row: bits 2 and 3 of r are swapped so that the 8
// rows a lane needs for one k-step of the second MFMA — {16t + 4hi + e, 16t + 8 + 4hi + e}, e<4, the
// C-layout rows of accumulator registers 8t..8t+7 — are 8 CONSECUTIVE elements (one 16-byte read).
__device__ __forceinline__ int tpos(int r) { return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1); }
// Transposed tiles are additionally XOR-swizzled in 8-element (16-byte) blocks by the low bits of
// (row d >> 3): with the coalesced staging order (consecutive lanes = consecutive 16-byte chunks of one
// source row) the 8 lanes of a chunk group would otherwise hit one LDS bank; reads stay 16-byte.
__device__ __forceinline__ int tswz(int d, int pos) { return pos ^ (((d >> 3) & 7) << 3); }

template <typename T> struct Pair;
template <> struct Pair<bf16_t> { typedef bf16x2 type; };
template <> struct Pair<float> { typedef f32x2 type; };

// B-operand style fragments of one row held in registers: row[16 s + 8 hi + e], s = 0..HD/16-1
template <typename T, int HD>
__device__ __forceinline__ void load_row_frags(Frag<T> (&f)[HD / 16], const T* rowptr, int hi) {
#pragma unroll
    for (int s = 0; s < HD / 16; ++s) f[s] = ld_frag8(rowptr + 16 * s + 8 * hi);
}

// ===========================================================================================
// forward
// ===========================================================================================
// One wave owns 64 query rows (two 32-row blocks): every K / V^T fragment read from LDS feeds two
// MFMAs.  K/V tiles are double-buffered: the next tile's global loads are issued before the
// compute of the current one and land in LDS after it (one barrier per tile).  The running max is
// only raised (and O / l rescaled) when it grows by more than RESCALE_THR (0 in fp32 mode).
template <typename T> struct RescaleThr { static constexpr float value = 0.f; };
template <> struct RescaleThr<bf16_t> { static constexpr float value = 4.f; };   // P <= 2^4, log2 units

template <typename T, int HD> struct StageRegs {
    static constexpr int NKI = 64 * Lay<T, HD>::CPR, NVI = 32 * Lay<T, HD>::CPR;   // work items of a tile
    static constexpr int NK = (NKI + 255) / 256;            // row-major chunks per thread
    static constexpr int NV = (NVI + 255) / 256;            // row pairs x chunks per thread (bf16 at head_dim 32: half a round)
    u32x4 k[NK];
    u32x4 v0[NV], v1[NV];
};

template <typename T, int HD>
__device__ __forceinline__ void stage_load(StageRegs<T, HD>& rg, const T* kp, int64_t kld, const T* vp,
                                           int64_t vld, int row0, int nmax) {
    using L = Lay<T, HD>;
#pragma unroll
    for (int i = 0; i < StageRegs<T, HD>::NK; ++i) {
        int c = threadIdx.x + 256 * i;
        if (StageRegs<T, HD>::NKI % 256 && c >= StageRegs<T, HD>::NKI) continue;
        int r = c / L::CPR, cc = c % L::CPR;
        int gr = min(row0 + r, nmax - 1);
        rg.k[i] = *reinterpret_cast<const u32x4*>(kp + (int64_t)gr * kld + cc * L::VEC);
    }
#pragma unroll
    for (int i = 0; i < StageRegs<T, HD>::NV; ++i) {
        int it = threadIdx.x + 256 * i;
        if (StageRegs<T, HD>::NVI % 256 && it >= StageRegs<T, HD>::NVI) continue;
        int cc = it % L::CPR, p = it / L::CPR;
        int r0 = min(row0 + 2 * p, nmax - 1), r1 = min(row0 + 2 * p + 1, nmax - 1);
        rg.v0[i] = *reinterpret_cast<const u32x4*>(vp + (int64_t)r0 * vld + cc * L::VEC);
        rg.v1[i] = *reinterpret_cast<const u32x4*>(vp + (int64_t)r1 * vld + cc * L::VEC);
    }
}

template <typename T, int HD>
__device__ __forceinline__ void stage_store(const StageRegs<T, HD>& rg, T* Ks, T* Vt) {
    using L = Lay<T, HD>;
    typedef typename Pair<T>::type pair_t;
#pragma unroll
    for (int i = 0; i < StageRegs<T, HD>::NK; ++i) {
        int c = threadIdx.x + 256 * i;
        if (StageRegs<T, HD>::NKI % 256 && c >= StageRegs<T, HD>::NKI) continue;
        int r = c / L::CPR, cc = c % L::CPR;
        *reinterpret_cast<u32x4*>(Ks + r * L::LDR + cc * L::VEC) = rg.k[i];
    }
#pragma unroll
    for (int i = 0; i < StageRegs<T, HD>::NV; ++i) {
        int it = threadIdx.x + 256 * i;
        if (StageRegs<T, HD>::NVI % 256 && it >= StageRegs<T, HD>::NVI) continue;
        int cc = it % L::CPR, p = it / L::CPR;
        union { u32x4 u; T e[L::VEC]; } a, b;
        a.u = rg.v0[i];
        b.u = rg.v1[i];
#pragma unroll
        for (int e = 0; e < L::VEC; ++e) {
            pair_t pr = {a.e[e], b.e[e]};
            const int d = cc * L::VEC + e;
            *reinterpret_cast<pair_t*>(Vt + d * L::LDT + tswz(d, tpos(2 * p))) = pr;
        }
    }
}

template <typename T, int HD>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 2 : 1) void attn_fwd_kernel(AttnParams p) {
    using L = Lay<T, HD>;
    constexpr int BUF = L::ROWMAJOR + L::TRANSP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* lds = reinterpret_cast<T*>(smem);

    const int nqb = (p.Nq + 255) / 256;
    const int total = nqb * p.H * p.B;
    int lb = xcd_remap(blockIdx.x, total);
    const int qb = lb % nqb, h = (lb / nqb) % p.H, b = lb / (nqb * p.H);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int qrow0 = qb * 256 + wave * 64 + l31;

    const T* qp = reinterpret_cast<const T*>(p.q) + b * p.sqb + h * p.sqh;
    const T* kp = reinterpret_cast<const T*>(p.k) + b * p.skb + h * p.skh;
    const T* vp = reinterpret_cast<const T*>(p.v) + b * p.svb + h * p.svh;

    Frag<T> qf[2][HD / 16];
#pragma unroll
    for (int j = 0; j < 2; ++j)
        load_row_frags<T, HD>(qf[j], qp + (int64_t)min(qrow0 + 32 * j, p.Nq - 1) * p.sqn, hi);

    f32x16 o[2][HD / 32];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int db = 0; db < HD / 32; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[j][db][r] = 0.f;
    float m[2] = {GF_NEG_BIG, GF_NEG_BIG}, lsum[2] = {0.f, 0.f};
    const float c = p.scale * GF_LOG2E;

    StageRegs<T, HD> rg;
    stage_load<T, HD>(rg, kp, p.skn, vp, p.svn, 0, p.Nk);
    stage_store<T, HD>(rg, lds, lds + L::ROWMAJOR);
    __syncthreads();

    const int nt = (p.Nk + 63) / 64;
    for (int t = 0; t < nt; ++t) {
        const int kv0 = t * 64;
        const T* Ks = lds + (t & 1) * BUF;
        const T* Vt = Ks + L::ROWMAJOR;
        if (t + 1 < nt) stage_load<T, HD>(rg, kp, p.skn, vp, p.svn, kv0 + 64, p.Nk);

        f32x16 s[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[j][kb][r] = 0.f;
            const T* base = Ks + (kb * 32 + l31) * L::LDR + 8 * hi;
#pragma unroll
            for (int ks = 0; ks < HD / 16; ++ks) {
                Frag<T> kf = ld_frag8(base + 16 * ks);
                mma32(s[0][kb], kf, qf[0][ks]);
                mma32(s[1][kb], kf, qf[1][ks]);
            }
        }
        if (kv0 + 64 > p.Nk) {   // ragged last tile: keys past Nk never win the max and get P = 0
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (kv0 + kb * 32 + crow(r, hi) >= p.Nk) s[j][kb][r] = -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[j][kb][r]);
            mx = fmaxf(mx, xhalf(mx)) * c;
            if (__any(mx > m[j] + RescaleThr<T>::value)) {
                const float mnew = fmaxf(m[j], mx);
                const float alpha = fast_exp2(m[j] - mnew);
                m[j] = mnew;
                lsum[j] *= alpha;
#pragma unroll
                for (int db = 0; db < HD / 32; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[j][db][r] *= alpha;
            }
            float ps = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float e = fast_exp2(fmaf(s[j][kb][r], c, -m[j]));
                    s[j][kb][r] = e;
                    ps += e;
                }
            lsum[j] += ps;
        }
        // O^T[d][q] += V^T[d][key] P[key][q]; each V^T fragment feeds both query blocks
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                Frag<T> p0 = acc_to_frag<T>(s[0][kb], tt), p1 = acc_to_frag<T>(s[1][kb], tt);
#pragma unroll
                for (int db = 0; db < HD / 32; ++db) {
                    const int d = db * 32 + l31;
                    Frag<T> vf = ld_frag8(Vt + d * L::LDT + tswz(d, kb * 32 + 16 * tt + 8 * hi));
                    mma32(o[0][db], vf, p0);
                    mma32(o[1][db], vf, p1);
                }
            }
        if (t + 1 < nt) {
            T* nb = lds + ((t + 1) & 1) * BUF;
            stage_store<T, HD>(rg, nb, nb + L::ROWMAJOR);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int qrow = qrow0 + 32 * j;
        const float l = lsum[j] + xhalf(lsum[j]);
        if (qrow < p.Nq) {
            T* op = reinterpret_cast<T*>(p.o) + b * p.sob + h * p.soh + (int64_t)qrow * p.son;
            store_row<T, HD>(op, o[j], 1.f / l, hi);
            if (hi == 0) p.lse[((int64_t)b * p.H + h) * p.Nq + qrow] = (m[j] + fast_log2(l)) * GF_LN2;
        }
    }
}

// ===========================================================================================
// backward, part 1: dQ (and delta = rowsum(dO * O)); wave = 64 query rows, K/V tiles double-buffered
// ===========================================================================================
template <typename T, int HD> struct PairRegs {
    static constexpr int NI = 32 * Lay<T, HD>::CPR;         // (row pair, chunk) items of a tile
    static constexpr int N = (NI + 255) / 256;              // ... per thread
    u32x4 a[N], b[N];
};
template <typename T, int HD>
__device__ __forceinline__ void pair_load(PairRegs<T, HD>& rg, const T* g, int64_t ld, int row0, int nmax) {
    using L = Lay<T, HD>;
#pragma unroll
    for (int i = 0; i < PairRegs<T, HD>::N; ++i) {
        int it = threadIdx.x + 256 * i;
        if (PairRegs<T, HD>::NI % 256 && it >= PairRegs<T, HD>::NI) continue;
        int cc = it % L::CPR, p = it / L::CPR;
        int r0 = min(row0 + 2 * p, nmax - 1), r1 = min(row0 + 2 * p + 1, nmax - 1);
        rg.a[i] = *reinterpret_cast<const u32x4*>(g + (int64_t)r0 * ld + cc * L::VEC);
        rg.b[i] = *reinterpret_cast<const u32x4*>(g + (int64_t)r1 * ld + cc * L::VEC);
    }
}
template <typename T, int HD, bool ROWM, bool TRAN>
__device__ __forceinline__ void pair_store(const PairRegs<T, HD>& rg, T* ldsR, T* ldsT) {
    using L = Lay<T, HD>;
    typedef typename Pair<T>::type pair_t;
#pragma unroll
    for (int i = 0; i < PairRegs<T, HD>::N; ++i) {
        int it = threadIdx.x + 256 * i;
        if (PairRegs<T, HD>::NI % 256 && it >= PairRegs<T, HD>::NI) continue;
        int cc = it % L::CPR, p = it / L::CPR;
        if (ROWM) {
            *reinterpret_cast<u32x4*>(ldsR + (2 * p) * L::LDR + cc * L::VEC) = rg.a[i];
            *reinterpret_cast<u32x4*>(ldsR + (2 * p + 1) * L::LDR + cc * L::VEC) = rg.b[i];
        }
        if (TRAN) {
            union { u32x4 u; T e[L::VEC]; } x, y;
            x.u = rg.a[i];
            y.u = rg.b[i];
#pragma unroll
            for (int e = 0; e < L::VEC; ++e) {
                pair_t pr = {x.e[e], y.e[e]};
                const int d = cc * L::VEC + e;
                *reinterpret_cast<pair_t*>(ldsT + d * L::LDT + tswz(d, tpos(2 * p))) = pr;
            }
        }
    }
}

template <typename T, int HD>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 2 : 1) void attn_bwd_dq_kernel(AttnParams p) {
    using L = Lay<T, HD>;
    constexpr int BUF = 2 * L::ROWMAJOR + L::TRANSP;   // K row-major | V row-major | K^T
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* lds = reinterpret_cast<T*>(smem);

    const int nqb = (p.Nq + 255) / 256;
    const int total = nqb * p.H * p.B;
    int lb = xcd_remap(blockIdx.x, total);
    const int qb = lb % nqb, h = (lb / nqb) % p.H, b = lb / (nqb * p.H);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int qrow0 = qb * 256 + wave * 64 + l31;

    const T* qp = reinterpret_cast<const T*>(p.q) + b * p.sqb + h * p.sqh;
    const T* kp = reinterpret_cast<const T*>(p.k) + b * p.skb + h * p.skh;
    const T* vp = reinterpret_cast<const T*>(p.v) + b * p.svb + h * p.svh;
    const T* op = reinterpret_cast<const T*>(p.o) + b * p.sob + h * p.soh;
    const T* dop = reinterpret_cast<const T*>(p.dout) + b * p.sdob + h * p.sdoh;

    Frag<T> qf[2][HD / 16], dof[2][HD / 16];
    float delta[2], lse2[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int qld = min(qrow0 + 32 * j, p.Nq - 1);
        load_row_frags<T, HD>(qf[j], qp + (int64_t)qld * p.sqn, hi);
        load_row_frags<T, HD>(dof[j], dop + (int64_t)qld * p.sdon, hi);
        Frag<T> of[HD / 16];
        load_row_frags<T, HD>(of, op + (int64_t)qld * p.son, hi);
        float d = 0.f;
#pragma unroll
        for (int s = 0; s < HD / 16; ++s)
#pragma unroll
            for (int e = 0; e < 8; ++e) d += to_f32(of[s].v[e]) * to_f32(dof[j][s].v[e]);
        d += xhalf(d);
        delta[j] = d;
        const int64_t stat = ((int64_t)b * p.H + h) * p.Nq + qld;
        lse2[j] = p.lse[stat] * GF_LOG2E;
        if (qrow0 + 32 * j < p.Nq && hi == 0) {
            if (sizeof(T) == 2 && !(p.flags & ATTN_PLAIN_STATS)) {   // what attn_bwd_dkv_bf16_kernel starts its accumulators from (attention_bwd3.hip)
                p.delta[stat] = -lse2[j] / p.rr;
                p.delta[(int64_t)p.B * p.H * p.Nq + stat] = -d;
            } else {                             // the generic dK/dV kernel reads lse and delta as they are
                p.delta[stat] = d;
            }
        }
    }
    const float c = p.scale * GF_LOG2E;

    f32x16 dq[2][HD / 32];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int db = 0; db < HD / 32; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) dq[j][db][r] = 0.f;

    PairRegs<T, HD> kr, vr;
    pair_load<T, HD>(kr, kp, p.skn, 0, p.Nk);
    pair_load<T, HD>(vr, vp, p.svn, 0, p.Nk);
    pair_store<T, HD, true, true>(kr, lds, lds + 2 * L::ROWMAJOR);
    pair_store<T, HD, true, false>(vr, lds + L::ROWMAJOR, nullptr);
    __syncthreads();

    const int nt = (p.Nk + 63) / 64;
    for (int t = 0; t < nt; ++t) {
        const int kv0 = t * 64;
        const T* Ks = lds + (t & 1) * BUF;
        const T* Vs = Ks + L::ROWMAJOR;
        const T* Kt = Vs + L::ROWMAJOR;
        if (t + 1 < nt) {
            pair_load<T, HD>(kr, kp, p.skn, kv0 + 64, p.Nk);
            pair_load<T, HD>(vr, vp, p.svn, kv0 + 64, p.Nk);
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            f32x16 s[2], dp[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[j][r] = 0.f; dp[j][r] = 0.f; }
            const T* kbase = Ks + (kb * 32 + l31) * L::LDR + 8 * hi;
            const T* vbase = Vs + (kb * 32 + l31) * L::LDR + 8 * hi;
#pragma unroll
            for (int ks = 0; ks < HD / 16; ++ks) {
                Frag<T> kf = ld_frag8(kbase + 16 * ks);
                mma32(s[0], kf, qf[0][ks]);
                mma32(s[1], kf, qf[1][ks]);
                Frag<T> vf = ld_frag8(vbase + 16 * ks);
                mma32(dp[0], vf, dof[0][ks]);
                mma32(dp[1], vf, dof[1][ks]);
            }
            const bool ragged = kv0 + 64 > p.Nk;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float pr = fast_exp2(fmaf(s[j][r], c, -lse2[j]));
                    if (ragged && kv0 + kb * 32 + crow(r, hi) >= p.Nk) pr = 0.f;
                    s[j][r] = pr * (dp[j][r] - delta[j]);
                }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                Frag<T> d0 = acc_to_frag<T>(s[0], tt), d1 = acc_to_frag<T>(s[1], tt);
#pragma unroll
                for (int db = 0; db < HD / 32; ++db) {
                    const int d = db * 32 + l31;
                    Frag<T> kt = ld_frag8(Kt + d * L::LDT + tswz(d, kb * 32 + 16 * tt + 8 * hi));
                    mma32(dq[0][db], kt, d0);
                    mma32(dq[1][db], kt, d1);
                }
            }
        }
        if (t + 1 < nt) {
            T* nb = lds + ((t + 1) & 1) * BUF;
            pair_store<T, HD, true, true>(kr, nb, nb + 2 * L::ROWMAJOR);
            pair_store<T, HD, true, false>(vr, nb + L::ROWMAJOR, nullptr);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int qrow = qrow0 + 32 * j;
        if (qrow < p.Nq) {
            T* dqp = reinterpret_cast<T*>(p.dq) + b * p.sdqb + h * p.sdqh + (int64_t)qrow * p.sdqn;
            if (p.flags & GF_ATTN_ACC_DQ) add_row<HD>(dqp, dq[j], p.scale, hi); else store_row<T, HD>(dqp, dq[j], p.scale, hi);
        }
    }
}

// ===========================================================================================
// backward, part 2: dK, dV (one workgroup per 128 keys, Q / dO tiles double-buffered)
// ===========================================================================================
template <typename T, int HD>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 2 : 1) void attn_bwd_dkv_kernel(AttnParams p) {
    using L = Lay<T, HD>;
    constexpr int BUF = 2 * L::ROWMAJOR + 2 * L::TRANSP + 128 * (int)(sizeof(float) / sizeof(T));
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* lds = reinterpret_cast<T*>(smem);

    const int nkb = (p.Nk + 127) / 128;
    const int total = nkb * p.H * p.B;
    int lb = xcd_remap(blockIdx.x, total);
    const int kb_ = lb % nkb, h = (lb / nkb) % p.H, b = lb / (nkb * p.H);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const int krow = kb_ * 128 + wave * 32 + l31;
    const int kld = min(krow, p.Nk - 1);

    const T* qp = reinterpret_cast<const T*>(p.q) + b * p.sqb + h * p.sqh;
    const T* kp = reinterpret_cast<const T*>(p.k) + b * p.skb + h * p.skh;
    const T* vp = reinterpret_cast<const T*>(p.v) + b * p.svb + h * p.svh;
    const T* dop = reinterpret_cast<const T*>(p.dout) + b * p.sdob + h * p.sdoh;
    const float* lsep = p.lse + ((int64_t)b * p.H + h) * p.Nq;
    const float* delp = p.delta + ((int64_t)b * p.H + h) * p.Nq;

    Frag<T> kf[HD / 16], vf[HD / 16];
    load_row_frags<T, HD>(kf, kp + (int64_t)kld * p.skn, hi);
    load_row_frags<T, HD>(vf, vp + (int64_t)kld * p.svn, hi);
    const float c = p.scale * GF_LOG2E;

    f32x16 dk[HD / 32], dv[HD / 32];
#pragma unroll
    for (int db = 0; db < HD / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[db][r] = 0.f; dv[db][r] = 0.f; }

    auto stats_of = [&](T* buf) { return reinterpret_cast<float*>(buf + 2 * L::ROWMAJOR + 2 * L::TRANSP); };
    // raw prefetch only: consuming the values here (scale / select) would force the wave to wait for the
    // whole prefetch batch at the top of the iteration; they are finished in store_stats, after the MFMAs.
    auto load_stats = [&](int q0, float& l, float& d) {
        if (threadIdx.x < 64) {
            int qi = min(q0 + (int)threadIdx.x, p.Nq - 1);
            l = lsep[qi];
            d = delp[qi];
        }
    };
    auto store_stats = [&](T* buf, int q0, float l, float d) {
        if (threadIdx.x < 64) {
            float* st = stats_of(buf);
            const bool ok = q0 + (int)threadIdx.x < p.Nq;     // rows past Nq: lse = +inf makes P exactly 0
            st[threadIdx.x] = ok ? l * GF_LOG2E : INFINITY;
            st[64 + threadIdx.x] = ok ? d : 0.f;
        }
    };

    PairRegs<T, HD> qr, dor;
    float ls = 0.f, dl = 0.f;
    pair_load<T, HD>(qr, qp, p.sqn, 0, p.Nq);
    pair_load<T, HD>(dor, dop, p.sdon, 0, p.Nq);
    load_stats(0, ls, dl);
    pair_store<T, HD, true, true>(qr, lds, lds + 2 * L::ROWMAJOR);
    pair_store<T, HD, true, true>(dor, lds + L::ROWMAJOR, lds + 2 * L::ROWMAJOR + L::TRANSP);
    store_stats(lds, 0, ls, dl);
    __syncthreads();

    const int nt = (p.Nq + 63) / 64;
    for (int t = 0; t < nt; ++t) {
        const int q0 = t * 64;
        T* cur = lds + (t & 1) * BUF;
        const T* Qs = cur;
        const T* dOs = Qs + L::ROWMAJOR;
        const T* Qt = dOs + L::ROWMAJOR;
        const T* dOt = Qt + L::TRANSP;
        const float* lse_s = stats_of(cur);
        const float* del_s = lse_s + 64;
        if (t + 1 < nt) {
            pair_load<T, HD>(qr, qp, p.sqn, q0 + 64, p.Nq);
            pair_load<T, HD>(dor, dop, p.sdon, q0 + 64, p.Nq);
            load_stats(q0 + 64, ls, dl);
        }
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            // every LDS fragment of a phase is requested before the phase's first MFMA, so the reads
            // overlap instead of forming a read -> wait -> MFMA chain
            Frag<T> qa[HD / 16], da[HD / 16];
            {
                const T* qb_ = Qs + (qb * 32 + l31) * L::LDR + 8 * hi;
                const T* db_ = dOs + (qb * 32 + l31) * L::LDR + 8 * hi;
#pragma unroll
                for (int s_ = 0; s_ < HD / 16; ++s_) qa[s_] = ld_frag8(qb_ + 16 * s_);
#pragma unroll
                for (int s_ = 0; s_ < HD / 16; ++s_) da[s_] = ld_frag8(db_ + 16 * s_);
            }
            __builtin_amdgcn_sched_barrier(0);
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int s_ = 0; s_ < HD / 16; ++s_) mma32(s, qa[s_], kf[s_]);      // S[q][key]
#pragma unroll
            for (int s_ = 0; s_ < HD / 16; ++s_) mma32(dp, da[s_], vf[s_]);     // dP[q][key]
            f32x4 l4[4], d4[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                l4[g] = *reinterpret_cast<const f32x4*>(lse_s + qb * 32 + 8 * g + 4 * hi);
                d4[g] = *reinterpret_cast<const f32x4*>(del_s + qb * 32 + 8 * g + 4 * hi);
            }
            Frag<T> dot[2][HD / 32], qt[2][HD / 32];
#pragma unroll
            for (int t_ = 0; t_ < 2; ++t_)
#pragma unroll
                for (int db = 0; db < HD / 32; ++db) {
                    const int d = db * 32 + l31;
                    const int off = d * L::LDT + tswz(d, qb * 32 + 16 * t_ + 8 * hi);
                    dot[t_][db] = ld_frag8(dOt + off);
                    qt[t_][db] = ld_frag8(Qt + off);
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int r = 4 * g + e;
                    float pr = fast_exp2(fmaf(s[r], c, -l4[g][e]));
                    s[r] = pr;
                    dp[r] = pr * (dp[r] - d4[g][e]);             // dS overwrites dP
                }
#pragma unroll
            for (int t_ = 0; t_ < 2; ++t_) {
                Frag<T> pf = acc_to_frag<T>(s, t_);
#pragma unroll
                for (int db = 0; db < HD / 32; ++db) mma32(dv[db], dot[t_][db], pf);
            }
#pragma unroll
            for (int t_ = 0; t_ < 2; ++t_) {
                Frag<T> pf = acc_to_frag<T>(dp, t_);
#pragma unroll
                for (int db = 0; db < HD / 32; ++db) mma32(dk[db], qt[t_][db], pf);
            }
        }
        if (t + 1 < nt) {
            T* nb = lds + ((t + 1) & 1) * BUF;
            pair_store<T, HD, true, true>(qr, nb, nb + 2 * L::ROWMAJOR);
            pair_store<T, HD, true, true>(dor, nb + L::ROWMAJOR, nb + 2 * L::ROWMAJOR + L::TRANSP);
            store_stats(nb, q0 + 64, ls, dl);
        }
        __syncthreads();
    }
    if (krow < p.Nk) {
        T* dkp = reinterpret_cast<T*>(p.dk) + b * p.sdkb + h * p.sdkh + (int64_t)krow * p.sdkn;
        T* dvp = reinterpret_cast<T*>(p.dv) + b * p.sdvb + h * p.sdvh + (int64_t)krow * p.sdvn;
        if (p.flags & GF_ATTN_ACC_DK) add_row<HD>(dkp, dk, p.scale, hi); else store_row<T, HD>(dkp, dk, p.scale, hi);
        store_row<T, HD>(dvp, dv, 1.f, hi);
    }
}

template <typename T, int HD> size_t fwd_lds() { return 2 * (Lay<T, HD>::ROWMAJOR + Lay<T, HD>::TRANSP) * sizeof(T); }
template <typename T, int HD> size_t dq_lds() { return 2 * (2 * Lay<T, HD>::ROWMAJOR + Lay<T, HD>::TRANSP) * sizeof(T); }
template <typename T, int HD> size_t dkv_lds() {
    return 2 * ((2 * Lay<T, HD>::ROWMAJOR + 2 * Lay<T, HD>::TRANSP) * sizeof(T) + 128 * sizeof(float));
}
constexpr size_t ATTN_LDS_MAX = 160 * 1024;

template <typename T, int HD> int fwd(const AttnParams& p, hipStream_t st) {
    const size_t lds = fwd_lds<T, HD>();
    if (lds > ATTN_LDS_MAX) return GF_ERR_UNSUPPORTED;
    if (int e = set_lds(attn_fwd_kernel<T, HD>, lds)) return e;
    attn_fwd_kernel<T, HD><<<dim3(((p.Nq + 255) / 256) * p.H * p.B), dim3(256), lds, st>>>(p);
    return gf_launched();
}
template <typename T, int HD> int dq(const AttnParams& p, hipStream_t st) {
    const size_t lds = dq_lds<T, HD>();
    if (lds > ATTN_LDS_MAX) return GF_ERR_UNSUPPORTED;
    if (int e = set_lds(attn_bwd_dq_kernel<T, HD>, lds)) return e;
    attn_bwd_dq_kernel<T, HD><<<dim3(((p.Nq + 255) / 256) * p.H * p.B), dim3(256), lds, st>>>(p);
    return gf_launched();
}
template <typename T, int HD> int bwd(const AttnParams& p_, hipStream_t st) {
    if constexpr (sizeof(T) == 2 && HD == 64) {
        return GF_ERR_UNSUPPORTED;               // bf16 at head_dim 64: dK/dV is attn_bwd_dkv_bf16_kernel's (attention_dkv.hip)
    } else {
        AttnParams p = p_;
        p.flags |= ATTN_PLAIN_STATS;
        const size_t lds = dkv_lds<T, HD>();
        if (dq_lds<T, HD>() > ATTN_LDS_MAX || lds > ATTN_LDS_MAX) return GF_ERR_UNSUPPORTED;
        if (int e = dq<T, HD>(p, st)) return e;
        if (int e = set_lds(attn_bwd_dkv_kernel<T, HD>, lds)) return e;
        attn_bwd_dkv_kernel<T, HD><<<dim3(((p.Nk + 127) / 128) * p.H * p.B), dim3(256), lds, st>>>(p);
        return gf_launched();
    }
}

// f(element type, head_dim) for the run-time dtype and D
template <typename F> int by_type_and_dim(int dtype, int D, F f) {
    return gf_by_dtype(dtype, [&](auto t) {
        if (D == 32) return f(t, std::integral_constant<int, 32>());
        if (D == 64) return f(t, std::integral_constant<int, 64>());
        if (D == 128) return f(t, std::integral_constant<int, 128>());
        return (int)GF_ERR_UNSUPPORTED;
    });
}

}  // namespace

namespace gfattn {

int launch_fwd_generic(const AttnParams& p, hipStream_t st, int dtype, int D) {
    return by_type_and_dim(dtype, D, [&](auto t, auto hd) { return fwd<decltype(t), decltype(hd)::value>(p, st); });
}
int launch_dq_generic(const AttnParams& p, hipStream_t st, int dtype, int D) {
    return by_type_and_dim(dtype, D, [&](auto t, auto hd) { return dq<decltype(t), decltype(hd)::value>(p, st); });
}
int launch_bwd_generic(const AttnParams& p, hipStream_t st, int dtype, int D) {
    return by_type_and_dim(dtype, D, [&](auto t, auto hd) { return bwd<decltype(t), decltype(hd)::value>(p, st); });
}

}  // namespace gfattn
