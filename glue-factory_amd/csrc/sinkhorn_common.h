// Log-domain Sinkhorn optimal transport with dustbins, forward and backward (HBM/MALL-bound).
//
// Replaces gluefactory_nonfree/superglue.py:186-191 (log_sinkhorn_iterations) and the
// iteration part of :194-214 (log_optimal_transport).  Z is the [B, R=M+1, C=N+1] fp32
// coupling matrix (scores augmented with the bin score).  Per iteration
//     u_i = log_mu_i - LSE_j(Z_ij + v_j),      v_j = log_nu_j - LSE_i(Z_ij + u_i)
// the reference makes >= 6 full-matrix passes; here ONE pass: a workgroup pulls RB (<=16) whole
// rows of Z into LDS with coalesced loads, finishes the row log-sum-exp with wave-level
// reductions (new u), then sweeps the SAME LDS-resident rows column-wise to emit per-block
// column (max, sum) partials for the new v, which a tiny second kernel combines.  Only the
// iterates u^k, v^k are stored (2(N+1) floats per iteration) — no autograd tape of matrices.
// Three implementations, chosen per call by select_tier() in sinkhorn.hip: this generic LDS form (sinkhorn_generic.hip) serves
// N + 1 > 2304; narrower problems keep their rows in registers and stream them once per iteration (sinkhorn_stream.hip) or,
// when the batch fills the chip, keep a chunk of pairs resident for all iterations (sinkhorn_resident.hip).
//
// Backward (oracle/sinkhorn_oracle.py::backward_recurrence, verified against autograd):
//   ubar^k_i    = [k==T] rowsum(G)_i - sum_j exp(Z_ij + u^k_i + v^k_j - log_nu_j) vbar^k_j
//   vbar^{k-1}_j = - sum_i exp(Z_ij + u^k_i - log_mu_i + v^{k-1}_j) ubar^k_i
//   dZ_ij = G_ij - sum_k [ exp(Z_ij+u^k_i+v^k_j-log_nu_j) vbar^k_j + exp(Z_ij+u^k_i-log_mu_i+v^{k-1}_j) ubar^k_i ]
// i.e. T passes of the same one-read shape plus one final pass; every exponent is <= 0 up to
// rounding (Q, R are sub-stochastic), so no max-shift is needed in the reverse sweep.
//
// This header: what the Sinkhorn translation units (sinkhorn*.hip) share -- the problem geometry, the workspace carve, the
// resident plan and the launch functions sinkhorn.hip dispatches to.  Everything is in a named namespace or inline so that
// every unit can include it; the kernels themselves stay in their unit's anonymous namespace.
#pragma once
#include "gf_launch.h"

namespace gfsk {

struct Geo {
    int B, M, N, R, C, RB, nblk;
    int Cp;                           // fast path: row stride of the padded copy (C rounded up to 4)
    bool fast;                        // register-resident kernels (C <= 64*4*SKF_MAX_NS)
    float norm, lmu_last, lnu_last;   // log_mu = norm (i<M) | lmu_last ; log_nu = norm (j<N) | lnu_last
};
__device__ __forceinline__ float lmu(const Geo& g, int i) { return i < g.M ? g.norm : g.lmu_last; }
__device__ __forceinline__ float lnu(const Geo& g, int j) { return j < g.N ? g.norm : g.lnu_last; }
__device__ __forceinline__ f32x4 splat4(float x) { f32x4 v = {x, x, x, x}; return v; }

// ---- geometry constants the host side needs
#ifndef SK_CHUNK_MB
#define SK_CHUNK_MB 300     // bytes of one batch chunk (MB): measured, 16-pair chunks stream fastest
#endif
#ifndef SKF_RPW_V
#define SKF_RPW_V 8
#endif
constexpr int SKF_RPW = SKF_RPW_V;             // streaming tier: rows per wave
constexpr int SKF_RPB = 4 * SKF_RPW;           // rows per workgroup (4 waves)
constexpr float SKF_SHIFT = 64.f;
constexpr int SKF_MAX_NS = 9;                  // float4 per lane and row: C <= 2304
const size_t LDS_BUDGET = 160 * 1024 - 512;
constexpr int SKR_PART_CUS = 320;              // partial rows reserved for the resident path: 4 waves x this many CUs
constexpr int SKR_MAX_BC = 16;                 // resident pairs per launch (counter slots; the failure flags follow them)

// distribution of one launch of the resident tier over the chip (skr_plan; the fields are gf_sinkhorn_plan's out[8])
struct SkrPlan {
    int bc, wpp, nw, base, extra, cs, nsm;
    size_t lds;
};

// workspace carve (floats): [ partials | u cur | v cur | ubar hist | vbar hist | Zp (fast path) ]
struct Ws { float *part, *ucur, *vcur, *ubar_hist, *vbar_hist, *zp, *a2p, *vbp, *P, *Q; unsigned* ctr; int KP; size_t part_rows, total; };

// what one launch of the resident kernel gets (sinkhorn_resident.hip); by value in its kernel arguments
struct SkrArgs {
    const float* Zraw;          // forward, round 6: the couplings themselves [bc, R, C] -- scaled by log2(e) while they are loaded,
                                // rows only 4-byte aligned (C = N + 1): no pre-scaled padded copy is made for the resident forward
    float* out;                 // forward, round 6: out = Z + u + v - norm written by the kernel's last iteration (null: not fused)
    const float* Zp;            // backward: [bc, R, Cp] prescaled padded copy
    float* part;                // [bc, nw, Cp] per-wave column partials
    unsigned* ctr;              // [4 SKR_MAX_BC]: barrier counters, failure flags, XCD masks, same-XCD counters; zeroed before the launch
    int safe_only;              // 1: placement-independent (write-through) hand-offs even when a pair sits on one XCD
    long long wait_ticks;       // bound of every wait in wall_clock64() ticks
    float* colA;                // [bc, Cp]  forward: running v (log2 units); backward: a2p
    float* colB;                // [bc, Cp]  backward: vbp
    float* u_hist;              // forward: written; backward: read           (chunk-offset, iteration stride ustride)
    float* v_hist;
    const float* base_row;      // backward: rowsum(G) of the chunk (k == T)
    float* ubar_hist;           // backward: written (index k - 1)
    float* vbar_hist;           // backward: written (index k - 1)
    size_t ustride, vstride;
    int iters;
    SkrPlan d;
    Geo g;
};

// ---- sinkhorn.hip
Geo make_geo(int B, int M, int N);
int batch_chunk(const Geo& g);                       // pairs per chunk of the generic and the streaming tier
Ws carve(void* ws, const Geo& g, int iters);

// ---- launch functions.  Pointers are offset to the chunk's first pair (`bc` pairs from there); histories keep the whole
// batch's iteration stride g.B * R (or C).  The int ones return a hipError_t / GF_ERR_* code, 0 on success.
// sinkhorn_generic.hip
int sk_fwd_launch(const float* Z, float* ucur, float* vcur, float* u_hist, float* v_hist, float* pm, float* ps, const Geo& g,
                  int bc, int iters, hipStream_t st);
void sk_final_fwd_launch(const float* Z, const float* u, const float* v, float* out, const Geo& g, int bc, hipStream_t st);
int sk_bwd_launch(const float* Z, const float* G, const float* gsum_row, const float* u_hist, const float* v_hist,
                  float* ubar_hist, float* vbar_hist, float* psum, float* gZ, const Geo& g, int bc, int iters, hipStream_t st);
// sinkhorn_stream.hip
void skf_prescale_launch(const float* Z, float* Zp, const Geo& g, int bc, hipStream_t st);
int skf_fwd_launch(const float* Zp, float* v2, float* u2, float* u_hist, float* v_hist, float* part, const Geo& g, int bc,
                   int iters, hipStream_t st);
void skf_bwd_prep_launch(const float* vT, const float* gsum_col, float* a2p, float* vbp, const Geo& g, int bc, hipStream_t st);
int skf_bwd_launch(const float* Zp, const float* u_hist, const float* v_hist, const float* gsum_row, float* ubar_hist,
                   float* vbar_hist, float* part, float* a2p, float* vbp, const Geo& g, int bc, int iters, hipStream_t st);
void skf_final_bwd_launch(const float* Z, const float* G, const float* u_hist, const float* v_hist, const float* ubar_hist,
                          const float* vbar_hist, float* P, float* Q, int KP, float* gZ, const Geo& g, int bc, int iters,
                          hipStream_t st);
// sinkhorn_resident.hip
bool skr_plan(const Geo& g, int B, int ncu, bool bwd, int mode, SkrPlan& d);   // false: the problem does not fit the layout
int skr_cus();                                                                  // CU count of the current device
// the fields of SkrArgs that do not depend on the direction or the chunk (asks the device: once per call, not per chunk)
SkrArgs skr_shared_args(const Geo& g, const Ws& w, const SkrPlan& d, int iters, int schedule);
int skr_fwd_launch(const SkrArgs& a, hipStream_t st);
int skr_bwd_launch(const SkrArgs& a, hipStream_t st);

}  // namespace gfsk
