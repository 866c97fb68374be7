// Nearest-neighbour matcher kernels: top-2 of every row of S = a b^T without the [B,M,N] tensor, the ratio / distance /
// mutual filter on the top-2 vectors, and the dense N-pair loss on a materialised similarity.
//
// Replaces (reference) gluefactory/models/matchers/nearest_neighbor_matcher.py:15-25 (find_nn: topk(2) over the einsum
// of :53), :28-35 (mutual_check), :63-64 (matching scores) and :76-93 (the N_pair loss and its autograd).
//
// gf_rows_top2 uses the skeleton of assignment.hip (assign_common.h): the owner rows' fragments stay in registers, the
// other matrix streams through LDS in 64-row MFMA tiles, and the running (best, arg, second) of a row is lane-local until
// the two half waves meet once at the end.  The N-pair kernels are dense element-wise passes with reductions: no MFMA.
#include "gf_launch.h"
#include "gf_common.h"
#include "assign_common.h"
#include "gf_amd.h"

namespace {

// Running top-2 of one lane.  "second" is the second element of the visited scores as a MULTISET: a duplicated maximum
// gives second == best.  With s2 <= v always, one new score x updates s2 = max(s2, min(x, v)) (x > v: the old maximum steps
// down; else x competes for second place) before TileArg::see moves the maximum -- min, max in front of its compare +
// two selects.  The strict > of TileArg keeps the lowest index of a tie (a lane visits its rows in ascending order).
struct TileTop2 {
    TileArg a; float s2;
    __device__ __forceinline__ void reset() { a.reset(); s2 = -INFINITY; }
    __device__ __forceinline__ void see(float x, int off_const) {
        s2 = fmaxf(s2, fminf(x, a.v));
        a.see(x, off_const);
    }
    // the tile's (v, s2) meets the running (best, second): top-2 of the union of two sorted pairs
    __device__ __forceinline__ void merge(int s0, int hi, float& best, int& bidx, float& second) const {
        second = fmaxf(fmaxf(second, s2), fminf(a.v, best));
        a.merge(s0, hi, best, bidx);
    }
};

// best / arg / second over streamed rows s < Ns of own . oth_s
template <typename T, int D>
__global__ __launch_bounds__(256) void rows_top2_kernel(HeadParams p) {
    GF_HEAD_PROLOGUE(T, D)
    float best = -INFINITY, second = -INFINITY;
    int bidx = 0x7fffffff;
    auto bias = [&](int si, float& v0, float& v1) {
        v0 = si < p.Ns ? 0.f : -INFINITY;                         // rows past Ns never win
        v1 = 0.f;
    };
    auto body = [&](const T* tile, const float* vec0, const float*, int s0) {
        TileTop2 tt;
        tt.reset();
        const bool full = s0 + 64 <= p.Ns;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
            mma_tile<T, D>(s, tile, kb * 32, of, l31, hi);
            if (full) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) tt.see(s[4 * g + e], kb * 32 + 8 * g + e);
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 b4 = *reinterpret_cast<const f32x4*>(vec0 + kb * 32 + 8 * g + 4 * hi);
#pragma unroll
                    for (int e = 0; e < 4; ++e) tt.see(s[4 * g + e] + b4[e], kb * 32 + 8 * g + e);
                }
            }
        }
        tt.merge(s0, hi, best, bidx, second);
    };
    stream_tiles<T, D>(tiles, vecs, othp, 0, p.Ns, p.Ns, bias, body);
    // the two half waves hold disjoint streamed rows of the same owner row
    const float ob_ = xhalf(best), os_ = xhalf(second);
    const int oi = __shfl_xor(bidx, 32);
    second = fmaxf(fmaxf(second, os_), fminf(best, ob_));
    if (ob_ > best || (ob_ == best && oi < bidx)) { best = ob_; bidx = oi; }
    if (orow < p.No && hi == 0) {
        p.f0[(int64_t)b * p.No + orow] = best;
        p.i0[(int64_t)b * p.No + orow] = (bidx == 0x7fffffff) ? 0 : bidx;
        p.f1[(int64_t)b * p.No + orow] = second;
    }
}

template <typename T, int D> int launch_top2_td(const HeadParams& p, hipStream_t st) {
    const int total = ((p.No + 127) / 128) * p.B;
    const size_t lds = head_lds<T, D>();
    if (int e = set_lds(rows_top2_kernel<T, D>, lds)) return e;
    rows_top2_kernel<T, D><<<dim3(total), dim3(256), lds, st>>>(p);
    return gf_launched();
}

template <typename T> int launch_top2_t(const HeadParams& p, int D, hipStream_t st) {
    switch (D) {
        case 64: return launch_top2_td<T, 64>(p, st);
        case 128: return launch_top2_td<T, 128>(p, st);
        case 256: return launch_top2_td<T, 256>(p, st);
        default: return GF_ERR_UNSUPPORTED;
    }
}

// find_nn's thresholds on one row's top-2, in fp32 and in the reference's form (dist = 2 (1 - sim); a negative threshold
// is "not set")
__device__ __forceinline__ bool nn_keep(float best, float second, float ratio2, float dist2) {
    const float d0 = 2.f * (1.f - best), d1 = 2.f * (1.f - second);
    bool ok = true;
    if (ratio2 >= 0.f) ok = ok && (d0 <= ratio2 * d1);
    if (dist2 >= 0.f) ok = ok && (d0 <= dist2);
    return ok;
}

__global__ void nn_filter_kernel(const float* best0, const int64_t* arg0, const float* sec0,
                                 const float* best1, const int64_t* arg1, const float* sec1,
                                 float ratio2, float dist2, int mutual,
                                 int64_t* m0, int64_t* m1, float* s0, float* s1, int B, int M, int N) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)B * (M + N)) return;
    const int b = (int)(t / (M + N)), k = (int)(t % (M + N));
    const bool side1 = k >= M;
    // this side's vectors (length n_me) and the partner side's (length n_ot)
    const int i = side1 ? k - M : k;
    const int n_me = side1 ? N : M, n_ot = side1 ? M : N;
    const float* bm = (side1 ? best1 : best0) + (int64_t)b * n_me;
    const float* sm = (side1 ? sec1 : sec0) + (int64_t)b * n_me;
    const int64_t* am = (side1 ? arg1 : arg0) + (int64_t)b * n_me;
    const float* bo = (side1 ? best0 : best1) + (int64_t)b * n_ot;
    const float* so = (side1 ? sec0 : sec1) + (int64_t)b * n_ot;
    const int64_t* ao = (side1 ? arg0 : arg1) + (int64_t)b * n_ot;
    const int64_t j = am[i];
    bool ok = nn_keep(bm[i], sm[i], ratio2, dist2);
    // mutual_check on the THRESHOLDED matches: a partner that fails its own threshold has match -1 and supports nobody
    ok = ok && j >= 0 && j < n_ot;
    if (ok && mutual) ok = (ao[j] == i) && nn_keep(bo[j], so[j], ratio2, dist2);
    (side1 ? m1 : m0)[(int64_t)b * n_me + i] = ok ? j : -1;
    (side1 ? s1 : s0)[(int64_t)b * n_me + i] = ok ? 1.f : 0.f;
}

// ---- N-pair loss on a dense similarity ---------------------------------------------------------------------------
// score = T (2 - sqrt(max(2 (1 - sim), 1e-6)))
__device__ __forceinline__ float npair_root(float sim) { return sqrtf(fmaxf(2.f * (1.f - sim), 1e-6f)); }

__device__ __forceinline__ void lse_push(float& m, float& s, float x) {
    const float mn = fmaxf(m, x);
    s = s * expf(m - mn) + expf(x - mn);
    m = mn;
}
__device__ __forceinline__ void lse_join(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    s = s * expf(m - mn) + s2 * expf(m2 - mn);
    m = mn;
}

// one wave per row (b, i): lse over j
__global__ __launch_bounds__(256) void npair_row_lse_kernel(const float* sim, const float* temp, float* lse_row,
                                                            int64_t rows, int N) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float T = temp[0];
    const float* sp = sim + row * N;
    float m = GF_NEG_BIG, s = 0.f;
    for (int j = lane; j < N; j += 64) lse_push(m, s, T * (2.f - npair_root(sp[j])));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) lse_join(m, s, __shfl_xor(m, d), __shfl_xor(s, d));
    if (lane == 0) lse_row[row] = m + logf(s);
}

// one workgroup per 64 columns of one pair: wave w takes rows w, w + 4, ...; the four partial (max, sum) meet in LDS
__global__ __launch_bounds__(256) void npair_col_lse_kernel(const float* sim, const float* temp, float* lse_col,
                                                            int B, int M, int N) {
    __shared__ float sm_[4][64], ss_[4][64];
    const int ncb = (N + 63) / 64;
    const int b = blockIdx.x / ncb, j = (blockIdx.x % ncb) * 64 + (threadIdx.x & 63);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float T = temp[0];
    float m = GF_NEG_BIG, s = 0.f;
    if (j < N) {
        const float* sp = sim + (int64_t)b * M * N + j;
        for (int i = w; i < M; i += 4) lse_push(m, s, T * (2.f - npair_root(sp[(int64_t)i * N])));
    }
    sm_[w][lane] = m;
    ss_[w][lane] = s;
    __syncthreads();
    if (w == 0 && j < N) {
#pragma unroll
        for (int k = 1; k < 4; ++k) lse_join(m, s, sm_[k][lane], ss_[k][lane]);
        lse_col[(int64_t)b * N + j] = m + logf(s);
    }
}

// positives (pb, pi, pj), pj < 0 = padding: acc[b] += 2 score - lse_row - lse_col; counts per pair / row / column
__global__ void npair_pos_kernel(const float* sim, const float* temp, const float* lse_row, const float* lse_col,
                                 const int64_t* pb, const int64_t* pi, const int64_t* pj, int64_t P,
                                 float* acc, float* cnt, float* cnt_row, float* cnt_col, int B, int M, int N) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P) return;
    const int64_t b = pb[t], i = pi[t], j = pj[t];
    if (j < 0 || j >= N || i < 0 || i >= M || b < 0 || b >= B) return;
    const float score = temp[0] * (2.f - npair_root(sim[(b * M + i) * N + j]));
    atomicAdd(acc + b, 2.f * score - lse_row[b * M + i] - lse_col[b * N + j]);
    atomicAdd(cnt + b, 1.f);
    atomicAdd(cnt_row + b * M + i, 1.f);
    atomicAdd(cnt_col + b * N + j, 1.f);
}

// dense part of the backward: dscore = coef_b (cnt_row_i softmax_row + cnt_col_j softmax_col); dsim = dscore T / root
// where the clamp is inactive (0 where it is active); dT += dscore (2 - root), one atomic per wave
__global__ __launch_bounds__(256) void npair_bwd_dense_kernel(const float* sim, const float* temp, const float* lse_row,
                                                              const float* lse_col, const float* cnt_row,
                                                              const float* cnt_col, const float* coef, float* dsim,
                                                              float* dT, int B, int M, int N) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t tot = (int64_t)B * M * N;
    float dt = 0.f;
    if (t < tot) {
        const int j = (int)(t % N);
        const int64_t bi = t / N;               // b * M + i
        const int b = (int)(bi / M);
        const float T = temp[0];
        const float x = sim[t];
        const float root = npair_root(x);
        const float score = T * (2.f - root);
        const float ds = coef[b] * (cnt_row[bi] * __expf(score - lse_row[bi]) +
                                    cnt_col[(int64_t)b * N + j] * __expf(score - lse_col[(int64_t)b * N + j]));
        const bool clamped = 2.f * (1.f - x) < 1e-6f;
        dsim[t] = clamped ? 0.f : ds * T / root;
        dt = ds * (2.f - root);
    }
    dt = wave_allsum(dt);
    if ((threadIdx.x & 63) == 0 && dt != 0.f) atomicAdd(dT, dt);
}

// the positives' direct term: dscore -= 2 coef_b at (b, i, j), added atomically after the dense pass on the same stream: a
// (b, i, j) listed twice counts twice, here as in the forward's sums and counts
__global__ void npair_bwd_pos_kernel(const float* sim, const float* temp, const float* coef, const int64_t* pb,
                                     const int64_t* pi, const int64_t* pj, int64_t P, float* dsim, float* dT,
                                     int B, int M, int N) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P) return;
    const int64_t b = pb[t], i = pi[t], j = pj[t];
    if (j < 0 || j >= N || i < 0 || i >= M || b < 0 || b >= B) return;
    const int64_t at = (b * M + i) * N + j;
    const float T = temp[0];
    const float x = sim[at];
    const float root = npair_root(x);
    const float ds = -2.f * coef[b];
    if (!(2.f * (1.f - x) < 1e-6f)) atomicAdd(dsim + at, ds * T / root);
    atomicAdd(dT, ds * (2.f - root));
}

inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" int gf_rows_top2(const void* a, const void* b, float* best, int64_t* arg, float* second,
                            int B, int M, int N, int D, int dtype, void* stream) {
    if (B <= 0 || M <= 0 || N <= 0) return GF_ERR_SHAPE;
    if (best == nullptr || arg == nullptr || second == nullptr) return GF_ERR_SHAPE;
    HeadParams p = {};
    p.own = a; p.oth = b; p.B = B; p.No = M; p.Ns = N; p.f0 = best; p.i0 = arg; p.f1 = second;
    return gf_by_dtype(dtype, [&](auto t) { return launch_top2_t<decltype(t)>(p, D, gf_stream(stream)); });
}

extern "C" int gf_nn_filter(const float* best0, const int64_t* arg0, const float* second0,
                            const float* best1, const int64_t* arg1, const float* second1,
                            float ratio2, float dist2, int mutual,
                            int64_t* m0, int64_t* m1, float* s0, float* s1, int B, int M, int N, void* stream) {
    if (B <= 0 || M <= 0 || N <= 0) return GF_ERR_SHAPE;
    const int64_t tot = (int64_t)B * (M + N);
    if (tot >= ((int64_t)1 << 31)) return GF_ERR_UNSUPPORTED;
    nn_filter_kernel<<<dim3(blocks_for(tot, 256)), dim3(256), 0, gf_stream(stream)>>>(
        best0, arg0, second0, best1, arg1, second1, ratio2, dist2, mutual, m0, m1, s0, s1, B, M, N);
    return gf_launched();
}

extern "C" int gf_npair_fwd(const float* sim, const float* temperature, const int64_t* pb, const int64_t* pi,
                            const int64_t* pj, int64_t P, float* lse_row, float* lse_col, float* acc, float* cnt,
                            float* cnt_row, float* cnt_col, int B, int M, int N, void* stream) {
    if (B <= 0 || M <= 0 || N <= 0 || P < 0) return GF_ERR_SHAPE;
    if ((int64_t)B * M * N >= ((int64_t)1 << 31)) return GF_ERR_UNSUPPORTED;
    hipStream_t st = gf_stream(stream);
    if (hipError_t e = gf_zero_f32(acc, (size_t)B, st)) return (int)e;
    if (hipError_t e = gf_zero_f32(cnt, (size_t)B, st)) return (int)e;
    if (hipError_t e = gf_zero_f32(cnt_row, (size_t)B * M, st)) return (int)e;
    if (hipError_t e = gf_zero_f32(cnt_col, (size_t)B * N, st)) return (int)e;
    const int64_t rows = (int64_t)B * M;
    npair_row_lse_kernel<<<dim3(blocks_for(rows, 4)), dim3(256), 0, st>>>(sim, temperature, lse_row, rows, N);
    npair_col_lse_kernel<<<dim3((unsigned)(B * ((N + 63) / 64))), dim3(256), 0, st>>>(sim, temperature, lse_col, B, M, N);
    if (P > 0)
        npair_pos_kernel<<<dim3(blocks_for(P, 256)), dim3(256), 0, st>>>(sim, temperature, lse_row, lse_col, pb, pi, pj, P,
                                                                         acc, cnt, cnt_row, cnt_col, B, M, N);
    return gf_launched();
}

extern "C" int gf_npair_bwd(const float* sim, const float* temperature, const float* lse_row, const float* lse_col,
                            const float* cnt_row, const float* cnt_col, const float* coef, const int64_t* pb,
                            const int64_t* pi, const int64_t* pj, int64_t P, float* dsim, float* dT,
                            int B, int M, int N, void* stream) {
    if (B <= 0 || M <= 0 || N <= 0 || P < 0) return GF_ERR_SHAPE;
    const int64_t tot = (int64_t)B * M * N;
    if (tot >= ((int64_t)1 << 31)) return GF_ERR_UNSUPPORTED;      // one thread per element of the dense similarity
    hipStream_t st = gf_stream(stream);
    if (hipError_t e = gf_zero_f32(dT, 1, st)) return (int)e;
    npair_bwd_dense_kernel<<<dim3(blocks_for(tot, 256)), dim3(256), 0, st>>>(sim, temperature, lse_row, lse_col, cnt_row,
                                                                             cnt_col, coef, dsim, dT, B, M, N);
    if (P > 0)
        npair_bwd_pos_kernel<<<dim3(blocks_for(P, 256)), dim3(256), 0, st>>>(sim, temperature, coef, pb, pi, pj, P, dsim, dT,
                                                                             B, M, N);
    return gf_launched();
}
