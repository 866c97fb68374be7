// Relative-pose solver: batched RANSAC over 5-point hypotheses on normalised image coordinates, eight-point refit projected
// onto the essential manifold, local optimisation, pose recovery by the depth test.
//
// Stands in for (reference) gluefactory/robust_estimators/relative_pose/opencv.py:23-64 (cv2.findEssentialMat with RANSAC on
// normalised coordinates and the threshold ransac_th / f_mean, then cv2.recoverPose) and for decompose_essential_matrix of
// gluefactory/geometry/epipolar.py:97-122.
//
// A call is a fixed chain of kernels on one stream (5 + 2 lo_iters for gf_e_ransac: compact, solve, score, select,
// lo_iters x (refit, rescore), pose; 2 for gf_e_pose: compact, pose).  Nothing depends on a count the host reads: every
// kernel takes its pair's match count K_b from the workspace.
//
// Sampling (restated on the host by tests/e_solver_cases.py, bit for bit).  All arithmetic is uint32 with wrap-around:
//   hash(seed, pair, hyp, draw): x = seed * 0x9E3779B1 + pair * 0x85EBCA77 + hyp * 0xC2B2AE3D + draw * 0x27D4EB2F + 0x165667B1;
//                                x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16
//   (the hash of h_solver.hip).  Draw d = 0..4 of a pair with K matches: r = (uint64(hash) * (K - d)) >> 32, uniform in
//   [0, K - d); then the skip mapping: the earlier draws are visited in ASCENDING order of their value p, and r += 1 whenever
//   r >= p.  The five values are distinct indices into the pair's ordered match list.
//
// Solve: one hypothesis per lane, 64 lanes per workgroup, fp64, the arithmetic of e_fivept.h (Nister's solver: null space by
// elimination, the 10 x 20 cubic constraints, elimination to a degree-10 polynomial, bisection on fixed brackets, back-
// substitution).  Its per-lane arrays (5 x 9, 10 x 20, 6 x 20 doubles and the polynomial work) live in scratch: this is the
// one kernel of the file that uses any.  Up to GF_E_MAXSOL candidates per hypothesis go to the workspace as fp32 with
// ||E||_F = 1; unused slots are zero.
//
// Score: one candidate per lane, candidate index = hypothesis * GF_E_MAXSOL + slot.  Correspondence (x0, x1) is an inlier of
// E when, in fp32 with e = x1^T E x0, a = (E x0)[0:2], b = (E^T x1)[0:2]:  e^2 < th^2 (|a|^2 + |b|^2)  and the right-hand
// side is finite and > 0 (the squared Sampson error against th^2 without a division).  The compacted correspondences stream
// through LDS in tiles of GF_E_TILE, read as broadcasts.  A workgroup's best (count, lowest candidate index) is one 64-bit
// key, the select kernel takes the maximum key: deterministic, no floating-point atomics.
//
// Refit (skipped under 8 inliers): fp64.  Hartley normalisation of both point sets over the flagged correspondences, the 45
// distinct sums of A^T A (rows (u x, u y, u, v x, v y, v, x, y, 1)) through a fixed-order block reduction, GF_E_JACOBI cyclic
// sweeps (gf_jacobi9.h), the eigenvector of the smallest eigenvalue, de-normalisation E = T1^T G T0, projection to singular
// values (1, 1, 0) / sqrt 2 through GF_E_JACOBI3 sweeps on E^T E.
//
// Pose: one workgroup per pair, fp64.  R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2] with det U = det V = +1; the four
// candidates in the order (R1, t), (R1, -t), (R2, t), (R2, -t).  Every flagged correspondence is triangulated linearly
// (X = d0 x0 from the least squares of x1 x (d0 R x0 + t) = 0) and counts for a candidate when d0 > 0 and (R X + t)_z > 0;
// fixed-order integer reduction; the highest count wins, ties to the lowest index.  |t| = 1.
#include "gf_common.h"
#include "gf_amd.h"
#include "gf_jacobi9.h"
#include "e_fivept.h"

namespace {

constexpr int TILE = GF_E_TILE;
constexpr int HYPS = GF_E_HYPS;
constexpr int MAXSOL = GF_E_MAXSOL;
constexpr int SOLVE_LANES = 64;
static_assert(HYPS == 256, "one candidate per lane of a 256-lane workgroup");
static_assert(TILE == 256, "one correspondence per lane when a tile is staged");

struct Ws {
    int* K;                     // [B] matches of the pair
    int* idx;                   // [B, M] ordered indices of the matched keypoints of view 0
    float4* corr;               // [B, M] (x0, y0, x1, y1) of the ordered matches
    float* cand;                // [B, T, MAXSOL, 9] candidates of every hypothesis
    int* ncand;                 // [B, T]
    unsigned long long* best;   // [B, nblk] best key of every scoring workgroup
    float* Ecur;                // [B, 12] current model (9 used)
    float* Enew;                // [B, 12] refitted model
    int* state;                 // [B, 4] {count of the current model, current model valid, refit valid, unused}
    uint8_t* flags;             // [B, M] inlier flags of the current model over the ordered matches
};

inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
inline int64_t nblk_of(int T) { return ((int64_t)T * MAXSOL + HYPS - 1) / HYPS; }

inline size_t carve(void* base, int B, int M, int T, Ws* w) {
    size_t off = 0;
    char* p = reinterpret_cast<char*>(base);
    auto take = [&](size_t bytes) { size_t o = off; off = al16(off + bytes); return p + o; };
    Ws t;
    t.K = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B));
    t.idx = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * M));
    t.corr = reinterpret_cast<float4*>(take(sizeof(float4) * (size_t)B * M));
    t.cand = reinterpret_cast<float*>(take(sizeof(float) * 9 * MAXSOL * (size_t)B * T));
    t.ncand = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * T));
    t.best = reinterpret_cast<unsigned long long*>(take(sizeof(unsigned long long) * (size_t)B * nblk_of(T)));
    t.Ecur = reinterpret_cast<float*>(take(sizeof(float) * 12 * (size_t)B));
    t.Enew = reinterpret_cast<float*>(take(sizeof(float) * 12 * (size_t)B));
    t.state = reinterpret_cast<int*>(take(sizeof(int) * 4 * (size_t)B));
    t.flags = reinterpret_cast<uint8_t*>(take((size_t)B * M));
    if (w) *w = t;
    return off;
}

// ---- sampling ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t e_hash(uint32_t seed, uint32_t pair, uint32_t hyp, uint32_t draw) {
    uint32_t x = seed * 0x9E3779B1u + pair * 0x85EBCA77u + hyp * 0xC2B2AE3Du + draw * 0x27D4EB2Fu + 0x165667B1u;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// five distinct indices in [0, K), K >= 5
__device__ __forceinline__ void sample5(uint32_t seed, int pair, int hyp, int K, int s[5]) {
    int o[5];                                      // the earlier draws in ascending order
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        int r = (int)(((unsigned long long)e_hash(seed, (uint32_t)pair, (uint32_t)hyp, (uint32_t)d) * (uint32_t)(K - d)) >> 32);
#pragma unroll
        for (int q = 0; q < d; ++q)
            if (r >= o[q]) ++r;
        s[d] = r;
        int at = d;
#pragma unroll
        for (int q = d - 1; q >= 0; --q)
            if (o[q] > r) { o[q + 1] = o[q]; at = q; }
        o[at] = r;
    }
}

__device__ __forceinline__ bool is_inlier(const float E[9], float4 c, float th2) {
    const float a0 = E[0] * c.x + E[1] * c.y + E[2], a1 = E[3] * c.x + E[4] * c.y + E[5], a2 = E[6] * c.x + E[7] * c.y + E[8];
    const float e = c.z * a0 + c.w * a1 + a2;
    const float b0 = E[0] * c.z + E[3] * c.w + E[6], b1 = E[1] * c.z + E[4] * c.w + E[7];
    const float rhs = th2 * (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
    return (e * e < rhs) && (rhs > 0.f) && isfinite(rhs);           // a NaN compares false
}

// ---- block reductions (256 lanes = 4 waves), results in every lane ---------------------------------------------------------
__device__ __forceinline__ int block_sum_int(int v, int* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();                              // red may still be read from an earlier call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

template <int NV> __device__ __forceinline__ void block_sum_f64(double (&v)[NV], double* red /* [4][NV] */) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[i] += __shfl_xor(v[i], d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) red[(threadIdx.x >> 6) * NV + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = ((red[i] + red[NV + i]) + red[2 * NV + i]) + red[3 * NV + i];
}

__device__ __forceinline__ unsigned long long block_max_key(unsigned long long key, unsigned long long* red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
    __syncthreads();
    unsigned long long m = red[0];
    for (int q = 1; q < 4; ++q) m = red[q] > m ? red[q] : m;
    return m;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------
// ordered compaction of the matches of one pair (ascending i); a match index outside [0, N) counts as no match
__global__ __launch_bounds__(256) void e_compact_kernel(const float* kp0, const float* kp1, const int64_t* m0, Ws w, int M,
                                                        int N) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int base = 0;
    for (int i0 = 0; i0 < M; i0 += 256) {
        const int i = i0 + tid;
        const int64_t j = i < M ? m0[(int64_t)b * M + i] : -1;
        const bool f = j >= 0 && j < N;
        const unsigned long long mask = __ballot(f);
        const int pre = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(mask);
        __syncthreads();
        int off = base;
        for (int q = 0; q < wv; ++q) off += wsum[q];
        const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (f) {
            const int64_t at = (int64_t)b * M + off + pre;
            const float* p = kp0 + ((int64_t)b * M + i) * 2;
            const float* q = kp1 + ((int64_t)b * N + j) * 2;
            w.idx[at] = i;
            w.corr[at] = make_float4(p[0], p[1], q[0], q[1]);
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0) w.K[b] = base;
}

// one 5-point hypothesis per lane -> its candidates in the workspace (and in the debug outputs)
__global__ __launch_bounds__(SOLVE_LANES) void e_solve_kernel(Ws w, int M, int T, int nsb, uint32_t seed, int* samples,
                                                              float* cand_out, int* ncand_out) {
    const int b = blockIdx.x / nsb, t = (blockIdx.x % nsb) * SOLVE_LANES + threadIdx.x;
    if (t >= T) return;
    const int K = w.K[b];
    const float4* corr = w.corr + (int64_t)b * M;
    float* cand = w.cand + ((int64_t)b * T + t) * (MAXSOL * 9);
    int s[5] = {-1, -1, -1, -1, -1};
    int n = 0;
    if (K >= 5) {
        sample5(seed, b, t, K, s);
        double pts[20];
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            const float4 c = corr[s[d]];
            pts[4 * d] = c.x; pts[4 * d + 1] = c.y; pts[4 * d + 2] = c.z; pts[4 * d + 3] = c.w;
        }
        n = gf_e5::solve5(pts, cand);
    }
    for (int i = n * 9; i < MAXSOL * 9; ++i) cand[i] = 0.f;
    w.ncand[(int64_t)b * T + t] = n;
    if (samples != nullptr)
        for (int d = 0; d < 5; ++d) samples[((int64_t)b * T + t) * 5 + d] = s[d];
    if (ncand_out != nullptr) ncand_out[(int64_t)b * T + t] = n;
    if (cand_out != nullptr)
        for (int i = 0; i < MAXSOL * 9; ++i) cand_out[((int64_t)b * T + t) * (MAXSOL * 9) + i] = cand[i];
}

// one candidate per lane: count inliers over the pair's matches; the workgroup's best key to the workspace
__global__ __launch_bounds__(256) void e_score_kernel(Ws w, const float* th, int M, int T, int nblk, int* cand_counts) {
    __shared__ float4 tile[TILE];
    __shared__ unsigned long long red[4];
    const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk, tid = threadIdx.x;
    const int ci = blk * HYPS + tid;                           // candidate index: hypothesis * MAXSOL + slot
    const int K = w.K[b];
    const float thb = th[b], th2 = thb * thb;
    const float4* corr = w.corr + (int64_t)b * M;
    float E[9];
    bool ok = false;
    if (ci < T * MAXSOL) ok = (ci % MAXSOL) < w.ncand[(int64_t)b * T + ci / MAXSOL];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = ok ? w.cand[((int64_t)b * T * MAXSOL + ci) * 9 + i] : 0.f;   // zero: no inlier
    int count = 0;
    for (int k0 = 0; k0 < K; k0 += TILE) {
        const int n = min(TILE, K - k0);
        __syncthreads();
        if (tid < n) tile[tid] = corr[k0 + tid];
        __syncthreads();
        for (int k = 0; k < n; ++k) count += is_inlier(E, tile[k], th2) ? 1 : 0;
    }
    if (cand_counts != nullptr && ci < T * MAXSOL) cand_counts[(int64_t)b * T * MAXSOL + ci] = ok ? count : -1;
    // key: (count + 1) in the high word (0 = no candidate), ~index in the low word: the maximum key is the highest count at
    // the lowest index
    const unsigned long long key =
        ok ? (((unsigned long long)(uint32_t)(count + 1) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)ci)) : 0ull;
    const unsigned long long m = block_max_key(key, red);
    if (tid == 0) w.best[(int64_t)b * nblk + blk] = m;
}

// flags and count of model E over the ordered matches of pair b; the count is returned in every lane
__device__ __forceinline__ int flag_pass(const float* E, const float4* corr, uint8_t* flags, int K, float th2, int* red) {
    int count = 0;
    for (int k = threadIdx.x; k < K; k += 256) {
        const bool in = is_inlier(E, corr[k], th2);
        if (flags != nullptr) flags[k] = in ? 1 : 0;
        count += in ? 1 : 0;
    }
    return block_sum_int(count, red);
}

// winner of the pair's workgroups -> current model, its flags and its count
__global__ __launch_bounds__(256) void e_select_kernel(Ws w, const float* th, int M, int T, int nblk) {
    __shared__ unsigned long long red[4];
    __shared__ int ired[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = w.K[b];
    const float thb = th[b], th2 = thb * thb;
    const float4* corr = w.corr + (int64_t)b * M;
    unsigned long long key = 0ull;
    for (int q = tid; q < nblk; q += 256) {
        const unsigned long long o = w.best[(int64_t)b * nblk + q];
        key = o > key ? o : key;
    }
    const unsigned long long m = block_max_key(key, red);
    const bool ok = m != 0ull && K >= 5;
    float E[9];
    const int64_t ci = ok ? (int64_t)(0xFFFFFFFFu - (uint32_t)(m & 0xFFFFFFFFull)) : 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = ok ? w.cand[((int64_t)b * T * MAXSOL + ci) * 9 + i] : 0.f;   // zero flags nothing
    const int count = flag_pass(E, corr, w.flags + (int64_t)b * M, K, th2, ired);
    if (tid < 9) w.Ecur[(int64_t)b * 12 + tid] = E[tid];
    if (tid == 0) {
        w.state[b * 4 + 0] = count;
        w.state[b * 4 + 1] = ok ? 1 : 0;
        w.state[b * 4 + 2] = 0;
    }
}

// Hartley-normalised eight-point fit over the flagged matches, projected onto the essential manifold -> Enew, state[2]
__global__ __launch_bounds__(256) void e_refit_kernel(Ws w, int M) {
    __shared__ double red[4 * 45];
    __shared__ double A[9][9], V[9][9];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = w.K[b];
    const float4* corr = w.corr + (int64_t)b * M;
    const uint8_t* flags = w.flags + (int64_t)b * M;
    float* En = w.Enew + (int64_t)b * 12;
    if (w.state[b * 4 + 1] == 0 || w.state[b * 4 + 0] < 8) {        // uniform over the workgroup
        if (tid == 0) w.state[b * 4 + 2] = 0;
        return;
    }
    // pass 1: count and centroids
    double s5[5] = {0., 0., 0., 0., 0.};
    for (int k = tid; k < K; k += 256)
        if (flags[k]) {
            const float4 c = corr[k];
            s5[0] += 1.; s5[1] += c.x; s5[2] += c.y; s5[3] += c.z; s5[4] += c.w;
        }
    block_sum_f64<5>(s5, red);
    const double n = s5[0];
    const double cx0 = s5[1] / n, cy0 = s5[2] / n, cx1 = s5[3] / n, cy1 = s5[4] / n;
    // pass 2: mean distances to the centroids
    double s2[2] = {0., 0.};
    for (int k = tid; k < K; k += 256)
        if (flags[k]) {
            const float4 c = corr[k];
            const double dx0 = c.x - cx0, dy0 = c.y - cy0, dx1 = c.z - cx1, dy1 = c.w - cy1;
            s2[0] += sqrt(dx0 * dx0 + dy0 * dy0);
            s2[1] += sqrt(dx1 * dx1 + dy1 * dy1);
        }
    block_sum_f64<2>(s2, red);
    const double sc0 = 1.4142135623730951 / (s2[0] / n), sc1 = 1.4142135623730951 / (s2[1] / n);
    // pass 3: the 45 distinct sums of A^T A
    double acc[45];
#pragma unroll
    for (int i = 0; i < 45; ++i) acc[i] = 0.;
    for (int k = tid; k < K; k += 256)
        if (flags[k]) {
            const float4 c = corr[k];
            const double x = (c.x - cx0) * sc0, y = (c.y - cy0) * sc0, u = (c.z - cx1) * sc1, v = (c.w - cy1) * sc1;
            const double r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.};
            int at = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j) { acc[at] += r[i] * r[j]; ++at; }
        }
    block_sum_f64<45>(acc, red);
    __syncthreads();
    if (tid == 0) {
        int at = 0;
        for (int i = 0; i < 9; ++i)
            for (int j = i; j < 9; ++j) { A[i][j] = acc[at]; A[j][i] = acc[at]; ++at; }
        for (int i = 0; i < 9; ++i)
            for (int j = 0; j < 9; ++j) V[i][j] = i == j ? 1. : 0.;
    }
    __syncthreads();
    gf_jacobi9(A, V, GF_E_JACOBI, tid);
    if (tid == 0) {
        int best = 0;
        for (int i = 1; i < 9; ++i)
            if (A[i][i] < A[best][best]) best = i;
        double g[9], m[9], e[9];
        for (int i = 0; i < 9; ++i) g[i] = V[i][best];
        // E = T1^T G T0 with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
        for (int r = 0; r < 3; ++r) {
            m[3 * r + 0] = g[3 * r + 0] * sc0;
            m[3 * r + 1] = g[3 * r + 1] * sc0;
            m[3 * r + 2] = g[3 * r + 2] - sc0 * (g[3 * r + 0] * cx0 + g[3 * r + 1] * cy0);
        }
        for (int c = 0; c < 3; ++c) {
            e[0 + c] = sc1 * m[0 + c];
            e[3 + c] = sc1 * m[3 + c];
            e[6 + c] = m[6 + c] - sc1 * (cx1 * m[0 + c] + cy1 * m[3 + c]);
        }
        bool ok = gf_e5::project_essential(e);
        float out[9];
        for (int i = 0; i < 9; ++i) { out[i] = (float)e[i]; ok = ok && isfinite(out[i]); }
        for (int i = 0; i < 9; ++i) En[i] = ok ? out[i] : 0.f;
        w.state[b * 4 + 2] = ok ? 1 : 0;
    }
}

// rescore the refit; it replaces the current model when it is valid and its count does not drop
__global__ __launch_bounds__(256) void e_rescore_kernel(Ws w, const float* th, int M) {
    __shared__ int ired[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (w.state[b * 4 + 1] == 0 || w.state[b * 4 + 2] == 0) return;           // uniform
    const int K = w.K[b];
    const float thb = th[b], th2 = thb * thb;
    const float4* corr = w.corr + (int64_t)b * M;
    float E[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = w.Enew[(int64_t)b * 12 + i];
    const int count = flag_pass(E, corr, nullptr, K, th2, ired);
    if (count < w.state[b * 4 + 0]) return;                                   // uniform
    flag_pass(E, corr, w.flags + (int64_t)b * M, K, th2, ired);
    __syncthreads();
    if (tid < 9) w.Ecur[(int64_t)b * 12 + tid] = E[tid];
    if (tid == 0) w.state[b * 4 + 0] = count;
}

// pose of the model by the depth test, and the outputs.  ransac != 0: the current model and its flags from the workspace,
// every output written; else E and the per-keypoint flags of the caller, R, t and num_front alone.
__global__ __launch_bounds__(256) void e_pose_kernel(Ws w, int M, int ransac, const float* E_in, const uint8_t* inl_in,
                                                     float* E_out, float* R, float* t, uint8_t* inliers, int* num_inliers,
                                                     uint8_t* success, int* num_front) {
    __shared__ double Rs[2][9], ts[3];
    __shared__ int oks, ired[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = w.K[b];
    const float4* corr = w.corr + (int64_t)b * M;
    const int* idx = w.idx + (int64_t)b * M;
    const float* Esrc = ransac ? w.Ecur + (int64_t)b * 12 : E_in + (int64_t)b * 9;
    const bool model = ransac ? w.state[b * 4 + 1] != 0 : true;
    if (tid == 0) {
        double E[9];
        bool ok = model;
        for (int i = 0; i < 9; ++i) { E[i] = Esrc[i]; ok = ok && isfinite(Esrc[i]); }
        ok = ok && gf_e5::decompose(E, Rs[0], Rs[1], ts);
        for (int i = 0; i < 9; ++i) ok = ok && isfinite(Rs[0][i]) && isfinite(Rs[1][i]);
        for (int i = 0; i < 3; ++i) ok = ok && isfinite(ts[i]);
        oks = ok ? 1 : 0;
    }
    __syncthreads();
    const bool ok = oks != 0;
    int cnt[4] = {0, 0, 0, 0};
    if (ok) {
        double Ra[9], Rb[9];
        const double tp[3] = {ts[0], ts[1], ts[2]}, tm[3] = {-ts[0], -ts[1], -ts[2]};
#pragma unroll
        for (int i = 0; i < 9; ++i) { Ra[i] = Rs[0][i]; Rb[i] = Rs[1][i]; }
        for (int k = tid; k < K; k += 256) {
            const bool f = ransac ? w.flags[(int64_t)b * M + k] != 0 : inl_in[(int64_t)b * M + idx[k]] != 0;
            if (!f) continue;
            const float4 c = corr[k];
            cnt[0] += gf_e5::in_front(Ra, tp, c.x, c.y, c.z, c.w) ? 1 : 0;
            cnt[1] += gf_e5::in_front(Ra, tm, c.x, c.y, c.z, c.w) ? 1 : 0;
            cnt[2] += gf_e5::in_front(Rb, tp, c.x, c.y, c.z, c.w) ? 1 : 0;
            cnt[3] += gf_e5::in_front(Rb, tm, c.x, c.y, c.z, c.w) ? 1 : 0;
        }
    }
    int win = 0, wc = -1;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int c = block_sum_int(cnt[d], ired);
        if (c > wc) { wc = c; win = d; }                       // ties stay with the lowest index
    }
    if (tid < 9) {
        const double r = Rs[win >> 1][tid];
        R[(int64_t)b * 9 + tid] = ok ? (float)r : (tid % 4 == 0 ? 1.f : 0.f);
        if (ransac) E_out[(int64_t)b * 9 + tid] = ok ? Esrc[tid] : 0.f;
    }
    if (tid < 3) t[(int64_t)b * 3 + tid] = ok ? (float)((win & 1) ? -ts[tid] : ts[tid]) : 0.f;
    if (tid == 0 && num_front != nullptr) num_front[b] = ok ? wc : 0;
    if (!ransac) return;
    if (tid == 0) {
        success[b] = ok ? 1 : 0;
        num_inliers[b] = ok ? w.state[b * 4 + 0] : 0;
    }
    for (int i = tid; i < M; i += 256) inliers[(int64_t)b * M + i] = 0;
    __syncthreads();
    if (!ok) return;
    for (int k = tid; k < K; k += 256)
        if (w.flags[(int64_t)b * M + k]) inliers[(int64_t)b * M + idx[k]] = 1;
}

inline int check_common(const void* p0, const void* p1, const void* m0, int B, int M, int N, int T, const void* ws,
                        int64_t ws_bytes) {
    if (B <= 0 || M <= 0 || N <= 0 || T < 1) return GF_ERR_SHAPE;
    if (p0 == nullptr || p1 == nullptr || m0 == nullptr || ws == nullptr) return GF_ERR_SHAPE;
    if ((int64_t)B * nblk_of(T) >= ((int64_t)1 << 31) || (int64_t)B * T * MAXSOL >= ((int64_t)1 << 31)) return GF_ERR_UNSUPPORTED;
    if (ws_bytes < (int64_t)carve(nullptr, B, M, T, nullptr)) return GF_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(ws) % 16 != 0) return GF_ERR_ALIGN;
    return 0;
}

}  // namespace

extern "C" int64_t gf_e_ws_bytes(int B, int M, int T) {
    if (B <= 0 || M <= 0 || T < 1) return 0;
    return (int64_t)carve(nullptr, B, M, T, nullptr);
}

extern "C" int gf_e_ransac(const float* pts0n, const float* pts1n, const int64_t* matches0, const float* th, int B, int M,
                           int N, int T, int lo_iters, uint32_t seed, void* ws, int64_t ws_bytes, float* E, float* R,
                           float* t, uint8_t* inliers, int32_t* num_inliers, uint8_t* success, int32_t* samples, float* cand,
                           int32_t* ncand, int32_t* cand_counts, void* stream) {
    if (int e = check_common(pts0n, pts1n, matches0, B, M, N, T, ws, ws_bytes)) return e;
    if (th == nullptr || E == nullptr || R == nullptr || t == nullptr || inliers == nullptr || num_inliers == nullptr ||
        success == nullptr)
        return GF_ERR_SHAPE;
    if (lo_iters < 0 || lo_iters > 64) return GF_ERR_SHAPE;
    Ws w;
    carve(ws, B, M, T, &w);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nblk = (int)nblk_of(T), nsb = (T + SOLVE_LANES - 1) / SOLVE_LANES;
    e_compact_kernel<<<dim3(B), dim3(256), 0, st>>>(pts0n, pts1n, matches0, w, M, N);
    e_solve_kernel<<<dim3((unsigned)(B * nsb)), dim3(SOLVE_LANES), 0, st>>>(w, M, T, nsb, seed, samples, cand, ncand);
    e_score_kernel<<<dim3((unsigned)(B * nblk)), dim3(256), 0, st>>>(w, th, M, T, nblk, cand_counts);
    e_select_kernel<<<dim3(B), dim3(256), 0, st>>>(w, th, M, T, nblk);
    for (int it = 0; it < lo_iters; ++it) {
        e_refit_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M);
        e_rescore_kernel<<<dim3(B), dim3(256), 0, st>>>(w, th, M);
    }
    e_pose_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, 1, nullptr, nullptr, E, R, t, inliers, num_inliers, success, nullptr);
    return (int)hipGetLastError();
}

extern "C" int gf_e_pose(const float* pts0n, const float* pts1n, const int64_t* matches0, const uint8_t* inliers,
                         const float* E, int B, int M, int N, void* ws, int64_t ws_bytes, float* R, float* t,
                         int32_t* num_front, void* stream) {
    if (int e = check_common(pts0n, pts1n, matches0, B, M, N, 1, ws, ws_bytes)) return e;
    if (inliers == nullptr || E == nullptr || R == nullptr || t == nullptr || num_front == nullptr) return GF_ERR_SHAPE;
    Ws w;
    carve(ws, B, M, 1, &w);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    e_compact_kernel<<<dim3(B), dim3(256), 0, st>>>(pts0n, pts1n, matches0, w, M, N);
    e_pose_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, 0, E, inliers, nullptr, R, t, nullptr, nullptr, nullptr, num_front);
    return (int)hipGetLastError();
}
