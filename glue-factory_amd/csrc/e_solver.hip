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
// The RANSAC machinery (workspace core, sampling, reductions and the winner key, compaction, the feature parts with the
// tile-streamed count, flag pass and rescore over them, the skeleton of the refit, flag scatter) is ransac_common.h, shared
// with h_solver.hip and hl_solver.hip; what is here is the model: the 5-point solve, the Sampson rule, the rows and the
// view-1 side of the eight-point fit, the pose.
//
// Sampling: five draws per hypothesis by the rule in the header of ransac_common.h.
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
// through LDS in tiles of GF_E_TILE.
//
// Refit (skipped under 8 inliers): the skeleton of ransac_common.h over the flagged correspondences with the rows
// (u x, u y, u, v x, v y, v, x, y, 1) of A^T A and GF_E_JACOBI sweeps, then E = T1^T G T0 and the projection to singular
// values (1, 1, 0) / sqrt 2 through GF_E_JACOBI3 sweeps on E^T E.
//
// Pose: one workgroup per pair, fp64.  R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2] with det U = det V = +1; the four
// candidates in the order (R1, t), (R1, -t), (R2, t), (R2, -t).  Every flagged correspondence is triangulated linearly
// (X = d0 x0 from the least squares of x1 x (d0 R x0 + t) = 0) and counts for a candidate when d0 > 0 and (R X + t)_z > 0;
// fixed-order integer reduction; the highest count wins, ties to the lowest index.  |t| = 1.
#include "ransac_common.h"
#include "e_fivept.h"

namespace {

constexpr int TILE = GF_E_TILE;
constexpr int HYPS = GF_E_HYPS;
constexpr int MAXSOL = GF_E_MAXSOL;
constexpr int SOLVE_LANES = 64;
static_assert(HYPS == 256, "one candidate per lane of a 256-lane workgroup");

struct Ws : RansacWs {          // the models (cur, refit) are essential matrices with ||E||_F = 1
    float* cand;                // [B, T, MAXSOL, 9] candidates of every hypothesis
    int* ncand;                 // [B, T]
};

inline int64_t nblk_of(int T) { return ((int64_t)T * MAXSOL + HYPS - 1) / HYPS; }

inline size_t carve(void* base, int B, int M, int T, Ws* w) {
    Carver c{reinterpret_cast<char*>(base)};
    Ws t;
    carve_core(c, B, M, nblk_of(T), t);
    t.cand = c.take<float>(9 * MAXSOL * (size_t)B * T);
    t.ncand = c.take<int>((size_t)B * T);
    if (w) *w = t;
    return c.off;
}

struct Inlier {
    __device__ __forceinline__ bool operator()(const float* E, float4 c, float th2) const {
        const float a0 = E[0] * c.x + E[1] * c.y + E[2], a1 = E[3] * c.x + E[4] * c.y + E[5], a2 = E[6] * c.x + E[7] * c.y + E[8];
        const float e = c.z * a0 + c.w * a1 + a2;
        const float b0 = E[0] * c.z + E[3] * c.w + E[6], b1 = E[1] * c.z + E[4] * c.w + E[7];
        const float rhs = th2 * (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
        return (e * e < rhs) && (rhs > 0.f) && isfinite(rhs);           // a NaN compares false
    }
};

// ---- kernels ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void e_compact_kernel(const float* kp0, const float* kp1, const int64_t* m0, Ws w, int M,
                                                        int N) {
    __shared__ int wsum[4];
    compact_pair(kp0, kp1, m0, w, blockIdx.x, M, N, wsum);
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
        sample_distinct<5>(seed, b, t, K, s);
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
    const int count = tile_count<TILE>(E, PointPart{corr, nullptr, K, th2}, tile, Inlier());
    if (cand_counts != nullptr && ci < T * MAXSOL) cand_counts[(int64_t)b * T * MAXSOL + ci] = ok ? count : -1;
    const unsigned long long m = block_max_key(pack_key(ok, count, ci), red);
    if (tid == 0) w.best[(int64_t)b * nblk + blk] = m;
}

// winner of the pair's workgroups, read back from the candidates -> current model, its flags and its count
__global__ __launch_bounds__(256) void e_select_kernel(Ws w, const float* th, int M, int T, int nblk) {
    __shared__ unsigned long long red[4];
    __shared__ int ired[4];
    const int b = blockIdx.x;
    const float thb = th[b];
    const PointPart part = point_part(w, b, M, thb * thb);
    const unsigned long long m = pair_max_key(w, b, nblk, red);
    const bool ok = m != 0ull && part.K >= 5;
    float E[9];
    const int64_t ci = ok ? (int64_t)key_index(m) : 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = ok ? w.cand[((int64_t)b * T * MAXSOL + ci) * 9 + i] : 0.f;   // zero flags nothing
    set_current(w, b, E, E, ok, ired, Inlier(), part);
}

// Hartley-normalised eight-point fit over the flagged matches, projected onto the essential manifold -> refit,
// state[ST_REFIT_OK]
__global__ __launch_bounds__(256) void e_refit_kernel(Ws w, int M) {
    __shared__ double red[4 * 45];
    __shared__ double A[9][9], V[9][9];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = w.K[b];
    const float4* corr = w.corr + (int64_t)b * M;
    const uint8_t* flags = w.flags + (int64_t)b * M;
    float* En = w.refit + (int64_t)b * 12;
    if (w.state[b * 4 + ST_CUR_OK] == 0 || w.state[b * 4 + ST_COUNT] < 8) {        // uniform over the workgroup
        if (tid == 0) w.state[b * 4 + ST_REFIT_OK] = 0;
        return;
    }
    const auto part = point_refit(
        corr, K, [=](int k) { return flags[k] != 0; },
        [](double (&acc)[45], int, double x, double y, double u, double v) {
            const double r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.};
            int at = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j) { acc[at] += r[i] * r[j]; ++at; }
        });
    Hartley t;
    refit_moments(red, t, part);
    double m[9];
    refit_solve(red, A, V, GF_E_JACOBI, t, m, part);
    if (tid == 0) {
        // E = T1^T (G T0) with T1 = [[s1, 0, -s1 cx1], [0, s1, -s1 cy1], [0, 0, 1]]
        double e[9];
        for (int c = 0; c < 3; ++c) {
            e[0 + c] = t.sc1 * m[0 + c];
            e[3 + c] = t.sc1 * m[3 + c];
            e[6 + c] = m[6 + c] - t.sc1 * (t.cx1 * m[0 + c] + t.cy1 * m[3 + c]);
        }
        bool ok = gf_e5::project_essential(e);
        float out[9];
        for (int i = 0; i < 9; ++i) { out[i] = (float)e[i]; ok = ok && isfinite(out[i]); }
        for (int i = 0; i < 9; ++i) En[i] = ok ? out[i] : 0.f;
        w.state[b * 4 + ST_REFIT_OK] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void e_rescore_kernel(Ws w, const float* th, int M) {
    __shared__ int ired[4];
    const int b = blockIdx.x;
    const float thb = th[b];
    rescore_pair(w, b, ired, Inlier(), point_part(w, b, M, thb * thb));
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
    const float* Esrc = ransac ? w.cur + (int64_t)b * 12 : E_in + (int64_t)b * 9;
    const bool model = ransac ? w.state[b * 4 + ST_CUR_OK] != 0 : true;
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
        num_inliers[b] = ok ? w.state[b * 4 + ST_COUNT] : 0;
    }
    scatter_flags(w.flags + (int64_t)b * M, idx, K, M, ok, inliers + (int64_t)b * M);
}

inline int check_common(const void* p0, const void* p1, const void* m0, int B, int M, int N, int T, const void* ws,
                        int64_t ws_bytes) {
    return ransac_check(p0, p1, m0, B, M, N, T, ws, ws_bytes, nblk_of(T), (int64_t)T * MAXSOL, carve(nullptr, B, M, T, nullptr));
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
    hipStream_t st = gf_stream(stream);
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
    return gf_launched();
}

extern "C" int gf_e_pose(const float* pts0n, const float* pts1n, const int64_t* matches0, const uint8_t* inliers,
                         const float* E, int B, int M, int N, void* ws, int64_t ws_bytes, float* R, float* t,
                         int32_t* num_front, void* stream) {
    if (int e = check_common(pts0n, pts1n, matches0, B, M, N, 1, ws, ws_bytes)) return e;
    if (inliers == nullptr || E == nullptr || R == nullptr || t == nullptr || num_front == nullptr) return GF_ERR_SHAPE;
    Ws w;
    carve(ws, B, M, 1, &w);
    hipStream_t st = gf_stream(stream);
    e_compact_kernel<<<dim3(B), dim3(256), 0, st>>>(pts0n, pts1n, matches0, w, M, N);
    e_pose_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, 0, E, inliers, nullptr, R, t, nullptr, nullptr, nullptr, num_front);
    return gf_launched();
}
