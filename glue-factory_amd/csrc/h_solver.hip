// Homography solver: batched RANSAC over 4-point hypotheses, Hartley-normalised (weighted) DLT refit, local optimisation.
//
// Stands in for (reference) gluefactory/robust_estimators/homography/opencv.py:27-53 (cv2.findHomography with RANSAC:
// forward transfer error against ransac_th, identity + all-false inliers when nothing is found) and for
// kornia's find_homography_dlt(pts0, pts1, weights) as gluefactory/eval/utils.py:253 calls it.
//
// A call is a fixed chain of kernels on one stream (4 + 2 lo_iters for gf_h_ransac, 3 for gf_h_dlt), one workgroup of 256
// lanes per pair except the scoring kernel (one workgroup per GF_H_HYPS hypotheses of a pair).  Nothing depends on a count
// the host reads: every kernel takes its pair's match count K_b from the workspace.
//
// The RANSAC machinery (workspace core, sampling, reductions and the winner key, compaction, the feature parts with the
// tile-streamed count, flag pass and rescore over them, the skeleton of the refit, flag scatter) is ransac_common.h, shared
// with e_solver.hip and hl_solver.hip; the inlier rule, the rows and the view-1 side of the DLT are h_model.h, shared with
// hl_solver.hip; what is here is the rest of the model: the 4-point fit, the gates of the refit, and the kernels' names.
//
// Sampling: four draws per hypothesis by the rule in the header of ransac_common.h.
//
// 4-point fit (fp32, closed form, nine values per lane).  Both images are translated so that sample point 1 is the origin;
// with twice the signed area  area(a, b, c) = (b - a) x (c - a)  the source gives
//   s = area(P1,P2,P3), l1 = area(P2,P3,P4), l2 = area(P3,P1,P4), l3 = area(P1,P2,P4)
// (l = adj([P1 P2 P3]) P4 in homogeneous coordinates) and the target the same four numbers (d, m1, m2, m3).  The sample is
// rejected when any of the eight has magnitude below GF_H_EPS_AREA, when a source / target pair of them differs in sign, or
// when an entry of the result is non-finite.  l and m are divided by their largest magnitude, g = (m1 l2 l3, m2 l1 l3,
// m3 l1 l2), H' = [Q1 Q2 Q3] diag(g) adj([P1 P2 P3]), H' is divided by its largest magnitude, the two translations are
// composed back, and the result is divided by h22 -- unless |h22| < GF_H_H22_FRAC ||H||_F, which rejects the sample too.
//
// Scoring: correspondence (x0, x1) is an inlier of H when w = h20 x + h21 y + h22 is finite and > 0 and
// |(H x0) / w - x1|^2 < th^2, in fp32.  The compacted correspondences of a pair stream through LDS in tiles of GF_H_TILE.
//
// Refit: the skeleton of ransac_common.h over the flagged correspondences (the weights do not enter the normalisation, as in
// kornia) with the two rows per correspondence of A^T W A and GF_H_JACOBI sweeps, then H = T1^-1 G T0 and h22 = 1.
#include "h_model.h"

namespace {

constexpr int TILE = GF_H_TILE;
constexpr int HYPS = GF_H_HYPS;
static_assert(HYPS == 256, "one hypothesis per lane of a 256-lane workgroup");

using Ws = RansacWs;            // the models (cur, refit) are homographies with h22 = 1

inline int nblk_of(int T) { return (T + HYPS - 1) / HYPS; }

inline size_t carve(void* base, int B, int M, int T, Ws* w) {
    Carver c{reinterpret_cast<char*>(base)};
    Ws t;
    carve_core(c, B, M, nblk_of(T), t);
    if (w) *w = t;
    return c.off;
}

// ---- 4-point fit ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float area2(float ax, float ay, float bx, float by, float cx, float cy) {
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}
__device__ __forceinline__ bool same_sign(float a, float b) { return (a > 0.f) == (b > 0.f); }

__device__ __forceinline__ bool fit4(const float4 c[4], float h[9]) {
    // translated coordinates: point 1 of either image is the origin
    const float x2 = c[1].x - c[0].x, y2 = c[1].y - c[0].y, x3 = c[2].x - c[0].x, y3 = c[2].y - c[0].y;
    const float x4 = c[3].x - c[0].x, y4 = c[3].y - c[0].y;
    const float u2 = c[1].z - c[0].z, v2 = c[1].w - c[0].w, u3 = c[2].z - c[0].z, v3 = c[2].w - c[0].w;
    const float u4 = c[3].z - c[0].z, v4 = c[3].w - c[0].w;
    const float s = area2(0.f, 0.f, x2, y2, x3, y3), d = area2(0.f, 0.f, u2, v2, u3, v3);
    float l1 = area2(x2, y2, x3, y3, x4, y4), l2 = area2(x3, y3, 0.f, 0.f, x4, y4), l3 = area2(0.f, 0.f, x2, y2, x4, y4);
    float m1 = area2(u2, v2, u3, v3, u4, v4), m2 = area2(u3, v3, 0.f, 0.f, u4, v4), m3 = area2(0.f, 0.f, u2, v2, u4, v4);
    const float eps = GF_H_EPS_AREA;
    bool ok = fabsf(s) >= eps && fabsf(l1) >= eps && fabsf(l2) >= eps && fabsf(l3) >= eps &&
              fabsf(d) >= eps && fabsf(m1) >= eps && fabsf(m2) >= eps && fabsf(m3) >= eps;
    ok = ok && same_sign(s, d) && same_sign(l1, m1) && same_sign(l2, m2) && same_sign(l3, m3);
    const float ln = 1.f / fmaxf(fmaxf(fabsf(l1), fabsf(l2)), fabsf(l3));
    const float mn = 1.f / fmaxf(fmaxf(fabsf(m1), fabsf(m2)), fabsf(m3));
    l1 *= ln; l2 *= ln; l3 *= ln; m1 *= mn; m2 *= mn; m3 *= mn;
    const float g1 = m1 * l2 * l3, g2 = m2 * l1 * l3, g3 = m3 * l1 * l2;
    // rows of adj([P1 P2 P3]) = P2 x P3, P3 x P1, P1 x P2 with P1 = (0, 0, 1)
    const float a00 = y2 - y3, a01 = x3 - x2, a02 = s;
    const float a10 = y3, a11 = -x3;
    const float a20 = -y2, a21 = x2;
    // H' = [Q1 Q2 Q3] diag(g) adj, Q1 = (0, 0, 1), Q2 = (u2, v2, 1), Q3 = (u3, v3, 1)
    float k[9];
    k[0] = u2 * g2 * a10 + u3 * g3 * a20; k[1] = u2 * g2 * a11 + u3 * g3 * a21; k[2] = 0.f;
    k[3] = v2 * g2 * a10 + v3 * g3 * a20; k[4] = v2 * g2 * a11 + v3 * g3 * a21; k[5] = 0.f;
    k[6] = g1 * a00 + g2 * a10 + g3 * a20; k[7] = g1 * a01 + g2 * a11 + g3 * a21; k[8] = g1 * a02;
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) mx = fmaxf(mx, fabsf(k[i]));
    const float inv = 1.f / mx;
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] *= inv;
    // H = T(q1) H' T(-p1)
    const float px = c[0].x, py = c[0].y, qx = c[0].z, qy = c[0].w;
    k[2] -= k[0] * px + k[1] * py;
    k[5] -= k[3] * px + k[4] * py;
    k[8] -= k[6] * px + k[7] * py;
    k[0] += qx * k[6]; k[1] += qx * k[7]; k[2] += qx * k[8];
    k[3] += qy * k[6]; k[4] += qy * k[7]; k[5] += qy * k[8];
    float fro = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) fro += k[i] * k[i];
    ok = ok && fabsf(k[8]) >= GF_H_H22_FRAC * sqrtf(fro);
    const float i22 = 1.f / k[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) { h[i] = k[i] * i22; ok = ok && isfinite(h[i]); }
    return ok;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void h_compact_kernel(const float* kp0, const float* kp1, const int64_t* m0, Ws w,
                                                        int M, int N) {
    __shared__ int wsum[4];
    compact_pair(kp0, kp1, m0, w, blockIdx.x, M, N, wsum);
}

// the sample of hypothesis t of pair b and its fit
__device__ __forceinline__ bool sample_fit(uint32_t seed, int b, int t, int K, const float4* corr, int s[4], float h[9]) {
    sample_distinct<4>(seed, b, t, K, s);
    float4 c[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) c[d] = corr[s[d]];
    return fit4(c, h);
}

// one hypothesis per lane: sample, fit, count inliers over the pair's matches; the workgroup's best key to the workspace
__global__ __launch_bounds__(256) void h_score_kernel(Ws w, int M, int T, int nblk, float th2, uint32_t seed,
                                                      int* samples, int* hyp_counts) {
    __shared__ float4 tile[TILE];
    __shared__ unsigned long long red[4];
    const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk, tid = threadIdx.x;
    const int t = blk * HYPS + tid;
    const int K = w.K[b];
    const float4* corr = w.corr + (int64_t)b * M;
    float h[9];
    bool ok = false;
    int s[4] = {-1, -1, -1, -1};
    if (t < T && K >= 4) ok = sample_fit(seed, b, t, K, corr, s, h);
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = 0.f;                   // w = 0: nothing is an inlier
    }
    if (samples != nullptr && t < T) {
        int* sp = samples + ((int64_t)b * T + t) * 4;
#pragma unroll
        for (int d = 0; d < 4; ++d) sp[d] = s[d];
    }
    const int count = tile_count<TILE>(h, PointPart{corr, nullptr, K, th2}, tile, TransferInlier());
    if (hyp_counts != nullptr && t < T) hyp_counts[(int64_t)b * T + t] = ok ? count : -1;
    const unsigned long long m = block_max_key(pack_key(ok, count, t), red);
    if (tid == 0) w.best[(int64_t)b * nblk + blk] = m;
}

// winner of the pair's workgroups, fitted again from its sample -> current model, its flags and its count
__global__ __launch_bounds__(256) void h_select_kernel(Ws w, int M, int nblk, float th2, uint32_t seed) {
    __shared__ unsigned long long red[4];
    __shared__ int ired[4];
    __shared__ float hs[9];
    __shared__ int oks;
    const int b = blockIdx.x, tid = threadIdx.x;
    const PointPart part = point_part(w, b, M, th2);
    const int K = part.K;
    const unsigned long long m = pair_max_key(w, b, nblk, red);
    if (tid == 0) {
        float h[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        bool ok = false;
        int s[4];
        if (m != 0ull && K >= 4)                                  // the same arithmetic as the scoring lane's
            ok = sample_fit(seed, b, key_index(m), K, part.corr, s, h);
        for (int i = 0; i < 9; ++i) hs[i] = ok ? h[i] : (i % 4 == 0 ? 1.f : 0.f);
        oks = ok ? 1 : 0;
    }
    __syncthreads();
    const bool ok = oks != 0;
    float h[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = ok ? hs[i] : 0.f;          // an all-zero model flags nothing
    set_current(w, b, h, hs, ok, ired, TransferInlier(), part);
}

// Hartley-normalised weighted DLT over the flagged matches (use_flags == 0: over all of them) -> refit, state[ST_REFIT_OK]
__global__ __launch_bounds__(256) void h_refit_kernel(Ws w, const float* weights, int M, int use_flags, int gate) {
    __shared__ double red[4 * 45];
    __shared__ double A[9][9], V[9][9];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float4* corr = w.corr + (int64_t)b * M;
    const uint8_t* flags = w.flags + (int64_t)b * M;
    const int* idx = w.idx + (int64_t)b * M;
    float* Hn = w.refit + (int64_t)b * 12;
    int* refit_ok = w.state + b * 4 + ST_REFIT_OK;
    // gate: refit only where the pair has a current model (the local optimisation of gf_h_ransac); else nothing is kept
    const int K = (gate == 0 || w.state[b * 4 + ST_CUR_OK] != 0) ? w.K[b] : 0;
    const auto part = point_refit(
        corr, K, [=](int k) { return !use_flags || flags[k]; },
        [=](double (&acc)[45], int k, double x, double y, double u, double v) {
            add_point_rows<true>(acc, x, y, u, v, weights != nullptr ? (double)weights[(int64_t)b * M + idx[k]] : 1.);
        });
    Hartley t;
    refit_moments(red, t, part);
    if (!(t.n >= 4.)) {                                             // uniform over the workgroup
        h_refit_none(Hn, refit_ok);
        return;
    }
    double m[9];
    refit_solve(red, A, V, GF_H_JACOBI, t, m, part);
    if (tid == 0) h_refit_tail(m, t, (double)GF_H_H22_FRAC, Hn, refit_ok);
}

__global__ __launch_bounds__(256) void h_rescore_kernel(Ws w, int M, float th2) {
    __shared__ int ired[4];
    rescore_pair(w, blockIdx.x, ired, TransferInlier(), point_part(w, blockIdx.x, M, th2));
}

// outputs.  ransac != 0: the current model, its flags scattered to the keypoints of view 0, its count; else the refit alone
__global__ __launch_bounds__(256) void h_final_kernel(Ws w, int M, int ransac, float* H, uint8_t* inliers, int* num_inliers,
                                                      uint8_t* success) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool ok = w.state[b * 4 + (ransac ? ST_CUR_OK : ST_REFIT_OK)] != 0;
    const float* src = (ransac ? w.cur : w.refit) + (int64_t)b * 12;
    if (tid < 9) H[(int64_t)b * 9 + tid] = ok ? src[tid] : (tid % 4 == 0 ? 1.f : 0.f);
    if (tid == 0) {
        success[b] = ok ? 1 : 0;
        if (num_inliers != nullptr) num_inliers[b] = (ok && ransac) ? w.state[b * 4 + ST_COUNT] : 0;
    }
    if (inliers != nullptr)
        scatter_flags(w.flags + (int64_t)b * M, w.idx + (int64_t)b * M, w.K[b], M, ok, inliers + (int64_t)b * M);
}

inline int check_common(const void* kp0, const void* kp1, const void* m0, int B, int M, int N, int T, const void* ws,
                        int64_t ws_bytes) {
    return ransac_check(kp0, kp1, m0, B, M, N, T, ws, ws_bytes, nblk_of(T), T, carve(nullptr, B, M, T, nullptr));
}

}  // namespace

extern "C" int64_t gf_h_ws_bytes(int B, int M, int T) {
    if (B <= 0 || M <= 0 || T < 1) return 0;
    return (int64_t)carve(nullptr, B, M, T, nullptr);
}

extern "C" int gf_h_ransac(const float* kpts0, const float* kpts1, const int64_t* matches0, int B, int M, int N, int T,
                           float ransac_th, int lo_iters, uint32_t seed, void* ws, int64_t ws_bytes, float* H,
                           uint8_t* inliers, int32_t* num_inliers, uint8_t* success, int32_t* samples, int32_t* hyp_counts,
                           void* stream) {
    if (int e = check_common(kpts0, kpts1, matches0, B, M, N, T, ws, ws_bytes)) return e;
    if (H == nullptr || inliers == nullptr || num_inliers == nullptr || success == nullptr) return GF_ERR_SHAPE;
    if (!(ransac_th > 0.f) || !(ransac_th < 1e18f) || lo_iters < 0 || lo_iters > 64) return GF_ERR_SHAPE;
    Ws w;
    carve(ws, B, M, T, &w);
    hipStream_t st = gf_stream(stream);
    const int nblk = nblk_of(T);
    const float th2 = ransac_th * ransac_th;
    h_compact_kernel<<<dim3(B), dim3(256), 0, st>>>(kpts0, kpts1, matches0, w, M, N);
    h_score_kernel<<<dim3((unsigned)(B * nblk)), dim3(256), 0, st>>>(w, M, T, nblk, th2, seed, samples, hyp_counts);
    h_select_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, nblk, th2, seed);
    for (int it = 0; it < lo_iters; ++it) {
        h_refit_kernel<<<dim3(B), dim3(256), 0, st>>>(w, nullptr, M, 1, 1);
        h_rescore_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, th2);
    }
    h_final_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, 1, H, inliers, num_inliers, success);
    return gf_launched();
}

extern "C" int gf_h_dlt(const float* kpts0, const float* kpts1, const int64_t* matches0, const float* weights, int B, int M,
                        int N, void* ws, int64_t ws_bytes, float* H, uint8_t* success, void* stream) {
    if (int e = check_common(kpts0, kpts1, matches0, B, M, N, 1, ws, ws_bytes)) return e;
    if (H == nullptr || success == nullptr) return GF_ERR_SHAPE;
    Ws w;
    carve(ws, B, M, 1, &w);
    hipStream_t st = gf_stream(stream);
    h_compact_kernel<<<dim3(B), dim3(256), 0, st>>>(kpts0, kpts1, matches0, w, M, N);
    h_refit_kernel<<<dim3(B), dim3(256), 0, st>>>(w, weights, M, 0, 0);
    h_final_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, 0, H, nullptr, nullptr, success);
    return gf_launched();
}

