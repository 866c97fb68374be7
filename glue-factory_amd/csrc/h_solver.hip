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
// Sampling (restated on the host by tests/h_solver_cases.py, bit for bit).  All arithmetic is uint32 with wrap-around:
//   hash(seed, pair, hyp, draw): x = seed * 0x9E3779B1 + pair * 0x85EBCA77 + hyp * 0xC2B2AE3D + draw * 0x27D4EB2F + 0x165667B1;
//                                x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16
//   draw d = 0..3 of a pair with K matches: r = (uint64(hash) * (K - d)) >> 32, i.e. uniform in [0, K - d); then the skip
//   mapping: the earlier draws are visited in ASCENDING order of their value p, and r += 1 whenever r >= p.  The four
//   values are distinct indices into the pair's ordered match list.
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
// |(H x0) / w - x1|^2 < th^2, in fp32.  The compacted correspondences of a pair stream through LDS in tiles of GF_H_TILE;
// every lane reads the same address (a broadcast).  A workgroup's best (count, lowest index) goes to the workspace as one
// 64-bit key, the select kernel takes the maximum key: deterministic, no floating-point atomics.
//
// Refit: fp64 throughout.  Hartley normalisation over the flagged correspondences (centroid, mean distance sqrt 2; the
// weights do not enter it, as in kornia), the 45 distinct sums of A^T W A through a fixed-order block reduction, GF_H_JACOBI
// cyclic Jacobi sweeps on the 9 x 9 matrix in LDS (lanes 0..8 own one row each), the eigenvector of the smallest eigenvalue,
// de-normalisation, h22 = 1.
#include "gf_common.h"
#include "gf_amd.h"
#include "gf_jacobi9.h"

namespace {

constexpr int TILE = GF_H_TILE;
constexpr int HYPS = GF_H_HYPS;
constexpr int JACOBI_SWEEPS = GF_H_JACOBI;
static_assert(HYPS == 256, "one hypothesis per lane of a 256-lane workgroup");
static_assert(TILE % 256 == 0 || 256 % TILE == 0, "tile staging assumes a simple ratio to the workgroup size");

struct Ws {
    int* K;                     // [B] matches of the pair
    int* idx;                   // [B, M] ordered indices of the matched keypoints of view 0
    float4* corr;               // [B, M] (x0, y0, x1, y1) of the ordered matches
    unsigned long long* best;   // [B, nblk] best key of every scoring workgroup
    float* Hcur;                // [B, 12] current model (9 used)
    float* Hnew;                // [B, 12] refitted model
    int* state;                 // [B, 4] {count of the current model, current model valid, refit valid, unused}
    uint8_t* flags;             // [B, M] inlier flags of the current model over the ordered matches
};

inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
inline int nblk_of(int T) { return (T + HYPS - 1) / HYPS; }

inline size_t carve(void* base, int B, int M, int T, Ws* w) {
    size_t off = 0;
    char* p = reinterpret_cast<char*>(base);
    auto take = [&](size_t bytes) { size_t o = off; off = al16(off + bytes); return p + o; };
    Ws t;
    t.K = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B));
    t.idx = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * M));
    t.corr = reinterpret_cast<float4*>(take(sizeof(float4) * (size_t)B * M));
    t.best = reinterpret_cast<unsigned long long*>(take(sizeof(unsigned long long) * (size_t)B * nblk_of(T)));
    t.Hcur = reinterpret_cast<float*>(take(sizeof(float) * 12 * (size_t)B));
    t.Hnew = reinterpret_cast<float*>(take(sizeof(float) * 12 * (size_t)B));
    t.state = reinterpret_cast<int*>(take(sizeof(int) * 4 * (size_t)B));
    t.flags = reinterpret_cast<uint8_t*>(take((size_t)B * M));
    if (w) *w = t;
    return off;
}

// ---- sampling ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t h_hash(uint32_t seed, uint32_t pair, uint32_t hyp, uint32_t draw) {
    uint32_t x = seed * 0x9E3779B1u + pair * 0x85EBCA77u + hyp * 0xC2B2AE3Du + draw * 0x27D4EB2Fu + 0x165667B1u;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// four distinct indices in [0, K), K >= 4
__device__ __forceinline__ void sample4(uint32_t seed, int pair, int hyp, int K, int s[4]) {
    int o0 = 0, o1 = 0, o2 = 0;                    // the earlier draws in ascending order
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        int r = (int)(((unsigned long long)h_hash(seed, (uint32_t)pair, (uint32_t)hyp, (uint32_t)d) * (uint32_t)(K - d)) >> 32);
        if (d >= 1 && r >= o0) ++r;
        if (d >= 2 && r >= o1) ++r;
        if (d >= 3 && r >= o2) ++r;
        s[d] = r;
        // insert r into (o0, o1, o2)
        if (d == 0) o0 = r;
        else if (d == 1) { if (r < o0) { o1 = o0; o0 = r; } else o1 = r; }
        else if (d == 2) {
            if (r < o0) { o2 = o1; o1 = o0; o0 = r; }
            else if (r < o1) { o2 = o1; o1 = r; }
            else o2 = r;
        }
    }
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

__device__ __forceinline__ bool is_inlier(const float h[9], float4 c, float th2) {
    const float w = h[6] * c.x + h[7] * c.y + h[8];
    const float iw = 1.f / w;
    const float dx = (h[0] * c.x + h[1] * c.y + h[2]) * iw - c.z;
    const float dy = (h[3] * c.x + h[4] * c.y + h[5]) * iw - c.w;
    return (w > 0.f) && isfinite(w) && (dx * dx + dy * dy < th2);      // a NaN error compares false
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

// ---- kernels ----------------------------------------------------------------------------------------------------------
// ordered compaction of the matches of one pair (ascending i); a match index outside [0, N) counts as no match
__global__ __launch_bounds__(256) void h_compact_kernel(const float* kp0, const float* kp1, const int64_t* m0, Ws w,
                                                        int M, int N) {
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
    if (t < T && K >= 4) {
        sample4(seed, b, t, K, s);
        float4 c[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) c[d] = corr[s[d]];
        ok = fit4(c, h);
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = 0.f;                   // w = 0: nothing is an inlier
    }
    if (samples != nullptr && t < T) {
        int* sp = samples + ((int64_t)b * T + t) * 4;
#pragma unroll
        for (int d = 0; d < 4; ++d) sp[d] = s[d];
    }
    int count = 0;
    for (int k0 = 0; k0 < K; k0 += TILE) {
        const int n = min(TILE, K - k0);
        __syncthreads();
        for (int k = tid; k < n; k += 256) tile[k] = corr[k0 + k];
        __syncthreads();
        for (int k = 0; k < n; ++k) count += is_inlier(h, tile[k], th2) ? 1 : 0;
    }
    if (hyp_counts != nullptr && t < T) hyp_counts[(int64_t)b * T + t] = ok ? count : -1;
    // key: (count + 1) in the high word (0 = rejected), ~index in the low word: the maximum key is the highest count at
    // the lowest index
    unsigned long long key = ok ? (((unsigned long long)(uint32_t)(count + 1) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)t)) : 0ull;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d);
        key = o > key ? o : key;
    }
    if ((tid & 63) == 0) red[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = red[0];
        for (int q = 1; q < 4; ++q) m = red[q] > m ? red[q] : m;
        w.best[(int64_t)b * nblk + blk] = m;
    }
}

// flags and count of model h over the ordered matches of pair b; the count is returned in every lane
__device__ __forceinline__ int flag_pass(const float* h, const float4* corr, uint8_t* flags, int K, float th2, int* red) {
    int count = 0;
    for (int k = threadIdx.x; k < K; k += 256) {
        const bool in = is_inlier(h, corr[k], th2);
        if (flags != nullptr) flags[k] = in ? 1 : 0;
        count += in ? 1 : 0;
    }
    return block_sum_int(count, red);
}

// winner of the pair's workgroups -> current model, its flags and its count
__global__ __launch_bounds__(256) void h_select_kernel(Ws w, int M, int nblk, float th2, uint32_t seed) {
    __shared__ unsigned long long red[4];
    __shared__ int ired[4];
    __shared__ float hs[9];
    __shared__ int oks;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = w.K[b];
    const float4* corr = w.corr + (int64_t)b * M;
    unsigned long long key = 0ull;
    for (int q = tid; q < nblk; q += 256) {
        const unsigned long long o = w.best[(int64_t)b * nblk + q];
        key = o > key ? o : key;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d);
        key = o > key ? o : key;
    }
    if ((tid & 63) == 0) red[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = red[0];
        for (int q = 1; q < 4; ++q) m = red[q] > m ? red[q] : m;
        float h[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        bool ok = false;
        if (m != 0ull && K >= 4) {
            const int t = (int)(0xFFFFFFFFu - (uint32_t)(m & 0xFFFFFFFFull));
            int s[4];
            sample4(seed, b, t, K, s);
            float4 c[4];
            for (int d = 0; d < 4; ++d) c[d] = corr[s[d]];
            ok = fit4(c, h);                              // the same arithmetic as the scoring lane's
        }
        for (int i = 0; i < 9; ++i) hs[i] = ok ? h[i] : (i % 4 == 0 ? 1.f : 0.f);
        oks = ok ? 1 : 0;
    }
    __syncthreads();
    const bool ok = oks != 0;
    float h[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = ok ? hs[i] : 0.f;          // an all-zero model flags nothing
    const int count = flag_pass(h, corr, w.flags + (int64_t)b * M, K, th2, ired);
    if (tid < 9) w.Hcur[(int64_t)b * 12 + tid] = hs[tid];
    if (tid == 0) {
        w.state[b * 4 + 0] = count;
        w.state[b * 4 + 1] = ok ? 1 : 0;
        w.state[b * 4 + 2] = 0;
    }
}

// Hartley-normalised weighted DLT over the flagged matches (use_flags == 0: over all of them) -> Hnew, state[2]
__global__ __launch_bounds__(256) void h_refit_kernel(Ws w, const float* weights, int M, int use_flags, int gate) {
    __shared__ double red[4 * 45];
    __shared__ double A[9][9], V[9][9];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = w.K[b];
    const float4* corr = w.corr + (int64_t)b * M;
    const uint8_t* flags = w.flags + (int64_t)b * M;
    const int* idx = w.idx + (int64_t)b * M;
    float* Hn = w.Hnew + (int64_t)b * 12;
    // gate: refit only where the pair has a current model (the local optimisation of gf_h_ransac)
    const bool live = gate == 0 || w.state[b * 4 + 1] != 0;
    auto fail = [&]() {
        if (tid < 9) Hn[tid] = (tid % 4 == 0) ? 1.f : 0.f;
        if (tid == 0) w.state[b * 4 + 2] = 0;
    };
    // pass 1: count and centroids
    double s5[5] = {0., 0., 0., 0., 0.};
    if (live)
        for (int k = tid; k < K; k += 256)
            if (!use_flags || flags[k]) {
                const float4 c = corr[k];
                s5[0] += 1.; s5[1] += c.x; s5[2] += c.y; s5[3] += c.z; s5[4] += c.w;
            }
    block_sum_f64<5>(s5, red);
    const double n = s5[0];
    if (!(n >= 4.)) { fail(); return; }                             // uniform over the workgroup
    const double cx0 = s5[1] / n, cy0 = s5[2] / n, cx1 = s5[3] / n, cy1 = s5[4] / n;
    // pass 2: mean distances to the centroids
    double s2[2] = {0., 0.};
    for (int k = tid; k < K; k += 256)
        if (!use_flags || flags[k]) {
            const float4 c = corr[k];
            const double dx0 = c.x - cx0, dy0 = c.y - cy0, dx1 = c.z - cx1, dy1 = c.w - cy1;
            s2[0] += sqrt(dx0 * dx0 + dy0 * dy0);
            s2[1] += sqrt(dx1 * dx1 + dy1 * dy1);
        }
    block_sum_f64<2>(s2, red);
    const double sc0 = 1.4142135623730951 / (s2[0] / n), sc1 = 1.4142135623730951 / (s2[1] / n);
    // pass 3: the 45 distinct sums of A^T W A
    double acc[45];
#pragma unroll
    for (int i = 0; i < 45; ++i) acc[i] = 0.;
    for (int k = tid; k < K; k += 256)
        if (!use_flags || flags[k]) {
            const float4 c = corr[k];
            const double wt = weights != nullptr ? (double)weights[(int64_t)b * M + idx[k]] : 1.;
            const double x = (c.x - cx0) * sc0, y = (c.y - cy0) * sc0, u = (c.z - cx1) * sc1, v = (c.w - cy1) * sc1;
            const double r0[9] = {0., 0., 0., -x, -y, -1., v * x, v * y, v};
            const double r1[9] = {x, y, 1., 0., 0., 0., -u * x, -u * y, -u};
            int at = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#pragma unroll
                for (int j = i; j < 9; ++j) { acc[at] += wt * (r0[i] * r0[j] + r1[i] * r1[j]); ++at; }
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
    gf_jacobi9(A, V, JACOBI_SWEEPS, tid);       // lane k < 9 owns row k of A (kept symmetric) and of V
    if (tid == 0) {
        int best = 0;
        for (int i = 1; i < 9; ++i)
            if (A[i][i] < A[best][best]) best = i;
        double g[9];
        for (int i = 0; i < 9; ++i) g[i] = V[i][best];
        // H = T1^-1 G T0 with T0 = [[s0, 0, -s0 cx0], [0, s0, -s0 cy0], [0, 0, 1]], T1^-1 = [[1/s1, 0, cx1], [0, 1/s1, cy1], [0, 0, 1]]
        double m[9];
        for (int r = 0; r < 3; ++r) {
            m[3 * r + 0] = g[3 * r + 0] * sc0;
            m[3 * r + 1] = g[3 * r + 1] * sc0;
            m[3 * r + 2] = g[3 * r + 2] - sc0 * (g[3 * r + 0] * cx0 + g[3 * r + 1] * cy0);
        }
        double hh[9];
        for (int c = 0; c < 3; ++c) {
            hh[0 + c] = m[0 + c] / sc1 + cx1 * m[6 + c];
            hh[3 + c] = m[3 + c] / sc1 + cy1 * m[6 + c];
            hh[6 + c] = m[6 + c];
        }
        double fro = 0.;
        for (int i = 0; i < 9; ++i) fro += hh[i] * hh[i];
        bool ok = fabs(hh[8]) >= (double)GF_H_H22_FRAC * sqrt(fro);
        float out[9];
        for (int i = 0; i < 9; ++i) { out[i] = (float)(hh[i] / hh[8]); ok = ok && isfinite(out[i]); }
        for (int i = 0; i < 9; ++i) Hn[i] = ok ? out[i] : (i % 4 == 0 ? 1.f : 0.f);
        w.state[b * 4 + 2] = ok ? 1 : 0;
    }
}

// rescore the refit; it replaces the current model when it is valid and its count does not drop
__global__ __launch_bounds__(256) void h_rescore_kernel(Ws w, int M, float th2) {
    __shared__ int ired[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (w.state[b * 4 + 1] == 0 || w.state[b * 4 + 2] == 0) return;           // uniform
    const int K = w.K[b];
    const float4* corr = w.corr + (int64_t)b * M;
    float h[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = w.Hnew[(int64_t)b * 12 + i];
    const int count = flag_pass(h, corr, nullptr, K, th2, ired);
    if (count < w.state[b * 4 + 0]) return;                                   // uniform
    flag_pass(h, corr, w.flags + (int64_t)b * M, K, th2, ired);
    __syncthreads();
    if (tid < 9) w.Hcur[(int64_t)b * 12 + tid] = h[tid];
    if (tid == 0) w.state[b * 4 + 0] = count;
}

// outputs.  ransac != 0: the current model, its flags scattered to the keypoints of view 0, its count; else the refit alone
__global__ __launch_bounds__(256) void h_final_kernel(Ws w, int M, int ransac, float* H, uint8_t* inliers, int* num_inliers,
                                                      uint8_t* success) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool ok = w.state[b * 4 + (ransac ? 1 : 2)] != 0;
    const float* src = (ransac ? w.Hcur : w.Hnew) + (int64_t)b * 12;
    if (tid < 9) H[(int64_t)b * 9 + tid] = ok ? src[tid] : (tid % 4 == 0 ? 1.f : 0.f);
    if (tid == 0) {
        success[b] = ok ? 1 : 0;
        if (num_inliers != nullptr) num_inliers[b] = (ok && ransac) ? w.state[b * 4 + 0] : 0;
    }
    if (inliers == nullptr) return;
    for (int i = tid; i < M; i += 256) inliers[(int64_t)b * M + i] = 0;
    __syncthreads();
    if (!ok) return;
    const int K = w.K[b];
    for (int k = tid; k < K; k += 256)
        if (w.flags[(int64_t)b * M + k]) inliers[(int64_t)b * M + w.idx[(int64_t)b * M + k]] = 1;
}

inline int check_common(const void* kp0, const void* kp1, const void* m0, int B, int M, int N, int T, const void* ws,
                        int64_t ws_bytes) {
    if (B <= 0 || M <= 0 || N <= 0 || T < 1) return GF_ERR_SHAPE;
    if (kp0 == nullptr || kp1 == nullptr || m0 == nullptr || ws == nullptr) return GF_ERR_SHAPE;
    if ((int64_t)B * nblk_of(T) >= ((int64_t)1 << 31) || (int64_t)B * T >= ((int64_t)1 << 31)) return GF_ERR_UNSUPPORTED;
    if (ws_bytes < (int64_t)carve(nullptr, B, M, T, nullptr)) return GF_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(ws) % 16 != 0) return GF_ERR_ALIGN;
    return 0;
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
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
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
    return (int)hipGetLastError();
}

extern "C" int gf_h_dlt(const float* kpts0, const float* kpts1, const int64_t* matches0, const float* weights, int B, int M,
                        int N, void* ws, int64_t ws_bytes, float* H, uint8_t* success, void* stream) {
    if (int e = check_common(kpts0, kpts1, matches0, B, M, N, 1, ws, ws_bytes)) return e;
    if (H == nullptr || success == nullptr) return GF_ERR_SHAPE;
    Ws w;
    carve(ws, B, M, 1, &w);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    h_compact_kernel<<<dim3(B), dim3(256), 0, st>>>(kpts0, kpts1, matches0, w, M, N);
    h_refit_kernel<<<dim3(B), dim3(256), 0, st>>>(w, weights, M, 0, 0);
    h_final_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, 0, H, nullptr, nullptr, success);
    return (int)hipGetLastError();
}
