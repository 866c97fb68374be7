// Point-and-line homography solver: batched RANSAC whose hypotheses are drawn from point matches, line matches or a mix of
// both, Hartley-normalised DLT refit over both kinds, local optimisation.
//
// Fills the place of the reference's hybrid estimator (gluefactory/robust_estimators/homography/homography_est.py, selected by
// `estimator: homography_est` in configs/superpoint+lsd+gluestick.yaml and fed m_lines0 / m_lines1 by eval/utils.py:197-238).
// That estimator is a CPU C++ package this project cannot install, so nothing here was compared against it: THE SEMANTICS
// BELOW AND IN hl_fit.h ARE THE DEFINITION OF THIS SOLVER, not a restatement of that library.  The yardstick is the fp64
// numpy restatement of this text in tests/hl_solver_cases.py.
//
// A call is a fixed chain of kernels on one stream, 4 + 2 lo_iters launches (compact, score, select, lo_iters x (refit,
// rescore), outputs), one workgroup of 256 lanes per pair except the scoring kernel (one workgroup per GF_HL_HYPS hypotheses
// of a pair, one hypothesis per lane).  Kernel nodes only, nothing allocated, no host read: every kernel takes the pair's
// counts K_p, K_l from the workspace.  The skeleton is ransac_common.h (its two-part templates); what is here is the model.
//
// Compaction.  Point matches exactly as compact_pair orders them (ascending i, an index outside [0, N) is no match).  Line
// match i is j = line_matches0[b, i] with 0 <= j < L1: the endpoints p, q of segment i of view 0 and r, s of segment j of
// view 1; it counts as no match where a coordinate is non-finite or either segment is shorter than GF_HL_EPS_LEN pixels
// (lengths in fp64).  The unit-normal view-1 line (a, b, c) = (-(sy - ry), sx - rx, rx sy - sx ry) / |s - r| is computed once,
// in fp64, and kept in fp32.
//
// Sampling.  One sample_distinct<4> draw per hypothesis over K = K_p + K_l (the rule in the header of ransac_common.h): index
// s < K_p is ordered point match s, otherwise ordered line match s - K_p.  K < 4: no model.
//
// Fit: hl_fit.h (fp64 in the lane, the sample's own frame, 8 x 9 Gauss-Jordan with full pivoting, the rejections).
//
// Scoring, fp32.  A point match is an inlier by gf_h_ransac's rule: w = h20 x + h21 y + h22 finite and > 0 and
// |(H x0) / w - x1|^2 < th^2.  A line match is an inlier when w(p) and w(q) are finite and > 0 and
// max(|l . pi(H p)|, |l . pi(H q)|) < th  with l . (X, Y) = a X + b Y + c.  A hypothesis' score is the integer point inliers +
// line inliers; the winner key and the tie rule (lowest index) are pack_key's.  Points stream through LDS in tiles of
// GF_HL_TILE, then lines (endpoints and line, two tiles), all as broadcast reads.  The lane that holds its workgroup's best key
// leaves its model in the workspace, so the select kernel fits nothing again.
//
// Refit, fp64.  Hartley normalisation (centroid, mean distance sqrt 2) of view 0 over the flagged points and the endpoints
// p, q of the flagged lines, of view 1 over the flagged points and the endpoints r, s of the flagged lines.  Two rows per
// flagged feature: a point's two DLT rows; a line's rows (a x, a y, a, b x, b y, b, c x, c y, c) at p' and q' with (a, b, c) the
// unit-normal line through the normalised r', s'.  The 45 sums, GF_HL_JACOBI sweeps of gf_jacobi9, H = T1^-1 G T0, h22 = 1.
// At least 4 flagged features.  The rescore replaces the current model only when the refit is valid and the total count
// does not drop.
#include "hl_fit.h"
#include "ransac_common.h"

namespace {

constexpr int TILE = GF_HL_TILE;
constexpr int HYPS = GF_HL_HYPS;
static_assert(HYPS == 256, "one hypothesis per lane of a 256-lane workgroup");

struct Ws {
    RansacWs p;                 // the point part, the models, the keys and the state
    LineWs l;                   // the line part
    float* blk_model;           // [B, nblk, 12] model of the best key of every scoring workgroup (9 used)
};

inline int nblk_of(int T) { return (T + HYPS - 1) / HYPS; }

inline size_t carve(void* base, int B, int M, int L, int T, Ws* w) {
    Carver c{reinterpret_cast<char*>(base)};
    Ws t;
    carve_core(c, B, M, nblk_of(T), t.p);
    carve_lines(c, B, L, t.l);
    t.blk_model = c.take<float>(12 * (size_t)B * nblk_of(T));
    if (w) *w = t;
    return c.off;
}

struct PointInlier {
    __device__ __forceinline__ bool operator()(const float* h, float4 c, float th2) const {
        const float w = h[6] * c.x + h[7] * c.y + h[8];
        const float iw = 1.f / w;
        const float dx = (h[0] * c.x + h[1] * c.y + h[2]) * iw - c.z;
        const float dy = (h[3] * c.x + h[4] * c.y + h[5]) * iw - c.w;
        return (w > 0.f) && isfinite(w) && (dx * dx + dy * dy < th2);      // a NaN error compares false
    }
};

struct LineInlier {
    __device__ __forceinline__ bool operator()(const float* h, float4 e, float4 l, float th) const {
        const float w0 = h[6] * e.x + h[7] * e.y + h[8], w1 = h[6] * e.z + h[7] * e.w + h[8];
        const float i0 = 1.f / w0, i1 = 1.f / w1;
        const float d0 = l.x * ((h[0] * e.x + h[1] * e.y + h[2]) * i0) + l.y * ((h[3] * e.x + h[4] * e.y + h[5]) * i0) + l.z;
        const float d1 = l.x * ((h[0] * e.z + h[1] * e.w + h[2]) * i1) + l.y * ((h[3] * e.z + h[4] * e.w + h[5]) * i1) + l.z;
        // max(|d0|, |d1|) < th as two comparisons: a NaN distance compares false (fmaxf would drop it)
        return (w0 > 0.f) && (w1 > 0.f) && isfinite(w0) && isfinite(w1) && (fabsf(d0) < th) && (fabsf(d1) < th);
    }
};

// ---- kernels ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hl_compact_kernel(const float* kp0, const float* kp1, const int64_t* m0, const float* l0,
                                                         const float* l1, const int64_t* lm0, Ws w, int M, int N, int L, int L1) {
    __shared__ int wsum[4];
    compact_pair(kp0, kp1, m0, w.p, blockIdx.x, M, N, wsum);          // M == 0: K_p = 0, nothing is read
    __syncthreads();
    compact_lines(l0, l1, lm0, w.l, blockIdx.x, L, L1, (double)GF_HL_EPS_LEN, wsum);
}

// one hypothesis per lane: sample, fit, count inliers over the pair's points and lines; the workgroup's best key and its model
// to the workspace
__global__ __launch_bounds__(256) void hl_score_kernel(Ws w, int M, int L, int T, int nblk, float th, uint32_t seed,
                                                       int* samples, float* hyp_H, int* hyp_counts) {
    __shared__ float4 tile[TILE];
    __shared__ float4 tile_l[TILE];
    __shared__ unsigned long long red[4];
    const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk, tid = threadIdx.x;
    const int t = blk * HYPS + tid;
    const int Kp = w.p.K[b], Kl = w.l.K[b], K = Kp + Kl;
    const float4* corr = w.p.corr + (int64_t)b * M;
    const float4* seg = w.l.seg + 2 * (int64_t)b * L;
    const float4* line = w.l.line + (int64_t)b * L;
    float h[9];
    bool ok = false;
    int s[4] = {-1, -1, -1, -1};
    if (t < T && K >= 4) {
        sample_distinct<4>(seed, b, t, K, s);
        double f[4][8];
        bool isl[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            isl[d] = s[d] >= Kp;
            float4 a, c;
            if (isl[d]) {
                a = seg[2 * (s[d] - Kp)];
                c = seg[2 * (s[d] - Kp) + 1];
            } else {
                const float4 pc = corr[s[d]];
                a = make_float4(pc.x, pc.y, pc.x, pc.y);
                c = make_float4(pc.z, pc.w, pc.z, pc.w);
            }
            f[d][0] = a.x; f[d][1] = a.y; f[d][2] = a.z; f[d][3] = a.w;
            f[d][4] = c.x; f[d][5] = c.y; f[d][6] = c.z; f[d][7] = c.w;
        }
        ok = gf_hl::fit(f, isl, h);
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
    if (hyp_H != nullptr && t < T) {
        float* hp = hyp_H + ((int64_t)b * T + t) * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) hp[i] = h[i];
    }
    const int np = tile_count<TILE>(h, corr, Kp, th * th, tile, PointInlier());
    const int nl = tile_count_lines<TILE>(h, seg, line, Kl, th, tile, tile_l, LineInlier());
    if (hyp_counts != nullptr && t < T) {
        hyp_counts[((int64_t)b * T + t) * 2] = ok ? np : -1;
        hyp_counts[((int64_t)b * T + t) * 2 + 1] = ok ? nl : -1;
    }
    const unsigned long long key = pack_key(ok, np + nl, t);
    const unsigned long long m = block_max_key(key, red);
    if (tid == 0) w.p.best[(int64_t)b * nblk + blk] = m;
    if (ok && key == m) {                                          // keys of accepted lanes are distinct: one lane
        float* bm = w.blk_model + ((int64_t)b * nblk + blk) * 12;
#pragma unroll
        for (int i = 0; i < 9; ++i) bm[i] = h[i];
    }
}

// winner of the pair's workgroups -> current model, its flags and its counts
__global__ __launch_bounds__(256) void hl_select_kernel(Ws w, int M, int L, int nblk, float th) {
    __shared__ unsigned long long red[4];
    __shared__ int ired[4];
    __shared__ float hs[9];
    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned long long m = pair_max_key(w.p, b, nblk, red);
    const bool ok = m != 0ull;
    if (tid < 9) hs[tid] = ok ? w.blk_model[((int64_t)b * nblk + key_index(m) / HYPS) * 12 + tid] : (tid % 4 == 0 ? 1.f : 0.f);
    __syncthreads();
    float h[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = ok ? hs[i] : 0.f;          // an all-zero model flags nothing
    set_current2(w.p, w.l, b, M, L, h, hs, ok, th, ired, PointInlier(), LineInlier());
}

// Hartley-normalised DLT over the flagged points and lines of the current model -> refit, state[ST_REFIT_OK]
__global__ __launch_bounds__(256) void hl_refit_kernel(Ws w, int M, int L) {
    __shared__ double red[4 * 45];
    __shared__ double A[9][9], V[9][9];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float4* corr = w.p.corr + (int64_t)b * M;
    const float4* seg = w.l.seg + 2 * (int64_t)b * L;
    const uint8_t* pf = w.p.flags + (int64_t)b * M;
    const uint8_t* lf = w.l.flags + (int64_t)b * L;
    float* Hn = w.p.refit + (int64_t)b * 12;
    const bool have = w.p.state[b * 4 + ST_CUR_OK] != 0;            // nothing is kept where the pair has no current model
    const int Kp = have ? w.p.K[b] : 0, Kl = have ? w.l.K[b] : 0;
    // pass 1: the feature count, the point count (a line has two) and the centroids
    double s6[6] = {0., 0., 0., 0., 0., 0.};
    for (int k = tid; k < Kp; k += 256)
        if (pf[k]) {
            const float4 c = corr[k];
            s6[0] += 1.; s6[1] += 1.; s6[2] += c.x; s6[3] += c.y; s6[4] += c.z; s6[5] += c.w;
        }
    for (int k = tid; k < Kl; k += 256)
        if (lf[k]) {
            const float4 e = seg[2 * k], g = seg[2 * k + 1];
            s6[0] += 1.; s6[1] += 2.; s6[2] += (double)e.x + e.z; s6[3] += (double)e.y + e.w;
            s6[4] += (double)g.x + g.z; s6[5] += (double)g.y + g.w;
        }
    block_sum_f64<6>(s6, red);
    if (!(s6[0] >= 4.)) {                                           // uniform over the workgroup
        if (tid < 9) Hn[tid] = (tid % 4 == 0) ? 1.f : 0.f;
        if (tid == 0) w.p.state[b * 4 + ST_REFIT_OK] = 0;
        return;
    }
    const double npts = s6[1], cx0 = s6[2] / npts, cy0 = s6[3] / npts, cx1 = s6[4] / npts, cy1 = s6[5] / npts;
    // pass 2: mean distances to the centroids
    double s2[2] = {0., 0.};
    auto dist = [](double x, double y, double cx, double cy) { return sqrt((x - cx) * (x - cx) + (y - cy) * (y - cy)); };
    for (int k = tid; k < Kp; k += 256)
        if (pf[k]) {
            const float4 c = corr[k];
            s2[0] += dist(c.x, c.y, cx0, cy0);
            s2[1] += dist(c.z, c.w, cx1, cy1);
        }
    for (int k = tid; k < Kl; k += 256)
        if (lf[k]) {
            const float4 e = seg[2 * k], g = seg[2 * k + 1];
            s2[0] += dist(e.x, e.y, cx0, cy0) + dist(e.z, e.w, cx0, cy0);
            s2[1] += dist(g.x, g.y, cx1, cy1) + dist(g.z, g.w, cx1, cy1);
        }
    block_sum_f64<2>(s2, red);
    const double sc0 = 1.4142135623730951 / (s2[0] / npts), sc1 = 1.4142135623730951 / (s2[1] / npts);
    // pass 3: the 45 distinct sums of the normal matrix
    double acc[45];
#pragma unroll
    for (int i = 0; i < 45; ++i) acc[i] = 0.;
    auto add = [&](const double (&r0)[9], const double (&r1)[9]) {
        int at = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int j = i; j < 9; ++j) { acc[at] += r0[i] * r0[j] + r1[i] * r1[j]; ++at; }
    };
    for (int k = tid; k < Kp; k += 256)
        if (pf[k]) {
            const float4 c = corr[k];
            const double x = (c.x - cx0) * sc0, y = (c.y - cy0) * sc0, u = (c.z - cx1) * sc1, v = (c.w - cy1) * sc1;
            const double r0[9] = {0., 0., 0., -x, -y, -1., v * x, v * y, v};
            const double r1[9] = {x, y, 1., 0., 0., 0., -u * x, -u * y, -u};
            add(r0, r1);
        }
    for (int k = tid; k < Kl; k += 256)
        if (lf[k]) {
            const float4 e = seg[2 * k], g = seg[2 * k + 1];
            const double x0 = (e.x - cx0) * sc0, y0 = (e.y - cy0) * sc0, x1 = (e.z - cx0) * sc0, y1 = (e.w - cy0) * sc0;
            const double u0 = (g.x - cx1) * sc1, v0 = (g.y - cy1) * sc1, u1 = (g.z - cx1) * sc1, v1 = (g.w - cy1) * sc1;
            const double la = v0 - v1, lb = u1 - u0, lc = u0 * v1 - u1 * v0;
            const double inv = 1. / sqrt(la * la + lb * lb);
            const double a = la * inv, bb = lb * inv, c = lc * inv;
            const double r0[9] = {a * x0, a * y0, a, bb * x0, bb * y0, bb, c * x0, c * y0, c};
            const double r1[9] = {a * x1, a * y1, a, bb * x1, bb * y1, bb, c * x1, c * y1, c};
            add(r0, r1);
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
    gf_jacobi9(A, V, GF_HL_JACOBI, tid);
    if (tid == 0) {
        int best = 0;
        for (int i = 1; i < 9; ++i)
            if (A[i][i] < A[best][best]) best = i;
        double g[9], m[9], hh[9];
        for (int i = 0; i < 9; ++i) g[i] = V[i][best];
        for (int r = 0; r < 3; ++r) {                               // m = G T0
            m[3 * r + 0] = g[3 * r + 0] * sc0;
            m[3 * r + 1] = g[3 * r + 1] * sc0;
            m[3 * r + 2] = g[3 * r + 2] - sc0 * (g[3 * r + 0] * cx0 + g[3 * r + 1] * cy0);
        }
        for (int c = 0; c < 3; ++c) {                               // H = T1^-1 m
            hh[0 + c] = m[0 + c] / sc1 + cx1 * m[6 + c];
            hh[3 + c] = m[3 + c] / sc1 + cy1 * m[6 + c];
            hh[6 + c] = m[6 + c];
        }
        double fro = 0.;
        for (int i = 0; i < 9; ++i) fro += hh[i] * hh[i];
        bool ok = fabs(hh[8]) >= (double)GF_HL_H22_FRAC * sqrt(fro);
        float out[9];
        for (int i = 0; i < 9; ++i) { out[i] = (float)(hh[i] / hh[8]); ok = ok && isfinite(out[i]); }
        for (int i = 0; i < 9; ++i) Hn[i] = ok ? out[i] : (i % 4 == 0 ? 1.f : 0.f);
        w.p.state[b * 4 + ST_REFIT_OK] = ok ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void hl_rescore_kernel(Ws w, int M, int L, float th) {
    __shared__ int ired[4];
    rescore_pair2(w.p, w.l, blockIdx.x, M, L, th, ired, PointInlier(), LineInlier());
}

// outputs: the current model, its flags scattered to the keypoints and the segments of view 0, its counts
__global__ __launch_bounds__(256) void hl_final_kernel(Ws w, int M, int L, float* H, uint8_t* inliers, uint8_t* line_inliers,
                                                       int* num_inliers, uint8_t* success) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const bool ok = w.p.state[b * 4 + ST_CUR_OK] != 0;
    const float* src = w.p.cur + (int64_t)b * 12;
    if (tid < 9) H[(int64_t)b * 9 + tid] = ok ? src[tid] : (tid % 4 == 0 ? 1.f : 0.f);
    if (tid == 0) {
        success[b] = ok ? 1 : 0;
        const int total = w.p.state[b * 4 + ST_COUNT], nl = w.p.state[b * 4 + ST_LINES];
        num_inliers[2 * b] = ok ? total - nl : 0;
        num_inliers[2 * b + 1] = ok ? nl : 0;
    }
    if (M > 0) scatter_flags(w.p, b, M, ok, inliers);
    __syncthreads();
    if (L > 0) scatter_line_flags(w.l, b, L, ok, line_inliers);
}

inline bool sizes_ok(int B, int M, int L, int T) {
    return B > 0 && M >= 0 && L >= 0 && (int64_t)M + L > 0 && T >= 1;
}

}  // namespace

extern "C" int64_t gf_hl_ws_bytes(int B, int M, int L, int T) {
    if (!sizes_ok(B, M, L, T)) return 0;
    return (int64_t)carve(nullptr, B, M, L, T, nullptr);
}

extern "C" int gf_hl_ransac(const float* kpts0, const float* kpts1, const int64_t* matches0, const float* lines0,
                            const float* lines1, const int64_t* line_matches0, int B, int M, int N, int L, int L1, int T,
                            float ransac_th, int lo_iters, uint32_t seed, void* ws, int64_t ws_bytes, float* H,
                            uint8_t* inliers, uint8_t* line_inliers, int32_t* num_inliers, uint8_t* success, int32_t* samples,
                            float* hyp_H, int32_t* hyp_counts, void* stream) {
    if (!sizes_ok(B, M, L, T)) return GF_ERR_SHAPE;
    if (M > 0 && (N <= 0 || kpts0 == nullptr || kpts1 == nullptr || matches0 == nullptr || inliers == nullptr)) return GF_ERR_SHAPE;
    if (L > 0 && (L1 <= 0 || lines0 == nullptr || lines1 == nullptr || line_matches0 == nullptr || line_inliers == nullptr))
        return GF_ERR_SHAPE;
    if (ws == nullptr || H == nullptr || num_inliers == nullptr || success == nullptr) return GF_ERR_SHAPE;
    const int64_t nblk = nblk_of(T);
    if ((int64_t)B * nblk >= ((int64_t)1 << 31) || (int64_t)B * T >= ((int64_t)1 << 31) || (int64_t)M + L >= ((int64_t)1 << 31))
        return GF_ERR_UNSUPPORTED;
    if (ws_bytes < (int64_t)carve(nullptr, B, M, L, T, nullptr)) return GF_ERR_SHAPE;
    if (reinterpret_cast<uintptr_t>(ws) % 16 != 0) return GF_ERR_ALIGN;
    if (!(ransac_th > 0.f) || !(ransac_th < 1e18f) || lo_iters < 0 || lo_iters > 64) return GF_ERR_SHAPE;
    Ws w;
    carve(ws, B, M, L, T, &w);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hl_compact_kernel<<<dim3(B), dim3(256), 0, st>>>(kpts0, kpts1, matches0, lines0, lines1, line_matches0, w, M, N, L, L1);
    hl_score_kernel<<<dim3((unsigned)(B * nblk)), dim3(256), 0, st>>>(w, M, L, T, (int)nblk, ransac_th, seed, samples, hyp_H,
                                                                      hyp_counts);
    hl_select_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, L, (int)nblk, ransac_th);
    for (int it = 0; it < lo_iters; ++it) {
        hl_refit_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, L);
        hl_rescore_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, L, ransac_th);
    }
    hl_final_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, L, H, inliers, line_inliers, num_inliers, success);
    return (int)hipGetLastError();
}
