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
// counts K_p, K_l from the workspace.  The skeleton is ransac_common.h, run over two parts (the points, then the lines); the
// point side of the model (inlier rule, DLT rows, the tail of the refit) is h_model.h, shared with h_solver.hip; what is here
// is the rest of the model: the fit's inputs, the line inlier rule and the line side of the refit.
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
// GF_HL_TILE, then lines (endpoints and line side by side, a tile of twice the bytes), all as broadcast reads.  The lane that
// holds its workgroup's best key leaves its model in the workspace, so the select kernel fits nothing again.
//
// Refit, fp64.  Hartley normalisation (centroid, mean distance sqrt 2) of view 0 over the flagged points and the endpoints
// p, q of the flagged lines, of view 1 over the flagged points and the endpoints r, s of the flagged lines.  Two rows per
// flagged feature: a point's two DLT rows; a line's rows (a x, a y, a, b x, b y, b, c x, c y, c) at p' and q' with (a, b, c) the
// unit-normal line through the normalised r', s'.  The 45 sums, GF_HL_JACOBI sweeps of gf_jacobi9, H = T1^-1 G T0, h22 = 1.
// At least 4 flagged features.  The rescore replaces the current model only when the refit is valid and the total count
// does not drop.
#include "hl_fit.h"
#include "h_model.h"

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

struct Inlier : TransferInlier {                                   // a point match by gf_h_ransac's rule
    using TransferInlier::operator();
    __device__ __forceinline__ bool operator()(const float* h, LineFeature f, float th) const {
        const float4 e = f.e, l = f.l;
        const float w0 = h[6] * e.x + h[7] * e.y + h[8], w1 = h[6] * e.z + h[7] * e.w + h[8];
        const float i0 = 1.f / w0, i1 = 1.f / w1;
        const float d0 = l.x * ((h[0] * e.x + h[1] * e.y + h[2]) * i0) + l.y * ((h[3] * e.x + h[4] * e.y + h[5]) * i0) + l.z;
        const float d1 = l.x * ((h[0] * e.z + h[1] * e.w + h[2]) * i1) + l.y * ((h[3] * e.z + h[4] * e.w + h[5]) * i1) + l.z;
        // max(|d0|, |d1|) < th as two comparisons: a NaN distance compares false (fmaxf would drop it)
        return (w0 > 0.f) && (w1 > 0.f) && isfinite(w0) && isfinite(w1) && (fabsf(d0) < th) && (fabsf(d1) < th);
    }
};

// the line part of the refit: the flagged line matches k < K; each has two points per view, the endpoints
struct LineRefit {
    const float4* seg;
    const uint8_t* flags;
    int K;
    __device__ __forceinline__ bool keep(int k) const { return flags[k] != 0; }
    __device__ __forceinline__ void moments(int k, double (&s)[6]) const {
        const float4 e = seg[2 * k], g = seg[2 * k + 1];
        s[0] += 1.; s[1] += 2.; s[2] += (double)e.x + e.z; s[3] += (double)e.y + e.w;
        s[4] += (double)g.x + g.z; s[5] += (double)g.y + g.w;
    }
    __device__ __forceinline__ void spread(int k, const Hartley& t, double (&s)[2]) const {
        auto dist = [](double x, double y, double cx, double cy) { return sqrt((x - cx) * (x - cx) + (y - cy) * (y - cy)); };
        const float4 e = seg[2 * k], g = seg[2 * k + 1];
        s[0] += dist(e.x, e.y, t.cx0, t.cy0) + dist(e.z, e.w, t.cx0, t.cy0);
        s[1] += dist(g.x, g.y, t.cx1, t.cy1) + dist(g.z, g.w, t.cx1, t.cy1);
    }
    // rows (a x, a y, a, b x, b y, b, c x, c y, c) at p' and q' with (a, b, c) the unit-normal line through r', s'
    __device__ __forceinline__ void rows(int k, const Hartley& t, double (&acc)[45]) const {
        const float4 e = seg[2 * k], g = seg[2 * k + 1];
        const double x0 = (e.x - t.cx0) * t.sc0, y0 = (e.y - t.cy0) * t.sc0, x1 = (e.z - t.cx0) * t.sc0, y1 = (e.w - t.cy0) * t.sc0;
        const double u0 = (g.x - t.cx1) * t.sc1, v0 = (g.y - t.cy1) * t.sc1, u1 = (g.z - t.cx1) * t.sc1, v1 = (g.w - t.cy1) * t.sc1;
        const double la = v0 - v1, lb = u1 - u0, lc = u0 * v1 - u1 * v0;
        const double inv = 1. / sqrt(la * la + lb * lb);
        const double a = la * inv, bb = lb * inv, c = lc * inv;
        const double r0[9] = {a * x0, a * y0, a, bb * x0, bb * y0, bb, c * x0, c * y0, c};
        const double r1[9] = {a * x1, a * y1, a, bb * x1, bb * y1, bb, c * x1, c * y1, c};
        add_rows<false>(acc, r0, r1);
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
    __shared__ LineFeature tile[TILE];                            // the point pass uses the first half
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
    const int np = tile_count<TILE>(h, PointPart{corr, nullptr, Kp, th * th}, reinterpret_cast<float4*>(tile), Inlier());
    const int nl = tile_count<TILE>(h, LinePart{seg, line, nullptr, Kl, th}, tile, Inlier());
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
    set_current(w.p, b, h, hs, ok, ired, Inlier(), point_part(w.p, b, M, th * th), line_part(w.l, b, L, th));
}

// Hartley-normalised DLT over the flagged points and lines of the current model -> refit, state[ST_REFIT_OK]
__global__ __launch_bounds__(256) void hl_refit_kernel(Ws w, int M, int L) {
    __shared__ double red[4 * 45];
    __shared__ double A[9][9], V[9][9];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint8_t* pf = w.p.flags + (int64_t)b * M;
    float* Hn = w.p.refit + (int64_t)b * 12;
    int* refit_ok = w.p.state + b * 4 + ST_REFIT_OK;
    const bool have = w.p.state[b * 4 + ST_CUR_OK] != 0;            // nothing is kept where the pair has no current model
    const auto pts = point_refit(
        w.p.corr + (int64_t)b * M, have ? w.p.K[b] : 0, [=](int k) { return pf[k] != 0; },
        [](double (&acc)[45], int, double x, double y, double u, double v) { add_point_rows<false>(acc, x, y, u, v); });
    const LineRefit lns{w.l.seg + 2 * (int64_t)b * L, w.l.flags + (int64_t)b * L, have ? w.l.K[b] : 0};
    Hartley t;
    refit_moments(red, t, pts, lns);
    if (!(t.n >= 4.)) {                                             // uniform over the workgroup
        h_refit_none(Hn, refit_ok);
        return;
    }
    double m[9];
    refit_solve(red, A, V, GF_HL_JACOBI, t, m, pts, lns);
    if (tid == 0) h_refit_tail(m, t, (double)GF_HL_H22_FRAC, Hn, refit_ok);
}

__global__ __launch_bounds__(256) void hl_rescore_kernel(Ws w, int M, int L, float th) {
    __shared__ int ired[4];
    const int b = blockIdx.x;
    rescore_pair(w.p, b, ired, Inlier(), point_part(w.p, b, M, th * th), line_part(w.l, b, L, th));
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
    if (M > 0) scatter_flags(w.p.flags + (int64_t)b * M, w.p.idx + (int64_t)b * M, w.p.K[b], M, ok, inliers + (int64_t)b * M);
    __syncthreads();
    if (L > 0)
        scatter_flags(w.l.flags + (int64_t)b * L, w.l.idx + (int64_t)b * L, w.l.K[b], L, ok, line_inliers + (int64_t)b * L);
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
    if ((int64_t)M + L >= ((int64_t)1 << 31)) return GF_ERR_UNSUPPORTED;
    if (int e = ws_check(B, ws, ws_bytes, nblk, T, carve(nullptr, B, M, L, T, nullptr))) return e;
    if (!(ransac_th > 0.f) || !(ransac_th < 1e18f) || lo_iters < 0 || lo_iters > 64) return GF_ERR_SHAPE;
    Ws w;
    carve(ws, B, M, L, T, &w);
    hipStream_t st = gf_stream(stream);
    hl_compact_kernel<<<dim3(B), dim3(256), 0, st>>>(kpts0, kpts1, matches0, lines0, lines1, line_matches0, w, M, N, L, L1);
    hl_score_kernel<<<dim3((unsigned)(B * nblk)), dim3(256), 0, st>>>(w, M, L, T, (int)nblk, ransac_th, seed, samples, hyp_H,
                                                                      hyp_counts);
    hl_select_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, L, (int)nblk, ransac_th);
    for (int it = 0; it < lo_iters; ++it) {
        hl_refit_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, L);
        hl_rescore_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, L, ransac_th);
    }
    hl_final_kernel<<<dim3(B), dim3(256), 0, st>>>(w, M, L, H, inliers, line_inliers, num_inliers, success);
    return gf_launched();
}
