// RANSAC skeleton shared by the two-view solvers (h_solver.hip, e_solver.hip, hl_solver.hip): the workspace core, the counter-based
// sampling, the fixed-order block reductions and the winner key, ordered compaction, the tile-streamed inlier count, the flag
// pass and the rescore, the Hartley-normalised 9 x 9 refit and the flag scatter.  A solver supplies its inlier rule and the
// rows of its design matrix as functors and keeps its own __global__ kernels: one workgroup of 256 lanes per pair, except
// where its header says otherwise.  Nothing depends on a count the host reads: every piece takes the pair's match count K_b
// from the workspace.
//
// Sampling (restated on the host by tests/ransac_cases.py, bit for bit).  All arithmetic is uint32 with wrap-around:
//   hash(seed, pair, hyp, draw): x = seed * 0x9E3779B1 + pair * 0x85EBCA77 + hyp * 0xC2B2AE3D + draw * 0x27D4EB2F + 0x165667B1;
//                                x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16
//   draw d = 0..S-1 of a pair with K matches: r = (uint64(hash) * (K - d)) >> 32, i.e. uniform in [0, K - d); then the skip
//   mapping: the earlier draws are visited in ASCENDING order of their value p, and r += 1 whenever r >= p.  The S values are
//   distinct indices into the pair's ordered match list.
//
// Winner: a scoring lane packs (count + 1) into the high word of a 64-bit key (0 = no model) and ~index into the low word, so
// the maximum key is the highest count at the lowest index: deterministic, no floating-point atomics.
//
// Parts: a pair's features are one ordered list (points) or two (hl_solver.hip: points, then lines).  A part is the view of
// one such list that the count, the flag pass, the rescore and the refit run over; each of those exists once, over one part
// or over a pack of at most two, in part order.
//
// Refit: fp64 throughout.  Hartley normalisation over the points of the kept features (centroid, mean distance sqrt 2; a
// line has two points per view), the 45 distinct sums of the normal matrix through a fixed-order block reduction, cyclic
// Jacobi sweeps on the 9 x 9 matrix in LDS (gf_jacobi9.h), the eigenvector of the smallest eigenvalue, de-normalisation on
// the view-0 side.
#pragma once
#include "gf_launch.h"
#include "gf_jacobi9.h"

namespace {

// ---- workspace --------------------------------------------------------------------------------------------------------
struct RansacWs {
    int* K;                     // [B] matches of the pair
    int* idx;                   // [B, M] ordered indices of the matched keypoints of view 0
    float4* corr;               // [B, M] (x0, y0, x1, y1) of the ordered matches
    unsigned long long* best;   // [B, nblk] best key of every scoring workgroup
    float* cur;                 // [B, 12] current model (9 used)
    float* refit;               // [B, 12] refitted model
    int* state;                 // [B, 4] the words below
    uint8_t* flags;             // [B, M] inlier flags of the current model over the ordered matches
};
// words of state[b * 4 + .]
constexpr int ST_COUNT = 0;      // inlier count of the current model, over all parts
constexpr int ST_CUR_OK = 1;     // the pair has a current model
constexpr int ST_REFIT_OK = 2;   // the last refit gave a valid model
constexpr int ST_LINES = 3;      // the second part's share of ST_COUNT (two-part solvers only)

// The line part of a workspace whose point part is a RansacWs.  A line match is two view-0 endpoints p, q and two view-1
// endpoints r, s: seg[2 k] = (px, py, qx, qy), seg[2 k + 1] = (rx, ry, sx, sy); line[k] = (a, b, c, 0) is the view-1 line through
// r and s in pixels with a^2 + b^2 = 1.
struct LineWs {
    int* K;                     // [B] line matches of the pair
    int* idx;                   // [B, L] ordered indices of the matched segments of view 0
    float4* seg;                // [B, 2 L] endpoints of the ordered line matches
    float4* line;               // [B, L] unit-normal view-1 lines of the ordered line matches
    uint8_t* flags;             // [B, L] inlier flags of the current model over the ordered line matches
};

// hands out consecutive 16-byte aligned arrays of a buffer (a null buffer: only the size is wanted)
struct Carver {
    char* p;
    size_t off = 0;
    template <typename T> T* take(size_t count) {
        const size_t o = off;
        off = (off + sizeof(T) * count + 15) & ~(size_t)15;
        return reinterpret_cast<T*>(p + o);
    }
};

inline void carve_core(Carver& c, int B, int M, int64_t nblk, RansacWs& w) {
    w.K = c.take<int>((size_t)B);
    w.idx = c.take<int>((size_t)B * M);
    w.corr = c.take<float4>((size_t)B * M);
    w.best = c.take<unsigned long long>((size_t)B * nblk);
    w.cur = c.take<float>(12 * (size_t)B);
    w.refit = c.take<float>(12 * (size_t)B);
    w.state = c.take<int>(4 * (size_t)B);
    w.flags = c.take<uint8_t>((size_t)B * M);
}

inline void carve_lines(Carver& c, int B, int L, LineWs& w) {
    w.K = c.take<int>((size_t)B);
    w.idx = c.take<int>((size_t)B * L);
    w.seg = c.take<float4>(2 * (size_t)B * L);
    w.line = c.take<float4>((size_t)B * L);
    w.flags = c.take<uint8_t>((size_t)B * L);
}

// the workspace half of the argument checks: nblk scoring workgroups and `lanes` scoring lanes per pair, `need` workspace bytes
inline int ws_check(int B, const void* ws, int64_t ws_bytes, int64_t nblk, int64_t lanes, size_t need) {
    if ((int64_t)B * nblk >= ((int64_t)1 << 31) || (int64_t)B * lanes >= ((int64_t)1 << 31)) return GF_ERR_UNSUPPORTED;
    if (ws_bytes < (int64_t)need) return GF_ERR_SHAPE;
    if (!gf_aligned16(ws)) return GF_ERR_ALIGN;
    return 0;
}

// argument checks common to the entry points with one list, which may not be empty
inline int ransac_check(const void* p0, const void* p1, const void* m0, int B, int M, int N, int T, const void* ws,
                        int64_t ws_bytes, int64_t nblk, int64_t lanes, size_t need) {
    if (B <= 0 || M <= 0 || N <= 0 || T < 1) return GF_ERR_SHAPE;
    if (p0 == nullptr || p1 == nullptr || m0 == nullptr || ws == nullptr) return GF_ERR_SHAPE;
    return ws_check(B, ws, ws_bytes, nblk, lanes, need);
}

// ---- sampling ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t hash32(uint32_t seed, uint32_t pair, uint32_t hyp, uint32_t draw) {
    uint32_t x = seed * 0x9E3779B1u + pair * 0x85EBCA77u + hyp * 0xC2B2AE3Du + draw * 0x27D4EB2Fu + 0x165667B1u;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return x;
}

// S distinct indices in [0, K), K >= S
template <int S> __device__ __forceinline__ void sample_distinct(uint32_t seed, int pair, int hyp, int K, int s[S]) {
    int o[S];                                      // the earlier draws in ascending order
#pragma unroll
    for (int d = 0; d < S; ++d) {
        int r = (int)(((unsigned long long)hash32(seed, (uint32_t)pair, (uint32_t)hyp, (uint32_t)d) * (uint32_t)(K - d)) >> 32);
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

// ---- winner key -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long pack_key(bool ok, int count, int index) {
    return ok ? (((unsigned long long)(uint32_t)(count + 1) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)index)) : 0ull;
}
__device__ __forceinline__ int key_index(unsigned long long key) {
    return (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
}

// maximum key of the pair's scoring workgroups
__device__ __forceinline__ unsigned long long pair_max_key(const RansacWs& w, int b, int nblk, unsigned long long* red) {
    unsigned long long key = 0ull;
    for (int q = threadIdx.x; q < nblk; q += 256) {
        const unsigned long long o = w.best[(int64_t)b * nblk + q];
        key = o > key ? o : key;
    }
    return block_max_key(key, red);
}

// ---- compaction -----------------------------------------------------------------------------------------------------------
// Ordered compaction of the n candidates of one pair, ascending i, 256 at a time.  match(i, payload) says whether candidate
// i < n is a match and leaves what store needs of it; store(at, i, payload) puts it at position `at` of the ordered list;
// *count = the matches of the pair.
template <typename Payload, typename Match, typename Store>
__device__ __forceinline__ void compact_ordered(int n, int* count, int* wsum /* [4] */, Match match, Store store) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        Payload p;
        const bool f = i < n && match(i, p);
        const unsigned long long mask = __ballot(f);
        const int pre = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(mask);
        __syncthreads();
        int off = base;
        for (int q = 0; q < wv; ++q) off += wsum[q];
        const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (f) store(off + pre, i, p);
        base += tot;
        __syncthreads();
    }
    if (tid == 0) *count = base;
}

// the point matches of pair b; a match index outside [0, N) counts as no match
__device__ __forceinline__ void compact_pair(const float* kp0, const float* kp1, const int64_t* m0, const RansacWs& w, int b,
                                             int M, int N, int* wsum /* [4] */) {
    compact_ordered<int64_t>(
        M, w.K + b, wsum,
        [&](int i, int64_t& j) {
            j = m0[(int64_t)b * M + i];
            return j >= 0 && j < N;
        },
        [&](int k, int i, int64_t j) {
            const int64_t at = (int64_t)b * M + k;
            const float* p = kp0 + ((int64_t)b * M + i) * 2;
            const float* q = kp1 + ((int64_t)b * N + j) * 2;
            w.idx[at] = i;
            w.corr[at] = make_float4(p[0], p[1], q[0], q[1]);
        });
}

// the line matches of pair b, as compact_pair orders the points; a match index outside [0, L1), a non-finite coordinate or a
// segment shorter than eps_len pixels in either view counts as no match
struct LineMatch {
    float4 a, c, ln;            // the endpoints in view 0 and in view 1, the unit-normal view-1 line
};
__device__ __forceinline__ void compact_lines(const float* l0, const float* l1, const int64_t* lm0, const LineWs& w, int b, int L,
                                              int L1, double eps_len, int* wsum /* [4] */) {
    compact_ordered<LineMatch>(
        L, w.K + b, wsum,
        [&](int i, LineMatch& m) {
            const int64_t j = lm0[(int64_t)b * L + i];
            if (!(j >= 0 && j < L1)) return false;
            const float* p = l0 + ((int64_t)b * L + i) * 4;
            const float* r = l1 + ((int64_t)b * L1 + j) * 4;
            const float4 a = make_float4(p[0], p[1], p[2], p[3]), c = make_float4(r[0], r[1], r[2], r[3]);
            const double dx0 = (double)a.z - a.x, dy0 = (double)a.w - a.y, dx1 = (double)c.z - c.x, dy1 = (double)c.w - c.y;
            const double n0 = dx0 * dx0 + dy0 * dy0, n1 = dx1 * dx1 + dy1 * dy1;
            const double inv = 1. / sqrt(n1);
            m.a = a;
            m.c = c;
            m.ln = make_float4((float)(-dy1 * inv), (float)(dx1 * inv), (float)(((double)c.x * c.w - (double)c.z * c.y) * inv), 0.f);
            return isfinite(n0) && isfinite(n1) && n0 >= eps_len * eps_len && n1 >= eps_len * eps_len;   // a NaN compares false
        },
        [&](int k, int i, const LineMatch& m) {
            const int64_t at = (int64_t)b * L + k;
            w.idx[at] = i;
            w.seg[2 * at] = m.a;
            w.seg[2 * at + 1] = m.c;
            w.line[at] = m.ln;
        });
}

// ---- feature parts ----------------------------------------------------------------------------------------------------------
// A part is one ordered feature list of one pair: the data already offset to the pair, the flags, the count K and the
// threshold in the form the rule wants.  load(k) is feature k; the solver's rule is inlier(model, feature, th).
struct PointPart {
    using Feature = float4;     // the correspondence (x0, y0, x1, y1)
    const float4* corr;
    uint8_t* flags;
    int K;
    float th;                   // th^2
    __device__ __forceinline__ Feature load(int k) const { return corr[k]; }
};

struct LineFeature {
    float4 e, l;                // the view-0 endpoints (px, py, qx, qy), the unit-normal view-1 line (a, b, c, 0)
};
struct LinePart {
    using Feature = LineFeature;
    const float4* seg;
    const float4* line;
    uint8_t* flags;
    int K;
    float th;                   // th
    __device__ __forceinline__ Feature load(int k) const { return {seg[2 * k], line[k]}; }
};

__device__ __forceinline__ PointPart point_part(const RansacWs& w, int b, int M, float th2) {
    return {w.corr + (int64_t)b * M, w.flags + (int64_t)b * M, w.K[b], th2};
}
__device__ __forceinline__ LinePart line_part(const LineWs& w, int b, int L, float th) {
    return {w.seg + 2 * (int64_t)b * L, w.line + (int64_t)b * L, w.flags + (int64_t)b * L, w.K[b], th};
}

// ---- scoring, flags, rescore ------------------------------------------------------------------------------------------------
// inlier count of this lane's model over one part: the part's features stream through LDS in tiles, every lane reads the
// same address (a broadcast)
template <int TILE, typename Part, typename Inlier>
__device__ __forceinline__ int tile_count(const float* model, const Part& part, typename Part::Feature* tile, Inlier inlier) {
    const int K = part.K;                          // a local copy: the compiler then keeps one tile counter, not two
    int count = 0;
    for (int k0 = 0; k0 < K; k0 += TILE) {
        const int n = min(TILE, K - k0);
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += 256) tile[k] = part.load(k0 + k);
        __syncthreads();
        for (int k = 0; k < n; ++k) count += inlier(model, tile[k], part.th) ? 1 : 0;
    }
    return count;
}

// flags (where wanted) and count of a model over one part; the count is returned in every lane
template <typename Part, typename Inlier>
__device__ __forceinline__ int flag_pass(const float* model, const Part& part, bool write, int* red, Inlier inlier) {
    int count = 0;
    for (int k = threadIdx.x; k < part.K; k += 256) {
        const bool in = inlier(model, part.load(k), part.th);
        if (write) part.flags[k] = in ? 1 : 0;
        count += in ? 1 : 0;
    }
    return block_sum_int(count, red);
}

// the select kernels end here: the flags and the counts of `model` (all zero where !ok: it flags nothing) and `kept`, what
// the workspace holds as the current model, become the state of pair b.  ST_COUNT is the total over the parts, ST_LINES the
// second part's share.
template <typename Inlier, typename... Parts>
__device__ __forceinline__ void set_current(const RansacWs& w, int b, const float* model, const float* kept, bool ok, int* red,
                                            Inlier inlier, const Parts&... parts) {
    constexpr int NP = sizeof...(Parts);
    static_assert(NP == 1 || NP == 2, "one part or two");
    const int tid = threadIdx.x;
    const int n[NP] = {flag_pass(model, parts, true, red, inlier)...};                      // a braced list: in part order
    const int total = n[0] + (NP == 2 ? n[NP - 1] : 0);
    if (tid < 9) w.cur[(int64_t)b * 12 + tid] = kept[tid];
    if (tid == 0) {
        w.state[b * 4 + ST_COUNT] = total;
        if (NP == 2) w.state[b * 4 + ST_LINES] = n[NP - 1];
        w.state[b * 4 + ST_CUR_OK] = ok ? 1 : 0;
        w.state[b * 4 + ST_REFIT_OK] = 0;
    }
}

// rescore the refit; it replaces the current model when it is valid and its total count does not drop
template <typename Inlier, typename... Parts>
__device__ __forceinline__ void rescore_pair(const RansacWs& w, int b, int* red, Inlier inlier, const Parts&... parts) {
    constexpr int NP = sizeof...(Parts);
    static_assert(NP == 1 || NP == 2, "one part or two");
    const int tid = threadIdx.x;
    if (w.state[b * 4 + ST_CUR_OK] == 0 || w.state[b * 4 + ST_REFIT_OK] == 0) return;       // uniform
    float model[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) model[i] = w.refit[(int64_t)b * 12 + i];
    const int n[NP] = {flag_pass(model, parts, false, red, inlier)...};                     // a braced list: in part order
    const int total = n[0] + (NP == 2 ? n[NP - 1] : 0);
    if (total < w.state[b * 4 + ST_COUNT]) return;                                          // uniform
    ((void)flag_pass(model, parts, true, red, inlier), ...);
    __syncthreads();
    if (tid < 9) w.cur[(int64_t)b * 12 + tid] = model[tid];
    if (tid == 0) {
        w.state[b * 4 + ST_COUNT] = total;
        if (NP == 2) w.state[b * 4 + ST_LINES] = n[NP - 1];
    }
}

// out[0..n) = the flags of the current model over one ordered list, scattered to the list's view-0 indices (all zero where !ok)
__device__ __forceinline__ void scatter_flags(const uint8_t* flags, const int* idx, int K, int n, bool ok, uint8_t* out) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += 256) out[i] = 0;
    __syncthreads();
    if (!ok) return;
    for (int k = tid; k < K; k += 256)
        if (flags[k]) out[idx[k]] = 1;
}

// ---- refit ------------------------------------------------------------------------------------------------------------------
// Hartley normalisation of the kept features: x' = (x - c) sc in either view; n features with npts points per view
struct Hartley {
    double n, npts, cx0, cy0, cx1, cy1, sc0, sc1;
};

// A refit part is the kept features k < K of one list (keep(k)) and what each of them adds in the three passes:
//   moments(k, s)    to s = {feature count, point count, sum x0, sum y0, sum x1, sum y1}
//   spread(k, t, s)  to s = the two sums of distances to the centroids of t
//   rows(k, t, acc)  to the 45 distinct sums (i <= j, row-major) of the 9 x 9 normal matrix, under the full transform t
// Every pass visits the parts in order, each lane striding by 256 within a part.
template <typename Part, typename Add> __device__ __forceinline__ void for_kept(const Part& part, Add add) {
    for (int k = threadIdx.x; k < part.K; k += 256)
        if (part.keep(k)) add(k);
}

// the point part of a refit: rows(acc, k, x, y, u, v) adds correspondence k's share from its normalised coordinates
template <typename Keep, typename Rows> struct PointRefit {
    const float4* corr;
    int K;
    Keep keep;
    Rows point_rows;
    __device__ __forceinline__ void moments(int k, double (&s)[6]) const {
        const float4 c = corr[k];
        s[0] += 1.; s[1] += 1.; s[2] += c.x; s[3] += c.y; s[4] += c.z; s[5] += c.w;
    }
    __device__ __forceinline__ void spread(int k, const Hartley& t, double (&s)[2]) const {
        const float4 c = corr[k];
        const double dx0 = c.x - t.cx0, dy0 = c.y - t.cy0, dx1 = c.z - t.cx1, dy1 = c.w - t.cy1;
        s[0] += sqrt(dx0 * dx0 + dy0 * dy0);
        s[1] += sqrt(dx1 * dx1 + dy1 * dy1);
    }
    __device__ __forceinline__ void rows(int k, const Hartley& t, double (&acc)[45]) const {
        const float4 c = corr[k];
        const double x = (c.x - t.cx0) * t.sc0, y = (c.y - t.cy0) * t.sc0, u = (c.z - t.cx1) * t.sc1, v = (c.w - t.cy1) * t.sc1;
        point_rows(acc, k, x, y, u, v);
    }
};
template <typename Keep, typename Rows>
__device__ __forceinline__ PointRefit<Keep, Rows> point_refit(const float4* corr, int K, Keep keep, Rows rows) {
    return {corr, K, keep, rows};
}

// pass 1: the counts and the centroids, in every lane.  The caller gates on t.n before refit_solve (no kept feature leaves
// the centroids undefined).
template <typename... Parts> __device__ __forceinline__ void refit_moments(double* red, Hartley& t, const Parts&... parts) {
    double s6[6] = {0., 0., 0., 0., 0., 0.};
    (for_kept(parts, [&](int k) { parts.moments(k, s6); }), ...);
    block_sum_f64<6>(s6, red);
    t.n = s6[0]; t.npts = s6[1];
    t.cx0 = s6[2] / t.npts; t.cy0 = s6[3] / t.npts; t.cx1 = s6[4] / t.npts; t.cy1 = s6[5] / t.npts;
}

// passes 2 and 3 and the eigenvector: the scales of t; the 45 sums; the eigenvector g of the smallest eigenvalue; m = G T0
// with T0 = [[s0, 0, -s0 cx0], [0, s0, -s0 cy0], [0, 0, 1]], in lane 0 alone.  red is [4][45], lane k < 9 owns row k of A
// and of V.
template <typename... Parts>
__device__ __forceinline__ void refit_solve(double* red, double (*A)[9], double (*V)[9], int sweeps, Hartley& t, double m[9],
                                            const Parts&... parts) {
    const int tid = threadIdx.x;
    // pass 2: mean distances to the centroids
    double s2[2] = {0., 0.};
    (for_kept(parts, [&](int k) { parts.spread(k, t, s2); }), ...);
    block_sum_f64<2>(s2, red);
    const double sc0 = 1.4142135623730951 / (s2[0] / t.npts), sc1 = 1.4142135623730951 / (s2[1] / t.npts);
    t.sc0 = sc0; t.sc1 = sc1;
    // pass 3: the 45 distinct sums
    double acc[45];
#pragma unroll
    for (int i = 0; i < 45; ++i) acc[i] = 0.;
    (for_kept(parts, [&](int k) { parts.rows(k, t, acc); }), ...);
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
    gf_jacobi9(A, V, sweeps, tid);
    if (tid == 0) {
        int best = 0;
        for (int i = 1; i < 9; ++i)
            if (A[i][i] < A[best][best]) best = i;
        double g[9];
        for (int i = 0; i < 9; ++i) g[i] = V[i][best];
        for (int r = 0; r < 3; ++r) {
            m[3 * r + 0] = g[3 * r + 0] * sc0;
            m[3 * r + 1] = g[3 * r + 1] * sc0;
            m[3 * r + 2] = g[3 * r + 2] - sc0 * (g[3 * r + 0] * t.cx0 + g[3 * r + 1] * t.cy0);
        }
    }
}

}  // namespace
