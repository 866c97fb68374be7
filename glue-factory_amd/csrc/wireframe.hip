// Wireframe extractor (gluefactory/models/lines/wireframe.py): line end points -> junctions, fused.
//
// The reference loops over the batch in Python, copies the end points to the host for sklearn's DBSCAN, reads a count back
// with .item(), re-samples descriptors image by image and builds [P,P] identity matrices with index writes.  The four
// entries below do the same work in five kernel launches for the whole batch, with no host round trip:
//
//   gf_wf_cluster        :43-98   connected components of the end-point graph (edge: dx^2 + dy^2 <= eps^2), junction means,
//                                 merged lines, the junction block of the concatenated point / score buffers
//   gf_wf_suppress       :186-201 keypoints closer than nms_radius to an end point -> caller's fill position, score 0
//   gf_wf_descriptors    :8-19, :118, :202-208, :252-254   the concatenated descriptor tensor in one pass
//   gf_wf_associativity  :100-104, :256-262   identity + both orientations of every line's junction pair
//
// Clustering.  DBSCAN(eps, min_samples=1) makes every point a core point, so its clusters are the connected components and
// its label order is the order of each component's lowest index.  The edge test is the kd-tree's: fp64 dx*dx + dy*dy <=
// eps*eps on the fp32 coordinates, inclusive.  fp32 subtraction is correctly rounded, so the fp32 value of dx*dx + dy*dy is
// within 4 * 2^-24 (relative) of the exact one: outside the band eps^2 (1 +- 1e-5) fp32 decides, inside it the fp64
// expression does.  Labels are point indices (the lowest index seen so far of a point's component), held in LDS with the
// coordinates; a sweep takes the minimum over the neighbours, then jumps label -> label[label].  Labels only decrease and
// stay inside their component, so the fixed point is the component's lowest index whatever the order.  The loop runs at
// most n sweeps and every barrier in it is reached by all threads (the exit test is __syncthreads_or).
//
// Means.  torch's CPU scatter_reduce_(mean, include_self=False) adds the members in ascending index order in fp32 and
// divides by the count; the thread that owns a cluster's root does exactly that.
//
// No contraction in this file: torch computes sqrt(dx*dx + dy*dy) and numpy dx*dx + dy*dy with separately rounded products.
#include "gf_launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int WF_THREADS = 1024;                 // one workgroup per image
constexpr int WF_MAXN = 4096;                    // end points per image: 3 n + max(n, WF_THREADS) words of LDS = 64 KB
constexpr int WF_PER = WF_MAXN / WF_THREADS;     // points owned by one thread, at most
constexpr int WF_TILE = 1024;                    // end points staged at a time by the suppress kernel

__global__ __launch_bounds__(WF_THREADS) void wf_cluster_kernel(
    const float* __restrict__ lines, const float* __restrict__ line_scores, const float* __restrict__ fill,
    int64_t* __restrict__ junc_idx, int64_t* __restrict__ num_junc, float* __restrict__ out_lines,
    float* __restrict__ points, float* __restrict__ scores, int n, int P, double eps2, float lo2, float hi2, int merge) {
    extern __shared__ __attribute__((aligned(16))) char wf_smem[];
    float* sx = reinterpret_cast<float*>(wf_smem);
    float* sy = sx + n;
    int* lab = reinterpret_cast<int*>(sy + n);
    int* aux = lab + n;                          // max(n, WF_THREADS) ints: scan scratch, then the cluster id of every root
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const float* ep = lines + b * n * 2;
    for (int i = tid; i < n; i += WF_THREADS) {
        sx[i] = ep[2 * i];
        sy[i] = ep[2 * i + 1];
        lab[i] = i;
    }
    __syncthreads();
    const int per = (n + WF_THREADS - 1) / WF_THREADS;           // this thread owns points [tid * per, tid * per + per)
    const int i0 = tid * per;
    float xi[WF_PER], yi[WF_PER];
    bool own[WF_PER];
#pragma unroll
    for (int k = 0; k < WF_PER; ++k) {
        own[k] = k < per && i0 + k < n;
        xi[k] = own[k] ? sx[i0 + k] : NAN;                       // NaN: adjacent to nothing
        yi[k] = own[k] ? sy[i0 + k] : NAN;
    }
    if (merge) {
        for (int sweep = 0; sweep < n; ++sweep) {
            int m[WF_PER];
#pragma unroll
            for (int k = 0; k < WF_PER; ++k) m[k] = own[k] ? lab[i0 + k] : 0;
            for (int j = 0; j < n; ++j) {
                const float xj = sx[j], yj = sy[j];
                const int lj = lab[j];
#pragma unroll
                for (int k = 0; k < WF_PER; ++k) {
                    if (k >= per) break;                         // workgroup-uniform
                    const float dx = xi[k] - xj, dy = yi[k] - yj;
                    const float d2 = dx * dx + dy * dy;
                    bool adj = d2 < lo2;
                    if (!adj && d2 <= hi2) {
                        const double ex = (double)xi[k] - (double)xj, ey = (double)yi[k] - (double)yj;
                        adj = ex * ex + ey * ey <= eps2;
                    }
                    if (adj) m[k] = min(m[k], lj);
                }
            }
            __syncthreads();                                     // every read of lab above is done
            int changed = 0;
#pragma unroll
            for (int k = 0; k < WF_PER; ++k)
                if (own[k] && m[k] < lab[i0 + k]) { lab[i0 + k] = m[k]; changed = 1; }
            __syncthreads();
            int l2[WF_PER];
#pragma unroll
            for (int k = 0; k < WF_PER; ++k) l2[k] = own[k] ? lab[lab[i0 + k]] : 0;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < WF_PER; ++k)
                if (own[k] && l2[k] < lab[i0 + k]) { lab[i0 + k] = l2[k]; changed = 1; }
            if (!__syncthreads_or(changed)) break;               // the same answer in every thread
        }
    }
    // cluster ids: rank of every root (lab[i] == i) among the roots = exclusive prefix sum over the point index
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < WF_PER; ++k) cnt += own[k] && lab[i0 + k] == i0 + k;
    aux[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < WF_THREADS; off <<= 1) {
        const int v = tid >= off ? aux[tid - off] : 0;
        __syncthreads();
        aux[tid] += v;
        __syncthreads();
    }
    int next = aux[tid] - cnt;
    const int nc = aux[WF_THREADS - 1];
    __syncthreads();
    const float* ls = line_scores + b * (n / 2);
#pragma unroll
    for (int k = 0; k < WF_PER; ++k) {
        const int i = i0 + k;
        if (!own[k] || lab[i] != i) continue;
        float ax = 0.f, ay = 0.f, as = 0.f;
        int c = 0;
        for (int j = i; j < n; ++j)
            if (lab[j] == i) { ax += sx[j]; ay += sy[j]; as += ls[j >> 1]; ++c; }
        const float fc = (float)c;
        const size_t row = b * P + next;
        aux[i] = next++;
        sx[i] = ax / fc;                                         // nobody else reads a root's coordinates: only members of
        sy[i] = ay / fc;                                         // their own cluster
        points[row * 2] = sx[i];
        points[row * 2 + 1] = sy[i];
        scores[row] = as / fc;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < WF_PER; ++k) {
        const int i = i0 + k;
        if (!own[k]) continue;
        const int r = lab[i];
        junc_idx[b * n + i] = aux[r];
        out_lines[(b * n + i) * 2] = sx[r];
        out_lines[(b * n + i) * 2 + 1] = sy[r];
    }
    for (int r = nc + tid; r < n; r += WF_THREADS) {             // the rest of the junction block: fill position, score 0
        const size_t row = b * P + r;
        points[row * 2] = fill ? fill[(b * n + r) * 2] : 0.f;
        points[row * 2 + 1] = fill ? fill[(b * n + r) * 2 + 1] : 0.f;
        scores[row] = 0.f;
    }
    if (tid == 0) num_junc[b] = nc;
}

__global__ __launch_bounds__(256) void wf_suppress_kernel(
    const float* __restrict__ kpts, const float* __restrict__ kscores, const float* __restrict__ ends,
    const float* __restrict__ fill, uint8_t* __restrict__ flag, float* __restrict__ points, float* __restrict__ scores,
    int N, int n, int P, int J, float radius) {
    __shared__ float2 se[WF_TILE];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.y;
    const int k = blockIdx.x * 256 + tid;
    const size_t src = b * N + min(k, N - 1);
    const float kx = kpts[src * 2], ky = kpts[src * 2 + 1];
    bool hit = false;
    for (int e0 = 0; e0 < n; e0 += WF_TILE) {
        const int ne = min(WF_TILE, n - e0);
        __syncthreads();
        for (int e = tid; e < ne; e += 256) se[e] = make_float2(ends[(b * n + e0 + e) * 2], ends[(b * n + e0 + e) * 2 + 1]);
        __syncthreads();
        for (int e = 0; e < ne; ++e) {
            const float dx = kx - se[e].x, dy = ky - se[e].y;
            hit |= sqrtf(dx * dx + dy * dy) < radius;
        }
    }
    if (k >= N) return;
    flag[src] = hit;
    const size_t row = b * P + J + k;
    points[row * 2] = hit ? (fill ? fill[src * 2] : 0.f) : kx;
    points[row * 2 + 1] = hit ? (fill ? fill[src * 2 + 1] : 0.f) : ky;
    scores[row] = hit ? 0.f : kscores[src];
}

// sample_descriptors_corner_conv (:8-19): pixel x / s - 0.5, bilinear with zero padding (grid_sample's corner weights),
// L2 normalisation with F.normalize's floor.  One wave per row of the concatenated tensor; the channels-last map makes each
// corner one contiguous C-vector.  Rows of keypoints that were not flagged are copies of the point extractor's descriptors.
template <typename T>
__global__ __launch_bounds__(256) void wf_desc_kernel(const T* __restrict__ map, const float* __restrict__ points,
                                                      const float* __restrict__ kdesc, const uint8_t* __restrict__ flag,
                                                      float* __restrict__ out, int64_t total, int P, int J, int h, int w,
                                                      int C, float s) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total) return;
    const int64_t b = row / P;
    const int r = (int)(row - b * P);
    const int nch = C / 64;                       // C % 64 == 0, at most 8 per lane
    float* dst = out + row * C;
    if (r >= J) {
        const int64_t k = b * (P - J) + (r - J);
        if (!flag[k]) {                           // wave-uniform
            const float* src = kdesc + k * C;
            for (int e = 0; e < nch; ++e) dst[e * 64 + lane] = src[e * 64 + lane];
            return;
        }
    }
    const float px = points[row * 2] / s - 0.5f, py = points[row * 2 + 1] / s - 0.5f;
    const float fx = floorf(px), fy = floorf(py);
    const float wx1 = px - fx, wx0 = (fx + 1.f) - px, wy1 = py - fy, wy0 = (fy + 1.f) - py;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float cx = fx + (float)(c & 1), cy = fy + (float)(c >> 1);
        if (!(cx >= 0.f && cx < (float)w && cy >= 0.f && cy < (float)h)) continue;      // wave-uniform; NaN / inf fall out
        const float wgt = ((c & 1) ? wx1 : wx0) * ((c >> 1) ? wy1 : wy0);
        const T* src = map + ((b * h + (int)cy) * (int64_t)w + (int)cx) * C;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < nch) acc[e] += to_f32(src[e * 64 + lane]) * wgt;
    }
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (e < nch) ss += acc[e] * acc[e];
    ss = wave_allsum(ss);
    const float den = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (e < nch) dst[e * 64 + lane] = acc[e] / den;
}

// zeros with 16-byte stores (the buffer's base is 16-byte aligned; the last total % 16 bytes go one by one)
__global__ __launch_bounds__(256) void wf_zero_kernel(uint8_t* __restrict__ out, int64_t total) {
    const int64_t nvec = total / 16;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) reinterpret_cast<uint4*>(out)[i] = z;
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(total - nvec * 16)) out[nvec * 16 + threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void wf_assoc_kernel(const int64_t* __restrict__ junc_idx, uint8_t* __restrict__ out, int L,
                                                       int P) {
    const int64_t b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    uint8_t* o = out + b * P * (int64_t)P;
    if (t < P) {
        o[(int64_t)t * P + t] = 1;
    } else if (t < P + L) {
        const int64_t i = junc_idx[(b * L + (t - P)) * 2], j = junc_idx[(b * L + (t - P)) * 2 + 1];
        if (i >= 0 && i < P && j >= 0 && j < P) {
            o[i * P + j] = 1;
            o[j * P + i] = 1;
        }
    }
}

}  // namespace

extern "C" int gf_wf_cluster(const float* lines, const float* line_scores, const float* fill, int64_t* junc_idx,
                             int64_t* num_junctions, float* out_lines, float* points, float* scores, int B, int L, int P,
                             double eps, int merge, void* stream) {
    if (B <= 0 || L <= 0 || P <= 0) return GF_ERR_UNSUPPORTED;
    if (L > WF_MAXN / 2) return GF_ERR_UNSUPPORTED;              // coordinates and labels stay resident in LDS
    const int n = 2 * L;
    if (P < n || !(eps >= 0.0)) return GF_ERR_SHAPE;
    const double eps2 = eps * eps;
    const float lo2 = (float)(eps2 * (1.0 - 1e-5)), hi2 = (float)(eps2 * (1.0 + 1e-5));
    const size_t lds = (size_t)(3 * n + (n > WF_THREADS ? n : WF_THREADS)) * 4;
    wf_cluster_kernel<<<dim3(B), WF_THREADS, lds, gf_stream(stream)>>>(
        lines, line_scores, fill, junc_idx, num_junctions, out_lines, points, scores, n, P, eps2, lo2, hi2, merge);
    return gf_launched();
}

extern "C" int gf_wf_suppress(const float* kpts, const float* kscores, const float* ends, const float* fill, uint8_t* flag,
                              float* points, float* scores, int B, int N, int n, int P, int J, float radius, void* stream) {
    if (B <= 0 || N <= 0 || P <= 0) return GF_ERR_UNSUPPORTED;
    if (n < 0 || J < 0 || J + N > P) return GF_ERR_SHAPE;
    if (B > 65535) return GF_ERR_UNSUPPORTED;
    wf_suppress_kernel<<<dim3((N + 255) / 256, B), 256, 0, gf_stream(stream)>>>(
        kpts, kscores, ends, fill, flag, points, scores, N, n, P, J, radius);
    return gf_launched();
}

extern "C" int gf_wf_descriptors(const void* map, const float* points, const float* kdesc, const uint8_t* flag, float* out,
                                 int B, int P, int J, int h, int w, int C, int stride, int dtype, void* stream) {
    if (B <= 0 || P <= 0 || h <= 0 || w <= 0 || C <= 0 || stride <= 0) return GF_ERR_UNSUPPORTED;
    if (J < 0 || J > P) return GF_ERR_SHAPE;
    if (C % 64 || C > 512) return GF_ERR_ALIGN;
    const int64_t total = (int64_t)B * P;
    if ((total + 3) / 4 > 0x7fffffff) return GF_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((total + 3) / 4));
    return gf_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        wf_desc_kernel<T><<<grid, 256, 0, gf_stream(stream)>>>((const T*)map, points, kdesc, flag, out, total, P, J, h, w, C, (float)stride);
        return gf_launched();
    });
}

extern "C" int gf_wf_associativity(const int64_t* junc_idx, uint8_t* out, int B, int L, int P, void* stream) {
    if (B <= 0 || L <= 0 || P <= 0) return GF_ERR_UNSUPPORTED;
    if (B > 65535) return GF_ERR_UNSUPPORTED;
    if (!gf_aligned16(out)) return GF_ERR_ALIGN;
    hipStream_t st = gf_stream(stream);
    const int64_t total = (int64_t)B * P * P;
    const int64_t want = (total / 16 + 255) / 256;
    wf_zero_kernel<<<dim3((unsigned)(want < 1 ? 1 : want > 8192 ? 8192 : want)), 256, 0, st>>>(out, total);
    if (int e = gf_launched()) return e;
    wf_assoc_kernel<<<dim3((P + L + 255) / 256, B), 256, 0, st>>>(junc_idx, out, L, P);
    return gf_launched();
}
