// Epipolar part of the depth ground truth, fused (no B x M x N intermediates).
//
// Replaces, in gluefactory/geometry/gt_generation.py:77-91, the all-pairs symmetric epipolar distance
// (gluefactory/geometry/epipolar.py:59-72), its masking to the pairs both labelled "ignore" and the row / column
// minima behind the epipolar extension of the negatives (gf_gt_epi_min, once per direction), and the dense `reward`
// of :95 (gf_gt_depth_reward: one pass, the only [B,M,N] tensor touched is the one written).  Same skeleton as
// gt_nn.hip: one thread per own point, the other view's points through LDS in tiles of 256, indices clamped at the
// ragged end.
//
// One arithmetic for both kernels and both directions (true division and sqrtf: the labels hang on a threshold):
//   l = F (x, y, 1)            the own point's line in the other image,  na = sqrtf(l0^2 + l1^2 + 1e-15f)
//   nb = sqrtf((F^T p)0^2 + (F^T p)1^2 + 1e-15f)   for the other point p (the norm of ITS line in the own image)
//   num = |p . l|,  d = 0.5f * (num / na + num / nb)
#include "gf_launch.h"

namespace {

constexpr float kEpiEps = 1e-15f;

struct Line { float l0, l1, l2, na; };

// F row-major [9]: the line of (x, y) and the norm of its direction part
__device__ __forceinline__ Line epi_line(const float* __restrict__ F, float x, float y) {
    Line r;
    r.l0 = F[0] * x + F[1] * y + F[2];
    r.l1 = F[3] * x + F[4] * y + F[5];
    r.l2 = F[6] * x + F[7] * y + F[8];
    r.na = sqrtf(r.l0 * r.l0 + r.l1 * r.l1 + kEpiEps);
    return r;
}

// norm of the first two components of F^T (x, y, 1)
__device__ __forceinline__ float epi_norm_t(const float* __restrict__ F, float x, float y) {
    const float t0 = F[0] * x + F[3] * y + F[6];
    const float t1 = F[1] * x + F[4] * y + F[7];
    return sqrtf(t0 * t0 + t1 * t1 + kEpiEps);
}

__device__ __forceinline__ float epi_dist(const Line& l, float x, float y, float nb) {
    const float num = fabsf(x * l.l0 + y * l.l1 + l.l2);
    return 0.5f * (num / l.na + num / nb);
}

__global__ __launch_bounds__(256) void gt_epi_min_kernel(const float* __restrict__ own, const float* __restrict__ oth,
                                                         const float* __restrict__ F, const uint8_t* __restrict__ own_flag,
                                                         const uint8_t* __restrict__ oth_flag, float* __restrict__ out_min,
                                                         int No, int Ns) {
    __shared__ float4 sp[256];                       // (x, y, nb, flag) of the staged other points
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int ic = min(i, No - 1);
    const float* Fb = F + (int64_t)b * 9;
    const Line l = epi_line(Fb, own[((int64_t)b * No + ic) * 2], own[((int64_t)b * No + ic) * 2 + 1]);
    float best = INFINITY;
    for (int j0 = 0; j0 < Ns; j0 += 256) {
        __syncthreads();
        const int j = min(j0 + (int)threadIdx.x, Ns - 1);
        const float x = oth[((int64_t)b * Ns + j) * 2], y = oth[((int64_t)b * Ns + j) * 2 + 1];
        const bool fl = oth_flag == nullptr || oth_flag[(int64_t)b * Ns + j] != 0;
        sp[threadIdx.x] = make_float4(x, y, epi_norm_t(Fb, x, y), fl ? 1.f : 0.f);
        __syncthreads();
        const int nj = min(256, Ns - j0);
        for (int t = 0; t < nj; ++t) {
            const float4 p = sp[t];
            const float d = epi_dist(l, p.x, p.y, p.z);
            best = p.w != 0.f ? fminf(best, d) : best;
        }
    }
    if (i < No) {
        const bool fl = own_flag == nullptr || own_flag[(int64_t)b * No + i] != 0;
        out_min[(int64_t)b * No + i] = fl ? best : INFINITY;
    }
}

// One workgroup: 256 columns (one per thread, its view-1 point in registers) x REWARD_ROWS rows (view-0 points staged in
// LDS, read as broadcasts); every row is stored as 256 consecutive floats.
constexpr int REWARD_ROWS = 64;

__global__ __launch_bounds__(256) void gt_depth_reward_kernel(
    const float* __restrict__ kp0, const float* __restrict__ kp0_1, const float* __restrict__ kp1,
    const float* __restrict__ kp1_0, const uint8_t* __restrict__ vis0, const uint8_t* __restrict__ vis1,
    const float* __restrict__ F, const uint8_t* __restrict__ flag0, const uint8_t* __restrict__ flag1,
    float* __restrict__ reward, float pos_th2, float neg_th, int M, int N) {
    __shared__ float4 sa[REWARD_ROWS];               // (kp0.x, kp0.y, kp0_1.x, kp0_1.y)
    __shared__ float4 sl[REWARD_ROWS];               // (l0, l1, l2, na)
    __shared__ int sf[REWARD_ROWS];                  // bit 0: visible, bit 1: flagged
    const int b = blockIdx.z;
    const int i0 = blockIdx.y * REWARD_ROWS;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int jc = min(j, N - 1);
    const float* Fb = F + (int64_t)b * 9;
    if (threadIdx.x < REWARD_ROWS) {
        const int64_t r = (int64_t)b * M + min(i0 + (int)threadIdx.x, M - 1);
        const float x = kp0[r * 2], y = kp0[r * 2 + 1];
        sa[threadIdx.x] = make_float4(x, y, kp0_1[r * 2], kp0_1[r * 2 + 1]);
        const Line l = epi_line(Fb, x, y);
        sl[threadIdx.x] = make_float4(l.l0, l.l1, l.l2, l.na);
        sf[threadIdx.x] = (vis0[r] != 0 ? 1 : 0) | ((flag0 == nullptr || flag0[r] != 0) ? 2 : 0);
    }
    const int64_t c = (int64_t)b * N + jc;
    const float qx = kp1[c * 2], qy = kp1[c * 2 + 1];
    const float wx = kp1_0[c * 2], wy = kp1_0[c * 2 + 1];
    const float nb = epi_norm_t(Fb, qx, qy);
    const bool v1 = vis1[c] != 0;
    const bool f1 = flag1 == nullptr || flag1[c] != 0;
    __syncthreads();
    if (j >= N) return;
    const int ni = min(REWARD_ROWS, M - i0);
    float* out = reward + ((int64_t)b * M + i0) * N + j;
    for (int t = 0; t < ni; ++t) {
        const float4 a = sa[t];
        const float4 lv = sl[t];
        const int f = sf[t];
        // visibility first: the reprojection of a point without depth is NaN
        float close = 0.f;
        if (v1 && (f & 1)) {
            const float dx0 = a.z - qx, dy0 = a.w - qy;
            const float dx1 = a.x - wx, dy1 = a.y - wy;
            close = fmaxf(dx0 * dx0 + dy0 * dy0, dx1 * dx1 + dy1 * dy1) < pos_th2 ? 1.f : 0.f;
        }
        const Line l = {lv.x, lv.y, lv.z, lv.w};
        const float epi = (f1 && (f & 2)) ? epi_dist(l, qx, qy, nb) : INFINITY;
        out[(int64_t)t * N] = close - (epi > neg_th ? 1.f : 0.f);
    }
}

}  // namespace

extern "C" int gf_gt_epi_min(const float* own, const float* oth, const float* F, const uint8_t* own_flag,
                             const uint8_t* oth_flag, float* out_min, int B, int No, int Ns, void* stream) {
    if (B <= 0 || No <= 0 || Ns <= 0) return GF_ERR_SHAPE;
    gt_epi_min_kernel<<<dim3((No + 255) / 256, B), 256, 0, gf_stream(stream)>>>(
        own, oth, F, own_flag, oth_flag, out_min, No, Ns);
    return gf_launched();
}

extern "C" int gf_gt_depth_reward(const float* kp0, const float* kp0_1, const float* kp1, const float* kp1_0,
                                  const uint8_t* vis0, const uint8_t* vis1, const float* F, const uint8_t* flag0,
                                  const uint8_t* flag1, float* reward, float pos_th2, float neg_th, int B, int M, int N,
                                  void* stream) {
    if (B <= 0 || M <= 0 || N <= 0) return GF_ERR_SHAPE;
    gt_depth_reward_kernel<<<dim3((N + 255) / 256, (M + REWARD_ROWS - 1) / REWARD_ROWS, B), 256, 0,
                             gf_stream(stream)>>>(kp0, kp0_1, kp1, kp1_0, vis0, vis1, F, flag0, flag1,
                                                                      reward, pos_th2, neg_th, M, N);
    return gf_launched();
}
