// What the two homography solvers (h_solver.hip, hl_solver.hip) share of their model: the transfer-error inlier rule of a
// point match, the two DLT rows of a point match and the tail of the refit (de-normalisation on the view-1 side, h22 = 1).
#pragma once
#include "ransac_common.h"

namespace {

// correspondence (x0, x1) is an inlier of H when w = h20 x + h21 y + h22 is finite and > 0 and |(H x0) / w - x1|^2 < th^2
struct TransferInlier {
    __device__ __forceinline__ bool operator()(const float* h, float4 c, float th2) const {
        const float w = h[6] * c.x + h[7] * c.y + h[8];
        const float iw = 1.f / w;
        const float dx = (h[0] * c.x + h[1] * c.y + h[2]) * iw - c.z;
        const float dy = (h[3] * c.x + h[4] * c.y + h[5]) * iw - c.w;
        return (w > 0.f) && isfinite(w) && (dx * dx + dy * dy < th2);      // a NaN error compares false
    }
};

// acc += wt (r0 r0^T + r1 r1^T) over the 45 pairs i <= j; without Weighted the factor stays out of the arithmetic
template <bool Weighted>
__device__ __forceinline__ void add_rows(double (&acc)[45], const double (&r0)[9], const double (&r1)[9], double wt = 1.) {
    int at = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j) {
            if constexpr (Weighted) acc[at] += wt * (r0[i] * r0[j] + r1[i] * r1[j]);
            else acc[at] += r0[i] * r0[j] + r1[i] * r1[j];
            ++at;
        }
}

// the two DLT rows of the normalised point match (x, y) -> (u, v)
template <bool Weighted>
__device__ __forceinline__ void add_point_rows(double (&acc)[45], double x, double y, double u, double v, double wt = 1.) {
    const double r0[9] = {0., 0., 0., -x, -y, -1., v * x, v * y, v};
    const double r1[9] = {x, y, 1., 0., 0., 0., -u * x, -u * y, -u};
    add_rows<Weighted>(acc, r0, r1, wt);
}

// no refit for this pair: the identity, ST_REFIT_OK = 0 (every lane calls it)
__device__ __forceinline__ void h_refit_none(float* Hn, int* refit_ok) {
    if (threadIdx.x < 9) Hn[threadIdx.x] = (threadIdx.x % 4 == 0) ? 1.f : 0.f;
    if (threadIdx.x == 0) *refit_ok = 0;
}

// the tail of the refit, in lane 0 alone: H = T1^-1 m with T1^-1 = [[1/s1, 0, cx1], [0, 1/s1, cy1], [0, 0, 1]] and m = G T0 of
// refit_solve, divided by h22; the identity and ST_REFIT_OK = 0 where |h22| < h22_frac ||H||_F or an entry is non-finite
__device__ __forceinline__ void h_refit_tail(const double m[9], const Hartley& t, double h22_frac, float* Hn, int* refit_ok) {
    double hh[9];
    for (int c = 0; c < 3; ++c) {
        hh[0 + c] = m[0 + c] / t.sc1 + t.cx1 * m[6 + c];
        hh[3 + c] = m[3 + c] / t.sc1 + t.cy1 * m[6 + c];
        hh[6 + c] = m[6 + c];
    }
    double fro = 0.;
    for (int i = 0; i < 9; ++i) fro += hh[i] * hh[i];
    bool ok = fabs(hh[8]) >= h22_frac * sqrt(fro);
    float out[9];
    for (int i = 0; i < 9; ++i) { out[i] = (float)(hh[i] / hh[8]); ok = ok && isfinite(out[i]); }
    for (int i = 0; i < 9; ++i) Hn[i] = ok ? out[i] : (i % 4 == 0 ? 1.f : 0.f);
    *refit_ok = ok ? 1 : 0;
}

}  // namespace
