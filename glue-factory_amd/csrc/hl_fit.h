// Per-lane fp64 arithmetic of the point-and-line homography solver (csrc/hl_solver.hip): the minimal fit from four
// features, each a point match or a line match.  Plain C++ behind GF_HL_HD so that the same text compiles for the device
// and, in a host-only build, for a CPU check of the arithmetic.
//
// THE SEMANTICS HERE ARE THIS SOLVER'S OWN DEFINITION.  The reference evaluates GlueStick with the homography_est package
// (gluefactory/robust_estimators/homography/homography_est.py), a CPU library that is not available to this project, so
// nothing below could be compared against it; tests/hl_solver_cases.py restates this text in numpy fp64.
//
// A feature is eight numbers (x0, y0, x1, y1 | u0, v0, u1, v1): two view-0 points X0, X1 and two view-1 points Y0, Y1.  A
// point match (x, y) -> (u, v) has X0 = X1 = (x, y) and Y0 = Y1 = (u, v); a line match has the endpoints p, q of the view-0
// segment and r, s of the view-1 segment.
//
// Frame.  Each view is conditioned in the sample's own frame: c = the mean of the sample's eight points of that view,
// sc = sqrt 2 / (their mean distance to c), x' = (x - c) sc.  (The eight are the four features' two points each: a point
// match counts twice.)
//
// Rows.  Every feature gives two rows of the 8 x 9 system A h = 0 in the row-major entries of the conditioned model G, each
// of the form (al x, al y, al, be x, be y, be, ga x, ga y, ga):
//   point match:  (al, be, ga) = (0, -1, v') at (x', y')   and   (1, 0, -u') at (x', y')          -- the two DLT rows
//   line match:   (al, be, ga) = l' = (a, b, c), the line through r', s' with a^2 + b^2 = 1, at p' and at q'
// (l' . G p' = 0 and l' . G q' = 0: G p and G q lie on the view-1 line, wherever along it).
//
// Two point matches with two line matches never determine a homography: their system always has the rank-one solution
// c n^T (c the intersection of the two view-1 lines, n the view-0 line through the two points; H x = 0 at both points, which
// satisfies their rows), so that is what its null vector holds, with w = 0 at the two points.  Such a sample is rejected
// before anything is computed; four points, three and one, one and three, and four lines are the minimal mixes.
//
// Null vector.  Gauss-Jordan elimination with FULL pivoting, in place: step k takes the entry of largest magnitude among
// the rows and columns not used yet (the first one in row-major order among equals), divides its row by it and clears its
// column from the seven other rows.  A pivot whose magnitude is not >= GF_HL_EPS_PIVOT rejects the sample.  The column
// left over, f, is free: g[f] = 1, g[column of row r] = -A[r][f].  Register arrays are indexed by compile-time constants
// only (the row and column choices are select chains).
//
// Model.  H = T1^-1 G T0; rejected when |h22| < GF_HL_H22_FRAC ||H||_F; H /= h22; rejected when an entry (rounded to fp32)
// is non-finite or when one of the sample's eight view-0 points has w = h20 x + h21 y + 1 <= 0.
//
// Arithmetic: fp64.  The fit runs once per hypothesis against K inlier tests, so its cost does not show, and fp64 keeps the
// residual of the fit on its own sample at 2^-53 cond(A) instead of 2^-24 cond(A) (tests/hl_solver_cases.py: fit_bound).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gf_amd.h"

#if defined(__HIPCC__)
#define GF_HL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GF_HL_HD inline
#endif

namespace gf_hl {

// f [4][8] the sampled features, line[i] whether feature i is a line match, h [9] the model in fp32 (h[8] == 1).  Returns
// false for a rejected sample.
GF_HL_HD bool fit(const double (&f)[4][8], const bool (&line)[4], float (&h)[9]) {
    if ((line[0] ? 1 : 0) + (line[1] ? 1 : 0) + (line[2] ? 1 : 0) + (line[3] ? 1 : 0) == 2) return false;
    // ---- the sample's own frame
    double cx0 = 0., cy0 = 0., cx1 = 0., cy1 = 0.;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        cx0 += f[i][0] + f[i][2]; cy0 += f[i][1] + f[i][3];
        cx1 += f[i][4] + f[i][6]; cy1 += f[i][5] + f[i][7];
    }
    cx0 *= 0.125; cy0 *= 0.125; cx1 *= 0.125; cy1 *= 0.125;
    double d0 = 0., d1 = 0.;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double ax = f[i][2 * e] - cx0, ay = f[i][2 * e + 1] - cy0;
            const double bx = f[i][4 + 2 * e] - cx1, by = f[i][5 + 2 * e] - cy1;
            d0 += sqrt(ax * ax + ay * ay);
            d1 += sqrt(bx * bx + by * by);
        }
    const double sc0 = 1.4142135623730951 / (d0 * 0.125), sc1 = 1.4142135623730951 / (d1 * 0.125);
    // ---- rows
    double A[8][9];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double x0 = (f[i][0] - cx0) * sc0, y0 = (f[i][1] - cy0) * sc0, x1 = (f[i][2] - cx0) * sc0, y1 = (f[i][3] - cy0) * sc0;
        const double u0 = (f[i][4] - cx1) * sc1, v0 = (f[i][5] - cy1) * sc1, u1 = (f[i][6] - cx1) * sc1, v1 = (f[i][7] - cy1) * sc1;
        const bool point = !line[i];
        const double la = v0 - v1, lb = u1 - u0, lc = u0 * v1 - u1 * v0;
        const double inv = 1. / sqrt(la * la + lb * lb);
        const double al0 = point ? 0. : la * inv, be0 = point ? -1. : lb * inv, ga0 = point ? v0 : lc * inv;
        const double al1 = point ? 1. : la * inv, be1 = point ? 0. : lb * inv, ga1 = point ? -u0 : lc * inv;
        A[2 * i][0] = al0 * x0; A[2 * i][1] = al0 * y0; A[2 * i][2] = al0;
        A[2 * i][3] = be0 * x0; A[2 * i][4] = be0 * y0; A[2 * i][5] = be0;
        A[2 * i][6] = ga0 * x0; A[2 * i][7] = ga0 * y0; A[2 * i][8] = ga0;
        A[2 * i + 1][0] = al1 * x1; A[2 * i + 1][1] = al1 * y1; A[2 * i + 1][2] = al1;
        A[2 * i + 1][3] = be1 * x1; A[2 * i + 1][4] = be1 * y1; A[2 * i + 1][5] = be1;
        A[2 * i + 1][6] = ga1 * x1; A[2 * i + 1][7] = ga1 * y1; A[2 * i + 1][8] = ga1;
    }
    // ---- Gauss-Jordan elimination with full pivoting, in place
    bool ok = true;
    unsigned rows_used = 0u, cols_used = 0u;
    int pcol[8];                                        // the pivot column of every row
#pragma unroll
    for (int i = 0; i < 8; ++i) pcol[i] = -1;
#pragma unroll
    for (int step = 0; step < 8; ++step) {
        double best = -1.;
        int br = 0, bc = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const double v = fabs(A[i][j]);
                const bool take = !((rows_used >> i) & 1u) && !((cols_used >> j) & 1u) && v > best;
                best = take ? v : best; br = take ? i : br; bc = take ? j : bc;
            }
        ok = ok && best >= GF_HL_EPS_PIVOT;              // a NaN compares false
        rows_used |= 1u << br; cols_used |= 1u << bc;
        double row[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            double v = A[0][j];
#pragma unroll
            for (int i = 1; i < 8; ++i) v = br == i ? A[i][j] : v;
            row[j] = v;
        }
        double piv = row[0];
#pragma unroll
        for (int j = 1; j < 9; ++j) piv = bc == j ? row[j] : piv;
        const double ipiv = 1. / piv;
#pragma unroll
        for (int j = 0; j < 9; ++j) row[j] = bc == j ? 1. : row[j] * ipiv;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double fac = A[i][0];
#pragma unroll
            for (int j = 1; j < 9; ++j) fac = bc == j ? A[i][j] : fac;
            const bool self = br == i;
            pcol[i] = self ? bc : pcol[i];
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const double v = bc == j ? 0. : A[i][j] - fac * row[j];
                A[i][j] = self ? row[j] : v;
            }
        }
    }
    // ---- the null vector: the free column is 1, the pivot columns are minus the free column's entries
    int fc = 0;
#pragma unroll
    for (int j = 1; j < 9; ++j) fc = ((cols_used >> j) & 1u) ? fc : j;
    fc = (cols_used & 1u) ? fc : 0;
    double g[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) g[j] = fc == j ? 1. : 0.;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        double v = A[i][0];
#pragma unroll
        for (int j = 1; j < 9; ++j) v = fc == j ? A[i][j] : v;
#pragma unroll
        for (int j = 0; j < 9; ++j) g[j] = pcol[i] == j ? -v : g[j];
    }
    // ---- H = T1^-1 G T0
    double k[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        k[3 * r + 0] = g[3 * r + 0] * sc0;
        k[3 * r + 1] = g[3 * r + 1] * sc0;
        k[3 * r + 2] = g[3 * r + 2] - sc0 * (g[3 * r + 0] * cx0 + g[3 * r + 1] * cy0);
    }
    const double is1 = 1. / sc1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        k[0 + c] = k[0 + c] * is1 + cx1 * k[6 + c];
        k[3 + c] = k[3 + c] * is1 + cy1 * k[6 + c];
    }
    double fro = 0.;
#pragma unroll
    for (int i = 0; i < 9; ++i) fro += k[i] * k[i];
    ok = ok && fabs(k[8]) >= (double)GF_HL_H22_FRAC * sqrt(fro);
    const double i22 = 1. / k[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        k[i] *= i22;
        h[i] = (float)k[i];
        ok = ok && isfinite(h[i]);
    }
    h[8] = 1.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double w = k[6] * f[i][2 * e] + k[7] * f[i][2 * e + 1] + 1.;
            ok = ok && w > 0.;
        }
    return ok;
}

}  // namespace gf_hl
