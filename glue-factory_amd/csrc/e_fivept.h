// Per-lane fp64 arithmetic of the relative-pose solver (csrc/e_solver.hip): Nister's 5-point minimal solver, the projection
// onto the essential manifold, the four-fold decomposition and the depth test.  Plain C++ behind GF_E_HD so that the same
// text compiles for the device and, in a host-only build, for a CPU check of the arithmetic.
//
// Minimal solver.  The five rows (x1 x0, x1 y0, x1, y1 x0, y1 y0, y1, x0, y0, 1) of x1^T E x0 = 0 are reduced by Gauss-
// Jordan elimination with FULL pivoting; the four free columns give the null-space basis X, Y, Z, W (each divided by its
// norm) and E = x X + y Y + z Z + W.  The ten cubic constraints (2 E E^T E - tr(E E^T) E = 0, nine rows; det E = 0, one)
// are expanded by polynomial arithmetic into a 10 x 20 matrix over the monomials, in this column order,
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1,
// every row is divided by its largest magnitude and the first ten columns are reduced by Gauss-Jordan elimination with
// partial (row) pivoting.  A pivot of either elimination whose magnitude is not >= GF_E_EPS_PIVOT rejects the sample.
// Rows (4,5), (6,7), (8,9) of the reduced matrix, as  row_even - z row_odd,  give three equations
// bx(z) x + by(z) y + b1(z) = 0 of degrees (3, 3, 4); the determinant of that 3 x 3 polynomial matrix is the degree-10
// polynomial p(z), divided by its largest coefficient.
// Roots: p on [-1, 1] and the reversed polynomial q(w) = w^10 p(1/w) on [-1, 1] (z = 1/w, w != 0), each through the chain
// of derivatives: the roots of the (k-1)-th derivative lie between consecutive roots of the k-th, so level d = 1..10 bisects
// d fixed slots (brackets -1, the roots of the level before, 1; empty slots collapse to [1, 1]) GF_E_BISECT times each,
// whatever the data.  Back-substitution: (x, y, 1) is the cross product of two rows of the numeric 3 x 3 matrix at the
// root, the pair with the longest product, then GF_E_POLISH Gauss-Newton steps on the reduced cubic system.  E is divided by
// its Frobenius norm; a candidate with a non-finite entry is dropped.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gf_amd.h"

#if defined(__HIPCC__)
#define GF_E_HD __host__ __device__ inline
#else
#define GF_E_HD inline
#endif

namespace gf_e5 {

// column of monomial(col) * {x, y, z, 1}; -1 above degree three
GF_E_HD int mul_col(int col, int l) {
    const signed char tab[20][4] = {
        {-1, -1, -1, 0},  {-1, -1, -1, 1},  {-1, -1, -1, 2},  {-1, -1, -1, 3},  {-1, -1, -1, 4},
        {0, 2, 4, 5},     {-1, -1, -1, 6},  {3, 1, 6, 7},     {-1, -1, -1, 8},  {2, 3, 8, 9},
        {-1, -1, -1, 10}, {4, 8, 10, 11},   {5, 9, 11, 12},   {-1, -1, -1, 13}, {8, 6, 13, 14},
        {9, 7, 14, 15},   {-1, -1, -1, 16}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
    return tab[col][l];
}

// out += s a b for two linear polynomials (coefficients of x, y, z, 1)
GF_E_HD void mul_ll(const double* a, const double* b, double s, double* out) {
    const int lc[4] = {12, 15, 18, 19};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) out[mul_col(lc[i], j)] += s * a[i] * b[j];
}

// out += s q l for a polynomial q of degree <= 2 (20 columns) and a linear polynomial l
GF_E_HD void mul_ql(const double* q, const double* l, double s, double* out) {
    for (int c = 0; c < 20; ++c)
        for (int j = 0; j < 4; ++j) {
            const int t = mul_col(c, j);
            if (t >= 0) out[t] += s * q[c] * l[j];
        }
}

GF_E_HD double horner(const double* a, int d, double x) {
    double v = a[d];
    for (int i = d - 1; i >= 0; --i) v = v * x + a[i];
    return v;
}

// real roots of the degree-10 polynomial c (c[i] the coefficient of x^i) inside [-1, 1], ascending; returns their number
GF_E_HD int roots_unit(const double* c, double* roots) {
    double prev[10], cur[10], a[11];
    int np = 0;
    for (int d = 1; d <= 10; ++d) {
        const int k = 10 - d;                       // a = the k-th derivative of c
        for (int i = 0; i <= d; ++i) {
            double f = c[i + k];
            for (int q = 0; q < k; ++q) f *= (double)(i + k - q);
            a[i] = f;
        }
        int nc = 0;
        double lo = -1., flo = horner(a, d, lo);
        for (int q = 0; q < d; ++q) {
            const double hi = q < np ? prev[q] : 1.;
            const double fhi = horner(a, d, hi);
            const bool has = (flo < 0.) != (fhi < 0.);
            double l = lo, h = hi, fl = flo;
            for (int it = 0; it < GF_E_BISECT; ++it) {
                const double m = 0.5 * (l + h), fm = horner(a, d, m);
                if ((fl < 0.) != (fm < 0.)) h = m;
                else { l = m; fl = fm; }
            }
            if (has) cur[nc++] = 0.5 * (l + h);
            lo = hi; flo = fhi;
        }
        for (int q = 0; q < nc; ++q) prev[q] = cur[q];
        np = nc;
    }
    for (int q = 0; q < np; ++q) roots[q] = prev[q];
    return np;
}

// c (degree da + db) += s a b
GF_E_HD void pmul(const double* a, int da, const double* b, int db, double s, double* c) {
    for (int i = 0; i <= da; ++i)
        for (int j = 0; j <= db; ++j) c[i + j] += s * a[i] * b[j];
}

// GF_E_POLISH Gauss-Newton steps of (x, y, z) on the ten reduced cubic equations A m(x, y, z) = 0 (3 x 3 normal equations by
// Cramer's rule); a step that is not finite is not taken
GF_E_HD void polish(const double (*A)[20], double& x, double& y, double& z) {
    const signed char ex[20][3] = {{3, 0, 0}, {0, 3, 0}, {2, 1, 0}, {1, 2, 0}, {2, 0, 1}, {2, 0, 0}, {0, 2, 1}, {0, 2, 0},
                                   {1, 1, 1}, {1, 1, 0}, {1, 0, 2}, {1, 0, 1}, {1, 0, 0}, {0, 1, 2}, {0, 1, 1}, {0, 1, 0},
                                   {0, 0, 3}, {0, 0, 2}, {0, 0, 1}, {0, 0, 0}};
    for (int it = 0; it < GF_E_POLISH; ++it) {
        const double px[4] = {1., x, x * x, x * x * x}, py[4] = {1., y, y * y, y * y * y}, pz[4] = {1., z, z * z, z * z * z};
        double m[20][4];
        for (int c = 0; c < 20; ++c) {
            const int a = ex[c][0], b = ex[c][1], d = ex[c][2];
            m[c][0] = px[a] * py[b] * pz[d];
            m[c][1] = a > 0 ? a * px[a - 1] * py[b] * pz[d] : 0.;
            m[c][2] = b > 0 ? b * px[a] * py[b - 1] * pz[d] : 0.;
            m[c][3] = d > 0 ? d * px[a] * py[b] * pz[d - 1] : 0.;
        }
        double n[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}}, g[3] = {0., 0., 0.};
        for (int i = 0; i < 10; ++i) {
            double r[4] = {0., 0., 0., 0.};
            for (int c = 0; c < 20; ++c)
                for (int k = 0; k < 4; ++k) r[k] += A[i][c] * m[c][k];
            for (int k = 0; k < 3; ++k) {
                g[k] += r[k + 1] * r[0];
                for (int l = 0; l < 3; ++l) n[k][l] += r[k + 1] * r[l + 1];
            }
        }
        const double c00 = n[1][1] * n[2][2] - n[1][2] * n[2][1], c01 = n[1][2] * n[2][0] - n[1][0] * n[2][2];
        const double c02 = n[1][0] * n[2][1] - n[1][1] * n[2][0];
        const double det = n[0][0] * c00 + n[0][1] * c01 + n[0][2] * c02;
        const double dx = (g[0] * c00 + g[1] * (n[0][2] * n[2][1] - n[0][1] * n[2][2]) + g[2] * (n[0][1] * n[1][2] - n[0][2] * n[1][1])) / det;
        const double dy = (g[0] * c01 + g[1] * (n[0][0] * n[2][2] - n[0][2] * n[2][0]) + g[2] * (n[0][2] * n[1][0] - n[0][0] * n[1][2])) / det;
        const double dz = (g[0] * c02 + g[1] * (n[0][1] * n[2][0] - n[0][0] * n[2][1]) + g[2] * (n[0][0] * n[1][1] - n[0][1] * n[1][0])) / det;
        if (isfinite(dx) && isfinite(dy) && isfinite(dz)) { x -= dx; y -= dy; z -= dz; }
    }
}

// pts: five correspondences (x0, y0, x1, y1), normalised coordinates.  cand [GF_E_MAXSOL][9] fp32 row-major, ||E||_F = 1.
// Returns the number of candidates, 0 for a rejected sample.
GF_E_HD int solve5(const double* pts, float* cand) {
    // ---- null space of the 5 x 9 system, full pivoting
    double Q[5][9];
    int perm[9];
    for (int i = 0; i < 5; ++i) {
        const double x0 = pts[4 * i], y0 = pts[4 * i + 1], x1 = pts[4 * i + 2], y1 = pts[4 * i + 3];
        const double r[9] = {x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, 1.};
        for (int j = 0; j < 9; ++j) Q[i][j] = r[j];
    }
    for (int j = 0; j < 9; ++j) perm[j] = j;
    for (int c = 0; c < 5; ++c) {
        int br = c, bc = c;
        double best = -1.;
        for (int i = c; i < 5; ++i)
            for (int j = c; j < 9; ++j) {
                const double v = fabs(Q[i][j]);
                if (v > best) { best = v; br = i; bc = j; }
            }
        if (!(best >= GF_E_EPS_PIVOT)) return 0;
        for (int j = 0; j < 9; ++j) { const double t = Q[c][j]; Q[c][j] = Q[br][j]; Q[br][j] = t; }
        for (int i = 0; i < 5; ++i) { const double t = Q[i][c]; Q[i][c] = Q[i][bc]; Q[i][bc] = t; }
        { const int t = perm[c]; perm[c] = perm[bc]; perm[bc] = t; }
        const double inv = 1. / Q[c][c];
        for (int j = c; j < 9; ++j) Q[c][j] *= inv;
        for (int i = 0; i < 5; ++i)
            if (i != c) {
                const double f = Q[i][c];
                for (int j = c; j < 9; ++j) Q[i][j] -= f * Q[c][j];
            }
    }
    // Ep[k][l]: entry k of E as a linear polynomial, l = x, y, z, 1
    double Ep[9][4];
    for (int l = 0; l < 4; ++l) {
        double v[9], n2 = 1.;
        for (int i = 0; i < 5; ++i) { v[i] = -Q[i][5 + l]; n2 += v[i] * v[i]; }
        for (int i = 5; i < 9; ++i) v[i] = i == 5 + l ? 1. : 0.;
        const double inv = 1. / sqrt(n2);
        for (int i = 0; i < 9; ++i) Ep[perm[i]][l] = v[i] * inv;
    }
    // ---- the ten cubic constraints
    double A[10][20], L[6][20];
    for (int i = 0; i < 10; ++i)
        for (int j = 0; j < 20; ++j) A[i][j] = 0.;
    {   // L = 2 E E^T - tr(E E^T) I, the six distinct entries (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
        double tr[20];
        for (int j = 0; j < 20; ++j) tr[j] = 0.;
        int at = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j) {
                for (int q = 0; q < 20; ++q) L[at][q] = 0.;
                for (int k = 0; k < 3; ++k) mul_ll(Ep[3 * i + k], Ep[3 * j + k], 2., L[at]);
                if (i == j)
                    for (int q = 0; q < 20; ++q) tr[q] += 0.5 * L[at][q];
                ++at;
            }
        for (int q = 0; q < 20; ++q) { L[0][q] -= tr[q]; L[3][q] -= tr[q]; L[5][q] -= tr[q]; }
    }
    const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) mul_ql(L[sym[i][k]], Ep[3 * k + j], 1., A[3 * i + j]);
    {   // det E along the first row; the cofactors reuse L as room
        for (int k = 0; k < 3; ++k) {
            const int a = (k + 1) % 3, b = (k + 2) % 3;
            for (int q = 0; q < 20; ++q) L[k][q] = 0.;
            mul_ll(Ep[3 + a], Ep[6 + b], 1., L[k]);
            mul_ll(Ep[3 + b], Ep[6 + a], -1., L[k]);
            mul_ql(L[k], Ep[k], 1., A[9]);
        }
    }
    for (int i = 0; i < 10; ++i) {
        double mx = 0.;
        for (int j = 0; j < 20; ++j) mx = fmax(mx, fabs(A[i][j]));
        if (!(mx > 0.) || !(mx < 1e300)) return 0;
        const double inv = 1. / mx;
        for (int j = 0; j < 20; ++j) A[i][j] *= inv;
    }
    for (int c = 0; c < 10; ++c) {
        int br = c;
        double best = -1.;
        for (int i = c; i < 10; ++i) {
            const double v = fabs(A[i][c]);
            if (v > best) { best = v; br = i; }
        }
        if (!(best >= GF_E_EPS_PIVOT)) return 0;
        for (int j = c; j < 20; ++j) { const double t = A[c][j]; A[c][j] = A[br][j]; A[br][j] = t; }
        const double inv = 1. / A[c][c];
        for (int j = c; j < 20; ++j) A[c][j] *= inv;
        for (int i = 0; i < 10; ++i)
            if (i != c) {
                const double f = A[i][c];
                for (int j = c; j < 20; ++j) A[i][j] -= f * A[c][j];
            }
    }
    // ---- the 3 x 3 polynomial matrix in z and its determinant
    double bx[3][4], by[3][4], b1[3][5];
    for (int i = 0; i < 3; ++i) {
        const double* e = A[4 + 2 * i];
        const double* f = A[5 + 2 * i];
        bx[i][0] = e[12]; bx[i][1] = e[11] - f[12]; bx[i][2] = e[10] - f[11]; bx[i][3] = -f[10];
        by[i][0] = e[15]; by[i][1] = e[14] - f[15]; by[i][2] = e[13] - f[14]; by[i][3] = -f[13];
        b1[i][0] = e[19]; b1[i][1] = e[18] - f[19]; b1[i][2] = e[17] - f[18]; b1[i][3] = e[16] - f[17]; b1[i][4] = -f[16];
    }
    double p[11], rev[11];
    for (int i = 0; i < 11; ++i) p[i] = 0.;
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        double m[8];                                 // the minor of bx_i; the cyclic (a, b) carries the cofactor's sign
        for (int q = 0; q < 8; ++q) m[q] = 0.;
        pmul(by[a], 3, b1[b], 4, 1., m);
        pmul(by[b], 3, b1[a], 4, -1., m);
        pmul(bx[i], 3, m, 7, 1., p);
    }
    double mx = 0.;
    for (int i = 0; i < 11; ++i) mx = fmax(mx, fabs(p[i]));
    if (!(mx > 0.) || !(mx < 1e300)) return 0;
    for (int i = 0; i < 11; ++i) p[i] /= mx;
    for (int i = 0; i < 11; ++i) rev[i] = p[10 - i];
    double zs[20];
    int nz = roots_unit(p, zs);
    {
        double ws[10];
        const int nw = roots_unit(rev, ws);
        for (int q = 0; q < nw; ++q)
            if (ws[q] != 0.) zs[nz++] = 1. / ws[q];
    }
    // ---- back-substitution
    int n = 0;
    for (int q = 0; q < nz && n < GF_E_MAXSOL; ++q) {
        const double z = zs[q];
        double r[3][3];
        for (int i = 0; i < 3; ++i) { r[i][0] = horner(bx[i], 3, z); r[i][1] = horner(by[i], 3, z); r[i][2] = horner(b1[i], 4, z); }
        double v[3] = {0., 0., 0.}, bn = -1.;
        for (int i = 0; i < 3; ++i) {
            const int a = (i + 1) % 3, b = (i + 2) % 3;
            const double c0 = r[a][1] * r[b][2] - r[a][2] * r[b][1], c1 = r[a][2] * r[b][0] - r[a][0] * r[b][2];
            const double c2 = r[a][0] * r[b][1] - r[a][1] * r[b][0];
            const double nn = c0 * c0 + c1 * c1 + c2 * c2;
            if (nn > bn) { bn = nn; v[0] = c0; v[1] = c1; v[2] = c2; }
        }
        double x = v[0] / v[2], y = v[1] / v[2], zz = z;
        polish(A, x, y, zz);
        double E[9], fro = 0.;
        for (int k = 0; k < 9; ++k) { E[k] = x * Ep[k][0] + y * Ep[k][1] + zz * Ep[k][2] + Ep[k][3]; fro += E[k] * E[k]; }
        const double inv = 1. / sqrt(fro);
        bool ok = true;
        for (int k = 0; k < 9; ++k) {
            const float f = (float)(E[k] * inv);
            cand[9 * n + k] = f;
            ok = ok && isfinite(f);
        }
        if (ok) ++n;
    }
    return n;
}

// ---- 3 x 3 helpers ----------------------------------------------------------------------------------------------------
// eigen-decomposition of the symmetric S (destroyed: its diagonal holds the eigenvalues), eigenvectors the columns of V
GF_E_HD void sym3_eig(double S[3][3], double V[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1. : 0.;
    for (int sweep = 0; sweep < GF_E_JACOBI3; ++sweep)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = S[p][q];
                double cs = 1., sn = 0.;
                if (apq != 0.) {
                    const double theta = (S[q][q] - S[p][p]) / (2. * apq);
                    const double tn = (theta >= 0. ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
                    cs = 1. / sqrt(tn * tn + 1.);
                    sn = tn * cs;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double skp = S[k][p], skq = S[k][q];
                    S[k][p] = cs * skp - sn * skq; S[k][q] = sn * skp + cs * skq;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double spk = S[p][k], sqk = S[q][k];
                    S[p][k] = cs * spk - sn * sqk; S[q][k] = sn * spk + cs * sqk;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = cs * vkp - sn * vkq; V[k][q] = sn * vkp + cs * vkq;
                }
            }
}

// the two leading right singular vectors v1, v2 of E (row-major) and u_k = E v_k / |E v_k|, u2 orthogonalised against u1
GF_E_HD bool lead2(const double* E, double u1[3], double u2[3], double v1[3], double v2[3]) {
    double S[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) S[i][j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
    sym3_eig(S, V);
    // the smallest eigenvalue is left out; the other two keep their order
    const int lo = S[0][0] <= S[1][1] ? (S[0][0] <= S[2][2] ? 0 : 2) : (S[1][1] <= S[2][2] ? 1 : 2);
#pragma unroll
    for (int k = 0; k < 3; ++k) { v1[k] = lo == 0 ? V[k][1] : V[k][0]; v2[k] = lo == 2 ? V[k][1] : V[k][2]; }
    double n1 = 0., n2 = 0., d = 0.;
    for (int r = 0; r < 3; ++r) {
        u1[r] = E[3 * r] * v1[0] + E[3 * r + 1] * v1[1] + E[3 * r + 2] * v1[2];
        u2[r] = E[3 * r] * v2[0] + E[3 * r + 1] * v2[1] + E[3 * r + 2] * v2[2];
        n1 += u1[r] * u1[r];
    }
    n1 = sqrt(n1);
    for (int r = 0; r < 3; ++r) { u1[r] /= n1; d += u1[r] * u2[r]; }
    for (int r = 0; r < 3; ++r) { u2[r] -= d * u1[r]; n2 += u2[r] * u2[r]; }
    n2 = sqrt(n2);
    for (int r = 0; r < 3; ++r) u2[r] /= n2;
    return n1 > 0. && n2 > 0. && isfinite(n1) && isfinite(n2);
}

// E <- U diag(1, 1, 0) V^T / sqrt 2 (Frobenius norm one)
GF_E_HD bool project_essential(double* E) {
    double u1[3], u2[3], v1[3], v2[3];
    if (!lead2(E, u1, u2, v1, v2)) return false;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) E[3 * r + c] = (u1[r] * v1[c] + u2[r] * v2[c]) * 0.70710678118654752;
    return true;
}

// R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2] with det U = det V = +1 (gluefactory/geometry/epipolar.py:97-122)
GF_E_HD bool decompose(const double* E, double* R1, double* R2, double* t) {
    double u1[3], u2[3], v1[3], v2[3];
    if (!lead2(E, u1, u2, v1, v2)) return false;
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    double nt = 0.;
    for (int r = 0; r < 3; ++r) nt += u3[r] * u3[r];
    nt = sqrt(nt);
    for (int r = 0; r < 3; ++r) {
        t[r] = u3[r] / nt;
        for (int c = 0; c < 3; ++c) {
            const double s = u2[r] * v1[c] - u1[r] * v2[c], k = u3[r] * v3[c];
            R1[3 * r + c] = s + k;
            R2[3 * r + c] = -s + k;
        }
    }
    return nt > 0.;
}

// both depths of the correspondence positive under (R, t): X = d0 (x0, y0, 1) from the least squares of
// x1 x (d0 R x0 + t) = 0, and the third coordinate of R X + t
GF_E_HD bool in_front(const double* R, const double* t, double x0, double y0, double x1, double y1) {
    const double a[3] = {R[0] * x0 + R[1] * y0 + R[2], R[3] * x0 + R[4] * y0 + R[5], R[6] * x0 + R[7] * y0 + R[8]};
    const double c[3] = {y1 * a[2] - a[1], a[0] - x1 * a[2], x1 * a[1] - y1 * a[0]};
    const double d[3] = {y1 * t[2] - t[1], t[0] - x1 * t[2], x1 * t[1] - y1 * t[0]};
    const double d0 = -(c[0] * d[0] + c[1] * d[1] + c[2] * d[2]) / (c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const double z1 = d0 * a[2] + t[2];
    return d0 > 0. && z1 > 0. && isfinite(d0);
}

}  // namespace gf_e5
