// Cyclic Jacobi sweeps on a symmetric 9 x 9 matrix in LDS, shared by the refit kernels of h_solver.hip and e_solver.hip.
// Every lane of the workgroup calls it (it synchronises); lane k < 9 owns row k of A (kept symmetric) and of V.  On return
// the diagonal of A holds the eigenvalues and the columns of V the eigenvectors.  The caller fills A and V = I and
// synchronises before the call.
#pragma once

__device__ __forceinline__ void gf_jacobi9(double (*A)[9], double (*V)[9], int sweeps, int tid) {
    for (int sweep = 0; sweep < sweeps; ++sweep)
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double app = A[p][p], aqq = A[q][q], apq = A[p][q];
                double cs = 1., sn = 0., tn = 0.;
                if (apq != 0.) {
                    const double theta = (aqq - app) / (2. * apq);
                    tn = (theta >= 0. ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
                    cs = 1. / sqrt(tn * tn + 1.);
                    sn = tn * cs;
                }
                double akp = 0., akq = 0., vkp = 0., vkq = 0.;
                if (tid < 9) { akp = A[tid][p]; akq = A[tid][q]; vkp = V[tid][p]; vkq = V[tid][q]; }
                __syncthreads();
                if (tid < 9) {
                    V[tid][p] = cs * vkp - sn * vkq;
                    V[tid][q] = sn * vkp + cs * vkq;
                    if (tid != p && tid != q) {
                        const double np_ = cs * akp - sn * akq, nq_ = sn * akp + cs * akq;
                        A[tid][p] = np_; A[p][tid] = np_;
                        A[tid][q] = nq_; A[q][tid] = nq_;
                    } else if (tid == p) {
                        A[p][p] = app - tn * apq;
                        A[p][q] = 0.; A[q][p] = 0.;
                    } else {
                        A[q][q] = aqq + tn * apq;
                    }
                }
                __syncthreads();
            }
}
