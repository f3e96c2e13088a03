// The K x K normal equations of the two continuum fits (contsub.hip, imcontsub.hip), solved in the
// thread: Cholesky A = L L^T without pivoting, then L y = b and L^T a = y, in float64 with every
// operation in one fixed order (the numpy twins, continuum.uvcontsub_host_double and
// imcontsub.imcontsub_host_double, take the same steps).  A is the lower triangle, row by row:
// A[k (k + 1) / 2 + l], l <= k.  K is small (1 .. 4) and every loop unrolls: the arrays stay in
// registers.  Everything here is local to the including translation unit.
#pragma once
#include "kimg_common.h"

namespace {

// A = L L^T in place
template <int K> __device__ inline void kimg_cholesky(double (&A)[K * (K + 1) / 2])
{
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int l = 0; l <= k; l++) {
            double s = A[k * (k + 1) / 2 + l];
#pragma unroll
            for (int i = 0; i < l; i++)
                s -= A[k * (k + 1) / 2 + i] * A[l * (l + 1) / 2 + i];
            A[k * (k + 1) / 2 + l] = l == k ? sqrt(s) : s / A[l * (l + 1) / 2 + l];
        }
    }
}

// a = the solution of L L^T a = b, one right-hand side
template <int K>
__device__ inline void kimg_cholesky_solve(const double (&L)[K * (K + 1) / 2], const double (&b)[K],
                                           double (&a)[K])
{
#pragma unroll
    for (int k = 0; k < K; k++) {
        double s = b[k];
#pragma unroll
        for (int i = 0; i < k; i++)
            s -= L[k * (k + 1) / 2 + i] * a[i];
        a[k] = s / L[k * (k + 1) / 2 + k];
    }
#pragma unroll
    for (int k = K - 1; k >= 0; k--) {
        double s = a[k];
#pragma unroll
        for (int i = k + 1; i < K; i++)
            s -= L[i * (i + 1) / 2 + k] * a[i];
        a[k] = s / L[k * (k + 1) / 2 + k];
    }
}

}  // namespace
