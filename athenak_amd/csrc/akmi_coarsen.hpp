// akmi_coarsen.hpp -- the per-cell arithmetic of the coarsened binary output (CoarsenedBinaryOutput::LoadOutputData,
// src/outputs/coarsened_binary.cpp:224-271), shared by the kernels of akmi_coarsen.hip and by the CPU build of
// tests/host_shim/coarsen_host.cpp.
//
// A coarse cell is the mean of f x f x f fine cells, and with moments also the means of x^2, x^3 and x^4.  The reference
// adds the terms with atomics, in no defined order.  Here the order is fixed: every accumulator starts at +0.0 and takes
// the fine cells in ascending kk, then jj, then ii (ii fastest) -- the order in which a serial execution of the reference's
// loop over idx visits them (offset = idx / total_coarsened_elements, :233-237) -- and is divided by (double)(f*f*f) at
// the end (:270).  The powers are the reference's left-associated products (:246-255): x*x, (x*x)*x, ((x*x)*x)*x.  The
// library is built with -ffp-contract=off, so a coarse value is a function of the bits of its fine cells alone, on the
// device and on the host: a NaN poisons its own coarse cell only, -0.0 + +0.0 = +0.0, and x^4 overflows to inf where the
// reference's does.
#ifndef AKMI_COARSEN_HPP_
#define AKMI_COARSEN_HPP_
#include <hip/hip_runtime.h>
#include <cstddef>

namespace akmi {

struct CoarsenAcc {
  double s1, s2, s3, s4;
};

__host__ __device__ __forceinline__ void coarsen_init(CoarsenAcc &a) { a.s1 = 0.0; a.s2 = 0.0; a.s3 = 0.0; a.s4 = 0.0; }

// one fine cell: all four terms from one read of x
template <bool MOM>
__host__ __device__ __forceinline__ void coarsen_add(CoarsenAcc &a, double x) {
  a.s1 += x;
  if (MOM) {
    const double x2 = x*x;
    const double x3 = x2*x;
    const double x4 = x3*x;
    a.s2 += x2;
    a.s3 += x3;
    a.s4 += x4;
  }
}

// the means into out[0], out[stride], ... (one element per moment)
template <bool MOM>
__host__ __device__ __forceinline__ void coarsen_store(const CoarsenAcc &a, double cube, double *out, size_t stride) {
  out[0] = a.s1/cube;
  if (MOM) {
    out[stride] = a.s2/cube;
    out[2*stride] = a.s3/cube;
    out[3*stride] = a.s4/cube;
  }
}

// one coarse cell from global memory: `a` points at its first fine cell, rows are n1 apart and planes n2*n1
template <bool MOM>
__host__ __device__ __forceinline__ void coarsen_cell(const double *a, size_t n1, size_t n2, int f, double *out,
                                                      size_t stride) {
  CoarsenAcc acc;
  coarsen_init(acc);
  for (int kk = 0; kk < f; ++kk)
    for (int jj = 0; jj < f; ++jj) {
      const double *row = a + ((size_t)kk*n2 + jj)*n1;
      for (int ii = 0; ii < f; ++ii) coarsen_add<MOM>(acc, row[ii]);
    }
  coarsen_store<MOM>(acc, (double)(f*f*f), out, stride);
}

}  // namespace akmi
#endif
