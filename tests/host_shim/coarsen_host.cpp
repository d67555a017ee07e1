// Test infrastructure: athenak_amd/csrc/akmi_coarsen.hpp (the per-cell arithmetic of the coarsened binary output) compiled
// for the CPU, so that the non-GPU tests can compare the very arithmetic of the kernels with the numpy restatement bit
// for bit, and run the cbin writer through the product's host logic on CPU tensors.  The loops over coarse cells stand
// in for the launch of csrc/akmi_coarsen.hip.
#include <hip/hip_runtime.h>
#include "../../include/akmi.h"
#include "akmi_coarsen.hpp"

using namespace akmi;

extern "C" {

// the signature of akmi_coarsen without staged and stream
int hc_coarsen(const akmi_pack *p, const akmi_coarsen_var *vars, int nvars, int factor, int moments, const int *lo,
               const int *nc, double *out) {
  const int multi_d = p->nx2 > 1, three_d = p->nx3 > 1;
  const size_t N1 = p->nx1 + 2*p->ng, N2 = multi_d ? p->nx2 + 2*p->ng : 1, N3 = three_d ? p->nx3 + 2*p->ng : 1;
  if (factor < 1) return AKMI_FAIL;
  for (int d = 0; d < 3; ++d) {
    const size_t N = d == 0 ? N1 : (d == 1 ? N2 : N3);
    if (lo[d] < 0 || nc[d] < 1 || (size_t)lo[d] + (size_t)nc[d]*factor > N) return AKMI_FAIL;
  }
  const size_t cs = N3*N2*N1, ncc = (size_t)nc[2]*nc[1]*nc[0], stride = (size_t)p->nmb*ncc;
  const int nmom = moments ? 4 : 1;
  for (int v = 0; v < nvars; ++v)
    for (int m = 0; m < p->nmb; ++m)
      for (int kc = 0; kc < nc[2]; ++kc)
        for (int jc = 0; jc < nc[1]; ++jc)
          for (int ic = 0; ic < nc[0]; ++ic) {
            const double *a = vars[v].array + ((size_t)m*vars[v].nvar + vars[v].comp)*cs
                              + ((size_t)(lo[2] + kc*factor)*N2 + (lo[1] + jc*factor))*N1 + (lo[0] + ic*factor);
            double *o = out + ((size_t)v*nmom*p->nmb + m)*ncc + ((size_t)kc*nc[1] + jc)*nc[0] + ic;
            if (moments) coarsen_cell<true>(a, N1, N2, factor, o, stride);
            else coarsen_cell<false>(a, N1, N2, factor, o, stride);
          }
  return AKMI_COMPLETE;
}

}  // extern "C"
