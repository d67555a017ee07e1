// Test infrastructure: athenak_amd/csrc/akmi_stats.hpp (the per-cell arithmetic of the turbulence history columns and of
// the pdf bins) compiled for the CPU, so that the non-GPU tests can compare the very arithmetic of the kernels with the
// numpy restatement bit for bit, and run the history and pdf writers through the product's host logic on CPU tensors.
// The loops over cells stand in for the launches of csrc/akmi_stats.hip; the sums here are plain sequential sums.
#include <hip/hip_runtime.h>
#include "../../include/akmi.h"
#include "akmi_stats.hpp"

using namespace akmi;

namespace {
DvIn make_in(const akmi_pack *p, const double *w0, const double *bcc0, const double *b1, const double *b2, const double *b3) {
  DvIn a;
  a.nvar = p->nvar; a.ng = p->ng;
  a.multi_d = p->nx2 > 1; a.three_d = p->nx3 > 1;
  a.N1 = p->nx1 + 2*p->ng;
  a.N2 = a.multi_d ? p->nx2 + 2*p->ng : 1;
  a.N3 = a.three_d ? p->nx3 + 2*p->ng : 1;
  a.is = p->ng; a.ie = a.is + p->nx1 - 1;
  a.js = a.multi_d ? p->ng : 0; a.je = a.multi_d ? a.js + p->nx2 - 1 : 0;
  a.ks = a.three_d ? p->ng : 0; a.ke = a.three_d ? a.ks + p->nx3 - 1 : 0;
  a.dx = p->dx; a.w0 = w0; a.bcc0 = bcc0; a.b1 = b1; a.b2 = b2; a.b3 = b3;
  return a;
}
}  // namespace

extern "C" {

// terms[11][nmb][nx3][nx2][nx1]
int hs_turb_terms(const akmi_pack *p, const double *w0, const double *bcc0, const double *b1, const double *b2,
                  const double *b3, double *terms) {
  const DvIn a = make_in(p, w0, bcc0, b1, b2, b3);
  const size_t nact = (size_t)p->nmb*p->nx3*p->nx2*p->nx1;
  size_t c = 0;
  for (int m = 0; m < p->nmb; ++m)
    for (int k = a.ks; k <= a.ke; ++k)
      for (int j = a.js; j <= a.je; ++j)
        for (int i = a.is; i <= a.ie; ++i, ++c) {
          double h[TURB_NHIST];
          turb_hist_cell(a, m, k, j, i, h);
          for (int q = 0; q < TURB_NHIST; ++q) terms[q*nact + c] = h[q];
        }
  return AKMI_COMPLETE;
}

// the signature of akmi_turb_history without work and stream: partial[m][11], summed cell after cell
int hs_turb_history(const akmi_pack *p, const double *w0, const double *bcc0, const double *b1, const double *b2,
                    const double *b3, double *partial) {
  const DvIn a = make_in(p, w0, bcc0, b1, b2, b3);
  for (int m = 0; m < p->nmb; ++m) {
    double *s = partial + (size_t)m*TURB_NHIST;
    for (int q = 0; q < TURB_NHIST; ++q) s[q] = 0.0;
    for (int k = a.ks; k <= a.ke; ++k)
      for (int j = a.js; j <= a.je; ++j)
        for (int i = a.is; i <= a.ie; ++i) {
          double h[TURB_NHIST];
          turb_hist_cell(a, m, k, j, i, h);
          for (int q = 0; q < TURB_NHIST; ++q) s[q] += h[q];
        }
  }
  return AKMI_COMPLETE;
}

int hs_pdf_bins(const double *x, long long n, int nbin, int logscale, double lo, double hi, double step, int *out) {
  for (long long q = 0; q < n; ++q) out[q] = pdf_bin(x[q], nbin, logscale, lo, hi, step);
  return AKMI_COMPLETE;
}

// the signature of akmi_pdf without force_global and stream
int hs_pdf(const akmi_pack *p, const akmi_pdf_axis *x, const akmi_pdf_axis *y, const double *u0_mass,
           unsigned long long *counts, double *weights, unsigned long long *nan_count) {
  const DvIn a = make_in(p, nullptr, nullptr, nullptr, nullptr, nullptr);
  const size_t cs = (size_t)a.N3*a.N2*a.N1;
  const int nent = (y ? y->nbin + 2 : 1)*(x->nbin + 2);
  for (int e = 0; e < nent; ++e) { counts[e] = 0; weights[e] = 0.0; }
  *nan_count = 0;
  for (int m = 0; m < p->nmb; ++m)
    for (int k = a.ks; k <= a.ke; ++k)
      for (int j = a.js; j <= a.je; ++j)
        for (int i = a.is; i <= a.ie; ++i) {
          const size_t off = ((size_t)k*a.N2 + j)*a.N1 + i;
          const int xb = pdf_bin(x->array[((size_t)m*x->nvar + x->comp)*cs + off], x->nbin, x->logscale, x->bin_lo, x->bin_hi, x->step);
          const int yb = y ? pdf_bin(y->array[((size_t)m*y->nvar + y->comp)*cs + off], y->nbin, y->logscale, y->bin_lo, y->bin_hi, y->step) : 0;
          if (xb < 0 || yb < 0) { ++*nan_count; continue; }
          double w = p->dx[3*m]*p->dx[3*m + 1]*p->dx[3*m + 2];
          if (u0_mass) w *= u0_mass[((size_t)m*p->nvar + AKMI_IDN)*cs + off];
          counts[yb*(x->nbin + 2) + xb] += 1;
          weights[yb*(x->nbin + 2) + xb] += w;
        }
  return AKMI_COMPLETE;
}

}  // extern "C"
