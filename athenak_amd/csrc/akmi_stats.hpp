// akmi_stats.hpp -- the per-cell arithmetic of the two run-time statistics, shared by the kernels of akmi_stats.hip and by
// the CPU build of tests/host_shim/stats_host.cpp:
//   turb_hist_cell   the eleven terms of TurbulentHistory (src/pgen/fluids/turb.cpp:287-379)
//   pdf_bin          the bin of one value (PDFOutput::LoadOutputData, src/outputs/pdf.cpp:249-279)
// Every expression keeps the reference's association (the library is built with -ffp-contract=off): a term is a function
// of the operands' bits alone, on the device and on the host.
//
// turb_hist_cell reads one layer of cells around the cell, of bcc0 and of w0 (velocities).  That layer is filled in the
// ghost zones by the last task of a stage: ConToPrim runs over the whole array, ghost cells included, after the boundary
// exchange and the physical boundary conditions of u0 and b0 (MHD::ConToPrim, mhd.py / akmi_host.cpp), and the problem
// generators end with the same call.
//
// One deviation, as for the curvature variables (akmi_derived.hpp): the reference indexes j+-1 and k+-1 whatever the
// dimension of the mesh, outside an array of extent one.  Here the CELL-CENTRED neighbour in a direction the mesh does
// not have is the cell itself, so those differences are exactly +0.  The face arrays have extent two in such a
// direction, so b.x2f(j+1) and b.x3f(k+1) are read as the reference reads them.
#ifndef AKMI_STATS_HPP_
#define AKMI_STATS_HPP_
#include "akmi_derived.hpp"

namespace akmi {

constexpr int TURB_NHIST = 11;     // Bx By Bz B^2 B^4 dB^2 BdB^2 |BxJ|^2 |B.J|^2 U^2 dU

// h[0..10] of cell (m, k, j, i).  NOTE h[0..2] (Bx, By, Bz) are NOT multiplied by the cell volume: turb.cpp:294-296 sums
// the bare field components, and so does this.
__host__ __device__ __forceinline__ void turb_hist_cell(const DvIn &a, int m, int k, int j, int i, double *h) {
  const double dx1 = a.dx[3*m], dx2 = a.dx[3*m + 1], dx3 = a.dx[3*m + 2];
  const double vol = dx1*dx2*dx3;
  const double dx_squared = dx1*dx1;
  const int jp = a.multi_d ? j + 1 : j, jm = a.multi_d ? j - 1 : j;
  const int kp = a.three_d ? k + 1 : k, km = a.three_d ? k - 1 : k;
  const DvCC b = dv_cc(a, a.bcc0, 3, m), w = dv_cc(a, a.w0, a.nvar, m);
  const size_t f1 = (((size_t)m*a.N3 + k)*a.N2 + j)*(a.N1 + 1) + i;
  const size_t f2 = (((size_t)m*a.N3 + k)*(a.N2 + 1) + j)*a.N1 + i;
  const size_t f3 = (((size_t)m*(a.N3 + 1) + k)*a.N2 + j)*a.N1 + i;
  const double Bx = b(0, k, j, i), By = b(1, k, j, i), Bz = b(2, k, j, i);
  // the differences every term is built from
  const double d1f = a.b1[f1 + 1] - a.b1[f1];                              // b.x1f(i+1) - b.x1f(i)
  const double d2f = a.b2[f2 + a.N1] - a.b2[f2];                           // b.x2f(j+1) - b.x2f(j)
  const double d3f = a.b3[f3 + (size_t)a.N2*a.N1] - a.b3[f3];              // b.x3f(k+1) - b.x3f(k)
  const double dxy = b(0, k, jp, i) - b(0, k, jm, i), dxz = b(0, kp, j, i) - b(0, km, j, i);   // d_y Bx, d_z Bx
  const double dyx = b(1, k, j, i + 1) - b(1, k, j, i - 1), dyz = b(1, kp, j, i) - b(1, km, j, i);
  const double dzx = b(2, k, j, i + 1) - b(2, k, j, i - 1), dzy = b(2, k, jp, i) - b(2, k, jm, i);

  h[0] = Bx;
  h[1] = By;
  h[2] = Bz;
  const double B_mag_sq = Bx*Bx + By*By + Bz*Bz;
  h[3] = B_mag_sq*vol;
  const double B_fourth = B_mag_sq*B_mag_sq;
  h[4] = B_fourth*vol;
  h[5] = ((d1f*d1f + d2f*d2f + d3f*d3f + 0.25*dxy*dxy + 0.25*dxz*dxz + 0.25*dyx*dyx + 0.25*dyz*dyz + 0.25*dzx*dzx
           + 0.25*dzy*dzy)/dx_squared)*vol;
  const double bdb1 = Bx*d1f + 0.5*By*dxy + 0.5*Bz*dxz;
  const double bdb2 = By*d2f + 0.5*Bz*dyz + 0.5*Bx*dyx;
  const double bdb3 = Bz*d3f + 0.5*Bx*dzx + 0.5*By*dzy;
  h[6] = ((bdb1*bdb1 + bdb2*bdb2 + bdb3*bdb3)/dx_squared)*vol;
  const double Jx = 0.5*dzy - 0.5*dyz;
  const double Jy = 0.5*dxz - 0.5*dzx;
  const double Jz = 0.5*dyx - 0.5*dxy;
  h[7] = (((By*Jz - Bz*Jy)*(By*Jz - Bz*Jy) + (Bz*Jx - Bx*Jz)*(Bz*Jx - Bx*Jz) + (Bx*Jy - By*Jx)*(Bx*Jy - By*Jx))
          /dx_squared)*vol;
  h[8] = (((Bx*Jx + By*Jy + Bz*Jz)*(Bx*Jx + By*Jy + Bz*Jz))/dx_squared)*vol;
  const double vx = w(1, k, j, i), vy = w(2, k, j, i), vz = w(3, k, j, i);
  h[9] = ((vx*vx) + (vy*vy) + (vz*vz))*vol;
  const double uxx = w(1, k, j, i + 1) - w(1, k, j, i - 1), uyy = w(2, k, jp, i) - w(2, k, jm, i);
  const double uzz = w(3, kp, j, i) - w(3, km, j, i);
  const double uxy = w(1, k, jp, i) - w(1, k, jm, i), uxz = w(1, kp, j, i) - w(1, km, j, i);
  const double uyx = w(2, k, j, i + 1) - w(2, k, j, i - 1), uyz = w(2, kp, j, i) - w(2, km, j, i);
  const double uzx = w(3, k, j, i + 1) - w(3, k, j, i - 1), uzy = w(3, k, jp, i) - w(3, k, jm, i);
  h[10] = (((0.25*uxx*uxx + 0.25*uyy*uyy + 0.25*uzz*uzz + 0.25*uxy*uxy + 0.25*uxz*uxz + 0.25*uyx*uyx + 0.25*uyz*uyz
             + 0.25*uzx*uzx + 0.25*uzy*uzy))/dx_squared)*vol;
}

// one axis of a histogram: the variable (array of nv variables per MeshBlock, component comp), the first and the last
// bin edge as the host formed them (pdf.cpp:82-93, bins(0) and bins(nbin)), the step (pdf.cpp:100-102)
struct PdfAxis {
  const double *a;
  int nv, comp, nbin, logscale;
  double lo, hi, step;
};

// bin of x in 0 .. nbin+1 (pdf.cpp:249-259), or -1 for a NaN: a NaN is below no edge and above none, and the reference
// casts it to int, which is undefined; here it belongs to no bin (the caller drops and counts it)
__host__ __device__ __forceinline__ int pdf_bin(double x, int nbin, int logscale, double lo, double hi, double step) {
  if (x != x) return -1;
  int bin;
  if (x < lo) {
    bin = 0;
  } else if (x >= hi) {
    bin = nbin + 1;
  } else {
    if (!logscale) bin = static_cast<int>((x - lo)/step) + 1;
    else bin = static_cast<int>(log10(x/lo)/step) + 1;
    // edges and step that belong together never leave 1 .. nbin+1; whatever a caller passes, no index leaves the array
    bin = bin < 0 ? 0 : (bin > nbin + 1 ? nbin + 1 : bin);
  }
  return bin;
}

}  // namespace akmi
#endif
