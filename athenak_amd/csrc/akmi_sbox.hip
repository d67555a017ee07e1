// akmi_sbox.hip -- the shearing box (src/shearing_box/): source terms, the shear-periodic x1 boundary and orbital
// advection of cell-centred variables (hydro and MHD) and of the face-centred field.
//   akmi_sbox_srcterms     ShearingBoxCC::SourceTermsCC            shearing_box_srcterms.cpp:27-84
//   akmi_sbox_remap_x1     ShearingBoxCC::PackAndSendCC, step 1    shearing_box_cc.cpp:48-116    (fractional remap)
//   akmi_sbox_shift_x1     ... step 2 + RecvAndUnpackCC            shearing_box_cc.cpp:118-266, :359-388 (integer shift)
//   akmi_sbox_orbital_cc   OrbitalAdvectionCC::RecvAndUnpackCC     orbital_advection_cc.cpp:215-288
//   akmi_sbox_srcterms_mhd ShearingBoxCC::SourceTermsCC (MHD)      shearing_box_srcterms.cpp:92-150
//   akmi_sbox_efield_2d    ShearingBoxFC::SourceTermsFC            shearing_box_srcterms.cpp:159-200
//   akmi_sbox_remap_x1_fc  ShearingBoxFC::PackAndSendFC, step 1    shearing_box_fc.cpp:48-136
//   akmi_sbox_shift_x1_fc  ... step 2 + RecvAndUnpackFC            shearing_box_fc.cpp:138-286, :379-431
//   akmi_sbox_orbital_emf  OrbitalAdvectionFC::RecvAndUnpackFC     orbital_advection_fc.cpp:223-329 (effective EMFs)
//   akmi_sbox_orbital_ct   ... the CT update                       orbital_advection_fc.cpp:331-358
//   akmi_mri_history       MRIHistory                              pgen/tests/mri3d.cpp:233-336
// The remap "fluxes" are DC_/PLM_/PPMX_RemapFlx of remap_fluxes.hpp, one face per call, with the reference's
// parenthesisation (the library is built with -ffp-contract=off; `/` is the IEEE division, fmod is exact), so every
// entry gives the reference's bits.  The reference stages each pencil in team scratch and fills a flux array; here a
// thread forms the faces it needs from global memory: the kernels move a few bytes per flop, the slabs are small
// (x1 boundary) or re-read from cache (orbital advection: neighbouring rows are neighbouring threads' loads).
#include "akmi_common.hpp"
#include "akmi_tile_reduce.hpp"

namespace akmi {
namespace {

// CellCenterX, src/coordinates/cell_locations.hpp:35-39
__device__ __forceinline__ double cell_center_x(int ith, int n, double xmin, double xmax) {
  const double x = ((double)ith + 0.5)/(double)n;
  return (x*xmax - x*xmin) - (0.5*xmax - 0.5*xmin) + (0.5*xmin + 0.5*xmax);
}

// LeftEdgeX, src/coordinates/cell_locations.hpp:23-28
__device__ __forceinline__ double left_edge_x(int ith, int n, double xmin, double xmax) {
  const double x = ((double)ith)/(double)n;
  return (x*xmax - x*xmin) - (0.5*xmax - 0.5*xmin) + (0.5*xmin + 0.5*xmax);
}

__device__ __forceinline__ double sign_of(double x) { return (x < 0.0) ? -1.0 : 1.0; }      // SIGN, athena.hpp:52

// ---- remap fluxes, remap_fluxes.hpp -------------------------------------------------------------------------------
// RC: 0 = DC_RemapFlx, 1 = PLM_RemapFlx, 2 = PPMX_RemapFlx.  u(j) reads row j of the pencil; the value is ust(j).
enum { RC_DC = 0, RC_PLM = 1, RC_PPMX = 2 };

// the limited parabola of cell j (remap_fluxes.hpp:72-135): ulv, urv
template <class U>
__device__ __forceinline__ void ppmx_cell(const U &u, int j, double &ulv, double &urv, double &uj) {
  const double um2 = u(j - 2), um1 = u(j - 1), u0 = u(j), up1 = u(j + 1), up2 = u(j + 2);
  ulv = (7.0*(um1 + u0) - (um2 + up1))/12.0;
  double d2uc = 3.0*(um1 - 2.0*ulv + u0);
  double d2ul = (um2 - 2.0*um1 + u0);
  double d2ur = (um1 - 2.0*u0 + up1);
  double d2ulim = 0.0;
  double lim_slope = fmin(fabs(d2ul), fabs(d2ur));
  if (d2uc > 0.0 && d2ul > 0.0 && d2ur > 0.0) d2ulim = sign_of(d2uc)*fmin(1.25*lim_slope, fabs(d2uc));
  if (d2uc < 0.0 && d2ul < 0.0 && d2ur < 0.0) d2ulim = sign_of(d2uc)*fmin(1.25*lim_slope, fabs(d2uc));
  ulv = 0.5*((um1 + u0) - d2ulim/3.0);

  urv = (7.0*(u0 + up1) - (um1 + up2))/12.0;
  d2uc = 3.0*(u0 - 2.0*urv + up1);
  d2ul = (um1 - 2.0*u0 + up1);
  d2ur = (u0 - 2.0*up1 + up2);
  d2ulim = 0.0;
  lim_slope = fmin(fabs(d2ul), fabs(d2ur));
  if (d2uc > 0.0 && d2ul > 0.0 && d2ur > 0.0) d2ulim = sign_of(d2uc)*fmin(1.25*lim_slope, fabs(d2uc));
  if (d2uc < 0.0 && d2ul < 0.0 && d2ur < 0.0) d2ulim = sign_of(d2uc)*fmin(1.25*lim_slope, fabs(d2uc));
  urv = 0.5*((u0 + up1) - d2ulim/3.0);

  double qa = (urv - u0)*(u0 - ulv);
  double qb = (um1 - u0)*(u0 - up1);
  if (qa <= 0.0 && qb <= 0.0) {
    const double d2u = -12.0*(u0 - 0.5*(ulv + urv));
    d2uc = (um1 - 2.0*u0 + up1);
    d2ul = (um2 - 2.0*um1 + u0);
    d2ur = (u0 - 2.0*up1 + up2);
    d2ulim = 0.0;
    lim_slope = fmin(fabs(d2ul), fabs(d2ur));
    lim_slope = fmin(fabs(d2uc), lim_slope);
    if (d2uc > 0.0 && d2ul > 0.0 && d2ur > 0.0 && d2u > 0.0) d2ulim = sign_of(d2u)*fmin(1.25*lim_slope, fabs(d2u));
    if (d2uc < 0.0 && d2ul < 0.0 && d2ur < 0.0 && d2u < 0.0) d2ulim = sign_of(d2u)*fmin(1.25*lim_slope, fabs(d2u));
    if (d2u == 0.0) {
      ulv = u0;
      urv = u0;
    } else {
      ulv = u0 + (ulv - u0)*d2ulim/d2u;
      urv = u0 + (urv - u0)*d2ulim/d2u;
    }
  }

  qa = (urv - u0)*(u0 - ulv);
  qb = urv - ulv;
  const double qc = 6.0*(u0 - 0.5*(ulv + urv));
  if (qa <= 0.0) {
    ulv = u0;
    urv = u0;
  } else if ((qb*qc) > (qb*qb)) {
    ulv = 3.0*u0 - 2.0*urv;
  } else if ((qb*qc) < -(qb*qb)) {
    urv = 3.0*u0 - 2.0*ulv;
  }
  uj = u0;
}

template <int RC, class U>
__device__ __forceinline__ double remap_flux(const U &u, int j, double eps) {
  if constexpr (RC == RC_DC) {                               // remap_fluxes.hpp:18-30
    return (eps > 0.0) ? eps*u(j - 1) : eps*u(j);
  } else if constexpr (RC == RC_PLM) {                       // remap_fluxes.hpp:36-61
    if (eps > 0.0) {
      const double um2 = u(j - 2), um1 = u(j - 1), u0 = u(j);
      const double dql = um1 - um2;
      const double dqr = u0 - um1;
      const double dq2 = dql*dqr;
      double dqm = 2.0*dq2/(dql + dqr);
      if (dq2 <= 0.0) dqm = 0.0;
      return eps*(um1 + 0.5*(1.0 - eps)*dqm);
    }
    const double um1 = u(j - 1), u0 = u(j), up1 = u(j + 1);
    const double dql = u0 - um1;
    const double dqr = up1 - u0;
    const double dq2 = dql*dqr;
    double dqm = 2.0*dq2/(dql + dqr);
    if (dq2 <= 0.0) dqm = 0.0;
    return eps*(u0 - 0.5*(1.0 + eps)*dqm);
  } else {                                                   // remap_fluxes.hpp:69-149: ust(c+1) / ust(c) of cell c
    double ulv, urv, uc;
    ppmx_cell(u, (eps > 0.0) ? j - 1 : j, ulv, urv, uc);
    const double du = urv - ulv;
    const double u6 = 6.0*(uc - 0.5*(ulv + urv));
    if (eps > 0.0) {
      const double qx = 0.6666666666666667*eps;              // TWO_3RDS, athena.hpp:54
      return eps*(urv - 0.75*qx*(du - (1.0 - qx)*u6));
    }
    const double qx = -0.6666666666666667*eps;
    return eps*(ulv + 0.75*qx*(du + (1.0 - qx)*u6));
  }
}

// ---- source terms ---------------------------------------------------------------------------------------------------
// One thread per active cell.  THREE_D: the 3-D branch (shearing_box_srcterms.cpp:39-62), else the 2-D r-z branch
// (:65-81, shearing_box_r_phi is always false).  Old primitives in, updated conserved variables read-modify-written.
// MHD: the form with the Maxwell stress in the energy term (:92-150); bcc0 is double[nmb][3][N3][N2][N1].
constexpr int SX = 64, SY = 4;

template <bool THREE_D, bool MHD>
__global__ void __launch_bounds__(SX*SY)
k_sbox_srcterms(Geo g, int is_ideal, int strat, double coef1, double coef2, double coef3, double bdt, double qo,
                const double *__restrict__ xlim, const double *__restrict__ w0, const double *__restrict__ bcc0,
                double *__restrict__ u0, int fm) {
  const Cell3 q = flat_cells(fm, g.N1, g.is, g.ie, g.js, g.nx2, g.ks, g.nx3);
  if (!q.in) return;
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const size_t c = ix5(g.nvar, g.N3, g.N2, g.N1, q.m, 0, q.k, q.j, q.i);
  constexpr int IO = THREE_D ? AKMI_IM2 : AKMI_IM3;         // the second horizontal direction: y in 3-D, z in r-z
  const double den = w0[c];
  const double mom1 = den*w0[c + AKMI_IM1*cs];
  const double momo = den*w0[c + IO*cs];
  u0[c + AKMI_IM1*cs] += coef1*momo;
  u0[c + IO*cs] -= coef2*mom1;
  if (THREE_D && strat) {
    const double x3v = cell_center_x(q.k - g.ks, g.nx3, xlim[6*q.m + 4], xlim[6*q.m + 5]);
    u0[c + AKMI_IM3*cs] -= coef3*den*x3v;
  }
  if constexpr (MHD) {
    if (is_ideal) {
      const size_t b = ix5(3, g.N3, g.N2, g.N1, q.m, 0, q.k, q.j, q.i);
      u0[c + AKMI_IEN*cs] += bdt*(mom1*momo/den - bcc0[b]*bcc0[b + (size_t)(IO - 1)*cs])*qo;   // IBX; IBY in 3-D, IBZ in r-z
    }
  } else {
    if (is_ideal) u0[c + AKMI_IEN*cs] += bdt*mom1*momo/den*qo;
  }
}

// SourceTermsFC, 2-D r-z only: E1 -= qo x1v b2 and E2 += qo x1f b1 at ks and ke + 1 (both from b at ks, as written)
__global__ void __launch_bounds__(256)
k_sbox_efield_2d(Geo g, double qo, const double *__restrict__ xlim, const double *__restrict__ b1,
                 const double *__restrict__ b2, double *__restrict__ e1, double *__restrict__ e2) {
  const unsigned p = blockIdx.x*256u + threadIdx.x;
  const unsigned ni = (unsigned)g.nx1 + 1u;
  const unsigned jj = p/ni;
  if (jj > (unsigned)g.nx2) return;
  const int m = (int)blockIdx.y, j = g.js + (int)jj, ii = (int)(p - jj*ni), i = g.is + ii;
  const double x1v = cell_center_x(ii, g.nx1, xlim[6*m], xlim[6*m + 1]);
  const double x1f = left_edge_x(ii, g.nx1, xlim[6*m], xlim[6*m + 1]);
  const double vb2 = b2[ix4(1, g.N2 + 1, g.N1, m, 0, j, i)], vb1 = b1[ix4(1, g.N2, g.N1 + 1, m, 0, j, i)];
  e1[ix4(2, g.N2 + 1, g.N1, m, 0, j, i)] -= qo*x1v*vb2;
  e1[ix4(2, g.N2 + 1, g.N1, m, 1, j, i)] -= qo*x1v*vb2;
  e2[ix4(2, g.N2, g.N1 + 1, m, 0, j, i)] += qo*x1f*vb1;
  e2[ix4(2, g.N2, g.N1 + 1, m, 1, j, i)] += qo*x1f*vb1;
}

// ---- shear-periodic x1 boundary -------------------------------------------------------------------------------------
// tab: int[2][nslot][2 + nmbx2] per face n and boundary MeshBlock slot: {local MeshBlock index, lx2 of the block, the slot
// of the block at lx2 = 0, 1, ... on the same face and the same lx3}.  buf: double[2][nslot][nvar][N3][nx2][ng].
struct XFace {
  int nb[2], nslot, stride;
  const int *tab;
};

// row j of the x1 ghost pencil (n, mm, v, k, i): the ghost slab itself, all nx2 + 2 ng rows are there
struct SlabRow {
  const double *p;       // element (mm, v, k, 0, column)
  size_t n1;
  __device__ __forceinline__ double operator()(int j) const { return p[(size_t)j*n1]; }
};

template <int RC>
__global__ void __launch_bounds__(256)
k_sbox_remap_x1(Geo g, XFace f, double yshear, const double *__restrict__ u0, double *__restrict__ buf) {
  // flat index over (face, slot, v, k, j - js, i), i fastest
  const unsigned long long per = (unsigned long long)g.nvar*g.N3*g.nx2*g.ng;
  const unsigned long long p = (unsigned long long)blockIdx.x*256u + threadIdx.x;
  const unsigned long long ns = p/per;
  if (ns >= (unsigned long long)(2*f.nslot)) return;
  const int n = (int)(ns/(unsigned)f.nslot), slot = (int)(ns - (unsigned long long)n*f.nslot);
  if (slot >= f.nb[n]) return;
  unsigned r = (unsigned)(p - ns*per);
  const int i = (int)(r % (unsigned)g.ng); r /= (unsigned)g.ng;
  const int jj = (int)(r % (unsigned)g.nx2); r /= (unsigned)g.nx2;
  const int k = (int)(r % (unsigned)g.N3);
  const int v = (int)(r/(unsigned)g.N3);
  const int mm = f.tab[((size_t)n*f.nslot + slot)*f.stride];
  const double dx2 = g.dx[3*mm + 1];
  double eps = fmod(yshear, dx2)/dx2;                        // shearing_box_cc.cpp:89-90
  if (n == 1) eps *= -1.0;
  const SlabRow u{u0 + ix5(g.nvar, g.N3, g.N2, g.N1, mm, v, k, 0, n == 0 ? i : g.ie + 1 + i), (size_t)g.N1};
  const int j = g.js + jj;
  const double flo = remap_flux<RC>(u, j, eps), fhi = remap_flux<RC>(u, j + 1, eps);
  buf[p] = u(j) - (fhi - flo);                               // shearing_box_cc.cpp:113
}

// every x1 ghost cell of every boundary MeshBlock, all rows j of the block: the buffer value at global row
// g -/+ joffset (modulo the Ny rows of the mesh), g the global active row of the destination.  That is the reference's
// cases 1/2/3 and FindTargetMB in one gather (tests/test_sbox_host.py compares the two for every offset).
__global__ void __launch_bounds__(256)
k_sbox_shift_x1(Geo g, XFace f, int nmbx2, int joffset, const double *__restrict__ buf, double *__restrict__ u0) {
  const unsigned long long per = (unsigned long long)g.nvar*g.N3*g.N2*g.ng;
  const unsigned long long p = (unsigned long long)blockIdx.x*256u + threadIdx.x;
  const unsigned long long ns = p/per;
  if (ns >= (unsigned long long)(2*f.nslot)) return;
  const int n = (int)(ns/(unsigned)f.nslot), slot = (int)(ns - (unsigned long long)n*f.nslot);
  if (slot >= f.nb[n]) return;
  unsigned r = (unsigned)(p - ns*per);
  const int i = (int)(r % (unsigned)g.ng); r /= (unsigned)g.ng;
  const int j = (int)(r % (unsigned)g.N2); r /= (unsigned)g.N2;
  const int k = (int)(r % (unsigned)g.N3);
  const int v = (int)(r/(unsigned)g.N3);
  const int *t = f.tab + ((size_t)n*f.nslot + slot)*f.stride;
  const int mm = t[0];
  const long long ny = (long long)nmbx2*g.nx2;
  long long gs = (long long)t[1]*g.nx2 + (j - g.js) + (n == 0 ? -(long long)joffset : (long long)joffset);
  gs %= ny;
  if (gs < 0) gs += ny;
  const int bx = (int)(gs/g.nx2), jr = (int)(gs - (long long)bx*g.nx2);
  const int ss = t[2 + bx];
  const size_t src = (((((size_t)n*f.nslot + ss)*g.nvar + v)*g.N3 + k)*g.nx2 + jr)*g.ng + i;
  u0[ix5(g.nvar, g.N3, g.N2, g.N1, mm, v, k, j, n == 0 ? i : g.ie + 1 + i)] = buf[src];
}

// ---- shear-periodic x1 boundary of the face-centred field ------------------------------------------------------------
// The three components as "variables" of different shapes: x1f [N3][N2][N1+1], x2f [N3][N2+1][N1], x3f [N3+1][N2][N1].
// Both launches touch planes k in [0, N3) and rows j in [0, N2) only: the last x2f row and the last x3f plane are left
// alone, as the reference's loops leave them (shearing_box_fc.cpp:59-61, :382-384).
// buf: double[2][nslot][3][N3][nx2][ng].
struct Face3 {
  double *f[3];
  __device__ __forceinline__ size_t n1(const Geo &g, int v) const { return (size_t)g.N1 + (v == 0 ? 1 : 0); }
  // element (mm, k, j, i) of component v
  __device__ __forceinline__ size_t at(const Geo &g, int v, int mm, int k, int j, int i) const {
    const int n3 = g.N3 + (v == 2 ? 1 : 0), n2 = g.N2 + (v == 1 ? 1 : 0), n1 = g.N1 + (v == 0 ? 1 : 0);
    return ix4(n3, n2, n1, mm, k, j, i);
  }
  // the ghost column i of face n: x1f has one face more than the cells (shearing_box_fc.cpp:77-105)
  __device__ __forceinline__ int col(const Geo &g, int v, int n, int i) const {
    return n == 0 ? i : (v == 0 ? g.ie + 2 + i : g.ie + 1 + i);
  }
};

template <int RC>
__global__ void __launch_bounds__(256)
k_sbox_remap_x1_fc(Geo g, XFace f, double yshear, Face3 b, double *__restrict__ buf) {
  // flat index over (face, slot, v, k, j - js, i), i fastest
  const unsigned long long per = 3ull*g.N3*g.nx2*g.ng;
  const unsigned long long p = (unsigned long long)blockIdx.x*256u + threadIdx.x;
  const unsigned long long ns = p/per;
  if (ns >= (unsigned long long)(2*f.nslot)) return;
  const int n = (int)(ns/(unsigned)f.nslot), slot = (int)(ns - (unsigned long long)n*f.nslot);
  if (slot >= f.nb[n]) return;
  unsigned r = (unsigned)(p - ns*per);
  const int i = (int)(r % (unsigned)g.ng); r /= (unsigned)g.ng;
  const int jj = (int)(r % (unsigned)g.nx2); r /= (unsigned)g.nx2;
  const int k = (int)(r % (unsigned)g.N3);
  const int v = (int)(r/(unsigned)g.N3);
  const int mm = f.tab[((size_t)n*f.nslot + slot)*f.stride];
  const double dx2 = g.dx[3*mm + 1];
  double eps = fmod(yshear, dx2)/dx2;                        // shearing_box_fc.cpp:109-110
  if (n == 1) eps *= -1.0;
  const SlabRow u{b.f[v] + b.at(g, v, mm, k, 0, b.col(g, v, n, i)), b.n1(g, v)};
  const int j = g.js + jj;
  const double flo = remap_flux<RC>(u, j, eps), fhi = remap_flux<RC>(u, j + 1, eps);
  buf[p] = u(j) - (fhi - flo);                               // shearing_box_fc.cpp:133
}

// the gather of k_sbox_shift_x1 for the three components: rows j in [0, N2), planes k in [0, N3)
__global__ void __launch_bounds__(256)
k_sbox_shift_x1_fc(Geo g, XFace f, int nmbx2, int joffset, const double *__restrict__ buf, Face3 b) {
  const unsigned long long per = 3ull*g.N3*g.N2*g.ng;
  const unsigned long long p = (unsigned long long)blockIdx.x*256u + threadIdx.x;
  const unsigned long long ns = p/per;
  if (ns >= (unsigned long long)(2*f.nslot)) return;
  const int n = (int)(ns/(unsigned)f.nslot), slot = (int)(ns - (unsigned long long)n*f.nslot);
  if (slot >= f.nb[n]) return;
  unsigned r = (unsigned)(p - ns*per);
  const int i = (int)(r % (unsigned)g.ng); r /= (unsigned)g.ng;
  const int j = (int)(r % (unsigned)g.N2); r /= (unsigned)g.N2;
  const int k = (int)(r % (unsigned)g.N3);
  const int v = (int)(r/(unsigned)g.N3);
  const int *t = f.tab + ((size_t)n*f.nslot + slot)*f.stride;
  const int mm = t[0];
  const long long ny = (long long)nmbx2*g.nx2;
  long long gs = (long long)t[1]*g.nx2 + (j - g.js) + (n == 0 ? -(long long)joffset : (long long)joffset);
  gs %= ny;
  if (gs < 0) gs += ny;
  const int bx = (int)(gs/g.nx2), jr = (int)(gs - (long long)bx*g.nx2);
  const int ss = t[2 + bx];
  const size_t src = (((((size_t)n*f.nslot + ss)*3 + v)*g.N3 + k)*g.nx2 + jr)*g.ng + i;
  b.f[v][b.at(g, v, mm, k, j, b.col(g, v, n, i))] = buf[src];
}

// ---- orbital advection ----------------------------------------------------------------------------------------------
// The x2 pencil (m, v, k, i) extended by ng + maxjshift rows on either side: row jv in [0, nx2) is active row js + jv of the
// block, rows below / above are the active rows of the x2 neighbours (the reference copies them into buffers first,
// orbital_advection_cc.cpp:53-128; u0's own x2 ghost rows are stale at this point of the stage).  The host has checked
// ng + maxjshift <= nx2 and |joffset| <= maxjshift, so one hop suffices; the clamp only keeps a violated contract inside
// the array.
struct OrbRow {
  const double *self, *lo, *hi;   // element (m', v, k, js, i) of the block and of its inner / outer x2 neighbour
  size_t n1;
  int nx2;
  __device__ __forceinline__ double operator()(int jv) const {
    const double *b = self;
    if (jv < 0) { b = lo; jv += nx2; } else if (jv >= nx2) { b = hi; jv -= nx2; }
    jv = jv < 0 ? 0 : (jv >= nx2 ? nx2 - 1 : jv);
    return b[(size_t)jv*n1];
  }
};

constexpr int OJ = 4;       // rows of one pencil per thread: OJ + 1 faces for OJ cells

template <int RC>
__global__ void __launch_bounds__(256)
k_sbox_orbital(Geo g, double qo, double dt, const int *__restrict__ nghbr, const double *__restrict__ xlim,
               const double *__restrict__ u0, double *__restrict__ out) {
  // lanes along i: the loads of a wave are rows of consecutive addresses, split where joffset changes (a cell or two)
  const unsigned p = blockIdx.x*256u + threadIdx.x;
  const unsigned jc = p/(unsigned)g.nx1;
  const int ii = (int)(p - jc*(unsigned)g.nx1);
  const int j0 = (int)jc*OJ;
  if (j0 >= g.nx2) return;
  const int k = g.ks + (int)blockIdx.y;
  const int m = (int)(blockIdx.z/(unsigned)g.nvar), v = (int)(blockIdx.z - (unsigned)m*(unsigned)g.nvar);
  const int i = g.is + ii;
  const double x1v = cell_center_x(ii, g.nx1, xlim[6*m], xlim[6*m + 1]);
  const double dx2 = g.dx[3*m + 1];
  const double yshear = -(qo)*x1v*dt;                        // orbital_advection_cc.cpp:244-245, :263
  const int joffset = static_cast<int>(yshear/dx2);
  const double epsi = fmod(yshear, dx2)/dx2;
  int ml = nghbr[27*m + 10], mh = nghbr[27*m + 16];          // (ox1, ox2, ox3) = (0, -1, 0) and (0, +1, 0)
  if (ml < 0) ml = m;
  if (mh < 0) mh = m;
  const OrbRow u{u0 + ix5(g.nvar, g.N3, g.N2, g.N1, m, v, k, g.js, i), u0 + ix5(g.nvar, g.N3, g.N2, g.N1, ml, v, k, g.js, i),
                 u0 + ix5(g.nvar, g.N3, g.N2, g.N1, mh, v, k, g.js, i), (size_t)g.N1, g.nx2};
  double *o = out + ix5(g.nvar, g.N3, g.N2, g.N1, m, v, k, g.js, i);
  const int j1 = (j0 + OJ < g.nx2) ? j0 + OJ : g.nx2;
  double flo = remap_flux<RC>(u, j0 - joffset, epsi);
  for (int jv = j0; jv < j1; ++jv) {
    const double fhi = remap_flux<RC>(u, jv + 1 - joffset, epsi);
    o[(size_t)jv*g.N1] = u(jv - joffset) - (fhi - flo);      // orbital_advection_cc.cpp:286
    flo = fhi;
  }
}

// Orbital advection of the face-centred field (orbital_advection_fc.cpp:223-329): the effective EMFs of the shift of
// B3 (v = 0, emfx = -Vy Bz at x1 cell centres) and B1 (v = 1, emfz = Vy Bx at x1 faces) along x2.  Per pencil
// (m, v, k in [ks, ke+1], i in [is, ie+1]) and row j in [js, je+1]: the remap flux at face j - joffset, then the whole
// cells the integer shift has carried across the face, summed in the reference's order.  One thread per row: a row needs
// one face flux, so nothing is carried from row to row (k_sbox_orbital carries the upper face of a cell); lanes run
// along i as there.  emfx, emfz: double[nmb][N3][N2][N1].
template <int RC>
__global__ void __launch_bounds__(256)
k_sbox_orbital_emf(Geo g, double qo, double dt, const int *__restrict__ nghbr, const double *__restrict__ xlim,
                   const double *__restrict__ x1f, const double *__restrict__ x3f, double *__restrict__ emfx,
                   double *__restrict__ emfz) {
  const unsigned p = blockIdx.x*256u + threadIdx.x;
  const unsigned ni = (unsigned)g.nx1 + 1u;
  const unsigned jv = p/ni;
  if (jv > (unsigned)g.nx2) return;
  const int ii = (int)(p - jv*ni), i = g.is + ii;
  const int k = g.ks + (int)blockIdx.y;
  const int m = (int)(blockIdx.z >> 1), v = (int)(blockIdx.z & 1u);
  const double x1 = (v == 0) ? cell_center_x(ii, g.nx1, xlim[6*m], xlim[6*m + 1])
                             : left_edge_x(ii, g.nx1, xlim[6*m], xlim[6*m + 1]);
  const double dx2 = g.dx[3*m + 1];
  const double yshear = -(qo)*x1*dt;                         // orbital_advection_fc.cpp:257-258, :280
  const int joffset = static_cast<int>(yshear/dx2);
  const double epsi = fmod(yshear, dx2)/dx2;
  int ml = nghbr[27*m + 10], mh = nghbr[27*m + 16];          // (ox1, ox2, ox3) = (0, -1, 0) and (0, +1, 0)
  if (ml < 0) ml = m;
  if (mh < 0) mh = m;
  const double *src = (v == 0) ? x3f : x1f;
  const int n3 = g.N3 + (v == 0 ? 1 : 0), n1 = g.N1 + (v == 0 ? 0 : 1);
  const OrbRow u{src + ix4(n3, g.N2, n1, m, k, g.js, i), src + ix4(n3, g.N2, n1, ml, k, g.js, i),
                 src + ix4(n3, g.N2, n1, mh, k, g.js, i), (size_t)n1, g.nx2};
  const int j = (int)jv;
  const double flx = remap_flux<RC>(u, j - joffset, epsi);
  double e = (v == 0) ? -flx : flx;                          // orbital_advection_fc.cpp:303-310, :318-325
  if (v == 0) {
    for (int jj = 1; jj <= joffset; jj++) e -= u(j - jj);
    for (int jj = joffset + 1; jj <= 0; jj++) e += u(j - jj);
  } else {
    for (int jj = 1; jj <= joffset; jj++) e += u(j - jj);
    for (int jj = joffset + 1; jj <= 0; jj++) e -= u(j - jj);
  }
  ((v == 0) ? emfx : emfz)[ix4(g.N3, g.N2, g.N1, m, k, g.js + j, i)] = e;
}

// the CT update by the effective EMFs (orbital_advection_fc.cpp:331-358), 3-D: one thread per (k, j, i) of
// [ks, ke+1] x [js, je+1] x [is, ie+1] updates the faces it owns, in place (every EMF is complete before the launch)
__global__ void __launch_bounds__(256)
k_sbox_orbital_ct(Geo g, const double *__restrict__ emfx, const double *__restrict__ emfz, double *__restrict__ x1f,
                  double *__restrict__ x2f, double *__restrict__ x3f) {
  const unsigned p = blockIdx.x*256u + threadIdx.x;
  const unsigned ni = (unsigned)g.nx1 + 1u;
  const unsigned jv = p/ni;
  if (jv > (unsigned)g.nx2) return;
  const int i = g.is + (int)(p - jv*ni), j = g.js + (int)jv, k = g.ks + (int)blockIdx.y, m = (int)blockIdx.z;
  const bool in_i = i <= g.ie, in_j = j <= g.je, in_k = k <= g.ke;
  const size_t c = ix4(g.N3, g.N2, g.N1, m, k, j, i), sj = (size_t)g.N1, sk = (size_t)g.N2*g.N1;
  if (in_k && in_j) x1f[ix4(g.N3, g.N2, g.N1 + 1, m, k, j, i)] -= (emfz[c + sj] - emfz[c]);
  if (in_k && in_i) {
    const double dydx = g.dx[3*m + 1]/g.dx[3*m];
    const double dydz = g.dx[3*m + 1]/g.dx[3*m + 2];
    double b2 = x2f[ix4(g.N3, g.N2 + 1, g.N1, m, k, j, i)];
    b2 += dydx*(emfz[c + 1] - emfz[c]);
    b2 -= dydz*(emfx[c + sk] - emfx[c]);
    x2f[ix4(g.N3, g.N2 + 1, g.N1, m, k, j, i)] = b2;
  }
  if (in_j && in_i) x3f[ix4(g.N3 + 1, g.N2, g.N1, m, k, j, i)] += (emfx[c + sj] - emfx[c]);
}

// ---- MRIHistory, src/pgen/tests/mri3d.cpp:233-336 --------------------------------------------------------------------
// The 15 (isothermal) or 16 (ideal) sums over the active cells: the conserved variables, the three kinetic and magnetic
// energies, the net fluxes, and the Reynolds and Maxwell stresses; nf = nmhd = 4 or 5.  Tiles and trees of
// akmi_tile_reduce.hpp, as akmi_turb_history: per-MeshBlock partials, no atomics.
template <int K>
__global__ void __launch_bounds__(NT)
k_mri_hist(TurbGeo g, const double *__restrict__ dxs, const double *__restrict__ u0, const double *__restrict__ bcc,
           const double *__restrict__ b1, const double *__restrict__ b2, const double *__restrict__ b3,
           double *__restrict__ tiles) {
  constexpr int nf = K - 11;
  const int m = blockIdx.x/g.ntile, tile = blockIdx.x - m*g.ntile;
  const double vol = dxs[3*m]*dxs[3*m + 1]*dxs[3*m + 2];
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  double acc[K];
  for (int q = 0; q < K; ++q) acc[q] = 0.0;
  for (int p = 0; p < PER; ++p) {
    const int c = tile*TILE + p*NT + threadIdx.x;
    if (c >= g.ncell) break;
    int k, j, i;
    cell_of(g, c, k, j, i);
    k += g.ks; j += g.js; i += g.is;
    const size_t u = ix5(g.nvar, g.N3, g.N2, g.N1, m, 0, k, j, i), b = ix5(3, g.N3, g.N2, g.N1, m, 0, k, j, i);
    const double d = u0[u], m1 = u0[u + cs], m2 = u0[u + 2*cs], m3 = u0[u + 3*cs];
    double h[K];
    h[0] = vol*d;
    h[1] = vol*m1;
    h[2] = vol*m2;
    h[3] = vol*m3;
    if constexpr (nf == 5) h[4] = vol*u0[u + 4*cs];
    h[nf] = vol*0.5*(m1*m1)/d;
    h[nf + 1] = vol*0.5*(m2*m2)/d;
    h[nf + 2] = vol*0.5*(m3*m3)/d;
    const double x1l = b1[ix4(g.N3, g.N2, g.N1 + 1, m, k, j, i)], x1r = b1[ix4(g.N3, g.N2, g.N1 + 1, m, k, j, i + 1)];
    const double x2l = b2[ix4(g.N3, g.N2 + 1, g.N1, m, k, j, i)], x2r = b2[ix4(g.N3, g.N2 + 1, g.N1, m, k, j + 1, i)];
    const double x3l = b3[ix4(g.N3 + 1, g.N2, g.N1, m, k, j, i)], x3r = b3[ix4(g.N3 + 1, g.N2, g.N1, m, k + 1, j, i)];
    h[nf + 3] = vol*0.25*(x1r*x1r + x1l*x1l);
    h[nf + 4] = vol*0.25*(x2r*x2r + x2l*x2l);
    h[nf + 5] = vol*0.25*(x3r*x3r + x3l*x3l);
    const double bx = bcc[b], by = bcc[b + cs], bz = bcc[b + 2*cs];
    h[nf + 6] = vol*bx;
    h[nf + 7] = vol*by;
    h[nf + 8] = vol*bz;
    h[nf + 9] = vol*m1*m2/d;
    h[nf + 10] = -vol*bx*by;
    for (int q = 0; q < K; ++q) acc[q] += h[q];
  }
  block_sum<K>(acc, tiles + (size_t)blockIdx.x*K);
}

// reconstruction of the run -> remap flux, as the switch of shearing_box_cc.cpp:93-108 / orbital_advection_cc.cpp:264-279
template <class F>
int dispatch_remap(int recon, const char *who, F &&f) {
  switch (recon) {
    case AKMI_RECON_DC: return f(IC<RC_DC>{});
    case AKMI_RECON_PLM: return f(IC<RC_PLM>{});
    case AKMI_RECON_PPM4: case AKMI_RECON_PPMX: case AKMI_RECON_WENOZ: case AKMI_RECON_TENO: return f(IC<RC_PPMX>{});
  }
  set_error("%s: reconstruct = %d has no remap flux", who, recon);
  return AKMI_FAIL;
}

int check_pack(const akmi_pack *p, const char *who) {
  if (!p || p->nmb < 1 || p->nvar < 1 || p->nx1 < 1 || p->nx2 < 1 || p->nx3 < 1 || p->ng < 2) {
    set_error("%s: null or empty pack", who);
    return AKMI_FAIL;
  }
  return AKMI_COMPLETE;
}

int check_xface(const akmi_pack *p, int recon, int nb_in, int nb_out, int nslot, const int *tab, int stride,
                const char *who) {
  if (check_pack(p, who) != AKMI_COMPLETE) return AKMI_FAIL;
  if (p->nx2 == 1) { set_error("%s: shear-periodic boundaries need 2-D or 3-D", who); return AKMI_FAIL; }
  if (nb_in < 0 || nb_out < 0 || nslot < 1 || nb_in > nslot || nb_out > nslot || nb_in > p->nmb || nb_out > p->nmb ||
      !tab || stride < 3) {
    set_error("%s: boundary MeshBlock table (%d inner, %d outer, %d slots, stride %d)", who, nb_in, nb_out, nslot, stride);
    return AKMI_FAIL;
  }
  // the stencil of the remap flux reaches 2 (PLM) / 3 (PPMX) rows beyond js, je + 1
  if (recon >= AKMI_RECON_PPM4 && p->ng < 3) { set_error("%s: the PPMX remap needs nghost >= 3", who); return AKMI_FAIL; }
  const Geo g = make_geo(p);
  if ((unsigned long long)g.nvar*g.N3*g.N2*g.ng >= (1ull << 31)) {
    set_error("%s: the x1 ghost slab of one MeshBlock has 2^31 elements or more", who);
    return AKMI_FAIL;
  }
  return AKMI_COMPLETE;
}

int check_orbital_fc(const akmi_pack *p, const char *who) {
  if (check_pack(p, who) != AKMI_COMPLETE) return AKMI_FAIL;
  if (p->nx2 == 1 || p->nx3 == 1) {
    // (the reference runs this in 3-D or 2-D r-phi, and r-phi is never set)
    set_error("%s: orbital advection of the field runs on 3-D meshes", who);
    return AKMI_FAIL;
  }
  const long long n = (long long)(p->nx1 + 1)*(p->nx2 + 1);
  if (p->nx3 + 1 > 65535 || 2ll*p->nmb > 65535 || (n + 255)/256 >= (1ll << 31)) {
    set_error("%s: %d MeshBlocks, nx3 = %d: outside one launch", who, p->nmb, p->nx3);
    return AKMI_FAIL;
  }
  return AKMI_COMPLETE;
}

}  // namespace
}  // namespace akmi

using namespace akmi;

extern "C" {

int akmi_sbox_srcterms(const akmi_pack *p, double coef1, double coef2, double coef3, double bdt, double qo, int stratified,
                       const double *xlim, const double *w0, double *u0, void *stream) {
  if (check_pack(p, "sbox_srcterms") != AKMI_COMPLETE) return AKMI_FAIL;
  if (p->nvar < (p->is_ideal ? 5 : 4)) {
    set_error("sbox_srcterms: nvar = %d is smaller than the fluid variable set of the EOS", p->nvar);
    return AKMI_FAIL;
  }
  if (p->nx2 == 1) { set_error("sbox_srcterms: the shearing box needs 2-D or 3-D"); return AKMI_FAIL; }
  if (stratified && p->nx3 > 1 && !xlim) { set_error("sbox_srcterms: stratified needs the MeshBlock bounds"); return AKMI_FAIL; }
  const Geo g = make_geo(p);
  const int fm = (g.three_d && g.nx1*g.nx2 <= SX*SY) ? (FLAT_K | FLAT_COLS) : 0;      // as akmi_srcterms_apply
  const dim3 grid = flat_cells_grid(fm, g.N1, g.is, g.ie, g.nx2, g.nx3, g.nmb, SX*SY), block(SX, SY);
  hipStream_t st = (hipStream_t)stream;
  if (g.three_d)
    k_sbox_srcterms<true, false><<<grid, block, 0, st>>>(g, p->is_ideal, stratified, coef1, coef2, coef3, bdt, qo, xlim, w0,
                                                        nullptr, u0, fm);
  else
    k_sbox_srcterms<false, false><<<grid, block, 0, st>>>(g, p->is_ideal, 0, coef1, coef2, coef3, bdt, qo, xlim, w0, nullptr,
                                                         u0, fm);
  AKMI_CHECK_LAUNCH("sbox_srcterms");
  return AKMI_COMPLETE;
}

int akmi_sbox_remap_x1(const akmi_pack *p, int recon, int nb_in, int nb_out, int nslot, const int *tab, int tab_stride,
                       double yshear, const double *u0, double *buf, void *stream) {
  if (check_xface(p, recon, nb_in, nb_out, nslot, tab, tab_stride, "sbox_remap_x1") != AKMI_COMPLETE) return AKMI_FAIL;
  if (nb_in + nb_out == 0) return AKMI_COMPLETE;
  const Geo g = make_geo(p);
  const XFace f{{nb_in, nb_out}, nslot, tab_stride, tab};
  const unsigned long long total = 2ull*nslot*g.nvar*g.N3*g.nx2*g.ng;
  if ((total + 255)/256 >= (1ull << 31)) { set_error("sbox_remap_x1: too many boundary cells for one launch"); return AKMI_FAIL; }
  const unsigned grid = (unsigned)((total + 255)/256);
  hipStream_t st = (hipStream_t)stream;
  return dispatch_remap(recon, "sbox_remap_x1", [&](auto R) {
    k_sbox_remap_x1<decltype(R)::value><<<grid, 256, 0, st>>>(g, f, yshear, u0, buf);
    AKMI_CHECK_LAUNCH("sbox_remap_x1");
    return (int)AKMI_COMPLETE;
  });
}

int akmi_sbox_shift_x1(const akmi_pack *p, int nb_in, int nb_out, int nslot, const int *tab, int tab_stride, int nmbx2,
                       int joffset, const double *buf, double *u0, void *stream) {
  if (check_xface(p, AKMI_RECON_DC, nb_in, nb_out, nslot, tab, tab_stride, "sbox_shift_x1") != AKMI_COMPLETE) return AKMI_FAIL;
  if (nmbx2 < 1 || tab_stride != 2 + nmbx2 || joffset < 0) {
    set_error("sbox_shift_x1: nmbx2 = %d, table stride %d, joffset = %d", nmbx2, tab_stride, joffset);
    return AKMI_FAIL;
  }
  if (nb_in + nb_out == 0) return AKMI_COMPLETE;
  const Geo g = make_geo(p);
  const XFace f{{nb_in, nb_out}, nslot, tab_stride, tab};
  const unsigned long long total = 2ull*nslot*g.nvar*g.N3*g.N2*g.ng;
  if ((total + 255)/256 >= (1ull << 31)) { set_error("sbox_shift_x1: too many boundary cells for one launch"); return AKMI_FAIL; }
  k_sbox_shift_x1<<<(unsigned)((total + 255)/256), 256, 0, (hipStream_t)stream>>>(g, f, nmbx2, joffset, buf, u0);
  AKMI_CHECK_LAUNCH("sbox_shift_x1");
  return AKMI_COMPLETE;
}

int akmi_sbox_orbital_cc(const akmi_pack *p, int recon, int maxjshift, double qo, double dt, const int *nghbr,
                         const double *xlim, const double *u0, double *out, void *stream) {
  if (check_pack(p, "sbox_orbital_cc") != AKMI_COMPLETE) return AKMI_FAIL;
  if (p->nx2 == 1) { set_error("sbox_orbital_cc: orbital advection needs an x2 direction"); return AKMI_FAIL; }
  if (!nghbr || !xlim || !u0 || !out || u0 == out) {
    set_error("sbox_orbital_cc: neighbour table, MeshBlock bounds, and two different arrays are needed");
    return AKMI_FAIL;
  }
  if (maxjshift < 1 || p->ng + maxjshift > p->nx2) {
    set_error("sbox_orbital_cc: nghost + maxjshift = %d + %d exceeds <meshblock>/nx2 = %d", p->ng, maxjshift, p->nx2);
    return AKMI_FAIL;
  }
  if (recon >= AKMI_RECON_PPM4 && p->ng < 3) { set_error("sbox_orbital_cc: the PPMX remap needs nghost >= 3"); return AKMI_FAIL; }
  const Geo g = make_geo(p);
  const long long pencils = (long long)g.nx1*((g.nx2 + OJ - 1)/OJ), mv = (long long)g.nmb*g.nvar;
  if (g.nx3 > 65535 || mv > 65535 || (pencils + 255)/256 >= (1ll << 31)) {
    set_error("sbox_orbital_cc: %lld MeshBlocks x variables, nx3 = %d: outside one launch", mv, g.nx3);
    return AKMI_FAIL;
  }
  const dim3 grid((unsigned)((pencils + 255)/256), (unsigned)g.nx3, (unsigned)mv);
  hipStream_t st = (hipStream_t)stream;
  return dispatch_remap(recon, "sbox_orbital_cc", [&](auto R) {
    k_sbox_orbital<decltype(R)::value><<<grid, 256, 0, st>>>(g, qo, dt, nghbr, xlim, u0, out);
    AKMI_CHECK_LAUNCH("sbox_orbital_cc");
    return (int)AKMI_COMPLETE;
  });
}

int akmi_sbox_srcterms_mhd(const akmi_pack *p, double coef1, double coef2, double coef3, double bdt, double qo,
                           int stratified, const double *xlim, const double *w0, const double *bcc0, double *u0,
                           void *stream) {
  if (check_pack(p, "sbox_srcterms_mhd") != AKMI_COMPLETE) return AKMI_FAIL;
  if (p->nvar < (p->is_ideal ? 5 : 4)) {
    set_error("sbox_srcterms_mhd: nvar = %d is smaller than the fluid variable set of the EOS", p->nvar);
    return AKMI_FAIL;
  }
  if (p->nx2 == 1) { set_error("sbox_srcterms_mhd: the shearing box needs 2-D or 3-D"); return AKMI_FAIL; }
  if (!w0 || !u0 || (p->is_ideal && !bcc0)) { set_error("sbox_srcterms_mhd: null array"); return AKMI_FAIL; }
  if (stratified && p->nx3 > 1 && !xlim) {
    set_error("sbox_srcterms_mhd: stratified needs the MeshBlock bounds");
    return AKMI_FAIL;
  }
  const Geo g = make_geo(p);
  const int fm = (g.three_d && g.nx1*g.nx2 <= SX*SY) ? (FLAT_K | FLAT_COLS) : 0;
  const dim3 grid = flat_cells_grid(fm, g.N1, g.is, g.ie, g.nx2, g.nx3, g.nmb, SX*SY), block(SX, SY);
  hipStream_t st = (hipStream_t)stream;
  if (g.three_d)
    k_sbox_srcterms<true, true><<<grid, block, 0, st>>>(g, p->is_ideal, stratified, coef1, coef2, coef3, bdt, qo, xlim, w0,
                                                       bcc0, u0, fm);
  else
    k_sbox_srcterms<false, true><<<grid, block, 0, st>>>(g, p->is_ideal, 0, coef1, coef2, coef3, bdt, qo, xlim, w0, bcc0,
                                                        u0, fm);
  AKMI_CHECK_LAUNCH("sbox_srcterms_mhd");
  return AKMI_COMPLETE;
}

int akmi_sbox_efield_2d(const akmi_pack *p, double qo, const double *xlim, const double *bx1f, const double *bx2f,
                        double *e1, double *e2, void *stream) {
  if (check_pack(p, "sbox_efield_2d") != AKMI_COMPLETE) return AKMI_FAIL;
  if (p->nx2 == 1 || p->nx3 > 1) { set_error("sbox_efield_2d: a 2-D mesh only (SourceTermsFC acts in r-z)"); return AKMI_FAIL; }
  if (!xlim || !bx1f || !bx2f || !e1 || !e2) { set_error("sbox_efield_2d: null array"); return AKMI_FAIL; }
  const Geo g = make_geo(p);
  const long long n = (long long)(g.nx1 + 1)*(g.nx2 + 1);
  if (g.nmb > 65535 || (n + 255)/256 >= (1ll << 31)) { set_error("sbox_efield_2d: outside one launch"); return AKMI_FAIL; }
  k_sbox_efield_2d<<<dim3((unsigned)((n + 255)/256), (unsigned)g.nmb), 256, 0, (hipStream_t)stream>>>(g, qo, xlim, bx1f,
                                                                                                       bx2f, e1, e2);
  AKMI_CHECK_LAUNCH("sbox_efield_2d");
  return AKMI_COMPLETE;
}

int akmi_sbox_remap_x1_fc(const akmi_pack *p, int recon, int nb_in, int nb_out, int nslot, const int *tab, int tab_stride,
                          double yshear, const double *bx1f, const double *bx2f, const double *bx3f, double *buf,
                          void *stream) {
  if (check_xface(p, recon, nb_in, nb_out, nslot, tab, tab_stride, "sbox_remap_x1_fc") != AKMI_COMPLETE) return AKMI_FAIL;
  if (!bx1f || !bx2f || !bx3f || !buf) { set_error("sbox_remap_x1_fc: null array"); return AKMI_FAIL; }
  if (nb_in + nb_out == 0) return AKMI_COMPLETE;
  const Geo g = make_geo(p);
  const XFace f{{nb_in, nb_out}, nslot, tab_stride, tab};
  const Face3 b{{const_cast<double *>(bx1f), const_cast<double *>(bx2f), const_cast<double *>(bx3f)}};
  const unsigned long long total = 2ull*nslot*3*g.N3*g.nx2*g.ng;
  if ((total + 255)/256 >= (1ull << 31)) { set_error("sbox_remap_x1_fc: too many boundary faces for one launch"); return AKMI_FAIL; }
  const unsigned grid = (unsigned)((total + 255)/256);
  hipStream_t st = (hipStream_t)stream;
  return dispatch_remap(recon, "sbox_remap_x1_fc", [&](auto R) {
    k_sbox_remap_x1_fc<decltype(R)::value><<<grid, 256, 0, st>>>(g, f, yshear, b, buf);
    AKMI_CHECK_LAUNCH("sbox_remap_x1_fc");
    return (int)AKMI_COMPLETE;
  });
}

int akmi_sbox_shift_x1_fc(const akmi_pack *p, int nb_in, int nb_out, int nslot, const int *tab, int tab_stride, int nmbx2,
                          int joffset, const double *buf, double *bx1f, double *bx2f, double *bx3f, void *stream) {
  if (check_xface(p, AKMI_RECON_DC, nb_in, nb_out, nslot, tab, tab_stride, "sbox_shift_x1_fc") != AKMI_COMPLETE)
    return AKMI_FAIL;
  if (nmbx2 < 1 || tab_stride != 2 + nmbx2 || joffset < 0) {
    set_error("sbox_shift_x1_fc: nmbx2 = %d, table stride %d, joffset = %d", nmbx2, tab_stride, joffset);
    return AKMI_FAIL;
  }
  if (!bx1f || !bx2f || !bx3f || !buf) { set_error("sbox_shift_x1_fc: null array"); return AKMI_FAIL; }
  if (nb_in + nb_out == 0) return AKMI_COMPLETE;
  const Geo g = make_geo(p);
  const XFace f{{nb_in, nb_out}, nslot, tab_stride, tab};
  const Face3 b{{bx1f, bx2f, bx3f}};
  const unsigned long long total = 2ull*nslot*3*g.N3*g.N2*g.ng;
  if ((total + 255)/256 >= (1ull << 31)) { set_error("sbox_shift_x1_fc: too many boundary faces for one launch"); return AKMI_FAIL; }
  k_sbox_shift_x1_fc<<<(unsigned)((total + 255)/256), 256, 0, (hipStream_t)stream>>>(g, f, nmbx2, joffset, buf, b);
  AKMI_CHECK_LAUNCH("sbox_shift_x1_fc");
  return AKMI_COMPLETE;
}

int akmi_sbox_orbital_emf(const akmi_pack *p, int recon, int maxjshift, double qo, double dt, const int *nghbr,
                          const double *xlim, const double *bx1f, const double *bx3f, double *emfx, double *emfz,
                          void *stream) {
  if (check_orbital_fc(p, "sbox_orbital_emf") != AKMI_COMPLETE) return AKMI_FAIL;
  if (!nghbr || !xlim || !bx1f || !bx3f || !emfx || !emfz || emfx == emfz) {
    set_error("sbox_orbital_emf: neighbour table, MeshBlock bounds, two face arrays and two EMF arrays are needed");
    return AKMI_FAIL;
  }
  if (maxjshift < 1 || p->ng + maxjshift > p->nx2) {
    set_error("sbox_orbital_emf: nghost + maxjshift = %d + %d exceeds <meshblock>/nx2 = %d", p->ng, maxjshift, p->nx2);
    return AKMI_FAIL;
  }
  if (recon >= AKMI_RECON_PPM4 && p->ng < 3) { set_error("sbox_orbital_emf: the PPMX remap needs nghost >= 3"); return AKMI_FAIL; }
  const Geo g = make_geo(p);
  const long long n = (long long)(g.nx1 + 1)*(g.nx2 + 1);
  const dim3 grid((unsigned)((n + 255)/256), (unsigned)(g.nx3 + 1), (unsigned)(2*g.nmb));
  hipStream_t st = (hipStream_t)stream;
  return dispatch_remap(recon, "sbox_orbital_emf", [&](auto R) {
    k_sbox_orbital_emf<decltype(R)::value><<<grid, 256, 0, st>>>(g, qo, dt, nghbr, xlim, bx1f, bx3f, emfx, emfz);
    AKMI_CHECK_LAUNCH("sbox_orbital_emf");
    return (int)AKMI_COMPLETE;
  });
}

int akmi_sbox_orbital_ct(const akmi_pack *p, const double *emfx, const double *emfz, double *bx1f, double *bx2f,
                         double *bx3f, void *stream) {
  if (check_orbital_fc(p, "sbox_orbital_ct") != AKMI_COMPLETE) return AKMI_FAIL;
  if (!emfx || !emfz || !bx1f || !bx2f || !bx3f) { set_error("sbox_orbital_ct: null array"); return AKMI_FAIL; }
  const Geo g = make_geo(p);
  const long long n = (long long)(g.nx1 + 1)*(g.nx2 + 1);
  const dim3 grid((unsigned)((n + 255)/256), (unsigned)(g.nx3 + 1), (unsigned)g.nmb);
  k_sbox_orbital_ct<<<grid, 256, 0, (hipStream_t)stream>>>(g, emfx, emfz, bx1f, bx2f, bx3f);
  AKMI_CHECK_LAUNCH("sbox_orbital_ct");
  return AKMI_COMPLETE;
}

long long akmi_mri_history_workspace_bytes(const akmi_pack *p) {
  if (!p || !pack_ok(p, "mri_history")) return -1;
  const TurbGeo g = make_tgeo(p);
  return (long long)p->nmb*g.ntile*AKMI_MRI_NHIST_MAX*sizeof(double);
}

int akmi_mri_history(const akmi_pack *p, const double *u0, const double *bcc0, const double *bx1f, const double *bx2f,
                     const double *bx3f, double *partial, double *work, void *stream) {
  if (!p || !pack_ok(p, "mri_history")) return AKMI_FAIL;
  if (!u0 || !bcc0 || !bx1f || !bx2f || !bx3f) {
    set_error("mri_history: needs u0, bcc0 and the three face fields (an MHD pack)");
    return AKMI_FAIL;
  }
  if (!partial || !work) { set_error("mri_history: null partial or work array"); return AKMI_FAIL; }
  if (p->nx2 == 1 || p->nx3 == 1) { set_error("mri_history: a 3-D pack"); return AKMI_FAIL; }
  if (p->nvar < (p->is_ideal ? 5 : 4)) { set_error("mri_history: nvar = %d", p->nvar); return AKMI_FAIL; }
  const TurbGeo g = make_tgeo(p);
  if ((long long)p->nmb*g.ntile >= (1ll << 31)) { set_error("mri_history: too many tiles for one launch"); return AKMI_FAIL; }
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)(p->nmb*g.ntile);
  if (p->is_ideal) {
    k_mri_hist<16><<<grid, NT, 0, st>>>(g, p->dx, u0, bcc0, bx1f, bx2f, bx3f, work);
    AKMI_CHECK_LAUNCH("mri_history");
    return finish_partials<16>(g, p->nmb, work, partial, st, "mri_history partials");
  }
  k_mri_hist<15><<<grid, NT, 0, st>>>(g, p->dx, u0, bcc0, bx1f, bx2f, bx3f, work);
  AKMI_CHECK_LAUNCH("mri_history");
  return finish_partials<15>(g, p->nmb, work, partial, st, "mri_history partials");
}

}  // extern "C"
