// akmi_mg.hip -- self-gravity: the multigrid Poisson solver (src/multigrid/, src/gravity/) and the SelfGravity
// source term (src/srcterms/srcterms.cpp:215-310).  DESIGN section 19.
//
// One MG level of the MeshBlock pack is an array (nmb, 1, n+2, n+2, n+2): n active cells per direction and ONE ghost
// layer (mg_nghost = 1).  The root grid is the same thing with nmb = 1 and (nrx3, nrx2, nrx1) active cells, so every
// operator below serves both.  One thread owns one cell (the smoother: one cell of its colour); every value is formed
// with the reference's sequence of roundings (the library is built with -ffp-contract=off), and no operator reads a
// cell that the same launch writes, so the results do not depend on the launch geometry.
//
// Sums (average, defect norm) have ONE order: the cells of a row (m, k, j) ascending in i, the rows of a plane
// ascending in j, the planes of a block ascending in k, the blocks ascending in m -- four small launches, each value
// written once (l_reduce).
//
// Physical (non-periodic) faces of the mesh -- mirror and multipole ghosts inside the exchange launch, the multipole
// moments, the source mask -- are DESIGN section 21; with mg_bc = none the solver runs the periodic kernels alone.
//
// akmi_mg_solve enqueues a whole MGGravityDriver::Solve from here through the same launch functions the
// single-operator entry points use; the host reads defect norms back only where threshold >= 0 asks for them.
#include <cmath>
#include "akmi_common.hpp"

namespace akmi {
namespace {

constexpr int TB = 256;
long long g_launches = 0;         // launches enqueued since the counter was last reset (akmi_mg_launch_count)

struct Lv { int nmb, nz, ny, nx; };     // active cells of one level

__host__ __device__ __forceinline__ long long cells_all(const Lv &g) {
  return (long long)g.nmb*(g.nz + 2)*(g.ny + 2)*(g.nx + 2);
}
__host__ __device__ __forceinline__ long long cells_act(const Lv &g) { return (long long)g.nmb*g.nz*g.ny*g.nx; }
__device__ __forceinline__ size_t at(const Lv &g, int m, int k, int j, int i) {
  return (((size_t)m*(g.nz + 2) + k)*(g.ny + 2) + j)*(g.nx + 2) + i;
}
// active cell t -> (m, k, j, i), array indices (ghost offset included)
__device__ __forceinline__ void act_of(const Lv &g, long long t, int &m, int &k, int &j, int &i) {
  i = (int)(t % g.nx) + 1; t /= g.nx;
  j = (int)(t % g.ny) + 1; t /= g.ny;
  k = (int)(t % g.nz) + 1;
  m = (int)(t / g.nz);
}
__device__ __forceinline__ void all_of(const Lv &g, long long t, int &m, int &k, int &j, int &i) {
  i = (int)(t % (g.nx + 2)); t /= (g.nx + 2);
  j = (int)(t % (g.ny + 2)); t /= (g.ny + 2);
  k = (int)(t % (g.nz + 2));
  m = (int)(t / (g.nz + 2));
}
inline dim3 grid_of(long long n) { return dim3((unsigned)((n + TB - 1)/TB)); }
__device__ __forceinline__ long long tid() { return (long long)blockIdx.x*TB + threadIdx.x; }

// GravityStencil::Apply, mg_gravity.hpp:32-34
__device__ __forceinline__ double lap7(const double *u, size_t c, size_t sy, size_t sz) {
  return 6.0*u[c] - u[c + sz] - u[c + sy] - u[c + 1] - u[c - sz] - u[c - sy] - u[c - 1];
}

// Multigrid::Smooth, multigrid.hpp:622-647: one colour.  t runs over (m, k, j, every second i)
__global__ void __launch_bounds__(TB)
k_smooth(Lv g, double dx2, double odiag, int color, double *__restrict__ u, const double *__restrict__ src) {
  const int nh = (g.nx + 1)/2;
  long long t = tid();
  if (t >= (long long)g.nmb*g.nz*g.ny*nh) return;
  const int ii = (int)(t % nh); t /= nh;
  const int j = (int)(t % g.ny) + 1; t /= g.ny;
  const int k = (int)(t % g.nz) + 1;
  const int m = (int)(t / g.nz);
  const int c = (color + k + j) & 1;
  const int i = 1 + c + 2*ii;
  if (i > g.nx) return;
  const size_t sy = g.nx + 2, sz = sy*(g.ny + 2), q = at(g, m, k, j, i);
  const double lap = lap7(u, q, sy, sz);
  u[q] -= (lap - src[q]*dx2)*odiag;
}

// Multigrid::CalculateDefect / CalculateFASRHS, multigrid.hpp:284-311
template <bool FAS>
__global__ void __launch_bounds__(TB)
k_defect(Lv g, double idx2, const double *__restrict__ u, double *src, double *def) {
  const long long t = tid();
  if (t >= cells_act(g)) return;
  int m, k, j, i;
  act_of(g, t, m, k, j, i);
  const size_t sy = g.nx + 2, sz = sy*(g.ny + 2), q = at(g, m, k, j, i);
  if (FAS) src[q] += lap7(u, q, sy, sz)*idx2;
  else def[q] = src[q] - lap7(u, q, sy, sz)*idx2;
}

// Multigrid::Restrict, multigrid.cpp:874-894; c = coarse level, the fine level has twice the cells
__global__ void __launch_bounds__(TB)
k_restrict(Lv c, const double *__restrict__ fine, double *__restrict__ coarse) {
  const long long t = tid();
  if (t >= cells_act(c)) return;
  int m, k, j, i;
  act_of(c, t, m, k, j, i);
  const Lv f{c.nmb, 2*c.nz, 2*c.ny, 2*c.nx};
  const int fk = 2*k - 1, fj = 2*j - 1, fi = 2*i - 1;
  coarse[at(c, m, k, j, i)] = 0.125*(
      fine[at(f, m, fk, fj, fi)] + fine[at(f, m, fk, fj, fi + 1)]
    + fine[at(f, m, fk, fj + 1, fi)] + fine[at(f, m, fk, fj + 1, fi + 1)]
    + fine[at(f, m, fk + 1, fj, fi)] + fine[at(f, m, fk + 1, fj, fi + 1)]
    + fine[at(f, m, fk + 1, fj + 1, fi)] + fine[at(f, m, fk + 1, fj + 1, fi + 1)]);
}

// Multigrid::ProlongateAndCorrect, trilinear branch, multigrid.cpp:1053-1092: the child (dk, dj, di) of coarse cell
// (k, j, i) leans towards the coarse neighbours on its side
__global__ void __launch_bounds__(TB)
k_prolong(Lv c, const double *__restrict__ s, double *__restrict__ fine) {
  const long long t = tid();
  if (t >= cells_act(c)) return;
  int m, k, j, i;
  act_of(c, t, m, k, j, i);
  const Lv f{c.nmb, 2*c.nz, 2*c.ny, 2*c.nx};
  const int fk = 2*(k - 1) + 1, fj = 2*(j - 1) + 1, fi = 2*(i - 1) + 1;
  const double s0 = s[at(c, m, k, j, i)];
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const int ck = n >> 2, cj = (n >> 1) & 1, ci = n & 1;
    const int dk = 2*ck - 1, dj = 2*cj - 1, di = 2*ci - 1;
    fine[at(f, m, fk + ck, fj + cj, fi + ci)] +=
        0.015625*(27.0*s0 + s[at(c, m, k + dk, j + dj, i + di)]
                  + 9.0*(s[at(c, m, k, j, i + di)] + s[at(c, m, k, j + dj, i)] + s[at(c, m, k + dk, j, i)])
                  + 3.0*(s[at(c, m, k + dk, j + dj, i)] + s[at(c, m, k + dk, j, i + di)]
                         + s[at(c, m, k, j + dj, i + di)]));
  }
}

// Multigrid::FMGProlongate, multigrid.cpp:1116-1218: tricubic, overwrites.  The 27 coefficients of a child are the
// products of the per-axis weights (5, 30, -3) for the lower child and (-3, 30, 5) for the upper one -- integers, so
// the product is the literal the reference writes; the terms are added in its order (k-1, j-1, i-1 first, i fastest).
__global__ void __launch_bounds__(TB)
k_fmg_prolong(Lv c, const double *__restrict__ s, double *__restrict__ fine) {
  const long long t = tid();
  if (t >= cells_act(c)) return;
  int m, k, j, i;
  act_of(c, t, m, k, j, i);
  const Lv f{c.nmb, 2*c.nz, 2*c.ny, 2*c.nx};
  const int fk = 2*(k - 1) + 1, fj = 2*(j - 1) + 1, fi = 2*(i - 1) + 1;
  double v[27];
#pragma unroll
  for (int n = 0; n < 27; ++n) v[n] = s[at(c, m, k + n/9 - 1, j + (n/3)%3 - 1, i + n%3 - 1)];
  const double w[2][3] = {{5.0, 30.0, -3.0}, {-3.0, 30.0, 5.0}};
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    const int ck = n >> 2, cj = (n >> 1) & 1, ci = n & 1;
    double acc = (w[ck][0]*w[cj][0]*w[ci][0])*v[0];
#pragma unroll
    for (int q = 1; q < 27; ++q) acc += (w[ck][q/9]*w[cj][(q/3)%3]*w[ci][q%3])*v[q];
    fine[at(f, m, fk + ck, fj + cj, fi + ci)] = acc/32768.0;
  }
}

// StoreOldData (op 0: dst = src), ComputeCorrection (1: dst -= src), ZeroClearData (2), SubtractAverage (3: dst -= *src)
template <int OP>
__global__ void __launch_bounds__(TB)
k_array(long long n, double *__restrict__ dst, const double *__restrict__ src) {
  const long long t = tid();
  if (t >= n) return;
  if (OP == 0) dst[t] = src[t];
  if (OP == 1) dst[t] -= src[t];
  if (OP == 2) dst[t] = 0.0;
  if (OP == 3) dst[t] -= src[0];
}

// periodic ghost exchange of one level: every ghost cell takes the active cell it is the image of, from the
// neighbour in its direction (nghbr == nullptr: every neighbour is the block itself -- the root grid, MGRootBoundary).
// Reads active cells and writes ghost cells only.
__global__ void __launch_bounds__(TB)
k_exchange(Lv g, const int *__restrict__ nghbr, double *u) {
  const long long t = tid();
  if (t >= cells_all(g)) return;
  int m, k, j, i;
  all_of(g, t, m, k, j, i);
  const int o3 = (k == 0) ? -1 : (k == g.nz + 1 ? 1 : 0);
  const int o2 = (j == 0) ? -1 : (j == g.ny + 1 ? 1 : 0);
  const int o1 = (i == 0) ? -1 : (i == g.nx + 1 ? 1 : 0);
  if (o1 == 0 && o2 == 0 && o3 == 0) return;
  const int nb = nghbr ? nghbr[m*27 + (o3 + 1)*9 + (o2 + 1)*3 + (o1 + 1)] : m;
  if (nb < 0 || nb >= g.nmb) return;
  u[at(g, m, k, j, i)] = u[at(g, nb, k - o3*g.nz, j - o2*g.ny, i - o1*g.nx)];
}

// ---- physical faces: mirror (zerofixed / zerograd) and multipole boundaries, DESIGN section 21 ----------------------
// CellCenterX, src/coordinates/cell_locations.hpp:35-39
__device__ __forceinline__ double cell_center_x(int ith, int n, double xmin, double xmax) {
  const double x = ((double)ith + 0.5)/(double)n;
  return (x*xmax - x*xmin) - (0.5*xmax - 0.5*xmin) + (0.5*xmin + 0.5*xmax);
}
constexpr int MP_NCOEF = 25, MP_ORIGIN = 25, MP_DOUBLES = 28;     // mp[0..24] coefficients, mp[25..27] origin (x, y, z)

// EvalMultipolePhi, multigrid.hpp:680-708
__device__ __forceinline__ double eval_multipole_phi(double x, double y, double z, const double *mpc, int order) {
  const double x2 = x*x, y2 = y*y, z2 = z*z;
  const double xy = x*y, yz = y*z, zx = z*x;
  const double r2 = x2 + y2 + z2;
  const double ir2 = 1.0/r2, ir1 = sqrt(ir2);
  const double ir3 = ir2*ir1, ir5 = ir3*ir2;
  const double hx2my2 = 0.5*(x2 - y2);
  double phis = ir1*mpc[0]
    + ir3*(mpc[1]*y + mpc[2]*z + mpc[3]*x)
    + ir5*(mpc[4]*xy + mpc[5]*yz + (3.0*z2 - r2)*mpc[6]
         + mpc[7]*zx + mpc[8]*hx2my2);
  if (order == 4) {
    const double ir7 = ir5*ir2, ir9 = ir7*ir2;
    const double x2mty2 = x2 - 3.0*y2;
    const double tx2my2 = 3.0*x2 - y2;
    phis += ir7*(y*tx2my2*mpc[9] + x*x2mty2*mpc[15]
               + xy*z*mpc[10] + z*hx2my2*mpc[14]
               + (5.0*z2 - r2)*(y*mpc[11] + x*mpc[13])
               + z*(z2 - 3.0*r2)*mpc[12])
         + ir9*(xy*hx2my2*mpc[16]
               + 0.125*(x2*x2mty2 - y2*tx2my2)*mpc[24]
               + yz*tx2my2*mpc[17] + zx*x2mty2*mpc[23]
               + (7.0*z2 - r2)*(xy*mpc[18] + hx2my2*mpc[22])
               + (7.0*z2 - 3.0*r2)*(yz*mpc[19] + zx*mpc[21])
               + (35.0*z2*z2 - 30.0*z2*r2 + 3.0*r2*r2)*mpc[20]);
  }
  return phis;
}

struct Bc {
  int type;              // AKMI_MGBC_*
  int order;             // mporder
  int periodic;          // root grid (nghbr == nullptr): bit f set = face f of the mesh (ix1, ox1, ix2, ...) is periodic
  const double *mp;      // multipole: MP_DOUBLES doubles
  const double *xlim;    // multipole, block levels: x1min, x1max, x2min, ... of every block
  double ext[6];         // multipole, root grid: the extents of the mesh
};

// MultigridBoundaryValues receive + PhysicalBoundary (multigrid_tasks.cpp:129-360) / MGRootBoundary
// (multigrid_driver.cpp:1835-2026) in one launch.  A direction in which the ghost cell lies beyond a physical face (no
// face neighbour: table entry < 0; root grid: the face is not periodic) is mirrored, the others take the neighbour's
// image, and the value is multiplied by -1 per mirrored direction under zerofixed: the composite of the reference's
// x1, x2, x3 sweeps over the full extent.  Multipole: face ghosts over active cells = 2*phis - interior, edge and
// corner ghosts that touch a physical face are left alone.  Reads active cells and writes ghost cells only.
__global__ void __launch_bounds__(TB)
k_exchange_bc(Lv g, const int *__restrict__ nghbr, Bc b, double *u) {
  const long long t = tid();
  if (t >= cells_all(g)) return;
  int m, k, j, i;
  all_of(g, t, m, k, j, i);
  const int n[3] = {g.nx, g.ny, g.nz};
  const int c[3] = {i, j, k};
  int o[3], ph[3], nphys = 0, nout = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    o[d] = (c[d] == 0) ? -1 : (c[d] == n[d] + 1 ? 1 : 0);
    ph[d] = 0;
    if (o[d] != 0) {
      ++nout;
      const int st = (d == 0) ? 1 : (d == 1 ? 3 : 9);
      if (nghbr) ph[d] = nghbr[m*27 + 13 + o[d]*st] < 0;
      else ph[d] = !((b.periodic >> (2*d + (o[d] > 0 ? 1 : 0))) & 1);
      nphys += ph[d];
    }
  }
  if (nout == 0) return;
  if (nphys > 0 && b.type == AKMI_MGBC_NONE) return;
  if (nphys > 0 && b.type == AKMI_MGBC_MULTIPOLE) {
    if (nout != 1) return;
    const double *e = nghbr ? b.xlim + 6*(size_t)m : b.ext;
    double x[3];
    int s[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double lo = e[2*d], hi = e[2*d + 1], org = b.mp[MP_ORIGIN + d];
      if (o[d] != 0) {
        x[d] = (o[d] < 0 ? lo : hi) - org;
        s[d] = (o[d] < 0) ? 1 : n[d];
      } else {
        const double dxl = (hi - lo)/static_cast<double>(n[d]);
        x[d] = lo + ((c[d] - 1) + 0.5)*dxl - org;
        s[d] = c[d];
      }
    }
    const double phis = eval_multipole_phi(x[0], x[1], x[2], b.mp, b.order);
    u[at(g, m, k, j, i)] = 2.0*phis - u[at(g, m, s[2], s[1], s[0])];
    return;
  }
  int s[3], on[3];
  double sign = 1.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (ph[d]) {
      on[d] = 0;
      s[d] = (o[d] < 0) ? 1 : n[d];
      if (b.type == AKMI_MGBC_ZEROFIXED) sign = -sign;
    } else {
      on[d] = o[d];
      s[d] = c[d] - o[d]*n[d];
    }
  }
  int nb = m;
  if (nghbr && (on[0] != 0 || on[1] != 0 || on[2] != 0)) nb = nghbr[m*27 + (on[2] + 1)*9 + (on[1] + 1)*3 + (on[0] + 1)];
  if (nb < 0 || nb >= g.nmb) return;
  const double v = u[at(g, nb, s[2], s[1], s[0])];
  u[at(g, m, k, j, i)] = (nphys > 0) ? sign*v : v;
}

// Multigrid::ApplyMask, multigrid.cpp:360-388: active cells of the finest level
__global__ void __launch_bounds__(TB)
k_mask(Lv g, const double *__restrict__ xlim, double mask_r2, double ox, double oy, double oz, double *__restrict__ src) {
  const long long t = tid();
  if (t >= cells_act(g)) return;
  int m, k, j, i;
  act_of(g, t, m, k, j, i);
  const double *e = xlim + 6*(size_t)m;
  const double x = cell_center_x(i - 1, g.nx, e[0], e[1]);
  const double y = cell_center_x(j - 1, g.ny, e[2], e[3]);
  const double z = cell_center_x(k - 1, g.nz, e[4], e[5]);
  const double r2 = (x - ox)*(x - ox) + (y - oy)*(y - oy) + (z - oz)*(z - oz);
  if (r2 > mask_r2) src[at(g, m, k, j, i)] = 0.0;
}

// CalculateCenterOfMass (nc = 4, multigrid_driver.cpp:2374-2434) / CalculateMultipoleCoefficients (nc = 9 or 25,
// :2213-2315): the sums of one row (m, k, j), ascending in i, component c at rows[c*nrows + row]
template <int NC>
__global__ void __launch_bounds__(TB)
k_mp_rows(Lv g, int nodipole, const double *__restrict__ xlim, const double *__restrict__ mpo,
          const double *__restrict__ src, double *__restrict__ rows) {
  long long t = tid();
  const long long nrows = (long long)g.nmb*g.nz*g.ny;
  if (t >= nrows) return;
  const long long r = t;
  const int j = (int)(t % g.ny) + 1; t /= g.ny;
  const int k = (int)(t % g.nz) + 1;
  const int m = (int)(t / g.nz);
  const double *e = xlim + 6*(size_t)m;
  const double dx1 = (e[1] - e[0])/static_cast<double>(g.nx);
  const double dx2 = (e[3] - e[2])/static_cast<double>(g.ny);
  const double dx3 = (e[5] - e[4])/static_cast<double>(g.nz);
  const double vol = dx1*dx2*dx3;
  const double *p = src + at(g, m, k, j, 1);
  double mp[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) mp[c] = 0.0;
  if constexpr (NC == 4) {
    const double z = e[4] + ((k - 1) + 0.5)*dx3;
    const double y = e[2] + ((j - 1) + 0.5)*dx2;
    for (int ii = 0; ii < g.nx; ++ii) {
      const double x = e[0] + (ii + 0.5)*dx1;
      const double s = p[ii]*vol;
      mp[0] += s;
      mp[1] += s*y;
      mp[2] += s*z;
      mp[3] += s*x;
    }
  } else {
    const double z = e[4] + ((k - 1) + 0.5)*dx3 - mpo[2];
    const double z2 = z*z;
    const double y = e[2] + ((j - 1) + 0.5)*dx2 - mpo[1];
    const double y2 = y*y;
    const double yz = y*z;
    for (int ii = 0; ii < g.nx; ++ii) {
      const double x = e[0] + (ii + 0.5)*dx1 - mpo[0];
      const double x2 = x*x;
      const double xy = x*y;
      const double zx = z*x;
      const double r2 = x2 + y2 + z2;
      const double s = p[ii]*vol;
      mp[0] += s;
      if (!nodipole) {
        mp[1] += s*y;
        mp[2] += s*z;
        mp[3] += s*x;
      }
      const double hx2my2 = 0.5*(x2 - y2);
      mp[4] += s*xy;
      mp[5] += s*yz;
      mp[6] += s*(3.0*z2 - r2);
      mp[7] += s*zx;
      mp[8] += s*hx2my2;
      if constexpr (NC == 25) {
        const double tx2my2 = 3.0*x2 - y2;
        const double x2mty2 = x2 - 3.0*y2;
        const double fz2mr2 = 5.0*z2 - r2;
        mp[9] += s*y*tx2my2;
        mp[10] += s*xy*z;
        mp[11] += s*y*fz2mr2;
        mp[12] += s*z*(z2 - 3.0*r2);
        mp[13] += s*x*fz2mr2;
        mp[14] += s*z*hx2my2;
        mp[15] += s*x*x2mty2;
        const double sz2mr2 = 7.0*z2 - r2;
        const double sz2mtr2 = 7.0*z2 - 3.0*r2;
        mp[16] += s*xy*hx2my2;
        mp[17] += s*yz*tx2my2;
        mp[18] += s*xy*sz2mr2;
        mp[19] += s*yz*sz2mtr2;
        mp[20] += s*(35.0*z2*z2 - 30.0*z2*r2 + 3.0*r2*r2);
        mp[21] += s*zx*sz2mtr2;
        mp[22] += s*hx2my2*sz2mr2;
        mp[23] += s*zx*x2mty2;
        mp[24] += s*0.125*(x2*x2mty2 - y2*tx2my2);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) rows[c*nrows + r] = mp[c];
}

// the blocks (ascending m) of component c = threadIdx.x, then: nc = 4: the origin 1/m0 * (m3, m1, m2) into
// mp[MP_ORIGIN..]; otherwise ScaleMultipoleCoefficients (multigrid_driver.cpp:2322-2367) into mp[c]
__global__ void k_mp_final(int nmb, int nc, const double *__restrict__ in, double *__restrict__ mp) {
  const int c = threadIdx.x;
  if (blockIdx.x != 0 || c >= nc) return;
  double s = 0.0;
  for (int m = 0; m < nmb; ++m) s += in[(size_t)c*nmb + m];
  if (nc == 4) {
    if (c == 0) return;
    double m0 = 0.0;
    for (int m = 0; m < nmb; ++m) m0 += in[m];
    const double im = 1.0/m0;
    mp[MP_ORIGIN + (c == 3 ? 0 : c)] = im*s;
    return;
  }
  constexpr double c0 = 0.25/M_PI, c1 = 0.25/M_PI, c2 = 0.0625/M_PI, c2a = 0.75/M_PI;
  constexpr double c30 = 0.0625/M_PI, c31 = 0.0625*1.5/M_PI, c32 = 0.25*15.0/M_PI, c33 = 0.0625*2.5/M_PI;
  constexpr double c40 = 0.0625*0.0625/M_PI, c41 = 0.0625*2.5/M_PI, c42 = 0.0625*5.0/M_PI, c43 = 0.0625*17.5/M_PI;
  constexpr double c44 = 0.25*35.0/M_PI;
  const double scale[MP_NCOEF] = {c0, c1, c1, c1, c2a, c2a, c2, c2a, c2a, c33, c32, c31, c30, c31, c32, c33,
                                  c44, c43, c42, c41, c40, c41, c42, c43, c44};
  mp[c] = s*scale[c];
}
__global__ void k_mp_set_origin(double x, double y, double z, double *__restrict__ mp) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  mp[MP_ORIGIN] = x; mp[MP_ORIGIN + 1] = y; mp[MP_ORIGIN + 2] = z;
}

// MultigridDriver::TransferFromBlocksToRoot, multigrid_driver.cpp:479-548: the one cell of every block's coarsest level
__global__ void __launch_bounds__(TB)
k_to_root(int nmb, Lv r, const int *__restrict__ lloc, int initflag, const double *__restrict__ bsrc,
          const double *__restrict__ bu, double *__restrict__ rsrc, double *__restrict__ ru) {
  const long long m = tid();
  if (m >= nmb) return;
  const int i = lloc[3*m], j = lloc[3*m + 1], k = lloc[3*m + 2];
  if (i < 0 || i >= r.nx || j < 0 || j >= r.ny || k < 0 || k >= r.nz) return;
  const size_t q = at(r, 0, k + 1, j + 1, i + 1);
  rsrc[q] = bsrc[m*27 + 13];
  if (!initflag) ru[q] = bu[m*27 + 13];
}

// Multigrid::SetFromRootGrid, multigrid.cpp:617-676: the 3^3 patch of the root grid around every block
__global__ void __launch_bounds__(TB)
k_from_root(int nmb, Lv r, const int *__restrict__ lloc, int fold, const double *__restrict__ ru,
            const double *__restrict__ ruold, double *__restrict__ bu, double *__restrict__ buold) {
  const long long t = tid();
  if (t >= (long long)nmb*27) return;
  const int m = (int)(t/27), n = (int)(t%27);
  const int ci = lloc[3*m], cj = lloc[3*m + 1], ck = lloc[3*m + 2];
  if (ci < 0 || ci >= r.nx || cj < 0 || cj >= r.ny || ck < 0 || ck >= r.nz) return;
  const size_t q = at(r, 0, ck + n/9, cj + (n/3)%3, ci + n%3);
  bu[t] = ru[q];
  if (fold) buold[t] = ruold[q];
}

// Multigrid::LoadSource / LoadFinestData / RetrieveResult, multigrid.cpp:261-320,420-451.  f: the fluid-shaped
// array (nmb, nvar, n+2ng, ...), variable 0; ghost = 1: the one ghost layer of the MG array takes part
template <int OP>    // 0: mg = f*fac (all cells), 1: mg = f (active cells), 2: f = mg (all cells)
__global__ void __launch_bounds__(TB)
k_load(Lv g, int ng, int nvar, double fac, double *mg, double *f) {
  const long long t = tid();
  int m, k, j, i;
  if (OP == 1) {
    if (t >= cells_act(g)) return;
    act_of(g, t, m, k, j, i);
  } else {
    if (t >= cells_all(g)) return;
    all_of(g, t, m, k, j, i);
  }
  const int off = ng - 1;
  const size_t N1 = g.nx + 2*ng, N2 = g.ny + 2*ng, N3 = g.nz + 2*ng;
  const size_t qf = ((((size_t)m*nvar)*N3 + (k + off))*N2 + (j + off))*N1 + (i + off);
  const size_t q = at(g, m, k, j, i);
  if (OP == 0) mg[q] = (fac == 1.0) ? f[qf] : f[qf]*fac;
  if (OP == 1) mg[q] = f[qf];
  if (OP == 2) f[qf] = mg[q];
}

// the sums: rows (ascending i), then one axis at a time.  kind 0: a*dV (CalculateAverage), 1: a*a (defect norm, l2)
__global__ void __launch_bounds__(TB)
k_sum_rows(Lv g, int kind, double dV, const double *__restrict__ a, double *__restrict__ rows) {
  long long t = tid();
  if (t >= (long long)g.nmb*g.nz*g.ny) return;
  const long long r = t;
  const int j = (int)(t % g.ny) + 1; t /= g.ny;
  const int k = (int)(t % g.nz) + 1;
  const int m = (int)(t / g.nz);
  const double *p = a + at(g, m, k, j, 1);
  double s = kind ? p[0]*p[0] : p[0]*dV;
  for (int i = 1; i < g.nx; ++i) s += kind ? p[i]*p[i] : p[i]*dV;
  rows[r] = s;
}
__global__ void __launch_bounds__(TB)
k_sum_axis(long long nout, int n, const double *__restrict__ in, double *__restrict__ out) {
  const long long t = tid();
  if (t >= nout) return;
  double s = in[t*n];
  for (int q = 1; q < n; ++q) s += in[t*n + q];
  out[t] = s;
}
// the blocks (ascending m), then kind 0: sum/volume (0 where volume <= 0), kind 1: sqrt(sum/volume)
__global__ void k_sum_final(int n, int kind, double volume, const double *__restrict__ in, double *__restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double s = in[0];
  for (int q = 1; q < n; ++q) s += in[q];
  if (kind == 0) out[0] = (volume > 0.0) ? (s/volume) : 0.0;
  else { s /= volume; out[0] = sqrt(s); }
}

// SourceTerms::SelfGravity, srcterms.cpp:248-303: the three directions for one cell, x1 then x2 then x3
__global__ void __launch_bounds__(TB)
k_selfgravity(int nmb, int nvar, int nx1, int nx2, int nx3, int ng, int is_ideal, int face, double bdt,
              const double *__restrict__ dx, const double *__restrict__ w0, const double *__restrict__ phi,
              const double *__restrict__ f1, const double *__restrict__ f2, const double *__restrict__ f3,
              double *__restrict__ u0) {
  long long t = tid();
  if (t >= (long long)nmb*nx1*nx2*nx3) return;
  const bool multi_d = nx2 > 1, three_d = nx3 > 1;
  const int i = (int)(t % nx1) + ng; t /= nx1;
  const int j = (int)(t % nx2) + (multi_d ? ng : 0); t /= nx2;
  const int k = (int)(t % nx3) + (three_d ? ng : 0);
  const int m = (int)(t / nx3);
  const size_t N1 = nx1 + 2*ng, N2 = multi_d ? nx2 + 2*ng : 1, N3 = three_d ? nx3 + 2*ng : 1;
  const size_t cs = N3*N2*N1, c = ((size_t)k*N2 + j)*N1 + i;
  const double *ph = phi + (size_t)m*cs;
  const double *wm = w0 + (size_t)m*nvar*cs;
  double *um = u0 + (size_t)m*nvar*cs;
  const double rho = wm[c];
  {
    const double hdtodx1 = 0.5*bdt/dx[3*m];
    const double dpl = -(ph[c] - ph[c - 1]);
    const double dpr = -(ph[c + 1] - ph[c]);
    um[cs + c] += hdtodx1*rho*(dpl + dpr);
    if (is_ideal) {
      const size_t F1 = N1 + face, fc = ((size_t)m*nvar*N3*N2 + (size_t)k*N2 + j)*F1 + i;
      um[4*cs + c] += hdtodx1*(f1[fc]*dpl + f1[fc + 1]*dpr);
    }
  }
  if (multi_d) {
    const double hdtodx2 = 0.5*bdt/dx[3*m + 1];
    const double dpl = -(ph[c] - ph[c - N1]);
    const double dpr = -(ph[c + N1] - ph[c]);
    um[2*cs + c] += hdtodx2*rho*(dpl + dpr);
    if (is_ideal) {
      const size_t F2 = N2 + face, fc = (((size_t)m*nvar*N3 + k)*F2 + j)*N1 + i;
      um[4*cs + c] += hdtodx2*(f2[fc]*dpl + f2[fc + N1]*dpr);
    }
  }
  if (three_d) {
    const double hdtodx3 = 0.5*bdt/dx[3*m + 2];
    const double dpl = -(ph[c] - ph[c - N2*N1]);
    const double dpr = -(ph[c + N2*N1] - ph[c]);
    um[3*cs + c] += hdtodx3*rho*(dpl + dpr);
    if (is_ideal) {
      const size_t F3 = N3 + face, fc = (((size_t)m*nvar*F3 + k)*N2 + j)*N1 + i;
      um[4*cs + c] += hdtodx3*(f3[fc]*dpl + f3[fc + N2*N1]*dpr);
    }
  }
}

// ---- launch functions: what the entry points and the solver share -----------------------------------------------
bool lv_ok(const Lv &g) {
  return g.nmb >= 1 && g.nz >= 1 && g.ny >= 1 && g.nx >= 1 && cells_all(g) < ((long long)1 << 40);
}
#define MG_LAUNCH(kernel, n, ...)                                            \
  do {                                                                       \
    if ((n) > 0) {                                                           \
      kernel<<<grid_of(n), TB, 0, st>>>(__VA_ARGS__);                        \
      ++g_launches;                                                          \
    }                                                                        \
  } while (0)

void l_smooth(hipStream_t st, const Lv &g, double dx, double omega, int color, int coffset, double *u, const double *src) {
  MG_LAUNCH(k_smooth, (long long)g.nmb*g.nz*g.ny*((g.nx + 1)/2), g, dx*dx, omega/6.0, color ^ coffset, u, src);
}
void l_defect(hipStream_t st, const Lv &g, double dx, const double *u, double *src, double *def) {
  MG_LAUNCH(k_defect<false>, cells_act(g), g, 1.0/(dx*dx), u, src, def);
}
void l_fas(hipStream_t st, const Lv &g, double dx, const double *u, double *src) {
  MG_LAUNCH(k_defect<true>, cells_act(g), g, 1.0/(dx*dx), u, src, nullptr);
}
void l_restrict(hipStream_t st, const Lv &c, const double *fine, double *coarse) {
  MG_LAUNCH(k_restrict, cells_act(c), c, fine, coarse);
}
void l_prolong(hipStream_t st, const Lv &c, const double *coarse, double *fine) {
  MG_LAUNCH(k_prolong, cells_act(c), c, coarse, fine);
}
void l_fmg_prolong(hipStream_t st, const Lv &c, const double *coarse, double *fine) {
  MG_LAUNCH(k_fmg_prolong, cells_act(c), c, coarse, fine);
}
void l_copy(hipStream_t st, long long n, double *dst, const double *src) { MG_LAUNCH(k_array<0>, n, n, dst, src); }
void l_sub(hipStream_t st, long long n, double *dst, const double *src) { MG_LAUNCH(k_array<1>, n, n, dst, src); }
void l_zero(hipStream_t st, long long n, double *dst) { MG_LAUNCH(k_array<2>, n, n, dst, nullptr); }
void l_sub_scalar(hipStream_t st, long long n, double *dst, const double *ave) { MG_LAUNCH(k_array<3>, n, n, dst, ave); }
void l_exchange(hipStream_t st, const Lv &g, const int *nghbr, double *u) {
  MG_LAUNCH(k_exchange, cells_all(g), g, nghbr, u);
}
void l_exchange_bc(hipStream_t st, const Lv &g, const int *nghbr, const Bc &b, double *u) {
  MG_LAUNCH(k_exchange_bc, cells_all(g), g, nghbr, b, u);
}
void l_mask(hipStream_t st, const Lv &g, const double *xlim, double radius, const double *origin, double *src) {
  MG_LAUNCH(k_mask, cells_act(g), g, xlim, radius*radius, origin[0], origin[1], origin[2], src);
}
// scratch: nmb*nz*ny + nmb*nz + nmb doubles
long long scratch_doubles(const Lv &g) { return (long long)g.nmb*g.nz*g.ny + (long long)g.nmb*g.nz + g.nmb; }
void l_reduce(hipStream_t st, const Lv &g, int kind, double dV, double volume, const double *a, double *scratch,
              double *out) {
  double *rows = scratch, *planes = rows + (long long)g.nmb*g.nz*g.ny, *blocks = planes + (long long)g.nmb*g.nz;
  MG_LAUNCH(k_sum_rows, (long long)g.nmb*g.nz*g.ny, g, kind, dV, a, rows);
  MG_LAUNCH(k_sum_axis, (long long)g.nmb*g.nz, (long long)g.nmb*g.nz, g.ny, rows, planes);
  MG_LAUNCH(k_sum_axis, (long long)g.nmb, (long long)g.nmb, g.nz, planes, blocks);
  k_sum_final<<<1, 64, 0, st>>>(g.nmb, kind, volume, blocks, out);
  ++g_launches;
}
// the sums of nc components in the order of l_reduce; scratch: nc*scratch_doubles(g); mp: MP_DOUBLES doubles
void l_mp_sums(hipStream_t st, const Lv &g, int nc, int nodipole, const double *xlim, const double *src,
               double *scratch, double *mp) {
  const long long nrows = (long long)g.nmb*g.nz*g.ny;
  double *rows = scratch, *planes = rows + nc*nrows, *blocks = planes + (long long)nc*g.nmb*g.nz;
  if (nc == 4) MG_LAUNCH(k_mp_rows<4>, nrows, g, 0, xlim, mp + MP_ORIGIN, src, rows);
  else if (nc == 9) MG_LAUNCH(k_mp_rows<9>, nrows, g, nodipole, xlim, mp + MP_ORIGIN, src, rows);
  else MG_LAUNCH(k_mp_rows<25>, nrows, g, nodipole, xlim, mp + MP_ORIGIN, src, rows);
  MG_LAUNCH(k_sum_axis, (long long)nc*g.nmb*g.nz, (long long)nc*g.nmb*g.nz, g.ny, rows, planes);
  MG_LAUNCH(k_sum_axis, (long long)nc*g.nmb, (long long)nc*g.nmb, g.nz, planes, blocks);
  k_mp_final<<<1, 64, 0, st>>>(g.nmb, nc, blocks, mp);
  ++g_launches;
}
// CalculateCenterOfMass (auto_origin) or the origin of the deck, then CalculateMultipoleCoefficients with
// ScaleMultipoleCoefficients: 8 launches with auto_origin, 5 without
void l_multipole(hipStream_t st, const Lv &g, int order, int nodipole, int auto_origin, const double *origin,
                 const double *xlim, const double *src, double *scratch, double *mp) {
  if (auto_origin) l_mp_sums(st, g, 4, 0, xlim, src, scratch, mp);
  else {
    k_mp_set_origin<<<1, 64, 0, st>>>(origin[0], origin[1], origin[2], mp);
    ++g_launches;
  }
  l_mp_sums(st, g, order == 4 ? 25 : 9, nodipole, xlim, src, scratch, mp);
}
// Multigrid::CalculateAverage, multigrid.cpp:763-818: dV of the level, the volume from nx1 of the FINEST level (len)
void l_average(hipStream_t st, const Lv &g, double dx, double len, const double *a, double *scratch, double *out) {
  double volume = 0.0;
  for (int m = 0; m < g.nmb; ++m) volume += len*len*len;
  l_reduce(st, g, 0, dx*dx*dx, volume, a, scratch, out);
}

// ---- the solver ---------------------------------------------------------------------------------------------------
struct Layout {
  int nmbl, nrl;
  long long boff[24], roff[24], bsz[24], rsz[24], scratch, scalars, total;
};
bool bc_ok(int type, int order, const void *geometry, const char *who) {
  if (type < AKMI_MGBC_NONE || type > AKMI_MGBC_MULTIPOLE) { set_error("%s: unknown boundary type %d", who, type); return false; }
  if (type == AKMI_MGBC_MULTIPOLE && ((order != 2 && order != 4) || !geometry)) {
    set_error("%s: multipole boundaries need mporder 2 or 4 (%d) and the extents", who, order);
    return false;
  }
  return true;
}
bool plan_ok(const akmi_mg_plan *p, const char *who) {
  if (!p) { set_error("%s: null plan", who); return false; }
  if (p->nmb < 1 || p->nxb < 1 || (p->nxb & (p->nxb - 1)) || p->nrx1 < 1 || p->nrx2 < 1 || p->nrx3 < 1) {
    set_error("%s: MeshBlocks must be cubic with a power-of-two edge (nmb %d, edge %d, root %d x %d x %d)", who,
              p->nmb, p->nxb, p->nrx1, p->nrx2, p->nrx3);
    return false;
  }
  int nl = 0;
  while ((1 << nl) < p->nxb) ++nl;
  int nr = 0;
  for (int l = 0; l < 20; ++l)
    if (p->nrx1 % (1 << l) == 0 && p->nrx2 % (1 << l) == 0 && p->nrx3 % (1 << l) == 0) nr = l + 1;
  if (p->nmblevel != nl + 1 || p->nrootlevel != nr || nl + 1 > 20) {
    set_error("%s: nmblevel = %d / nrootlevel = %d do not belong to edge %d and root grid %d x %d x %d", who,
              p->nmblevel, p->nrootlevel, p->nxb, p->nrx1, p->nrx2, p->nrx3);
    return false;
  }
  if ((long long)p->nrx1*p->nrx2*p->nrx3 != p->nmb) {
    set_error("%s: %d MeshBlocks do not tile the root grid %d x %d x %d (one rank, uniform mesh)", who, p->nmb,
              p->nrx1, p->nrx2, p->nrx3);
    return false;
  }
  return true;
}
Lv blk_lv(const akmi_mg_plan *p, int bl) { const int e = p->nxb >> (p->nmblevel - 1 - bl); return Lv{p->nmb, e, e, e}; }
Lv root_lv(const akmi_mg_plan *p, int rl) {
  const int s = p->nrootlevel - 1 - rl;
  return Lv{1, p->nrx3 >> s, p->nrx2 >> s, p->nrx1 >> s};
}
Layout make_layout(const akmi_mg_plan *p) {
  Layout L;
  L.nmbl = p->nmblevel; L.nrl = p->nrootlevel;
  long long o = 0;
  for (int l = 0; l < L.nmbl; ++l) { L.bsz[l] = cells_all(blk_lv(p, l)); L.boff[l] = o; o += 4*L.bsz[l]; }
  for (int l = 0; l < L.nrl; ++l) { L.rsz[l] = cells_all(root_lv(p, l)); L.roff[l] = o; o += 4*L.rsz[l]; }
  L.scratch = o;
  long long a = scratch_doubles(blk_lv(p, L.nmbl - 1));
  const long long b = scratch_doubles(root_lv(p, L.nrl - 1));
  if (p->mg_bc == AKMI_MGBC_MULTIPOLE) a *= MP_NCOEF;          // the moment sums, l_mp_sums
  o += (a > b ? a : b);
  L.scalars = o;
  o += 64 + MP_DOUBLES;          // average, norms; multipole coefficients and origin
  L.total = o;
  return L;
}

enum { U = 0, SRC = 1, DEF = 2, UOLD = 3 };

struct Solver {
  const akmi_mg_plan *p;
  hipStream_t st;
  Layout L;
  int coffset, cl, fmglevel, ntotal, nrl;
  double *ws;

  double *B(int bl, int w) const { return ws + L.boff[bl] + w*L.bsz[bl]; }
  double *R(int rl, int w) const { return ws + L.roff[rl] + w*L.rsz[rl]; }
  double *scratch() const { return ws + L.scratch; }
  double *scalar(int n) const { return ws + L.scalars + n; }
  double bdx(int bl) const { return p->rdx*static_cast<double>(1 << (p->nmblevel - 1 - bl)); }
  double rdx(int rl) const { return p->root_dx*static_cast<double>(1 << (p->nrootlevel - 1 - rl)); }
  int bl_of(int lev) const { return lev - nrl + 1; }

  double *mp() const { return ws + L.scalars + 64; }
  Bc bc() const {
    Bc b{};
    b.type = p->mg_bc; b.order = p->mporder; b.mp = mp(); b.xlim = p->xlim;
    for (int f = 0; f < 6; ++f) { b.periodic |= (p->periodic[f] ? 1 : 0) << f; b.ext[f] = p->mesh_ext[f]; }
    return b;
  }
  // mg_bc = none: the periodic exchange; otherwise the same launch also fills the ghosts beyond physical faces
  void bex(int bl) {
    if (p->mg_bc == AKMI_MGBC_NONE) l_exchange(st, blk_lv(p, bl), p->nghbr, B(bl, U));
    else l_exchange_bc(st, blk_lv(p, bl), p->nghbr, bc(), B(bl, U));
  }
  void rbnd(int rl) {
    if (p->mg_bc == AKMI_MGBC_NONE) l_exchange(st, root_lv(p, rl), nullptr, R(rl, U));
    else l_exchange_bc(st, root_lv(p, rl), nullptr, bc(), R(rl, U));
  }
  void bsmooth(int bl, int color) { l_smooth(st, blk_lv(p, bl), bdx(bl), p->omega, color, coffset, B(bl, U), B(bl, SRC)); }
  void rsmooth(int rl, int color) { l_smooth(st, root_lv(p, rl), rdx(rl), p->omega, color, coffset, R(rl, U), R(rl, SRC)); }

  // MultigridDriver::SubtractAverage: the average of the CURRENT level, taken off the FINEST level of the same
  // Multigrid object (multigrid_driver.cpp:171-174 with multigrid.cpp:763-852)
  void sub_avg_blocks(int w) {
    const int bl = p->nmblevel - 1;
    l_average(st, blk_lv(p, bl), bdx(bl), p->rdx*static_cast<double>(p->nxb), B(bl, w), scratch(), scalar(0));
    l_sub_scalar(st, L.bsz[bl], B(bl, w), scalar(0));
  }
  void sub_avg_root(int w) {
    l_average(st, root_lv(p, 0), rdx(0), p->root_dx*static_cast<double>(p->nrx1), R(0, w), scratch(), scalar(0));
    l_sub_scalar(st, L.rsz[nrl - 1], R(nrl - 1, w), scalar(0));
  }

  void to_root(int initflag) {
    MG_LAUNCH(k_to_root, (long long)p->nmb, p->nmb, root_lv(p, nrl - 1), p->lloc, initflag, B(0, SRC), B(0, U),
              R(nrl - 1, SRC), R(nrl - 1, U));
  }
  void from_root(int fold) {
    MG_LAUNCH(k_from_root, (long long)p->nmb*27, p->nmb, root_lv(p, nrl - 1), p->lloc, fold, R(nrl - 1, U),
              R(nrl - 1, UOLD), B(0, U), B(0, UOLD));
  }

  // OneStepToCoarser, multigrid_driver.cpp:661-706 with SetMGTaskListToCoarser, multigrid_tasks.cpp:537-635
  void to_coarser(int ns) {
    if (cl >= nrl) {
      const int bl = bl_of(cl);
      const Lv g = blk_lv(p, bl);
      bex(bl);
      if (cl < fmglevel) {
        l_copy(st, L.bsz[bl], B(bl, UOLD), B(bl, U));
        l_fas(st, g, bdx(bl), B(bl, U), B(bl, SRC));
      }
      if (ns > 0) {
        bsmooth(bl, coffset); bex(bl); bsmooth(bl, 1 - coffset); bex(bl);
        if (ns > 1) { bsmooth(bl, coffset); bex(bl); bsmooth(bl, 1 - coffset); bex(bl); }
      }
      l_defect(st, g, bdx(bl), B(bl, U), B(bl, SRC), B(bl, DEF));
      l_restrict(st, blk_lv(p, bl - 1), B(bl, DEF), B(bl - 1, SRC));
      l_restrict(st, blk_lv(p, bl - 1), B(bl, U), B(bl - 1, U));
      if (cl == nrl) to_root(0);
    } else {
      const int rl = cl;
      const Lv g = root_lv(p, rl);
      rbnd(rl);
      if (cl < fmglevel) {
        l_copy(st, L.rsz[rl], R(rl, UOLD), R(rl, U));
        l_fas(st, g, rdx(rl), R(rl, U), R(rl, SRC));
      }
      for (int n = 0; n < ns; ++n) { rsmooth(rl, coffset); rbnd(rl); rsmooth(rl, 1 - coffset); rbnd(rl); }
      l_defect(st, g, rdx(rl), R(rl, U), R(rl, SRC), R(rl, DEF));
      l_restrict(st, root_lv(p, rl - 1), R(rl, DEF), R(rl - 1, SRC));
      l_restrict(st, root_lv(p, rl - 1), R(rl, U), R(rl - 1, U));
    }
    --cl;
  }

  // OneStepToFiner, multigrid_driver.cpp:609-654 with SetMGTaskListToFiner, multigrid_tasks.cpp:368-488
  void to_finer(int ns) {
    if (cl == nrl - 1) { rbnd(nrl - 1); from_root(1); }
    if (cl >= nrl - 1) {
      const int bl = bl_of(cl);
      int flag = 0;
      if (cl == nrl - 1) flag = 1;
      if (cl == ntotal - 2) flag = 2;
      if (flag != 1) bex(bl);
      l_sub(st, L.bsz[bl], B(bl, U), B(bl, UOLD));
      l_prolong(st, blk_lv(p, bl), B(bl, U), B(bl + 1, U));
      const int fl = bl + 1;
      if (ns > 0) {
        bex(fl); bsmooth(fl, coffset); bex(fl); bsmooth(fl, 1 - coffset);
        if (ns > 1) { bex(fl); bsmooth(fl, coffset); bex(fl); bsmooth(fl, 1 - coffset); }
      }
      if (flag == 2) bex(fl);
      ++cl;
    } else {
      const int rl = cl;
      rbnd(rl);
      l_sub(st, L.rsz[rl], R(rl, U), R(rl, UOLD));
      l_prolong(st, root_lv(p, rl), R(rl, U), R(rl + 1, U));
      ++cl;
      for (int n = 0; n < ns; ++n) { rbnd(rl + 1); rsmooth(rl + 1, coffset); rbnd(rl + 1); rsmooth(rl + 1, 1 - coffset); }
    }
  }

  // MultigridDriver::FMGProlongate, multigrid_driver.cpp:570-602 with SetMGTaskListFMGProlongate
  void fmg_prolongate() {
    int flag = 0;
    if (cl == nrl - 1) { rbnd(nrl - 1); from_root(0); flag = 1; }
    if (cl >= nrl - 1) {
      const int bl = bl_of(cl);
      if (flag != 1) bex(bl);
      l_fmg_prolong(st, blk_lv(p, bl), B(bl, U), B(bl + 1, U));
    } else {
      rbnd(cl);
      l_fmg_prolong(st, root_lv(p, cl), R(cl, U), R(cl + 1, U));
    }
    ++cl;
  }

  // SolveCoarsestGrid, multigrid_driver.cpp:867-901
  void coarsest() {
    int mx = p->nrx1 > p->nrx2 ? p->nrx1 : p->nrx2;
    mx = mx > p->nrx3 ? mx : p->nrx3;
    const int ni = mx >> (nrl - 1);
    const Lv g = root_lv(p, 0);
    if (p->subtract_average && ni == 1) {
      rbnd(0);
      l_copy(st, L.rsz[0], R(0, UOLD), R(0, U));
      l_zero(st, L.rsz[0], R(0, U));
      return;
    }
    if (p->subtract_average) { sub_avg_root(SRC); sub_avg_root(U); }
    rbnd(0);
    l_copy(st, L.rsz[0], R(0, UOLD), R(0, U));
    l_fas(st, g, rdx(0), R(0, U), R(0, SRC));
    for (int i = 0; i < ni; ++i) { rsmooth(0, coffset); rbnd(0); rsmooth(0, 1 - coffset); rbnd(0); }
    if (p->subtract_average) sub_avg_root(U);
  }

  void vcycle() {
    const int start = cl;
    coffset ^= 1;
    while (cl > 0) to_coarser(p->npresmooth);
    coarsest();
    while (cl < start) to_finer(p->npostsmooth);
  }

  // CalculateDefectNorm(l2), multigrid.cpp:683-757 + multigrid_driver.cpp:908-937, into scalar(slot)
  void defect_norm(int slot) {
    const int bl = p->nmblevel - 1;
    const Lv g = blk_lv(p, bl);
    l_defect(st, g, bdx(bl), B(bl, U), B(bl, SRC), B(bl, DEF));
    l_reduce(st, g, 1, 0.0, p->vol, B(bl, DEF), scratch(), scalar(slot));
  }
  int read_norm(int slot, double *v) {
    if (hipMemcpyAsync(v, scalar(slot), sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      set_error("mg_solve: reading a defect norm back: %s", hipGetErrorString(hipGetLastError()));
      return AKMI_FAIL;
    }
    return AKMI_COMPLETE;
  }
};

}  // namespace
}  // namespace akmi

using namespace akmi;

extern "C" {

#define MG_LV(who)                                                                          \
  const Lv g{nmb, nz, ny, nx};                                                              \
  if (!lv_ok(g)) { set_error("%s: bad level %d x (%d, %d, %d)", who, nmb, nz, ny, nx); return AKMI_FAIL; } \
  hipStream_t st = (hipStream_t)stream

int akmi_mg_smooth(int nmb, int nz, int ny, int nx, double dx, double omega, int color, int coffset, double *u,
                   const double *src, void *stream) {
  MG_LV("mg_smooth");
  l_smooth(st, g, dx, omega, color, coffset, u, src);
  AKMI_CHECK_LAUNCH("mg_smooth");
  return AKMI_COMPLETE;
}

int akmi_mg_defect(int nmb, int nz, int ny, int nx, double dx, const double *u, const double *src, double *def,
                   void *stream) {
  MG_LV("mg_defect");
  l_defect(st, g, dx, u, const_cast<double *>(src), def);
  AKMI_CHECK_LAUNCH("mg_defect");
  return AKMI_COMPLETE;
}

int akmi_mg_fas_rhs(int nmb, int nz, int ny, int nx, double dx, const double *u, double *src, void *stream) {
  MG_LV("mg_fas_rhs");
  l_fas(st, g, dx, u, src);
  AKMI_CHECK_LAUNCH("mg_fas_rhs");
  return AKMI_COMPLETE;
}

int akmi_mg_restrict(int nmb, int nz, int ny, int nx, const double *fine, double *coarse, void *stream) {
  MG_LV("mg_restrict");
  l_restrict(st, g, fine, coarse);
  AKMI_CHECK_LAUNCH("mg_restrict");
  return AKMI_COMPLETE;
}

int akmi_mg_prolongate_correct(int nmb, int nz, int ny, int nx, const double *coarse, double *fine, void *stream) {
  MG_LV("mg_prolongate_correct");
  l_prolong(st, g, coarse, fine);
  AKMI_CHECK_LAUNCH("mg_prolongate_correct");
  return AKMI_COMPLETE;
}

int akmi_mg_fmg_prolongate(int nmb, int nz, int ny, int nx, const double *coarse, double *fine, void *stream) {
  MG_LV("mg_fmg_prolongate");
  l_fmg_prolong(st, g, coarse, fine);
  AKMI_CHECK_LAUNCH("mg_fmg_prolongate");
  return AKMI_COMPLETE;
}

int akmi_mg_store_old(long long n, double *uold, const double *u, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  l_copy(st, n, uold, u);
  AKMI_CHECK_LAUNCH("mg_store_old");
  return AKMI_COMPLETE;
}

int akmi_mg_correction(long long n, double *u, const double *uold, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  l_sub(st, n, u, uold);
  AKMI_CHECK_LAUNCH("mg_correction");
  return AKMI_COMPLETE;
}

int akmi_mg_zero_clear(long long n, double *u, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  l_zero(st, n, u);
  AKMI_CHECK_LAUNCH("mg_zero_clear");
  return AKMI_COMPLETE;
}

int akmi_mg_copy_source(long long n, double *u, const double *src, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  l_copy(st, n, u, src);
  AKMI_CHECK_LAUNCH("mg_copy_source");
  return AKMI_COMPLETE;
}

int akmi_mg_load_source(int nmb, int nz, int ny, int nx, int ng, int nvar, double fac, const double *u0, double *src,
                        void *stream) {
  MG_LV("mg_load_source");
  if (ng < 1 || nvar < 1) { set_error("mg_load_source: ng = %d, nvar = %d", ng, nvar); return AKMI_FAIL; }
  MG_LAUNCH(k_load<0>, cells_all(g), g, ng, nvar, fac, src, const_cast<double *>(u0));
  AKMI_CHECK_LAUNCH("mg_load_source");
  return AKMI_COMPLETE;
}

int akmi_mg_load_finest(int nmb, int nz, int ny, int nx, int ng, const double *phi, double *u, void *stream) {
  MG_LV("mg_load_finest");
  if (ng < 1) { set_error("mg_load_finest: ng = %d", ng); return AKMI_FAIL; }
  MG_LAUNCH(k_load<1>, cells_act(g), g, ng, 1, 1.0, u, const_cast<double *>(phi));
  AKMI_CHECK_LAUNCH("mg_load_finest");
  return AKMI_COMPLETE;
}

int akmi_mg_retrieve(int nmb, int nz, int ny, int nx, int ng, const double *u, double *phi, void *stream) {
  MG_LV("mg_retrieve");
  if (ng < 1) { set_error("mg_retrieve: ng = %d", ng); return AKMI_FAIL; }
  MG_LAUNCH(k_load<2>, cells_all(g), g, ng, 1, 1.0, const_cast<double *>(u), phi);
  AKMI_CHECK_LAUNCH("mg_retrieve");
  return AKMI_COMPLETE;
}

long long akmi_mg_reduce_scratch_doubles(int nmb, int nz, int ny, int nx) {
  return scratch_doubles(Lv{nmb, nz, ny, nx});
}

int akmi_mg_average(int nmb, int nz, int ny, int nx, double dx, double len, const double *a, double *scratch,
                    double *out, void *stream) {
  MG_LV("mg_average");
  l_average(st, g, dx, len, a, scratch, out);
  AKMI_CHECK_LAUNCH("mg_average");
  return AKMI_COMPLETE;
}

int akmi_mg_subtract_average(long long n, double *a, const double *ave, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  l_sub_scalar(st, n, a, ave);
  AKMI_CHECK_LAUNCH("mg_subtract_average");
  return AKMI_COMPLETE;
}

int akmi_mg_defect_norm(int nmb, int nz, int ny, int nx, double vol, const double *def, double *scratch, double *out,
                        void *stream) {
  MG_LV("mg_defect_norm");
  l_reduce(st, g, 1, 0.0, vol, def, scratch, out);
  AKMI_CHECK_LAUNCH("mg_defect_norm");
  return AKMI_COMPLETE;
}

int akmi_mg_exchange(int nmb, int nz, int ny, int nx, const int *nghbr, double *u, void *stream) {
  MG_LV("mg_exchange");
  l_exchange(st, g, nghbr, u);
  AKMI_CHECK_LAUNCH("mg_exchange");
  return AKMI_COMPLETE;
}

int akmi_mg_root_boundary(int nz, int ny, int nx, double *u, void *stream) {
  const int nmb = 1;
  MG_LV("mg_root_boundary");
  l_exchange(st, g, nullptr, u);
  AKMI_CHECK_LAUNCH("mg_root_boundary");
  return AKMI_COMPLETE;
}

int akmi_mg_exchange_bc(int nmb, int nz, int ny, int nx, const int *nghbr, int bc_type, int mporder, const double *mp,
                        const double *xlim, double *u, void *stream) {
  MG_LV("mg_exchange_bc");
  if (!nghbr || !u) { set_error("mg_exchange_bc: null argument"); return AKMI_FAIL; }
  if (!bc_ok(bc_type, mporder, (mp && xlim) ? xlim : nullptr, "mg_exchange_bc")) return AKMI_FAIL;
  Bc b{};
  b.type = bc_type; b.order = mporder; b.mp = mp; b.xlim = xlim;
  l_exchange_bc(st, g, nghbr, b, u);
  AKMI_CHECK_LAUNCH("mg_exchange_bc");
  return AKMI_COMPLETE;
}

int akmi_mg_root_boundary_bc(int nz, int ny, int nx, int bc_type, const int periodic[6], int mporder, const double *mp,
                             const double mesh_ext[6], double *u, void *stream) {
  const int nmb = 1;
  MG_LV("mg_root_boundary_bc");
  if (!periodic || !u) { set_error("mg_root_boundary_bc: null argument"); return AKMI_FAIL; }
  if (!bc_ok(bc_type, mporder, (mp && mesh_ext) ? mesh_ext : nullptr, "mg_root_boundary_bc")) return AKMI_FAIL;
  Bc b{};
  b.type = bc_type; b.order = mporder; b.mp = mp;
  for (int f = 0; f < 6; ++f) { b.periodic |= (periodic[f] ? 1 : 0) << f; b.ext[f] = mesh_ext ? mesh_ext[f] : 0.0; }
  l_exchange_bc(st, g, nullptr, b, u);
  AKMI_CHECK_LAUNCH("mg_root_boundary_bc");
  return AKMI_COMPLETE;
}

int akmi_mg_multipole_moments(int nmb, int nz, int ny, int nx, int mporder, int nodipole, int auto_origin,
                              const double *xlim, const double *src, double *scratch, double *mp, void *stream) {
  MG_LV("mg_multipole_moments");
  if (!src || !scratch || !mp) { set_error("mg_multipole_moments: null argument"); return AKMI_FAIL; }
  if (!bc_ok(AKMI_MGBC_MULTIPOLE, mporder, xlim, "mg_multipole_moments")) return AKMI_FAIL;
  if (auto_origin) l_mp_sums(st, g, 4, 0, xlim, src, scratch, mp);
  l_mp_sums(st, g, mporder == 4 ? 25 : 9, nodipole, xlim, src, scratch, mp);
  AKMI_CHECK_LAUNCH("mg_multipole_moments");
  return AKMI_COMPLETE;
}

int akmi_mg_mask(int nmb, int nz, int ny, int nx, const double *xlim, double mask_radius, double ox, double oy, double oz,
                 double *src, void *stream) {
  MG_LV("mg_mask");
  if (!xlim || !src) { set_error("mg_mask: null argument"); return AKMI_FAIL; }
  const double origin[3] = {ox, oy, oz};
  if (mask_radius > 0.0) l_mask(st, g, xlim, mask_radius, origin, src);
  AKMI_CHECK_LAUNCH("mg_mask");
  return AKMI_COMPLETE;
}

int akmi_mg_blocks_to_root(int nmb, int nz, int ny, int nx, const int *lloc, int initflag, const double *bsrc,
                           const double *bu, double *rsrc, double *ru, void *stream) {
  if (nmb < 1 || nz < 1 || ny < 1 || nx < 1) { set_error("mg_blocks_to_root: bad sizes"); return AKMI_FAIL; }
  hipStream_t st = (hipStream_t)stream;
  MG_LAUNCH(k_to_root, (long long)nmb, nmb, Lv{1, nz, ny, nx}, lloc, initflag, bsrc, bu, rsrc, ru);
  AKMI_CHECK_LAUNCH("mg_blocks_to_root");
  return AKMI_COMPLETE;
}

int akmi_mg_set_from_root(int nmb, int nz, int ny, int nx, const int *lloc, int folddata, const double *ru,
                          const double *ruold, double *bu, double *buold, void *stream) {
  if (nmb < 1 || nz < 1 || ny < 1 || nx < 1) { set_error("mg_set_from_root: bad sizes"); return AKMI_FAIL; }
  hipStream_t st = (hipStream_t)stream;
  MG_LAUNCH(k_from_root, (long long)nmb*27, nmb, Lv{1, nz, ny, nx}, lloc, folddata, ru, ruold, bu, buold);
  AKMI_CHECK_LAUNCH("mg_set_from_root");
  return AKMI_COMPLETE;
}

int akmi_mg_selfgravity(const akmi_pack *p, int face_shaped, double bdt, const double *w0, const double *phi,
                        const double *flx1, const double *flx2, const double *flx3, double *u0, void *stream) {
  if (!p || !w0 || !phi || !u0) { set_error("mg_selfgravity: null argument"); return AKMI_FAIL; }
  if (p->nvar < (p->is_ideal ? 5 : 4) || p->ng < 1) {
    set_error("mg_selfgravity: nvar = %d, ng = %d", p->nvar, p->ng);
    return AKMI_FAIL;
  }
  if (p->is_ideal && (!flx1 || (p->nx2 > 1 && !flx2) || (p->nx3 > 1 && !flx3))) {
    set_error("mg_selfgravity: the ideal-gas energy term needs the mass fluxes of the task-granular path");
    return AKMI_FAIL;
  }
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)p->nmb*p->nx1*p->nx2*p->nx3;
  MG_LAUNCH(k_selfgravity, n, p->nmb, p->nvar, p->nx1, p->nx2, p->nx3, p->ng, p->is_ideal, face_shaped ? 1 : 0, bdt,
            p->dx, w0, phi, flx1, flx2, flx3, u0);
  AKMI_CHECK_LAUNCH("mg_selfgravity");
  return AKMI_COMPLETE;
}

long long akmi_mg_workspace_doubles(const akmi_mg_plan *plan) {
  if (!plan_ok(plan, "mg_workspace_doubles")) return -1;
  return make_layout(plan).total;
}

long long akmi_mg_level_offset(const akmi_mg_plan *plan, int is_root, int level, int which) {
  if (!plan_ok(plan, "mg_level_offset")) return -1;
  const Layout L = make_layout(plan);
  if (which < 0 || which > 3 || level < 0 || level >= (is_root ? L.nrl : L.nmbl)) {
    set_error("mg_level_offset: level %d / array %d out of range", level, which);
    return -1;
  }
  return is_root ? L.roff[level] + which*L.rsz[level] : L.boff[level] + which*L.bsz[level];
}

long long akmi_mg_multipole_offset(const akmi_mg_plan *plan) {
  if (!plan_ok(plan, "mg_multipole_offset")) return -1;
  return make_layout(plan).scalars + 64;
}

long long akmi_mg_launch_count(int reset) {
  const long long n = g_launches;
  if (reset) g_launches = 0;
  return n;
}

int akmi_mg_solve(const akmi_mg_plan *plan, const double *u0, double *phi, int *coffset, double *norms, int *ncycles,
                  void *stream) {
  if (!plan_ok(plan, "mg_solve")) return AKMI_FAIL;
  if (!u0 || !phi || !coffset || !norms || !ncycles || !plan->ws || !plan->nghbr || !plan->lloc) {
    set_error("mg_solve: null argument");
    return AKMI_FAIL;
  }
  if (plan->eps < 0.0 && plan->niter < 0) {
    set_error("mg_solve: neither threshold nor niteration is set");
    return AKMI_FAIL;
  }
  if (!bc_ok(plan->mg_bc, plan->mporder, plan->xlim, "mg_solve")) return AKMI_FAIL;
  if (plan->mask_radius > 0.0 && !plan->xlim) { set_error("mg_solve: mask_radius > 0 needs xlim"); return AKMI_FAIL; }
  Solver s;
  s.p = plan;
  s.st = (hipStream_t)stream;
  s.L = make_layout(plan);
  s.ws = plan->ws;
  s.coffset = *coffset & 1;
  s.nrl = plan->nrootlevel;
  s.ntotal = plan->nrootlevel + plan->nmblevel - 1;
  hipStream_t st = s.st;
  for (int n = 0; n < AKMI_MG_NNORMS; ++n) norms[n] = -1.0;
  *ncycles = 0;
  const int fb = plan->nmblevel - 1;
  const Lv gf = blk_lv(plan, fb);

  // MGGravityDriver::Solve, mg_gravity.cpp:177-245
  MG_LAUNCH(k_load<0>, cells_all(gf), gf, plan->ng, plan->nvar, -plan->four_pi_G, s.B(fb, SRC),
            const_cast<double *>(u0));
  if (plan->mask_radius > 0.0) l_mask(st, gf, plan->xlim, plan->mask_radius, plan->mask_origin, s.B(fb, SRC));
  if (!plan->full_multigrid) MG_LAUNCH(k_load<1>, cells_act(gf), gf, plan->ng, 1, 1.0, s.B(fb, U), phi);
  if (plan->subtract_average) s.sub_avg_blocks(SRC);          // SetupMultigrid
  if (plan->mg_bc == AKMI_MGBC_MULTIPOLE)
    l_multipole(st, gf, plan->mporder, plan->nodipole, plan->auto_mporigin, plan->mporigin, plan->xlim, s.B(fb, SRC),
                s.scratch(), s.mp());
  s.cl = s.ntotal - 1;
  s.fmglevel = s.cl;

  if (plan->full_multigrid) {                                 // SolveFMG, multigrid_driver.cpp:742-783
    const int cycles = plan->fmg_ncycle > 1 ? plan->fmg_ncycle : 1;
    while (s.cl >= s.nrl) {
      const int bl = s.bl_of(s.cl);
      l_restrict(st, blk_lv(plan, bl - 1), s.B(bl, SRC), s.B(bl - 1, SRC));
      if (s.cl == s.nrl) s.to_root(1);
      --s.cl;
    }
    s.cl = s.nrl - 1;
    while (s.cl > 0) {
      l_restrict(st, root_lv(plan, s.cl - 1), s.R(s.cl, SRC), s.R(s.cl - 1, SRC));
      --s.cl;
    }
    while (s.cl < s.ntotal - 1) {
      s.fmglevel = s.cl + 1;
      s.fmg_prolongate();
      s.fmglevel = s.cl;
      for (int n = 0; n < cycles; ++n) s.vcycle();
    }
    s.fmglevel = s.ntotal - 1;
    if (plan->subtract_average) s.sub_avg_blocks(U);
  }

  int nnorm = 0;       // device slots 1.. hold the norms of a fixed-count run until the one read at the end
  if (plan->eps >= 0.0) {                                     // SolveIterative, multigrid_driver.cpp:790-829
    double def = 0.0;
    s.defect_norm(1);
    if (s.read_norm(1, &def) != AKMI_COMPLETE) return AKMI_FAIL;
    norms[0] = def;
    int n = 0;
    while (def > plan->eps) {
      s.vcycle();
      ++*ncycles;
      const double olddef = def;
      s.defect_norm(1);
      if (s.read_norm(1, &def) != AKMI_COMPLETE) return AKMI_FAIL;
      norms[1 + n] = def;
      if (def/olddef > 0.9 && plan->eps == 0.0) break;
      ++n;
      if (n >= 40) break;
    }
  } else {                                                    // SolveIterativeFixedTimes, :836-860
    if (plan->show_defect >= 2) s.defect_norm(1 + nnorm++);
    for (int n = 0; n < plan->niter; ++n) {
      s.vcycle();
      ++*ncycles;
      if (plan->show_defect >= 2 && nnorm < 41) s.defect_norm(1 + nnorm++);
    }
  }
  if (plan->show_defect >= 1) s.defect_norm(1 + 41);
  MG_LAUNCH(k_load<2>, cells_all(gf), gf, plan->ng, 1, 1.0, s.B(fb, U), phi);
  AKMI_CHECK_LAUNCH("mg_solve");
  if (nnorm > 0 || plan->show_defect >= 1) {
    double host[64];
    if (hipMemcpyAsync(host, s.scalar(0), sizeof(host), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      set_error("mg_solve: reading the defect norms back: %s", hipGetErrorString(hipGetLastError()));
      return AKMI_FAIL;
    }
    for (int n = 0; n < nnorm; ++n) norms[n] = host[1 + n];
    if (plan->show_defect >= 1) norms[41] = host[1 + 41];
  }
  *coffset = s.coffset;
  return AKMI_COMPLETE;
}

}  // extern "C"
