// akmi_derived.hpp -- the per-cell arithmetic of the derived output variables (BaseTypeOutput::ComputeDerivedVariable,
// src/outputs/derived_variables.cpp): pure functions of one cell, shared by the kernel of akmi_derived.hip and by the
// CPU build of tests/host_shim/derived_host.cpp.  Every expression keeps the reference's association (the library is
// built with -ffp-contract=off), so that the result is a function of the operands' bits alone: +, -, *, / and sqrt
// are correctly rounded in fp64 on the device and on the host.
//
// One deviation, in the two curvature variables on 1-D / 2-D meshes: the reference differences j+-1 and k+-1 whatever
// the dimension of the mesh, which reads outside an array of extent one.  Here the neighbour in a direction the mesh
// does not have is the cell itself, so that those differences are exactly +0.
#ifndef AKMI_DERIVED_HPP_
#define AKMI_DERIVED_HPP_
#include <cmath>
#include <cstddef>
#include <type_traits>

namespace akmi {

// what one launch reads: the pack's extents and the arrays of all its MeshBlocks
struct DvIn {
  int nvar, N1, N2, N3;
  int is, ie, js, je, ks, ke, ng;
  int multi_d, three_d;
  const double *dx;                       // [nmb][3]
  const double *w0, *bcc0, *b1, *b2, *b3; // (nmb,nvar,N3,N2,N1) (nmb,3,N3,N2,N1) and the three face arrays
};

// cell-centred array of block m: value of variable n at (k, j, i)
struct DvCC {
  const double *p; size_t cs; int N2, N1;
  __host__ __device__ __forceinline__ double operator()(int n, int k, int j, int i) const {
    return p[(size_t)n*cs + ((size_t)k*N2 + j)*N1 + i];
  }
};

__host__ __device__ __forceinline__ DvCC dv_cc(const DvIn &a, const double *base, int nv, int m) {
  const size_t cs = (size_t)a.N3*a.N2*a.N1;
  return DvCC{base + (size_t)m*nv*cs, cs, a.N2, a.N1};
}

// the index range the reference's loop covers: active cells, except for div B (derived_variables.cpp:1051-1061)
__host__ __device__ __forceinline__ bool dv_in_range(int which, const DvIn &a, int k, int j, int i) {
  if (which == 9 /* AKMI_DV_DIVB */) return true;      // every cell of the array: is-ng..ie+ng in each mesh direction
  return i >= a.is && i <= a.ie && j >= a.js && j <= a.je && k >= a.ks && k <= a.ke;
}

// curl of the vector field (c1, c2, c3) of `q` without the factor 1/2 of the centred difference
// (derived_variables.cpp:148-158, 192-202): the order of the += / -= is the reference's
struct Dv3 { double x, y, z; };
__host__ __device__ __forceinline__ Dv3 dv_curl2(const DvCC &q, int c1, int c2, int c3, const DvIn &a,
                                                 double dx1, double dx2, double dx3, int k, int j, int i) {
  double w1 = 0.0;
  double w2 = -(q(c3, k, j, i + 1) - q(c3, k, j, i - 1))/dx1;
  double w3 = (q(c2, k, j, i + 1) - q(c2, k, j, i - 1))/dx1;
  if (a.multi_d) {
    w1 += (q(c3, k, j + 1, i) - q(c3, k, j - 1, i))/dx2;
    w3 -= (q(c1, k, j + 1, i) - q(c1, k, j - 1, i))/dx2;
  }
  if (a.three_d) {
    w1 -= (q(c2, k + 1, j, i) - q(c2, k - 1, j, i))/dx3;
    w2 += (q(c1, k + 1, j, i) - q(c1, k - 1, j, i))/dx3;
  }
  return Dv3{w1, w2, w3};
}

// z component alone (derived_variables.cpp:128-132, 174-178)
__host__ __device__ __forceinline__ double dv_curlz(const DvCC &q, int c1, int c2, const DvIn &a, double dx1,
                                                    double dx2, int k, int j, int i) {
  double v = (q(c2, k, j, i + 1) - q(c2, k, j, i - 1))/dx1;
  if (a.multi_d) v -= (q(c1, k, j + 1, i) - q(c1, k, j - 1, i))/dx2;
  v *= 0.5;
  return v;
}

__host__ __device__ __forceinline__ double dv_bmag(const DvCC &b, int k, int j, int i) {
  return sqrt(b(0, k, j, i)*b(0, k, j, i) + b(1, k, j, i)*b(1, k, j, i) + b(2, k, j, i)*b(2, k, j, i));
}

template <int WHICH>
__host__ __device__ __forceinline__ double derived_cell(const DvIn &a, int m, int k, int j, int i) {
  const double dx1 = a.dx[3*m], dx2 = a.dx[3*m + 1], dx3 = a.dx[3*m + 2];
  // neighbours in a direction the mesh does not have: the cell itself (curvature variables only)
  const int jp = a.multi_d ? j + 1 : j, jm = a.multi_d ? j - 1 : j;
  const int kp = a.three_d ? k + 1 : k, km = a.three_d ? k - 1 : k;
  if (WHICH == 0) {                    // temperature: eint/dens (:112)
    const DvCC w = dv_cc(a, a.w0, a.nvar, m);
    return w(4, k, j, i)/w(0, k, j, i);
  } else if (WHICH == 1) {             // hydro_wz, mhd_wz
    return dv_curlz(dv_cc(a, a.w0, a.nvar, m), 1, 2, a, dx1, dx2, k, j, i);
  } else if (WHICH == 2) {             // hydro_w2, mhd_w2 (:159)
    const Dv3 w = dv_curl2(dv_cc(a, a.w0, a.nvar, m), 1, 2, 3, a, dx1, dx2, dx3, k, j, i);
    return 0.25*(w.x*w.x + w.y*w.y + w.z*w.z);
  } else if (WHICH == 3) {             // mhd_jz
    return dv_curlz(dv_cc(a, a.bcc0, 3, m), 0, 1, a, dx1, dx2, k, j, i);
  } else if (WHICH == 4) {             // mhd_j2 (:203)
    const Dv3 c = dv_curl2(dv_cc(a, a.bcc0, 3, m), 0, 1, 2, a, dx1, dx2, dx3, k, j, i);
    return 0.25*(c.x*c.x + c.y*c.y + c.z*c.z);
  } else if (WHICH == 5) {             // mhd_curv (:220-272)
    const DvCC b = dv_cc(a, a.bcc0, 3, m);
    const double Bx = b(0, k, j, i), By = b(1, k, j, i), Bz = b(2, k, j, i);
    const double B2 = (Bx*Bx + By*By + Bz*Bz);
    double d[3][3];                    // d[c][dir] = d B_c / d x_dir
    for (int c = 0; c < 3; ++c) {
      d[c][0] = (b(c, k, j, i + 1) - b(c, k, j, i - 1))/(2.0*dx1);
      d[c][1] = (b(c, k, jp, i) - b(c, k, jm, i))/(2.0*dx2);
      d[c][2] = (b(c, kp, j, i) - b(c, km, j, i))/(2.0*dx3);
    }
    const double gx = (Bx*d[0][0] + By*d[0][1] + Bz*d[0][2]);
    const double gy = (Bx*d[1][0] + By*d[1][1] + Bz*d[1][2]);
    const double gz = (Bx*d[2][0] + By*d[2][1] + Bz*d[2][2]);
    const double pxx = 1.0 - Bx*Bx/B2, pxy = 0.0 - Bx*By/B2, pxz = 0.0 - Bx*Bz/B2;
    const double pyx = 0.0 - By*Bx/B2, pyy = 1.0 - By*By/B2, pyz = 0.0 - By*Bz/B2;
    const double pzx = 0.0 - Bz*Bx/B2, pzy = 0.0 - Bz*By/B2, pzz = 1.0 - Bz*Bz/B2;
    const double c1 = (gx*pxx + gy*pyx + gz*pzx);
    const double c2 = (gx*pxy + gy*pyy + gz*pzy);
    const double c3 = (gx*pxz + gy*pyz + gz*pzz);
    return sqrt(c1*c1 + c2*c2 + c3*c3)/B2;
  } else if (WHICH == 6) {             // mhd_k_jxb (:789-811)
    const DvCC b = dv_cc(a, a.bcc0, 3, m);
    const Dv3 c = dv_curl2(b, 0, 1, 2, a, dx1, dx2, dx3, k, j, i);
    const double Bx = b(0, k, j, i), By = b(1, k, j, i), Bz = b(2, k, j, i);
    const double B2 = Bx*Bx + By*By + Bz*Bz;
    const double f1 = c.y*Bz - c.z*By;
    const double f2 = c.z*Bx - c.x*Bz;
    const double f3 = c.x*By - c.y*Bx;
    return sqrt(f1*f1 + f2*f2 + f3*f3)/B2;
  } else if (WHICH == 7) {             // mhd_curv_perp (:827-921)
    const DvCC b = dv_cc(a, a.bcc0, 3, m);
    const Dv3 c = dv_curl2(b, 0, 1, 2, a, dx1, dx2, dx3, k, j, i);
    const double Bx = b(0, k, j, i), By = b(1, k, j, i), Bz = b(2, k, j, i);
    const double B2 = Bx*Bx + By*By + Bz*Bz;
    const double f1 = (c.y*Bz - c.z*By)/(B2);
    const double f2 = (c.z*Bx - c.x*Bz)/(B2);
    const double f3 = (c.x*By - c.y*Bx)/(B2);
    const double h1 = Bx/sqrt(B2), h2 = By/sqrt(B2), h3 = Bz/sqrt(B2);
    // unit vectors of the six neighbours, d[c][dir] = d bhat_c / d x_dir
    const int kk[6] = {k, k, k, k, kp, km}, jj[6] = {j, j, jp, jm, j, j}, ii[6] = {i + 1, i - 1, i, i, i, i};
    double u[6][3];
    for (int q = 0; q < 6; ++q) {
      const double mag = dv_bmag(b, kk[q], jj[q], ii[q]);
      for (int n = 0; n < 3; ++n) u[q][n] = b(n, kk[q], jj[q], ii[q])/mag;
    }
    double d[3][3];
    for (int n = 0; n < 3; ++n) {
      d[n][0] = (u[0][n] - u[1][n])/(2.0*dx1);
      d[n][1] = (u[2][n] - u[3][n])/(2.0*dx2);
      d[n][2] = (u[4][n] - u[5][n])/(2.0*dx3);
    }
    const double c1 = h1*d[0][0] + h2*d[0][1] + h3*d[0][2];
    const double c2 = h1*d[1][0] + h2*d[1][1] + h3*d[1][2];
    const double c3 = h1*d[2][0] + h2*d[2][1] + h3*d[2][2];
    return sqrt((f1 - c1)*(f1 - c1) + (f2 - c2)*(f2 - c2) + (f3 - c3)*(f3 - c3));
  } else if (WHICH == 8) {             // mhd_bmag (:936-938)
    return dv_bmag(dv_cc(a, a.bcc0, 3, m), k, j, i);
  } else {                             // mhd_divb (:1063-1070), from the face fields
    const size_t f1 = (((size_t)m*a.N3 + k)*a.N2 + j)*(a.N1 + 1) + i;
    double divb = (a.b1[f1 + 1] - a.b1[f1])/dx1;
    if (a.multi_d) {
      const size_t f2 = (((size_t)m*a.N3 + k)*(a.N2 + 1) + j)*a.N1 + i;
      divb += (a.b2[f2 + a.N1] - a.b2[f2])/dx2;
    }
    if (a.three_d) {
      const size_t f3 = (((size_t)m*(a.N3 + 1) + k)*a.N2 + j)*a.N1 + i;
      divb += (a.b3[f3 + (size_t)a.N2*a.N1] - a.b3[f3])/dx3;
    }
    return divb;
  }
}

// f(integral constant) for the run-time variable: one switch for the kernel launch and for the host loop
template <class F>
inline bool dv_dispatch(int which, F &&f) {
  switch (which) {
    case 0: f(std::integral_constant<int, 0>{}); return true;
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 3: f(std::integral_constant<int, 3>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 5: f(std::integral_constant<int, 5>{}); return true;
    case 6: f(std::integral_constant<int, 6>{}); return true;
    case 7: f(std::integral_constant<int, 7>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
    case 9: f(std::integral_constant<int, 9>{}); return true;
  }
  return false;
}

}  // namespace akmi
#endif
