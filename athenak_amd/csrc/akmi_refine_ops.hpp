// akmi_refine_ops.hpp -- the per-cell restriction and prolongation operators, written once over accessors so
// that the boundary exchange of a refined mesh (akmi_refine.hip, akmi_smr.hip: a block and its own coarse buffer)
// and the regrid of an adaptive mesh (akmi_amr.hip: a new block and the old blocks it comes from) apply the same
// arithmetic in the same order.  An accessor is a callable (k, j, i) -> value (or, where written, a reference or an
// object assignable from a double that converts to one: akmi_smr.hip's owned faces).
#ifndef AKMI_REFINE_OPS_HPP_
#define AKMI_REFINE_OPS_HPP_
#include "akmi_common.hpp"

namespace akmi {

// the coarse index space of a MeshBlock and the thread mapping of every kernel over an index box
struct CGeo { int cN1, cN2, cN3, cis, cie, cjs, cje, cks, cke; };

inline CGeo make_cgeo(const Geo &g) {        // src/mesh/mesh.cpp:286-330
  CGeo c;
  const int cnx1 = g.nx1/2, cnx2 = g.multi_d ? g.nx2/2 : 1, cnx3 = g.three_d ? g.nx3/2 : 1;
  c.cN1 = cnx1 + 2*g.ng; c.cN2 = g.multi_d ? cnx2 + 2*g.ng : 1; c.cN3 = g.three_d ? cnx3 + 2*g.ng : 1;
  c.cis = g.ng; c.cie = c.cis + cnx1 - 1;
  c.cjs = g.multi_d ? g.ng : 0; c.cje = g.multi_d ? c.cjs + cnx2 - 1 : 0;
  c.cks = g.three_d ? g.ng : 0; c.cke = g.three_d ? c.cks + cnx3 - 1 : 0;
  return c;
}

struct Box { int il, iu, jl, ju, kl, ku; };

// thread -> (m, v, k, j, i) of a box; blockIdx.z = (m*nv + v)*nk + (k - kl)
__device__ __forceinline__ bool box_index(const Box &bx, int nv, int &m, int &v, int &k, int &j, int &i) {
  i = bx.il + blockIdx.x*64 + threadIdx.x;
  j = bx.jl + blockIdx.y*4 + threadIdx.y;
  const int nk = bx.ku - bx.kl + 1;
  int z = blockIdx.z;
  k = bx.kl + z%nk; z /= nk;
  v = z%nv; m = z/nv;
  return i <= bx.iu && j <= bx.ju;
}
inline dim3 box_grid(const Box &bx, int nv, int nmb) {
  return dim3(cdiv(bx.iu - bx.il + 1, 64), cdiv(bx.ju - bx.jl + 1, 4), (bx.ku - bx.kl + 1)*nv*nmb);
}

__device__ __forceinline__ double sgn1(double x) { return (x < 0.0) ? -1.0 : 1.0; }   // SIGN, athena.hpp:52
__device__ __forceinline__ double mm8(double dl, double dr) {
  return 0.125*(sgn1(dl) + sgn1(dr))*fmin(fabs(dl), fabs(dr));
}

// MeshRefinement::RestrictCC, src/mesh/mesh_refinement.cpp:1223-1277: the mean of the fine cells of one coarse
// cell, (fk, fj, fi) the lowest of them
template <class U>
__device__ __forceinline__ double restrict_cc_cell(int multi_d, int three_d, U &&u, int fk, int fj, int fi) {
  if (!multi_d) return 0.5*(u(fk, fj, fi) + u(fk, fj, fi + 1));
  if (!three_d) return 0.25*(u(fk, fj, fi) + u(fk, fj, fi + 1) + u(fk, fj + 1, fi) + u(fk, fj + 1, fi + 1));
  return 0.125*(u(fk, fj, fi) + u(fk, fj, fi + 1) + u(fk, fj + 1, fi) + u(fk, fj + 1, fi + 1)
              + u(fk + 1, fj, fi) + u(fk + 1, fj, fi + 1) + u(fk + 1, fj + 1, fi) + u(fk + 1, fj + 1, fi + 1));
}

// MeshRefinement::RestrictFC, src/mesh/mesh_refinement.cpp:1283-1382: the mean of the fine faces of one coarse
// face of component COMP, (fk, fj, fi) the lowest of them
template <int COMP, class B>
__device__ __forceinline__ double restrict_fc_face(int multi_d, int three_d, B &&b, int fk, int fj, int fi) {
  if constexpr (COMP == 0) {
    if (!multi_d) return b(fk, fj, fi);
    if (!three_d) return 0.5*(b(fk, fj, fi) + b(fk, fj + 1, fi));
    return 0.25*(b(fk, fj, fi) + b(fk, fj + 1, fi) + b(fk + 1, fj, fi) + b(fk + 1, fj + 1, fi));
  } else if constexpr (COMP == 1) {
    if (!three_d) return 0.5*(b(fk, fj, fi) + b(fk, fj, fi + 1));
    return 0.25*(b(fk, fj, fi) + b(fk, fj, fi + 1) + b(fk + 1, fj, fi) + b(fk + 1, fj, fi + 1));
  } else {
    if (!multi_d) return 0.5*(b(fk, fj, fi) + b(fk, fj, fi + 1));
    return 0.25*(b(fk, fj, fi) + b(fk, fj, fi + 1) + b(fk, fj + 1, fi) + b(fk, fj + 1, fi + 1));
  }
}

// A restricted face flux of direction DIR (PackAndSendFluxCC, src/bvals/flux_correct_cc.cpp:78-148) is
// restrict_fc_face<DIR> of the flux array.  The restricted edge EMF of component COMP (PackAndSendFluxFC,
// src/bvals/flux_correct_fc.cpp:84-360): the mean of the two fine edges along the edge's own direction, (fk, fj, fi)
// the lower of them; a single edge where that direction is collapsed
template <int COMP, class E>
__device__ __forceinline__ double restrict_edge(int multi_d, int three_d, E &&e, int fk, int fj, int fi) {
  if constexpr (COMP == 0) return multi_d ? 0.5*(e(fk, fj, fi) + e(fk, fj, fi + 1)) : e(fk, fj, fi);
  else if constexpr (COMP == 1) return multi_d ? 0.5*(e(fk, fj, fi) + e(fk, fj + 1, fi)) : e(fk, fj, fi);
  else return three_d ? 0.5*(e(fk, fj, fi) + e(fk + 1, fj, fi)) : e(fk, fj, fi);
}

// ProlongCC, src/mesh/prolongation.hpp:19-63: coarse cell (k, j, i) of ca into its fine cells of a
template <class CA, class A>
__device__ __forceinline__ void prolong_cc_cell(int multi_d, int three_d, CA &&ca, A &&a, int k, int j, int i,
                                                int fk, int fj, int fi) {
  const double q = ca(k, j, i);
  const double dvar1 = mm8(q - ca(k, j, i - 1), ca(k, j, i + 1) - q);
  double dvar2 = 0.0, dvar3 = 0.0;
  if (multi_d) dvar2 = mm8(q - ca(k, j - 1, i), ca(k, j + 1, i) - q);
  if (three_d) dvar3 = mm8(q - ca(k - 1, j, i), ca(k + 1, j, i) - q);
  a(fk, fj, fi) = q - dvar1 - dvar2 - dvar3;
  a(fk, fj, fi + 1) = q + dvar1 - dvar2 - dvar3;
  if (multi_d) {
    a(fk, fj + 1, fi) = q - dvar1 + dvar2 - dvar3;
    a(fk, fj + 1, fi + 1) = q + dvar1 + dvar2 - dvar3;
  }
  if (three_d) {
    a(fk + 1, fj, fi) = q - dvar1 - dvar2 + dvar3;
    a(fk + 1, fj, fi + 1) = q + dvar1 - dvar2 + dvar3;
    a(fk + 1, fj + 1, fi) = q - dvar1 + dvar2 + dvar3;
    a(fk + 1, fj + 1, fi + 1) = q + dvar1 + dvar2 + dvar3;
  }
}

// ProlongFCSharedX1Face / X2Face / X3Face, src/mesh/prolongation.hpp:69-160
template <int COMP, class CB, class B>
__device__ __forceinline__ void prolong_fc_shared_face(int multi_d, int three_d, CB &&cb, B &&b, int k, int j, int i,
                                                       int fk, int fj, int fi) {
  const double q = cb(k, j, i);
  if constexpr (COMP == 0) {
    double dvar2 = 0.0, dvar3 = 0.0;
    if (multi_d) dvar2 = mm8(q - cb(k, j - 1, i), cb(k, j + 1, i) - q);
    if (three_d) dvar3 = mm8(q - cb(k - 1, j, i), cb(k + 1, j, i) - q);
    b(fk, fj, fi) = q - dvar2 - dvar3;
    if (multi_d) b(fk, fj + 1, fi) = q + dvar2 - dvar3;
    if (three_d) {
      b(fk + 1, fj, fi) = q - dvar2 + dvar3;
      b(fk + 1, fj + 1, fi) = q + dvar2 + dvar3;
    }
  } else if constexpr (COMP == 1) {
    const double dvar1 = mm8(q - cb(k, j, i - 1), cb(k, j, i + 1) - q);
    double dvar3 = 0.0;
    if (three_d) dvar3 = mm8(q - cb(k - 1, j, i), cb(k + 1, j, i) - q);
    b(fk, fj, fi) = q - dvar1 - dvar3;
    b(fk, fj, fi + 1) = q + dvar1 - dvar3;
    if (three_d) {
      b(fk + 1, fj, fi) = q - dvar1 + dvar3;
      b(fk + 1, fj, fi + 1) = q + dvar1 + dvar3;
    }
  } else {
    const double dvar1 = mm8(q - cb(k, j, i - 1), cb(k, j, i + 1) - q);
    double dvar2 = 0.0;
    if (multi_d) dvar2 = mm8(q - cb(k, j - 1, i), cb(k, j + 1, i) - q);
    b(fk, fj, fi) = q - dvar1 - dvar2;
    b(fk, fj, fi + 1) = q + dvar1 - dvar2;
    if (multi_d) {
      b(fk, fj + 1, fi) = q - dvar1 + dvar2;
      b(fk, fj + 1, fi + 1) = q + dvar1 + dvar2;
    }
  }
}

// ProlongFCInternal, src/mesh/prolongation.hpp:166-230 (Toth & Roe 2002); 1-D: the mean of the two shared faces
// (src/bvals/prolongation.cpp:765-770, src/mesh/mesh_refinement.cpp:1171-1174).  B1/B2/B3 return what can be
// read and assigned.  Every inner face is assigned from shared faces only, none from another inner face.
template <class F1, class F2, class F3>
__device__ __forceinline__ void prolong_fc_internal_cell(int multi_d, int three_d, F1 &&B1, F2 &&B2, F3 &&B3,
                                                         int fk, int fj, int fi) {
  if (!multi_d) {
    B1(fk, fj, fi + 1) = 0.5*(B1(fk, fj, fi) + B1(fk, fj, fi + 2));
  } else if (three_d) {
    double Uxx = 0.0, Vyy = 0.0, Wzz = 0.0, Uxyz = 0.0, Vxyz = 0.0, Wxyz = 0.0;
#pragma unroll
    for (int jj = 0; jj < 2; jj++) {
      const int jsgn = 2*jj - 1;
      const int fjj = fj + jj, fjp = fj + 2*jj;
#pragma unroll
      for (int ii = 0; ii < 2; ii++) {
        const int isgn = 2*ii - 1;
        const int fii = fi + ii, fip = fi + 2*ii;
        Uxx += isgn*(jsgn*(B2(fk, fjp, fii) + B2(fk + 1, fjp, fii)) + (B3(fk + 2, fjj, fii) - B3(fk, fjj, fii)));
        Vyy += jsgn*((B3(fk + 2, fjj, fii) - B3(fk, fjj, fii)) + isgn*(B1(fk, fjj, fip) + B1(fk + 1, fjj, fip)));
        Wzz += isgn*(B1(fk + 1, fjj, fip) - B1(fk, fjj, fip)) + jsgn*(B2(fk + 1, fjp, fii) - B2(fk, fjp, fii));
        Uxyz += isgn*jsgn*(B1(fk + 1, fjj, fip) - B1(fk, fjj, fip));
        Vxyz += isgn*jsgn*(B2(fk + 1, fjp, fii) - B2(fk, fjp, fii));
        Wxyz += isgn*jsgn*(B3(fk + 2, fjj, fii) - B3(fk, fjj, fii));
      }
    }
    Uxx *= 0.125; Vyy *= 0.125; Wzz *= 0.125;
    Uxyz *= 0.0625; Vxyz *= 0.0625; Wxyz *= 0.0625;
    B1(fk, fj, fi + 1) = 0.5*(B1(fk, fj, fi) + B1(fk, fj, fi + 2)) + Uxx - Vxyz - Wxyz;
    B1(fk, fj + 1, fi + 1) = 0.5*(B1(fk, fj + 1, fi) + B1(fk, fj + 1, fi + 2)) + Uxx - Vxyz + Wxyz;
    B1(fk + 1, fj, fi + 1) = 0.5*(B1(fk + 1, fj, fi) + B1(fk + 1, fj, fi + 2)) + Uxx + Vxyz - Wxyz;
    B1(fk + 1, fj + 1, fi + 1) = 0.5*(B1(fk + 1, fj + 1, fi) + B1(fk + 1, fj + 1, fi + 2)) + Uxx + Vxyz + Wxyz;
    B2(fk, fj + 1, fi) = 0.5*(B2(fk, fj, fi) + B2(fk, fj + 2, fi)) + Vyy - Uxyz - Wxyz;
    B2(fk, fj + 1, fi + 1) = 0.5*(B2(fk, fj, fi + 1) + B2(fk, fj + 2, fi + 1)) + Vyy - Uxyz + Wxyz;
    B2(fk + 1, fj + 1, fi) = 0.5*(B2(fk + 1, fj, fi) + B2(fk + 1, fj + 2, fi)) + Vyy + Uxyz - Wxyz;
    B2(fk + 1, fj + 1, fi + 1) = 0.5*(B2(fk + 1, fj, fi + 1) + B2(fk + 1, fj + 2, fi + 1)) + Vyy + Uxyz + Wxyz;
    B3(fk + 1, fj, fi) = 0.5*(B3(fk + 2, fj, fi) + B3(fk, fj, fi)) + Wzz - Uxyz - Vxyz;
    B3(fk + 1, fj, fi + 1) = 0.5*(B3(fk + 2, fj, fi + 1) + B3(fk, fj, fi + 1)) + Wzz - Uxyz + Vxyz;
    B3(fk + 1, fj + 1, fi) = 0.5*(B3(fk + 2, fj + 1, fi) + B3(fk, fj + 1, fi)) + Wzz + Uxyz - Vxyz;
    B3(fk + 1, fj + 1, fi + 1) = 0.5*(B3(fk + 2, fj + 1, fi + 1) + B3(fk, fj + 1, fi + 1)) + Wzz + Uxyz + Vxyz;
  } else {
    const double tmp1 = 0.25*(B2(fk, fj + 2, fi + 1) - B2(fk, fj, fi + 1) - B2(fk, fj + 2, fi) + B2(fk, fj, fi));
    const double tmp2 = 0.25*(B1(fk, fj, fi) - B1(fk, fj, fi + 2) - B1(fk, fj + 1, fi) + B1(fk, fj + 1, fi + 2));
    B1(fk, fj, fi + 1) = 0.5*(B1(fk, fj, fi) + B1(fk, fj, fi + 2)) + tmp1;
    B1(fk, fj + 1, fi + 1) = 0.5*(B1(fk, fj + 1, fi) + B1(fk, fj + 1, fi + 2)) + tmp1;
    B2(fk, fj + 1, fi) = 0.5*(B2(fk, fj, fi) + B2(fk, fj + 2, fi)) + tmp2;
    B2(fk, fj + 1, fi + 1) = 0.5*(B2(fk, fj, fi + 1) + B2(fk, fj + 2, fi + 1)) + tmp2;
  }
}

}  // namespace akmi
#endif  // AKMI_REFINE_OPS_HPP_
