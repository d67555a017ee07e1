// akmi_refine.hip -- the operators between a MeshBlock and its coarse buffer that SMR/AMR boundary
// exchange is made of: restriction of cell- and face-centred data, slope-limited
// prolongation of cell-centred data, and the divergence-preserving prolongation of the face field
// (shared faces first, then the Toth & Roe interior).  The level-aware boundary exchange and the flux/EMF
// correction of a refined mesh are akmi_smr.hip, the regrid of an adaptive one akmi_amr.hip; here the
// operators are exposed through the C ABI over caller-given index boxes, which is how
// src/bvals/prolongation.cpp drives them (iprol boxes of the receive buffers).
#include "akmi_common.hpp"
#include "akmi_c2p.hpp"
#include "akmi_refine_ops.hpp"

namespace akmi {

// the per-cell operators: akmi_refine_ops.hpp (shared with the regrid kernels of akmi_amr.hip)

// MeshRefinement::RestrictCC, src/mesh/mesh_refinement.cpp:1223-1277
__global__ void __launch_bounds__(256)
k_restrict_cc(Geo g, CGeo c, int nvar, const unsigned char *__restrict__ mask, const double *__restrict__ u,
              double *__restrict__ cu) {
  const Box bx{c.cis, c.cie, c.cjs, c.cje, c.cks, c.cke};
  int m, n, k, j, i;
  if (!box_index(bx, nvar, m, n, k, j, i)) return;
  if (mask && !mask[m]) return;
  const int fi = 2*i - c.cis, fj = 2*j - c.cjs, fk = 2*k - c.cks;
  auto U = [&](int kk, int jj, int ii) { return u[ix5(nvar, g.N3, g.N2, g.N1, m, n, kk, jj, ii)]; };
  cu[ix5(nvar, c.cN3, c.cN2, c.cN1, m, n, k, j, i)] = restrict_cc_cell(g.multi_d, g.three_d, U, fk, fj, fi);
}

struct Faces { double *b1, *b2, *b3; };
struct CFaces { const double *b1, *b2, *b3; };

// MeshRefinement::RestrictFC, src/mesh/mesh_refinement.cpp:1283-1382: a face along a collapsed direction is
// written on both of its planes, the upper face of the last cell of an active direction from the fine faces there
__global__ void __launch_bounds__(256)
k_restrict_fc(Geo g, CGeo c, const unsigned char *__restrict__ mask, CFaces f, Faces cf) {
  const Box bx{c.cis, c.cie, c.cjs, c.cje, c.cks, c.cke};
  int m, v, k, j, i;
  if (!box_index(bx, 1, m, v, k, j, i)) return;
  if (mask && !mask[m]) return;
  const int N1 = g.N1, N2 = g.N2, N3 = g.N3;
  const int fi = 2*i - c.cis, fj = 2*j - c.cjs, fk = 2*k - c.cks;
  const int md = g.multi_d, td = g.three_d;
  auto B1 = [&](int kk, int jj, int ii) { return f.b1[ix4(N3, N2, N1 + 1, m, kk, jj, ii)]; };
  auto B2 = [&](int kk, int jj, int ii) { return f.b2[ix4(N3, N2 + 1, N1, m, kk, jj, ii)]; };
  auto B3 = [&](int kk, int jj, int ii) { return f.b3[ix4(N3 + 1, N2, N1, m, kk, jj, ii)]; };
  auto C1 = [&](int kk, int jj, int ii) -> double & { return cf.b1[ix4(c.cN3, c.cN2, c.cN1 + 1, m, kk, jj, ii)]; };
  auto C2 = [&](int kk, int jj, int ii) -> double & { return cf.b2[ix4(c.cN3, c.cN2 + 1, c.cN1, m, kk, jj, ii)]; };
  auto C3 = [&](int kk, int jj, int ii) -> double & { return cf.b3[ix4(c.cN3 + 1, c.cN2, c.cN1, m, kk, jj, ii)]; };
  C1(k, j, i) = restrict_fc_face<0>(md, td, B1, fk, fj, fi);
  if (i == c.cie) C1(k, j, i + 1) = restrict_fc_face<0>(md, td, B1, fk, fj, fi + 2);
  const double b2c = restrict_fc_face<1>(md, td, B2, fk, fj, fi);
  C2(k, j, i) = b2c;
  if (!md) C2(k, j + 1, i) = b2c;
  else if (j == c.cje) C2(k, j + 1, i) = restrict_fc_face<1>(md, td, B2, fk, fj + 2, fi);
  const double b3c = restrict_fc_face<2>(md, td, B3, fk, fj, fi);
  C3(k, j, i) = b3c;
  if (!td) C3(k + 1, j, i) = b3c;
  else if (k == c.cke) C3(k + 1, j, i) = restrict_fc_face<2>(md, td, B3, fk + 2, fj, fi);
}

// ProlongCC, src/mesh/prolongation.hpp:19-63
__global__ void __launch_bounds__(256)
k_prolong_cc(Geo g, CGeo c, Box bx, int nvar, const double *__restrict__ cu, double *__restrict__ u) {
  int m, v, k, j, i;
  if (!box_index(bx, nvar, m, v, k, j, i)) return;
  const int fi = (i - c.cis)*2 + g.is, fj = (j - c.cjs)*2 + g.js, fk = (k - c.cks)*2 + g.ks;
  auto CA = [&](int kk, int jj, int ii) { return cu[ix5(nvar, c.cN3, c.cN2, c.cN1, m, v, kk, jj, ii)]; };
  auto A = [&](int kk, int jj, int ii) -> double & { return u[ix5(nvar, g.N3, g.N2, g.N1, m, v, kk, jj, ii)]; };
  prolong_cc_cell(g.multi_d, g.three_d, CA, A, k, j, i, fk, fj, fi);
}

// ProlongFCSharedX1Face / X2Face / X3Face, src/mesh/prolongation.hpp:69-160
template <int COMP>
__global__ void __launch_bounds__(256)
k_prolong_fc_shared(Geo g, CGeo c, Box bx, const double *__restrict__ cb, double *__restrict__ b) {
  int m, v, k, j, i;
  if (!box_index(bx, 1, m, v, k, j, i)) return;
  const int fi = (i - c.cis)*2 + g.is;
  const int fj = g.multi_d ? (j - c.cjs)*2 + g.js : j;
  const int fk = g.three_d ? (k - c.cks)*2 + g.ks : k;
  constexpr int d1 = COMP == 0, d2 = COMP == 1, d3 = COMP == 2;
  auto CB = [&](int kk, int jj, int ii) { return cb[ix4(c.cN3 + d3, c.cN2 + d2, c.cN1 + d1, m, kk, jj, ii)]; };
  auto B = [&](int kk, int jj, int ii) -> double & { return b[ix4(g.N3 + d3, g.N2 + d2, g.N1 + d1, m, kk, jj, ii)]; };
  prolong_fc_shared_face<COMP>(g.multi_d, g.three_d, CB, B, k, j, i, fk, fj, fi);
}

// ProlongFCInternal, src/mesh/prolongation.hpp:166-230; 1-D: src/bvals/prolongation.cpp:765-770
__global__ void __launch_bounds__(256)
k_prolong_fc_internal(Geo g, CGeo c, Box bx, Faces f) {
  int m, v, k, j, i;
  if (!box_index(bx, 1, m, v, k, j, i)) return;
  const int N1 = g.N1, N2 = g.N2, N3 = g.N3;
  const int fi = (i - c.cis)*2 + g.is, fj = (j - c.cjs)*2 + g.js, fk = (k - c.cks)*2 + g.ks;
  auto B1 = [&](int kk, int jj, int ii) -> double & { return f.b1[ix4(N3, N2, N1 + 1, m, kk, jj, ii)]; };
  auto B2 = [&](int kk, int jj, int ii) -> double & { return f.b2[ix4(N3, N2 + 1, N1, m, kk, jj, ii)]; };
  auto B3 = [&](int kk, int jj, int ii) -> double & { return f.b3[ix4(N3 + 1, N2, N1, m, kk, jj, ii)]; };
  prolong_fc_internal_cell(g.multi_d, g.three_d, B1, B2, B3, fk, fj, fi);
}

// box of coarse indices: the two fine cells (faces) of every coarse index must lie inside the fine
// array, and the slope stencil (one coarse cell/face each side, `halo`) inside the coarse array
static int check_box(const Geo &g, const CGeo &c, const int *box, int halo, int d1, int d2, int d3,
                     const char *who) {
  if (g.nx1 % 2 || (g.multi_d && g.nx2 % 2) || (g.three_d && g.nx3 % 2)) {
    set_error("%s: MeshBlock sizes must be even for refinement", who); return AKMI_FAIL;
  }
  const int lo[3] = {box[0], box[2], box[4]}, hi[3] = {box[1], box[3], box[5]};
  const int cs[3] = {c.cis, c.cjs, c.cks}, fs[3] = {g.is, g.js, g.ks};
  const int cN[3] = {c.cN1 + d1, c.cN2 + d2, c.cN3 + d3}, fN[3] = {g.N1 + d1, g.N2 + d2, g.N3 + d3};
  const bool on[3] = {true, (bool)g.multi_d, (bool)g.three_d};
  const int own[3] = {d1, d2, d3};
  for (int q = 0; q < 3; ++q) {
    if (lo[q] > hi[q]) { set_error("%s: empty index box", who); return AKMI_FAIL; }
    if (!on[q]) {
      if (lo[q] != 0 || hi[q] != 0) { set_error("%s: index box in a collapsed direction", who); return AKMI_FAIL; }
      continue;
    }
    const int flo = (lo[q] - cs[q])*2 + fs[q];
    const int fhi = (hi[q] - cs[q])*2 + fs[q] + (own[q] ? 0 : 1);     // a face maps to ONE fine face
    const int h = own[q] ? 0 : halo;                                  // no slope along a face's own axis
    if (flo < 0 || fhi > fN[q] - 1 || lo[q] - h < 0 || hi[q] + h > cN[q] - 1) {
      set_error("%s: index box [%d,%d] of direction %d reaches outside the arrays", who, lo[q], hi[q], q + 1);
      return AKMI_FAIL;
    }
  }
  return AKMI_COMPLETE;
}

}  // namespace akmi

using namespace akmi;

// Restricted face fluxes for a coarser neighbour, buffer order of PackAndSendFluxCC
// (src/bvals/flux_correct_cc.cpp:78-148); box = coarse index box, one face thick along DIR
template <int DIR>
__global__ void k_restrict_flux_cc(Geo g, CGeo c, Box bx, int nvar, const double *__restrict__ flx,
                                   double *__restrict__ out) {
  int m, v, k, j, i;
  if (!box_index(bx, nvar, m, v, k, j, i)) return;
  const int ni = bx.iu - bx.il + 1, nj = bx.ju - bx.jl + 1, nk = bx.ku - bx.kl + 1;
  const int f3 = g.N3 + (DIR == 2), f2 = g.N2 + (DIR == 1), f1 = g.N1 + (DIR == 0);
  const int fi = 2*i - c.cis, fj = g.multi_d ? 2*j - c.cjs : 0, fk = g.three_d ? 2*k - c.cks : 0;
  auto FX = [&](int kk, int jj, int ii) { return flx[ix5(nvar, f3, f2, f1, m, v, kk, jj, ii)]; };
  const double r = restrict_fc_face<DIR>(g.multi_d, g.three_d, FX, fk, fj, fi);
  size_t o;
  if constexpr (DIR == 0) o = (size_t)(j - bx.jl) + (size_t)nj*((k - bx.kl) + (size_t)nk*v);
  else if constexpr (DIR == 1) o = (size_t)(i - bx.il) + (size_t)ni*((k - bx.kl) + (size_t)nk*v);
  else o = (size_t)(i - bx.il) + (size_t)ni*((j - bx.jl) + (size_t)nj*v);
  out[(size_t)m*nvar*ni*nj*nk + o] = r;
}

// Restricted edge EMFs for a coarser neighbour (PackAndSendFluxFC, src/bvals/flux_correct_fc.cpp:84-360):
// the two fine edges of a coarse edge averaged along the edge's own direction
template <int COMP>
__global__ void k_restrict_emf(Geo g, CGeo c, Box bx, const double *__restrict__ e,
                               double *__restrict__ out) {
  int m, v, k, j, i;
  if (!box_index(bx, 1, m, v, k, j, i)) return;
  const int ni = bx.iu - bx.il + 1, nj = bx.ju - bx.jl + 1, nk = bx.ku - bx.kl + 1;
  const int e3 = g.N3 + (COMP != 2), e2 = g.N2 + (COMP != 1), e1 = g.N1 + (COMP != 0);
  const int fi = 2*i - c.cis, fj = g.multi_d ? 2*j - c.cjs : 0, fk = g.three_d ? 2*k - c.cks : 0;
  auto EE = [&](int kk, int jj, int ii) { return e[ix4(e3, e2, e1, m, kk, jj, ii)]; };
  const double r = restrict_edge<COMP>(g.multi_d, g.three_d, EE, fk, fj, fi);
  out[(size_t)m*ni*nj*nk + (size_t)(i - bx.il) + (size_t)ni*((j - bx.jl) + (size_t)nj*(k - bx.kl))] = r;
}

// coarse box of a flux operator: inside the coarse index space incl. its upper faces/edges
static int check_flux_box(const CGeo &c, const int *box, const char *who) {
  if (box[0] > box[1] || box[2] > box[3] || box[4] > box[5] || box[0] < c.cis || box[1] > c.cie + 1 ||
      box[2] < c.cjs || box[3] > c.cje + 1 || box[4] < c.cks || box[5] > c.cke + 1) {
    set_error("%s: box [%d,%d]x[%d,%d]x[%d,%d] outside the coarse faces [%d,%d]x[%d,%d]x[%d,%d]", who, box[0],
              box[1], box[2], box[3], box[4], box[5], c.cis, c.cie + 1, c.cjs, c.cje + 1, c.cks, c.cke + 1);
    return AKMI_FAIL;
  }
  return AKMI_COMPLETE;
}

// Primitive -> conserved over a box of fine cells: SingleP2C_* (src/eos/ideal_c2p_hyd.hpp:76-83,
// ideal_c2p_mhd.hpp:75-84) as PrimToConsFineBndry applies them (src/bvals/prolong_prims.cpp:190-300)
__global__ void k_prim2cons(Geo g, Box bx, int is_ideal, const double *__restrict__ w,
                            const double *__restrict__ bcc, double *__restrict__ u) {
  int m, v, k, j, i;
  if (!box_index(bx, 1, m, v, k, j, i)) return;
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const size_t c = ix5(g.nvar, g.N3, g.N2, g.N1, m, 0, k, j, i);
  double bx_ = 0.0, by = 0.0, bz = 0.0;
  if (is_ideal && bcc) {
    const size_t b = ix5(3, g.N3, g.N2, g.N1, m, 0, k, j, i);
    bx_ = bcc[b]; by = bcc[b + cs]; bz = bcc[b + 2*cs];
  }
  p2c_at(g.nvar, is_ideal, bcc != nullptr, w, u, c, cs, bx_, by, bz);
}

extern "C" {

int akmi_restrict_cc_masked(const akmi_pack *p, int nvar, const unsigned char *mask, const double *u, double *cu,
                            void *stream) {
  Geo g = make_geo(p); CGeo c = make_cgeo(g);
  const Box bx{c.cis, c.cie, c.cjs, c.cje, c.cks, c.cke};
  k_restrict_cc<<<box_grid(bx, nvar, g.nmb), dim3(64, 4), 0, (hipStream_t)stream>>>(g, c, nvar, mask, u, cu);
  AKMI_CHECK_LAUNCH("restrict_cc");
  return AKMI_COMPLETE;
}
int akmi_restrict_cc(const akmi_pack *p, int nvar, const double *u, double *cu, void *stream) {
  return akmi_restrict_cc_masked(p, nvar, nullptr, u, cu, stream);
}

int akmi_restrict_fc_masked(const akmi_pack *p, const unsigned char *mask, const double *bx1f, const double *bx2f,
                            const double *bx3f, double *cbx1f, double *cbx2f, double *cbx3f, void *stream) {
  Geo g = make_geo(p); CGeo c = make_cgeo(g);
  const Box bx{c.cis, c.cie, c.cjs, c.cje, c.cks, c.cke};
  k_restrict_fc<<<box_grid(bx, 1, g.nmb), dim3(64, 4), 0, (hipStream_t)stream>>>(
      g, c, mask, CFaces{bx1f, bx2f, bx3f}, Faces{cbx1f, cbx2f, cbx3f});
  AKMI_CHECK_LAUNCH("restrict_fc");
  return AKMI_COMPLETE;
}
int akmi_restrict_fc(const akmi_pack *p, const double *bx1f, const double *bx2f, const double *bx3f,
                     double *cbx1f, double *cbx2f, double *cbx3f, void *stream) {
  return akmi_restrict_fc_masked(p, nullptr, bx1f, bx2f, bx3f, cbx1f, cbx2f, cbx3f, stream);
}

int akmi_restrict_flux_cc(const akmi_pack *p, int nvar, int dir, const int *box, const double *flx,
                          double *out, void *stream) {
  Geo g = make_geo(p); CGeo c = make_cgeo(g);
  if (dir < 0 || dir > 2 || (dir == 1 && !g.multi_d) || (dir == 2 && !g.three_d)) {
    set_error("restrict_flux_cc: dir = %d", dir); return AKMI_FAIL;
  }
  if (check_flux_box(c, box, "restrict_flux_cc") != AKMI_COMPLETE) return AKMI_FAIL;
  if (box[2*dir] != box[2*dir + 1]) { set_error("restrict_flux_cc: the box must be one face thick along dir"); return AKMI_FAIL; }
  // transverse extents are cells, not faces
  const int hi[3] = {c.cie, c.cje, c.cke};
  for (int d = 0; d < 3; ++d)
    if (d != dir && box[2*d + 1] > hi[d]) { set_error("restrict_flux_cc: transverse range beyond the coarse cells"); return AKMI_FAIL; }
  const Box bx{box[0], box[1], box[2], box[3], box[4], box[5]};
  const dim3 grid = box_grid(bx, nvar, g.nmb), block(64, 4);
  hipStream_t st = (hipStream_t)stream;
  if (dir == 0) k_restrict_flux_cc<0><<<grid, block, 0, st>>>(g, c, bx, nvar, flx, out);
  else if (dir == 1) k_restrict_flux_cc<1><<<grid, block, 0, st>>>(g, c, bx, nvar, flx, out);
  else k_restrict_flux_cc<2><<<grid, block, 0, st>>>(g, c, bx, nvar, flx, out);
  AKMI_CHECK_LAUNCH("restrict_flux_cc");
  return AKMI_COMPLETE;
}

int akmi_restrict_emf(const akmi_pack *p, int comp, const int *box, const double *e, double *out,
                      void *stream) {
  Geo g = make_geo(p); CGeo c = make_cgeo(g);
  if (comp < 0 || comp > 2) { set_error("restrict_emf: comp = %d", comp); return AKMI_FAIL; }
  if (check_flux_box(c, box, "restrict_emf") != AKMI_COMPLETE) return AKMI_FAIL;
  const int hi[3] = {c.cie, c.cje, c.cke};
  if (box[2*comp + 1] > hi[comp]) { set_error("restrict_emf: range along the edge beyond the coarse cells"); return AKMI_FAIL; }
  const Box bx{box[0], box[1], box[2], box[3], box[4], box[5]};
  const dim3 grid = box_grid(bx, 1, g.nmb), block(64, 4);
  hipStream_t st = (hipStream_t)stream;
  if (comp == 0) k_restrict_emf<0><<<grid, block, 0, st>>>(g, c, bx, e, out);
  else if (comp == 1) k_restrict_emf<1><<<grid, block, 0, st>>>(g, c, bx, e, out);
  else k_restrict_emf<2><<<grid, block, 0, st>>>(g, c, bx, e, out);
  AKMI_CHECK_LAUNCH("restrict_emf");
  return AKMI_COMPLETE;
}

int akmi_prim2cons(const akmi_pack *p, const int *box, const double *w, const double *bcc, double *u,
                   void *stream) {
  Geo g = make_geo(p);
  if (box[0] > box[1] || box[2] > box[3] || box[4] > box[5] || box[0] < 0 || box[1] >= g.N1 ||
      box[2] < 0 || box[3] >= g.N2 || box[4] < 0 || box[5] >= g.N3) {
    set_error("prim2cons: box [%d,%d]x[%d,%d]x[%d,%d] outside the block's cells", box[0], box[1], box[2],
              box[3], box[4], box[5]);
    return AKMI_FAIL;
  }
  const Box bx{box[0], box[1], box[2], box[3], box[4], box[5]};
  k_prim2cons<<<box_grid(bx, 1, g.nmb), dim3(64, 4), 0, (hipStream_t)stream>>>(g, bx, p->is_ideal, w, bcc, u);
  AKMI_CHECK_LAUNCH("prim2cons");
  return AKMI_COMPLETE;
}

int akmi_prolong_cc(const akmi_pack *p, int nvar, const int *box, const double *cu, double *u,
                    void *stream) {
  Geo g = make_geo(p); CGeo c = make_cgeo(g);
  if (check_box(g, c, box, 1, 0, 0, 0, "prolong_cc") != AKMI_COMPLETE) return AKMI_FAIL;
  const Box bx{box[0], box[1], box[2], box[3], box[4], box[5]};
  k_prolong_cc<<<box_grid(bx, nvar, g.nmb), dim3(64, 4), 0, (hipStream_t)stream>>>(g, c, bx, nvar, cu, u);
  AKMI_CHECK_LAUNCH("prolong_cc");
  return AKMI_COMPLETE;
}

int akmi_prolong_fc_shared(const akmi_pack *p, int comp, const int *box, const double *cb, double *b,
                           void *stream) {
  Geo g = make_geo(p); CGeo c = make_cgeo(g);
  if (comp < 0 || comp > 2) { set_error("prolong_fc_shared: comp = %d", comp); return AKMI_FAIL; }
  if (check_box(g, c, box, 1, comp == 0, comp == 1, comp == 2, "prolong_fc_shared") != AKMI_COMPLETE)
    return AKMI_FAIL;
  const Box bx{box[0], box[1], box[2], box[3], box[4], box[5]};
  const dim3 grid = box_grid(bx, 1, g.nmb), block(64, 4);
  hipStream_t st = (hipStream_t)stream;
  if (comp == 0) k_prolong_fc_shared<0><<<grid, block, 0, st>>>(g, c, bx, cb, b);
  else if (comp == 1) k_prolong_fc_shared<1><<<grid, block, 0, st>>>(g, c, bx, cb, b);
  else k_prolong_fc_shared<2><<<grid, block, 0, st>>>(g, c, bx, cb, b);
  AKMI_CHECK_LAUNCH("prolong_fc_shared");
  return AKMI_COMPLETE;
}

int akmi_prolong_fc_internal(const akmi_pack *p, const int *box, double *bx1f, double *bx2f,
                             double *bx3f, void *stream) {
  Geo g = make_geo(p); CGeo c = make_cgeo(g);
  if (check_box(g, c, box, 0, 0, 0, 0, "prolong_fc_internal") != AKMI_COMPLETE) return AKMI_FAIL;
  const Box bx{box[0], box[1], box[2], box[3], box[4], box[5]};
  k_prolong_fc_internal<<<box_grid(bx, 1, g.nmb), dim3(64, 4), 0, (hipStream_t)stream>>>(
      g, c, bx, Faces{bx1f, bx2f, bx3f});
  AKMI_CHECK_LAUNCH("prolong_fc_internal");
  return AKMI_COMPLETE;
}

}  // extern "C"
