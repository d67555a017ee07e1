// akmi_amr.hip -- the two device pieces of adaptive mesh refinement:
//   * the refinement criteria: one reduction per MeshBlock over its active cells and the update of its flag
//     (RefinementCriteria::CheckMinMax / CheckSlope / CheckSecondDeriv, src/mesh/refinement_criteria.cpp:177-338);
//   * the regrid: the evolved arrays of the new mesh written out of place from those of the old one -- kept
//     blocks copied whole, derefined blocks restricted from their nleaf children, refined blocks prolongated from
//     the octant of their parent (MeshRefinement::DerefineCC/FCSameRank, CopyCC/FC, CopyForRefinementCC/FC,
//     RefineCC/FC, RepairAMRFC, src/mesh/mesh_refinement.cpp:696-1220).
// The per-cell operators and the thread mapping are those of akmi_refine.hip (akmi_refine_ops.hpp).
#include <cfloat>
#include "akmi_common.hpp"
#include "akmi_refine_ops.hpp"

namespace akmi {

// ---- criteria ---------------------------------------------------------------------------------------------
// One workgroup of 256 per MeshBlock.  Max and min are order-independent, so the tree below is bit-defined.
// method: AKMI_AMR_MIN_MAX q itself; AKMI_AMR_SLOPE 0.5*sqrt(sum_d (q+ - q-)^2)/q; AKMI_AMR_SECOND_DERIV
// |sum_d (q+ - 2q + q-)|/q.  The stencils read one ghost cell at the block's edges.
__global__ void __launch_bounds__(256)
k_amr_check(Geo g, int method, const double *__restrict__ q, long long mstride, int use_max, int use_min,
            double value_max, double value_min, int *__restrict__ flags) {
  __shared__ double smax[256], smin[256];
  const int m = blockIdx.x;
  const int nji = g.nx2*g.nx1, nkji = g.nx3*nji;
  const double *qm = q + (size_t)m*(size_t)mstride;
  auto Q = [&](int k, int j, int i) { return qm[((size_t)k*g.N2 + j)*g.N1 + i]; };
  double vmax = -DBL_MAX, vmin = DBL_MAX;
  for (int idx = threadIdx.x; idx < nkji; idx += 256) {
    int k = idx/nji;
    int j = (idx - k*nji)/g.nx1;
    const int i = (idx - k*nji - j*g.nx1) + g.is;
    j += g.js; k += g.ks;
    const double q0 = Q(k, j, i);
    double val;
    if (method == AKMI_AMR_MIN_MAX) {
      val = q0;
    } else if (method == AKMI_AMR_SLOPE) {
      double a = Q(k, j, i + 1) - Q(k, j, i - 1);
      double d2 = a*a;
      if (g.multi_d) { a = Q(k, j + 1, i) - Q(k, j - 1, i); d2 += a*a; }
      if (g.three_d) { a = Q(k + 1, j, i) - Q(k - 1, j, i); d2 += a*a; }
      val = 0.5*sqrt(d2)/q0;
    } else {
      double d2q = Q(k, j, i + 1) - 2.0*q0 + Q(k, j, i - 1);
      if (g.multi_d) d2q += (Q(k, j + 1, i) - 2.0*q0 + Q(k, j - 1, i));
      if (g.three_d) d2q += (Q(k + 1, j, i) - 2.0*q0 + Q(k - 1, j, i));
      val = fabs(d2q)/q0;
    }
    vmax = fmax(val, vmax);
    vmin = fmin(val, vmin);
  }
  smax[threadIdx.x] = vmax; smin[threadIdx.x] = vmin;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
      smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // only derefine when the flag has not been set by an earlier criterion; equality leaves it alone
    int flag = flags[m];
    if (use_max) {
      if (smax[0] > value_max) flag = 1;
      if (smax[0] < value_max && flag == 0) flag = -1;
    }
    if (use_min) {
      if (smin[0] < value_min) flag = 1;
      if (smin[0] > value_min && flag == 0) flag = -1;
    }
    flags[m] = flag;
  }
}

// ---- regrid -----------------------------------------------------------------------------------------------
// plan: one row {kind, old, octant} per NEW block.  kind 0: the whole block, ghost zones included, is old block
// `old`; kind -1: the active region is the restriction of the nleaf old blocks old .. old+nleaf-1 (Z-ordered, so
// child l sits in octant l); kind +1: the active region is the prolongation of octant `octant` of old block `old`.
// A row that points outside the old pack writes nothing.
struct Plan { int kind, old, oct; };
__device__ __forceinline__ Plan plan_row(const int *__restrict__ plan, int m) {
  return Plan{plan[3*m], plan[3*m + 1], plan[3*m + 2]};
}

__global__ void __launch_bounds__(256)
k_amr_regrid_cc(Geo g, CGeo c, int nvar, int m0, int old_nmb, int nleaf, const int *__restrict__ plan,
                const double *__restrict__ uo, double *__restrict__ un) {
  const Box bx{0, g.N1 - 1, 0, g.N2 - 1, 0, g.N3 - 1};
  int m, v, k, j, i;
  if (!box_index(bx, nvar, m, v, k, j, i)) return;
  m += m0;
  const Plan pl = plan_row(plan, m);
  const int cnx1 = g.nx1/2, cnx2 = g.multi_d ? g.nx2/2 : 1, cnx3 = g.three_d ? g.nx3/2 : 1;
  if (pl.kind == 0) {
    if (pl.old < 0 || pl.old >= old_nmb) return;
    un[ix5(nvar, g.N3, g.N2, g.N1, m, v, k, j, i)] = uo[ix5(nvar, g.N3, g.N2, g.N1, pl.old, v, k, j, i)];
  } else if (pl.kind < 0) {
    if (pl.old < 0 || pl.old + nleaf - 1 >= old_nmb) return;
    if (i < g.is || i > g.ie || j < g.js || j > g.je || k < g.ks || k > g.ke) return;
    const int o1 = (i - g.is) >= cnx1, o2 = g.multi_d && (j - g.js) >= cnx2, o3 = g.three_d && (k - g.ks) >= cnx3;
    const int child = pl.old + o1 + 2*o2 + 4*o3;
    const int fi = g.is + 2*((i - g.is) - o1*cnx1);
    const int fj = g.multi_d ? g.js + 2*((j - g.js) - o2*cnx2) : 0;
    const int fk = g.three_d ? g.ks + 2*((k - g.ks) - o3*cnx3) : 0;
    auto U = [&](int kk, int jj, int ii) { return uo[ix5(nvar, g.N3, g.N2, g.N1, child, v, kk, jj, ii)]; };
    un[ix5(nvar, g.N3, g.N2, g.N1, m, v, k, j, i)] = restrict_cc_cell(g.multi_d, g.three_d, U, fk, fj, fi);
  } else {
    if (pl.old < 0 || pl.old >= old_nmb || pl.oct < 0 || pl.oct >= nleaf) return;
    if (i < c.cis || i > c.cie || j < c.cjs || j > c.cje || k < c.cks || k > c.cke) return;
    // the child's coarse array is the parent's fine array over the octant plus ng cells each side
    const int s1 = (pl.oct & 1)*cnx1, s2 = ((pl.oct >> 1) & 1)*cnx2, s3 = ((pl.oct >> 2) & 1)*cnx3;
    const int fi = (i - c.cis)*2 + g.is, fj = (j - c.cjs)*2 + g.js, fk = (k - c.cks)*2 + g.ks;
    auto CA = [&](int kk, int jj, int ii) {
      return uo[ix5(nvar, g.N3, g.N2, g.N1, pl.old, v, kk + s3, jj + s2, ii + s1)];
    };
    auto A = [&](int kk, int jj, int ii) -> double & { return un[ix5(nvar, g.N3, g.N2, g.N1, m, v, kk, jj, ii)]; };
    prolong_cc_cell(g.multi_d, g.three_d, CA, A, k, j, i, fk, fj, fi);
  }
}

// one component of the face field: copy / restriction over the active faces (the upper plane included, so a
// plane shared by two octants comes from the higher one, as the reference's later copy overwrites the earlier) /
// prolongation of the faces shared with the parent's.  The internal faces of a refined block follow in
// k_amr_internal_fc, once all three components are in place.
template <int COMP>
__global__ void __launch_bounds__(256)
k_amr_regrid_fc(Geo g, CGeo c, int m0, int old_nmb, int nleaf, const int *__restrict__ plan,
                const double *__restrict__ bo, double *__restrict__ bn) {
  constexpr int d1 = COMP == 0, d2 = COMP == 1, d3 = COMP == 2;
  const int F1 = g.N1 + d1, F2 = g.N2 + d2, F3 = g.N3 + d3;
  const Box bx{0, F1 - 1, 0, F2 - 1, 0, F3 - 1};
  int m, v, k, j, i;
  if (!box_index(bx, 1, m, v, k, j, i)) return;
  m += m0;
  const Plan pl = plan_row(plan, m);
  const int cnx1 = g.nx1/2, cnx2 = g.multi_d ? g.nx2/2 : 1, cnx3 = g.three_d ? g.nx3/2 : 1;
  if (pl.kind == 0) {
    if (pl.old < 0 || pl.old >= old_nmb) return;
    bn[ix4(F3, F2, F1, m, k, j, i)] = bo[ix4(F3, F2, F1, pl.old, k, j, i)];
  } else if (pl.kind < 0) {
    if (pl.old < 0 || pl.old + nleaf - 1 >= old_nmb) return;
    if (i < g.is || i > g.ie + d1 || j < g.js || j > g.je + d2 || k < g.ks || k > g.ke + d3) return;
    const int o1 = (i - g.is) >= cnx1, o2 = g.multi_d && (j - g.js) >= cnx2, o3 = g.three_d && (k - g.ks) >= cnx3;
    const int child = pl.old + o1 + 2*o2 + 4*o3;
    const int fi = g.is + 2*((i - g.is) - o1*cnx1);
    const int fj = g.multi_d ? g.js + 2*((j - g.js) - o2*cnx2) : 0;
    const int fk = g.three_d ? g.ks + 2*((k - g.ks) - o3*cnx3) : 0;
    auto B = [&](int kk, int jj, int ii) { return bo[ix4(F3, F2, F1, child, kk, jj, ii)]; };
    bn[ix4(F3, F2, F1, m, k, j, i)] = restrict_fc_face<COMP>(g.multi_d, g.three_d, B, fk, fj, fi);
  } else {
    if (pl.old < 0 || pl.old >= old_nmb || pl.oct < 0 || pl.oct >= nleaf) return;
    if (i < c.cis || i > c.cie + d1 || j < c.cjs || j > c.cje + d2 || k < c.cks || k > c.cke + d3) return;
    const int s1 = (pl.oct & 1)*cnx1, s2 = ((pl.oct >> 1) & 1)*cnx2, s3 = ((pl.oct >> 2) & 1)*cnx3;
    const int fi = (i - c.cis)*2 + g.is;
    const int fj = g.multi_d ? (j - c.cjs)*2 + g.js : j;
    const int fk = g.three_d ? (k - c.cks)*2 + g.ks : k;
    auto CB = [&](int kk, int jj, int ii) { return bo[ix4(F3, F2, F1, pl.old, kk + s3, jj + s2, ii + s1)]; };
    auto B = [&](int kk, int jj, int ii) -> double & { return bn[ix4(F3, F2, F1, m, kk, jj, ii)]; };
    prolong_fc_shared_face<COMP>(g.multi_d, g.three_d, CB, B, k, j, i, fk, fj, fi);
  }
}

// internal faces of the blocks m with flag[m*stride] > 0 (a plan's kind column, or RepairAMRFC's flags) from the
// faces shared with the coarse cells
__global__ void __launch_bounds__(256)
k_amr_internal_fc(Geo g, CGeo c, int m0, const int *__restrict__ flag, int stride, double *__restrict__ b1,
                  double *__restrict__ b2, double *__restrict__ b3) {
  const Box bx{c.cis, c.cie, c.cjs, c.cje, c.cks, c.cke};
  int m, v, k, j, i;
  if (!box_index(bx, 1, m, v, k, j, i)) return;
  m += m0;
  if (!(flag[(size_t)m*stride] > 0)) return;
  const int N1 = g.N1, N2 = g.N2, N3 = g.N3;
  const int fi = (i - c.cis)*2 + g.is, fj = (j - c.cjs)*2 + g.js, fk = (k - c.cks)*2 + g.ks;
  auto B1 = [&](int kk, int jj, int ii) -> double & { return b1[ix4(N3, N2, N1 + 1, m, kk, jj, ii)]; };
  auto B2 = [&](int kk, int jj, int ii) -> double & { return b2[ix4(N3, N2 + 1, N1, m, kk, jj, ii)]; };
  auto B3 = [&](int kk, int jj, int ii) -> double & { return b3[ix4(N3 + 1, N2, N1, m, kk, jj, ii)]; };
  prolong_fc_internal_cell(g.multi_d, g.three_d, B1, B2, B3, fk, fj, fi);
}

static int check_packs(const akmi_pack *po, const akmi_pack *pn, const char *who) {
  if (po->nx1 != pn->nx1 || po->nx2 != pn->nx2 || po->nx3 != pn->nx3 || po->ng != pn->ng) {
    set_error("%s: the old and the new pack differ in their MeshBlock sizes", who); return AKMI_FAIL;
  }
  if (pn->nx1 % 2 || (pn->nx2 > 1 && pn->nx2 % 2) || (pn->nx3 > 1 && pn->nx3 % 2) || pn->ng < 1) {
    set_error("%s: MeshBlock sizes must be even for refinement", who); return AKMI_FAIL;
  }
  if (po->nmb < 1 || pn->nmb < 1) { set_error("%s: empty pack", who); return AKMI_FAIL; }
  return AKMI_COMPLETE;
}

// gridDim.z holds (planes)*(variables)*(blocks): launch over runs of blocks that fit its 65535
template <class F>
static int for_block_runs(int nmb, int per_block, const char *who, F &&launch) {
  if (per_block > 65535) { set_error("%s: %d planes x variables per MeshBlock exceed one launch", who, per_block); return AKMI_FAIL; }
  const int run = 65535/per_block;
  for (int m0 = 0; m0 < nmb; m0 += run) launch(m0, nmb - m0 < run ? nmb - m0 : run);
  return AKMI_COMPLETE;
}

}  // namespace akmi

using namespace akmi;

extern "C" {

int akmi_amr_check(const akmi_pack *p, int method, const double *q, long long mstride, double value_min,
                   double value_max, int *flags, void *stream) {
  Geo g = make_geo(p);
  if (method != AKMI_AMR_MIN_MAX && method != AKMI_AMR_SLOPE && method != AKMI_AMR_SECOND_DERIV) {
    set_error("amr_check: method = %d (min_max 0, slope 1, second_deriv 2)", method); return AKMI_FAIL;
  }
  if (g.nmb < 1 || mstride < (long long)g.N1*g.N2*g.N3) { set_error("amr_check: empty pack or block stride too short"); return AKMI_FAIL; }
  if (method != AKMI_AMR_MIN_MAX && g.ng < 1) { set_error("amr_check: the stencil needs a ghost cell"); return AKMI_FAIL; }
  // refinement_criteria.cpp:192,213: a bound left at its default is not checked; value_min exists for min_max only
  const int use_max = value_max < (double)FLT_MAX;
  const int use_min = method == AKMI_AMR_MIN_MAX && value_min > -(double)FLT_MAX;
  if (!use_max && !use_min) return AKMI_COMPLETE;
  k_amr_check<<<dim3(g.nmb), dim3(256), 0, (hipStream_t)stream>>>(g, method, q, mstride, use_max, use_min, value_max,
                                                                   value_min, flags);
  AKMI_CHECK_LAUNCH("amr_check");
  return AKMI_COMPLETE;
}

int akmi_amr_regrid_cc(const akmi_pack *old_pack, const akmi_pack *new_pack, int nvar, const int *plan,
                       const double *u_old, double *u_new, void *stream) {
  if (check_packs(old_pack, new_pack, "amr_regrid_cc") != AKMI_COMPLETE) return AKMI_FAIL;
  if (nvar < 1) { set_error("amr_regrid_cc: nvar = %d", nvar); return AKMI_FAIL; }
  Geo g = make_geo(new_pack); CGeo c = make_cgeo(g);
  const int nleaf = g.three_d ? 8 : (g.multi_d ? 4 : 2), old_nmb = old_pack->nmb;
  const Box bx{0, g.N1 - 1, 0, g.N2 - 1, 0, g.N3 - 1};
  if (for_block_runs(g.nmb, g.N3*nvar, "amr_regrid_cc", [&](int m0, int n) {
        k_amr_regrid_cc<<<box_grid(bx, nvar, n), dim3(64, 4), 0, (hipStream_t)stream>>>(g, c, nvar, m0, old_nmb, nleaf,
                                                                                      plan, u_old, u_new);
      }) != AKMI_COMPLETE) return AKMI_FAIL;
  AKMI_CHECK_LAUNCH("amr_regrid_cc");
  return AKMI_COMPLETE;
}

int akmi_amr_regrid_fc(const akmi_pack *old_pack, const akmi_pack *new_pack, const int *plan, const double *bo1,
                       const double *bo2, const double *bo3, double *bn1, double *bn2, double *bn3, void *stream) {
  if (check_packs(old_pack, new_pack, "amr_regrid_fc") != AKMI_COMPLETE) return AKMI_FAIL;
  Geo g = make_geo(new_pack); CGeo c = make_cgeo(g);
  const int nleaf = g.three_d ? 8 : (g.multi_d ? 4 : 2), old_nmb = old_pack->nmb;
  hipStream_t st = (hipStream_t)stream;
  const Box b1{0, g.N1, 0, g.N2 - 1, 0, g.N3 - 1}, b2{0, g.N1 - 1, 0, g.N2, 0, g.N3 - 1}, b3{0, g.N1 - 1, 0, g.N2 - 1, 0, g.N3};
  if (for_block_runs(g.nmb, g.N3 + 1, "amr_regrid_fc", [&](int m0, int n) {
        k_amr_regrid_fc<0><<<box_grid(b1, 1, n), dim3(64, 4), 0, st>>>(g, c, m0, old_nmb, nleaf, plan, bo1, bn1);
        k_amr_regrid_fc<1><<<box_grid(b2, 1, n), dim3(64, 4), 0, st>>>(g, c, m0, old_nmb, nleaf, plan, bo2, bn2);
        k_amr_regrid_fc<2><<<box_grid(b3, 1, n), dim3(64, 4), 0, st>>>(g, c, m0, old_nmb, nleaf, plan, bo3, bn3);
      }) != AKMI_COMPLETE) return AKMI_FAIL;
  AKMI_CHECK_LAUNCH("amr_regrid_fc");
  // the internal faces of the refined blocks (plan kind +1), after their shared faces
  const Box bc{c.cis, c.cie, c.cjs, c.cje, c.cks, c.cke};
  if (for_block_runs(g.nmb, c.cke - c.cks + 1, "amr_regrid_fc", [&](int m0, int n) {
        k_amr_internal_fc<<<box_grid(bc, 1, n), dim3(64, 4), 0, st>>>(g, c, m0, plan, 3, bn1, bn2, bn3);
      }) != AKMI_COMPLETE) return AKMI_FAIL;
  AKMI_CHECK_LAUNCH("amr_regrid_fc internal");
  return AKMI_COMPLETE;
}

int akmi_amr_repair_fc(const akmi_pack *p, const int *repair, double *bx1f, double *bx2f, double *bx3f,
                       void *stream) {
  if (check_packs(p, p, "amr_repair_fc") != AKMI_COMPLETE) return AKMI_FAIL;
  Geo g = make_geo(p); CGeo c = make_cgeo(g);
  const Box bc{c.cis, c.cie, c.cjs, c.cje, c.cks, c.cke};
  if (for_block_runs(g.nmb, c.cke - c.cks + 1, "amr_repair_fc", [&](int m0, int n) {
        k_amr_internal_fc<<<box_grid(bc, 1, n), dim3(64, 4), 0, (hipStream_t)stream>>>(g, c, m0, repair, 1, bx1f, bx2f, bx3f);
      }) != AKMI_COMPLETE) return AKMI_FAIL;
  AKMI_CHECK_LAUNCH("amr_repair_fc");
  return AKMI_COMPLETE;
}

}  // extern "C"
