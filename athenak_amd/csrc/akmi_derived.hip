// akmi_derived.hip -- derived output variables (BaseTypeOutput::ComputeDerivedVariable, src/outputs/derived_variables.cpp):
// vorticity, current density, field-line curvature, |B|, div B and eint/dens, computed at output time from the stored
// arrays.  One thread owns one cell of the output array, ghost cells included: the linear index of the thread IS the
// offset of the cell inside its MeshBlock, so a wave stores 64 consecutive doubles and loads whole lines of every row
// its stencil touches (x1 fastest); blockIdx.y is the MeshBlock, all blocks of the pack in one launch.  Cells outside
// the reference's loop range are written as zero in the same pass (the reference's array is zero there from
// Kokkos::realloc), so the whole array is defined and a ghost_zones = true output is deterministic.
// The arithmetic lives in akmi_derived.hpp, shared with the CPU build the non-GPU tests use.
#include "akmi_common.hpp"
#include "akmi_derived.hpp"

namespace akmi {
namespace {

constexpr int DV_THREADS = 256;

template <int WHICH>
__global__ void __launch_bounds__(DV_THREADS) k_derived(DvIn a, double *__restrict__ out) {
  const unsigned cells = (unsigned)a.N3*(unsigned)a.N2*(unsigned)a.N1;
  const unsigned c = blockIdx.x*DV_THREADS + threadIdx.x;
  if (c >= cells) return;
  const int m = blockIdx.y;
  const unsigned r = c/(unsigned)a.N1;
  const int i = (int)(c - r*(unsigned)a.N1), j = (int)(r%(unsigned)a.N2), k = (int)(r/(unsigned)a.N2);
  double v = 0.0;
  if (dv_in_range(WHICH, a, k, j, i)) v = derived_cell<WHICH>(a, m, k, j, i);
  out[(size_t)m*cells + c] = v;
}

}  // namespace
}  // namespace akmi

using namespace akmi;

extern "C" {

int akmi_derived_ncomp(int which) {
  return (which >= AKMI_DV_TEMPERATURE && which <= AKMI_DV_DIVB) ? 1 : -1;
}

int akmi_derived_var(const akmi_pack *p, int which, const double *w0, const double *u0, const double *bcc0,
                     const double *bx1f, const double *bx2f, const double *bx3f, double *out, int ncomp_out,
                     void *stream) {
  (void)u0;
  if (!p || !out) { set_error("derived_var: null pack or output array"); return AKMI_FAIL; }
  const int nc = akmi_derived_ncomp(which);
  if (nc < 0) { set_error("derived_var: unknown variable %d", which); return AKMI_FAIL; }
  if (ncomp_out != nc) {
    set_error("derived_var: variable %d has %d component(s), the output array was given %d", which, nc, ncomp_out);
    return AKMI_FAIL;
  }
  const bool needs_w = which <= AKMI_DV_W2, needs_f = which == AKMI_DV_DIVB, needs_b = !needs_w && !needs_f;
  if (needs_w && !w0) { set_error("derived_var: variable %d needs w0", which); return AKMI_FAIL; }
  if (needs_b && !bcc0) { set_error("derived_var: variable %d needs bcc0 (MHD)", which); return AKMI_FAIL; }
  if (needs_f && (!bx1f || !bx2f || !bx3f)) { set_error("derived_var: mhd_divb needs the three face fields"); return AKMI_FAIL; }
  if (which == AKMI_DV_TEMPERATURE && (!p->is_ideal || p->nvar < 5)) {
    set_error("derived_var: temperature (eint/dens) needs the ideal-gas EOS: an isothermal pack stores no energy variable");
    return AKMI_FAIL;
  }
  if (needs_w && p->nvar < 4) { set_error("derived_var: nvar = %d holds no velocity", p->nvar); return AKMI_FAIL; }
  const Geo g = make_geo(p);
  if (g.ng < 1) { set_error("derived_var: the centred differences need a ghost cell"); return AKMI_FAIL; }
  const size_t cells = (size_t)g.N3*g.N2*g.N1;
  if (cells >= ((size_t)1 << 31) || g.nmb > 65535) {
    set_error("derived_var: a MeshBlock of %zu cells / a pack of %d MeshBlocks is outside the launch grid", cells, g.nmb);
    return AKMI_FAIL;
  }
  if (g.nmb <= 0) return AKMI_COMPLETE;
  DvIn a;
  a.nvar = g.nvar; a.N1 = g.N1; a.N2 = g.N2; a.N3 = g.N3;
  a.is = g.is; a.ie = g.ie; a.js = g.js; a.je = g.je; a.ks = g.ks; a.ke = g.ke; a.ng = g.ng;
  a.multi_d = g.multi_d; a.three_d = g.three_d;
  a.dx = g.dx; a.w0 = w0; a.bcc0 = bcc0; a.b1 = bx1f; a.b2 = bx2f; a.b3 = bx3f;
  const dim3 grid((unsigned)((cells + DV_THREADS - 1)/DV_THREADS), (unsigned)g.nmb);
  hipStream_t st = (hipStream_t)stream;
  dv_dispatch(which, [&](auto W) { k_derived<decltype(W)::value><<<grid, dim3(DV_THREADS), 0, st>>>(a, out); });
  AKMI_CHECK_LAUNCH("derived_var");
  return AKMI_COMPLETE;
}

}  // extern "C"
