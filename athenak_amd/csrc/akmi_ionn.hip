// akmi_ionn.hip -- the implicit part of the ImEx integrators of two-fluid (ion-neutral) MHD:
// IonNeutral::ImpRKUpdate, src/ion-neutral/ion-neutral_tasks.cpp:144-292.
//
// The reference walks every cell of the pack, ghost zones included, three times per implicit stage:
//   imex_exp  u += a_twid[istage-2][s]*dt * ru[s]   for s = 0 .. istage-2            (:160-184)
//   imex_imp  the analytic solution of the implicit difference equations of the drag (:189-246)
//   imex_rup  ru[istage-1] = R(U), the stiff source of the state just solved for     (:250-289)
// Nothing in them couples one cell to another, so one thread owns one cell and performs the three in that order on
// the eight values it holds in registers (ion and neutral density and momenta): one read and one write of the
// state instead of three and two, and ru[istage-1] is formed from registers.  Every value takes the reference's
// sequence of roundings (the library is built with -ffp-contract=off; division and sqrt of the device are correctly
// rounded), with one deliberate departure: a slab s whose coefficient is exactly 0.0 is not read and not added.
// The reference adds 0.0*ru[s] there, which changes nothing but the sign of a -0.0 (and would spread a NaN or Inf
// of an unused slab).  The host passes the non-zero coefficients only; imex2+ then reads one slab in one stage and
// none in the others.
//
// Layout: all cells take part, so a variable of a MeshBlock is one contiguous run of ncell = N1*N2*N3 doubles and
// the thread index is the flat cell index: no rows, no tails.  MeshBlocks sit on the second grid axis.  The variable
// strides of the two fluids (4 isothermal, 5 ideal gas, plus passive scalars) are independent; only the planes
// IDN, IM1..IM3 of either fluid are touched.  Pure streaming fp64: 8 + 8*(non-zero s) doubles read and 16 written
// per cell and stage (8 written by the last, explicit-only call); no LDS, no atomics.
#include "akmi_common.hpp"

namespace akmi {
namespace {

constexpr int NT = 256;               // four waves per workgroup
constexpr int MAX_SLABS = 4;          // nimp_stages <= 4: at most ru[0..3] enter one update

struct IonnSlabs { int n; int s[MAX_SLABS]; double adt[MAX_SLABS]; };
struct IonnCoef { double gamma_adt, xi_adt, alpha_adt, drag, xi, alpha; };

// SOLVE: parts (b) and (c); ALPHA: the alpha_adt > 0 branch of the density solve (uniform over the launch)
template <bool SOLVE, bool ALPHA>
__global__ void __launch_bounds__(NT)
k_ionn_imp_update(unsigned ncell, int nmb, int nvar_i, int nvar_n, int istage, IonnSlabs sl, IonnCoef c,
                  double *__restrict__ ui, double *__restrict__ un, double *__restrict__ ru) {
  const unsigned cell = blockIdx.x*NT + threadIdx.x;
  if (cell >= ncell) return;
  const size_t m = blockIdx.y;
  double *pi = ui + m*(size_t)nvar_i*ncell + cell;       // IDN of this cell; IM1..IM3 follow at stride ncell
  double *pn = un + m*(size_t)nvar_n*ncell + cell;
  double di = pi[0], mi1 = pi[(size_t)ncell], mi2 = pi[2*(size_t)ncell], mi3 = pi[3*(size_t)ncell];
  double dn = pn[0], mn1 = pn[(size_t)ncell], mn2 = pn[2*(size_t)ncell], mn3 = pn[3*(size_t)ncell];

  // (a) imex_exp, ascending s.  ru(0..2) -> ion momenta, ru(3..5) -> neutral momenta, ru(6), ru(7) -> densities
#pragma unroll
  for (int q = 0; q < MAX_SLABS; ++q) {
    if (q < sl.n) {
      const double adt = sl.adt[q];
      const double *r = ru + ((size_t)sl.s[q]*nmb + m)*8*(size_t)ncell + cell;
      mi1 += adt*r[0];
      mi2 += adt*r[(size_t)ncell];
      mi3 += adt*r[2*(size_t)ncell];
      mn1 += adt*r[3*(size_t)ncell];
      mn2 += adt*r[4*(size_t)ncell];
      mn3 += adt*r[5*(size_t)ncell];
      di += adt*r[6*(size_t)ncell];
      dn += adt*r[7*(size_t)ncell];
    }
  }

  if (SOLVE) {
    // (b) imex_imp
    const double gamma_adt = c.gamma_adt, xi_adt = c.xi_adt, alpha_adt = c.alpha_adt;
    double rho_i = di;
    if (ALPHA) {
      const double d = 1./4./alpha_adt/alpha_adt + xi_adt/2./alpha_adt/alpha_adt
                       + xi_adt*xi_adt/4./alpha_adt/alpha_adt + di/alpha_adt + xi_adt/alpha_adt*(di + dn);
      rho_i = -1./2./alpha_adt - xi_adt/2./alpha_adt + sqrt(d);
    }
    const double rho_n = di + dn - rho_i;
    di = rho_i;
    dn = rho_n;
    const double denom = 1.0 + gamma_adt*(rho_i + rho_n) + xi_adt + alpha_adt*rho_i;
    double sum = (mi1 + mn1);
    double u_i = (mi1 + (gamma_adt*rho_i + xi_adt)*sum)/denom;
    mn1 = sum - u_i;
    mi1 = u_i;
    sum = (mi2 + mn2);
    u_i = (mi2 + (gamma_adt*rho_i + xi_adt)*sum)/denom;
    mn2 = sum - u_i;
    mi2 = u_i;
    sum = (mi3 + mn3);
    u_i = (mi3 + (gamma_adt*rho_i + xi_adt)*sum)/denom;
    mn3 = sum - u_i;
    mi3 = u_i;

    // (c) imex_rup into ru[istage-1]
    const double drag = c.drag, xi = c.xi, alpha = c.alpha;
    double *r = ru + ((size_t)(istage - 1)*nmb + m)*8*(size_t)ncell + cell;
    r[0] = drag*(di*mn1 - dn*mi1) + xi*mn1 - alpha*di*mi1;
    r[(size_t)ncell] = drag*(di*mn2 - dn*mi2) + xi*mn2 - alpha*di*mi2;
    r[2*(size_t)ncell] = drag*(di*mn3 - dn*mi3) + xi*mn3 - alpha*di*mi3;
    r[3*(size_t)ncell] = drag*(dn*mi1 - di*mn1) - xi*mn1 + alpha*di*mi1;
    r[4*(size_t)ncell] = drag*(dn*mi2 - di*mn2) - xi*mn2 + alpha*di*mi2;
    r[5*(size_t)ncell] = drag*(dn*mi3 - di*mn3) - xi*mn3 + alpha*di*mi3;
    r[6*(size_t)ncell] = xi*dn - alpha*di*di;
    r[7*(size_t)ncell] = -xi*dn + alpha*di*di;
  }

  pi[0] = di; pi[(size_t)ncell] = mi1; pi[2*(size_t)ncell] = mi2; pi[3*(size_t)ncell] = mi3;
  pn[0] = dn; pn[(size_t)ncell] = mn1; pn[2*(size_t)ncell] = mn2; pn[3*(size_t)ncell] = mn3;
}

}  // namespace
}  // namespace akmi

using namespace akmi;

extern "C" {

int akmi_ionn_imp_update(int nmb, long long ncell, int nvar_i, int nvar_n, int nimp_stages, int istage, int do_solve,
                         const double *adt, double gamma_adt, double xi_adt, double alpha_adt, double drag_coeff,
                         double ionization_coeff, double recombination_coeff, double *ui, double *un, double *ru,
                         void *stream) {
  if (!ui || !un || !ru) { set_error("ionn_imp_update: null array"); return AKMI_FAIL; }
  if (nmb < 1 || nmb > 65535) { set_error("ionn_imp_update: nmb = %d, 1 .. 65535 MeshBlocks per pack", nmb); return AKMI_FAIL; }
  if (ncell < 1 || ncell >= (1ll << 31)) {
    set_error("ionn_imp_update: ncell = %lld, one variable of one MeshBlock holds 1 .. 2^31-1 cells", ncell);
    return AKMI_FAIL;
  }
  if (nvar_i < 4 || nvar_n < 4) {
    set_error("ionn_imp_update: nvar_i = %d, nvar_n = %d: each fluid carries at least IDN, IM1..IM3", nvar_i, nvar_n);
    return AKMI_FAIL;
  }
  if (nimp_stages < 1 || nimp_stages > MAX_SLABS) {
    set_error("ionn_imp_update: nimp_stages = %d (1 .. %d)", nimp_stages, MAX_SLABS);
    return AKMI_FAIL;
  }
  // istage = 1 .. nimp_stages solve and store ru[istage-1]; istage = nimp_stages+1 is the last, explicit-only call
  if (istage < 1 || istage > nimp_stages + 1 || (do_solve && istage > nimp_stages)) {
    set_error("ionn_imp_update: istage = %d with do_solve = %d is outside the %d slabs of ru", istage, do_solve,
              nimp_stages);
    return AKMI_FAIL;
  }
  if (istage > 1 && !adt) { set_error("ionn_imp_update: istage = %d needs %d coefficients", istage, istage - 1); return AKMI_FAIL; }
  IonnSlabs sl{};
  for (int s = 0; s <= istage - 2; ++s) {
    if (adt[s] == 0.0) continue;           // not read, not added (see the head of this file)
    sl.s[sl.n] = s;
    sl.adt[sl.n] = adt[s];
    ++sl.n;
  }
  if (!do_solve && sl.n == 0) return AKMI_COMPLETE;       // nothing changes
  const IonnCoef c{gamma_adt, xi_adt, alpha_adt, drag_coeff, ionization_coeff, recombination_coeff};
  const dim3 grid((unsigned)((ncell + NT - 1)/NT), (unsigned)nmb), block(NT);
  hipStream_t st = (hipStream_t)stream;
  if (!do_solve)
    k_ionn_imp_update<false, false><<<grid, block, 0, st>>>((unsigned)ncell, nmb, nvar_i, nvar_n, istage, sl, c, ui, un, ru);
  else if (alpha_adt > 0)
    k_ionn_imp_update<true, true><<<grid, block, 0, st>>>((unsigned)ncell, nmb, nvar_i, nvar_n, istage, sl, c, ui, un, ru);
  else
    k_ionn_imp_update<true, false><<<grid, block, 0, st>>>((unsigned)ncell, nmb, nvar_i, nvar_n, istage, sl, c, ui, un, ru);
  AKMI_CHECK_LAUNCH("ionn_imp_update");
  return AKMI_COMPLETE;
}

}  // extern "C"
