// akmi_srcterms.hip -- physical source terms of the fluid equations, <hydro_srcterms> / <mhd_srcterms>
// (SourceTerms, src/srcterms/srcterms.cpp, srcterms_newdt.cpp, ismcooling.hpp):
//   constant acceleration   src = (bdt*g)*rho;  u(dir) += src;  ideal gas: u(IEN) += src*v(dir)          srcterms.cpp:113-132
//   ISM cooling             T = temp_unit*e/rho*gm1;  u(IEN) -= (bdt*rho)*(rho*Lambda(T)/cu - hrate/hu)  srcterms.cpp:139-168
// Both read the OLD primitives w0 and read-modify-write the updated conserved state u0 of the active cells.  One
// thread owns one cell and applies the enabled terms in the reference's order (ApplySrcTerms, srcterms.cpp:93-101),
// every value with the reference's sequence of roundings (the library is built with -ffp-contract=off), so one
// launch gives the bits of the reference's two.  The cooling function calls the device's log10 / exp / pow, which
// are not glibc's: that term agrees with a CPU evaluation to a few 1e-13 relative, not bit for bit.
#include <cfloat>
#include "akmi_common.hpp"
#include "akmi_c2p.hpp"

namespace akmi {
namespace {

constexpr int SX = 64, SY = 4;        // 256 threads: four waves, lanes over i / the flattened (row, i) index

// log10 of the SPEX cooling rate [erg cm^3 / s] at log10 T = 4.12, 4.16, ... 8.16: Table 2 of Schure et al.,
// A&A 508, 751 (2009), the numbers the reference tabulates.  Single precision data, widened to double where used
// (ismcooling.hpp keeps them as float and multiplies by double operands).
__device__ const float spex_lhd[102] = {
  -22.5977f, -21.9689f, -21.5972f, -21.4615f, -21.4789f, -21.5497f, -21.6211f, -21.6595f, -21.6426f, -21.5688f,
  -21.4771f, -21.3755f, -21.2693f, -21.1644f, -21.0658f, -20.9778f, -20.8986f, -20.8281f, -20.7700f, -20.7223f,
  -20.6888f, -20.6739f, -20.6815f, -20.7051f, -20.7229f, -20.7208f, -20.7058f, -20.6896f, -20.6797f, -20.6749f,
  -20.6709f, -20.6748f, -20.7089f, -20.8031f, -20.9647f, -21.1482f, -21.2932f, -21.3767f, -21.4129f, -21.4291f,
  -21.4538f, -21.5055f, -21.5740f, -21.6300f, -21.6615f, -21.6766f, -21.6886f, -21.7073f, -21.7304f, -21.7491f,
  -21.7607f, -21.7701f, -21.7877f, -21.8243f, -21.8875f, -21.9738f, -22.0671f, -22.1537f, -22.2265f, -22.2821f,
  -22.3213f, -22.3462f, -22.3587f, -22.3622f, -22.3590f, -22.3512f, -22.3420f, -22.3342f, -22.3312f, -22.3346f,
  -22.3445f, -22.3595f, -22.3780f, -22.4007f, -22.4289f, -22.4625f, -22.4995f, -22.5353f, -22.5659f, -22.5895f,
  -22.6059f, -22.6161f, -22.6208f, -22.6213f, -22.6184f, -22.6126f, -22.6045f, -22.5945f, -22.5831f, -22.5707f,
  -22.5573f, -22.5434f, -22.5287f, -22.5140f, -22.4992f, -22.4844f, -22.4695f, -22.4543f, -22.4392f, -22.4237f,
  -22.4087f, -22.3928f};

// ISMCoolFn (ismcooling.hpp:19-60).  The three temperature ranges are per-lane branches: a wave of a cooling run
// usually sits in one of them (neighbouring cells have neighbouring temperatures) and then skips the other two;
// a wave that straddles a branch point runs both sides under the exec mask, which is what the expensive part --
// pow / exp, some 100 fp64 instructions each -- costs either way.
__device__ __forceinline__ double ism_cool_fn(double temp) {
  const double logt = log10(temp);
  if (logt <= 4.2)       // Koyama & Inutsuka (2002)
    return (2.0e-19*exp(-1.184e5/(temp + 1.0e3)) + 2.8e-28*sqrt(temp)*exp(-92.0/temp));
  if (logt > 8.15)       // power law above the table
    return pow(10.0, (0.45*logt - 26.065));
  int ipps = static_cast<int>(25.0*logt) - 103;
  ipps = (ipps < 100) ? ipps : 100;
  ipps = (ipps > 0) ? ipps : 0;           // (also what a NaN temperature ends as: the index stays inside the table)
  const double x0 = 4.12 + 0.04*static_cast<double>(ipps);
  const double dx = logt - x0;
  const double logcool = ((double)spex_lhd[ipps + 1]*dx - (double)spex_lhd[ipps]*(dx - 0.04))*25.0;
  return pow(10.0, logcool);
}

// rho*(rho*lambda_cooling - gamma_heating) without the leading factor: what both the source term and its time step use
struct Cool { double gm1, temp_unit, cooling_unit, heating_unit, hrate; };
__device__ __forceinline__ void cool_rates(const Cool &c, double rho, double eint, double &lambda_cooling,
                                           double &gamma_heating) {
  const double temp = c.temp_unit*eint/rho*c.gm1;
  lambda_cooling = ism_cool_fn(temp)/c.cooling_unit;
  gamma_heating = c.hrate/c.heating_unit;
}

// the cell of this thread: base of MeshBlock m / variable 0 in scalar registers, byte offset of the lane in 32 bits;
// threads outside the box read cell (ks, js, is) so that the loads need no branch
struct Lane { unsigned ob; size_t mb; bool in; };
__device__ __forceinline__ Lane lane_of(const Geo &g, int fm) {
  const Cell3 q = flat_cells(fm, g.N1, g.is, g.ie, g.js, g.nx2, g.ks, g.nx3);
  const int i = q.in ? q.i : g.is, j = q.in ? q.j : g.js, k = q.in ? q.k : g.ks;
  Lane l;
  l.ob = (unsigned)(((unsigned)k*(unsigned)g.N2 + (unsigned)j)*(unsigned)g.N1 + (unsigned)i)*8u;
  l.mb = (size_t)q.m*g.nvar*g.N3*g.N2*g.N1;
  l.in = q.in;
  return l;
}

template <bool ACCEL, bool COOL>
__global__ void __launch_bounds__(SX*SY)
k_srcterms(Geo g, int is_ideal, int dir, double gacc, Cool c, double beta, double dt, const double *__restrict__ dt_dev,
           const double *__restrict__ w0, double *__restrict__ u0, int fm) {
  const Lane l = lane_of(g, fm);
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const double *wm = w0 + l.mb;
  double *um = u0 + l.mb;
  const double bdt = beta*(dt_dev ? *dt_dev : dt);
  const double rho = ldu(wm, l.ob);
  double vdir = 0.0, eint = 0.0, udir = 0.0, uen = 0.0;
  if (ACCEL) { vdir = ldu(wm + dir*cs, l.ob); udir = ldu(um + dir*cs, l.ob); }
  if (COOL) eint = ldu(wm + 4*cs, l.ob);
  if (is_ideal) uen = ldu(um + 4*cs, l.ob);
  if (ACCEL) {
    const double src = bdt*gacc*rho;
    udir += src;
    if (is_ideal) uen += src*vdir;
  }
  if (COOL) {
    double lam, gh;
    cool_rates(c, rho, eint, lam, gh);
    uen -= bdt*rho*(rho*lam - gh);
  }
  if (!l.in) return;
  if (ACCEL) stu(um + dir*cs, l.ob, udir);
  if (is_ideal) stu(um + 4*cs, l.ob, uen);
}

// SourceTerms::NewTimeStep, srcterms_newdt.cpp:25-72 (ism_cooling): min over the active cells of
// eint/(FLT_MIN + |rho*(rho*lambda - gamma_heating)|).  The minimum over the workgroup, then one filtered atomic minimum
// (akmi_c2p.hpp); a minimum does not depend on the order.
__global__ void __launch_bounds__(SX*SY)
k_srcterms_newdt(Geo g, Cool c, const double *__restrict__ w0, double *__restrict__ dtmin, int fm) {
  __shared__ double sm[SY];
  const Lane l = lane_of(g, fm);
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const double *wm = w0 + l.mb;
  const double rho = ldu(wm, l.ob), eint = ldu(wm + 4*cs, l.ob);
  double lam, gh;
  cool_rates(c, rho, eint, lam, gh);
  const double cooling_heating = (double)FLT_MIN + fabs(rho*(rho*lam - gh));
  double v = l.in ? eint/cooling_heating : (double)FLT_MAX;
  v = wg_reduce<false>(v, sm, threadIdx.y*SX + threadIdx.x, SY);
  if (threadIdx.x == 0 && threadIdx.y == 0) atomic_min_positive(dtmin, v);
}

int check_args(const akmi_pack *p, const akmi_srcterms *s, const char *who) {
  if (!p || !s) { set_error("%s: null pack or parameter struct", who); return AKMI_FAIL; }
  if (p->nvar < (p->is_ideal ? 5 : 4)) {
    set_error("%s: nvar = %d is smaller than the fluid variable set of the EOS", who, p->nvar);
    return AKMI_FAIL;
  }
  if (s->const_accel && (s->const_accel_dir < 1 || s->const_accel_dir > 3)) {
    set_error("%s: const_accel_dir must be 1, 2 or 3 (got %d)", who, s->const_accel_dir);
    return AKMI_FAIL;
  }
  if (s->ism_cooling && !p->is_ideal) {
    set_error("%s: ism_cooling needs the ideal-gas EOS", who);
    return AKMI_FAIL;
  }
  // 32-bit byte offsets of a lane inside one variable of one MeshBlock
  const Geo g = make_geo(p);
  if ((size_t)g.N3*g.N2*g.N1*8 >= ((size_t)1 << 32)) {
    set_error("%s: one variable of one MeshBlock has to stay below 4 GB", who);
    return AKMI_FAIL;
  }
  return AKMI_COMPLETE;
}

Cool make_cool(const akmi_srcterms *s) {
  return Cool{s->gamma - 1.0, s->temp_unit, s->cooling_unit, s->heating_unit, s->hrate};
}

// same choice as akmi_rk_update (profiles/r06_lane_mapping.txt): small blocks flatten planes and columns
int lane_mode(const Geo &g) { return (g.three_d && g.nx1*g.nx2 <= SX*SY) ? (FLAT_K | FLAT_COLS) : 0; }

}  // namespace
}  // namespace akmi

using namespace akmi;

extern "C" {

int akmi_srcterms_apply(const akmi_pack *p, const akmi_srcterms *s, double beta, double dt, const double *dt_dev,
                        const double *w0, double *u0, void *stream) {
  if (check_args(p, s, "srcterms_apply") != AKMI_COMPLETE) return AKMI_FAIL;
  if (!s->const_accel && !s->ism_cooling) return AKMI_COMPLETE;
  const Geo g = make_geo(p);
  const int fm = lane_mode(g);
  const dim3 grid = flat_cells_grid(fm, g.N1, g.is, g.ie, g.nx2, g.nx3, g.nmb, SX*SY), block(SX, SY);
  hipStream_t st = (hipStream_t)stream;
  const Cool c = make_cool(s);
  const int dir = s->const_accel ? s->const_accel_dir : 1;
  if (s->const_accel && s->ism_cooling)
    k_srcterms<true, true><<<grid, block, 0, st>>>(g, p->is_ideal, dir, s->const_accel_val, c, beta, dt, dt_dev, w0, u0, fm);
  else if (s->const_accel)
    k_srcterms<true, false><<<grid, block, 0, st>>>(g, p->is_ideal, dir, s->const_accel_val, c, beta, dt, dt_dev, w0, u0, fm);
  else
    k_srcterms<false, true><<<grid, block, 0, st>>>(g, p->is_ideal, dir, s->const_accel_val, c, beta, dt, dt_dev, w0, u0, fm);
  AKMI_CHECK_LAUNCH("srcterms_apply");
  return AKMI_COMPLETE;
}

int akmi_srcterms_newdt(const akmi_pack *p, const akmi_srcterms *s, const double *w0, double *dtmin, void *stream) {
  if (check_args(p, s, "srcterms_newdt") != AKMI_COMPLETE) return AKMI_FAIL;
  hipStream_t st = (hipStream_t)stream;
  fill_fltmax(dtmin, 1, st);
  if (s->ism_cooling) {
    const Geo g = make_geo(p);
    const int fm = lane_mode(g);
    const dim3 grid = flat_cells_grid(fm, g.N1, g.is, g.ie, g.nx2, g.nx3, g.nmb, SX*SY), block(SX, SY);
    k_srcterms_newdt<<<grid, block, 0, st>>>(g, make_cool(s), w0, dtmin, fm);
  }
  AKMI_CHECK_LAUNCH("srcterms_newdt");
  return AKMI_COMPLETE;
}

}  // extern "C"
