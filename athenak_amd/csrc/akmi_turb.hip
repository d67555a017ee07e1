// akmi_turb.hip -- driven turbulence (<turb_driving>): TurbulenceDriver of src/srcterms/turb_driver.cpp.
//
// Host part (no GPU needed): the random generator (L'Ecuyer's combined generator with the Bays-Durham shuffle,
// Numerical Recipes ran2, and the Marsaglia polar form of Box-Muller), the mode list, the per-cycle amplitude
// table (InitializeModes, turb_driver.cpp:389-610) and the per-block sin/cos tables at cell centres
// (Initialize, turb_driver.cpp:226-270).
//
// Device part, per cycle:
//   k_turb_synth    force_tmp of all modes in ONE pass (the reference makes one pass per mode), each term
//                   ((amp*xt)*yt)*zt added in the reference's order from 0.0; emits per-tile partials of
//                   sum rho, sum rho*f1..3
//   k_turb_moments  force_tmp -= t_c/t0 (the mean), partials of sum rho*|f|^2, sum m.f
//   k_turb_force    OU update force = fcorr*force + gcorr*(s*force_tmp), push m += (rho*f)*dt, partials of
//                   sum rho, sum m
//   k_turb_netmom   m -= (rho*t_c)/t0
// Reductions: a fixed-shape tree inside a workgroup of TILE cells, the tiles of one MeshBlock summed by a
// fixed-shape tree (k_tile_sum) into per-MeshBlock partials.  No floating-point atomics: the per-block partials
// depend only on the block's cells, and the host sums them in gid order, so results do not depend on the rank count.
#include "akmi_common.hpp"
#include "akmi_tile_reduce.hpp"
#include <cfloat>
#include <cmath>
#include <vector>

namespace akmi {

// ---------------------------------------------------------------------------------------
// random numbers (host)
namespace {
constexpr int64_t IMR1 = 2147483563, IMR2 = 2147483399, IMM1 = IMR1 - 1;
constexpr int64_t IA1 = 40014, IA2 = 40692, IQ1 = 53668, IQ2 = 52774, IR1 = 12211, IR2 = 3791;
constexpr int NTAB = AKMI_RNG_NTAB;
constexpr int64_t NDIV = 1 + IMM1/NTAB;
constexpr double AM = 1.0/IMR1;
constexpr double RNMX = 1.0 - DBL_EPSILON;
}  // namespace

static double ran_uniform(akmi_rng_state *st) {
  long long *idum = &st->idum;
  int64_t k;
  if (*idum <= 0) {                       // initialise
    st->idum2 = 123456789;
    st->iy = 0;
    *idum = (-(*idum) < 1) ? 1 : -(*idum);
    st->idum2 = *idum;
    for (int j = NTAB + 7; j >= 0; j--) {  // load the shuffle table after 8 warm-ups
      k = (*idum)/IQ1;
      *idum = IA1*(*idum - k*IQ1) - k*IR1;
      if (*idum < 0) *idum += IMR1;
      if (j < NTAB) st->iv[j] = *idum;
    }
    st->iy = st->iv[0];
  }
  k = (*idum)/IQ1;                        // idum = (IA1*idum) % IMR1 by Schrage's method
  *idum = IA1*(*idum - k*IQ1) - k*IR1;
  if (*idum < 0) *idum += IMR1;
  k = st->idum2/IQ2;                      // idum2 = (IA2*idum2) % IMR2 likewise
  st->idum2 = IA2*(st->idum2 - k*IQ2) - k*IR2;
  if (st->idum2 < 0) st->idum2 += IMR2;
  const int j = static_cast<int>(st->iy/NDIV);
  st->iy = st->iv[j] - st->idum2;         // shuffle, combine
  st->iv[j] = *idum;
  if (st->iy < 1) st->iy += IMM1;
  const double temp = AM*st->iy;
  return temp > RNMX ? RNMX : temp;
}

// polar Box-Muller; the second deviate of a pair is cached IN the state (iset/gset), so a saved state continues
static double ran_gaussian(akmi_rng_state *st) {
  if (st->idum < 0) st->iset = 0;
  if (st->iset == 0) {
    double v1, v2, rsq;
    do {
      v1 = 2.0*ran_uniform(st) - 1.0;
      v2 = 2.0*ran_uniform(st) - 1.0;
      rsq = v1*v1 + v2*v2;
    } while (rsq >= 1.0 || rsq == 0.0);
    const double fac = std::sqrt(-2.0*std::log(rsq)/rsq);
    st->gset = v1*fac;
    st->iset = 1;
    return v2*fac;
  }
  st->iset = 0;
  return st->gset;
}

// the mode selection of turb_driver.cpp:70-94 / 394-408
static bool mode_selected(int nkx, int nky, int nkz, int nlow, int nhigh, int driving_type) {
  if (nkx == 0 && nky == 0 && nkz == 0) return false;
  const int nlow_sqr = nlow*nlow, nhigh_sqr = nhigh*nhigh;
  int nsqr = 0;
  bool flag_prl = true;
  if (driving_type == 0) {
    nsqr = nkx*nkx + nky*nky + nkz*nkz;
  } else {
    nsqr = nkx*nkx + nky*nky;
    const int nprlsqr = nkz*nkz;
    flag_prl = nprlsqr >= nlow_sqr && nprlsqr <= nhigh_sqr;
  }
  return nsqr >= nlow_sqr && nsqr <= nhigh_sqr && flag_prl;
}

static bool turb_args_ok(int nlow, int nhigh, int driving_type) {
  if (driving_type != 0 && driving_type != 1) {
    set_error("<turb_driving>/driving_type = %d: 0 (isotropic) or 1 (anisotropic)", driving_type);
    return false;
  }
  if (nlow < 0 || nhigh < nlow) {
    set_error("<turb_driving> nlow = %d, nhigh = %d: need 0 <= nlow <= nhigh", nlow, nhigh);
    return false;
  }
  return true;
}

// ---------------------------------------------------------------------------------------
// device kernels (tiles, trees and per-MeshBlock partials: akmi_tile_reduce.hpp)

// force_tmp of every mode in one pass.  amp[n][24]: component-major, per component the 8 terms
// ccc ccs csc css scc scs ssc sss (x-trig, y-trig, z-trig).  Tables x?(m,n,i) over the active cells only.
__global__ void __launch_bounds__(NT)
k_turb_synth(TurbGeo g, int nmode, const double *__restrict__ amp, const double *__restrict__ xs,
             const double *__restrict__ xc, const double *__restrict__ ys, const double *__restrict__ yc,
             const double *__restrict__ zs, const double *__restrict__ zc, const double *__restrict__ u0,
             double *__restrict__ ftmp, double *__restrict__ tiles) {
  const int m = blockIdx.x/g.ntile, tile = blockIdx.x - m*g.ntile;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = 0; p < PER; ++p) {
    const int c = tile*TILE + p*NT + threadIdx.x;
    if (c >= g.ncell) break;
    int k, j, i;
    cell_of(g, c, k, j, i);
    const double *xsm = xs + (size_t)m*nmode*g.nx1, *xcm = xc + (size_t)m*nmode*g.nx1;
    const double *ysm = ys + (size_t)m*nmode*g.nx2, *ycm = yc + (size_t)m*nmode*g.nx2;
    const double *zsm = zs + (size_t)m*nmode*g.nx3, *zcm = zc + (size_t)m*nmode*g.nx3;
    double f[3] = {0.0, 0.0, 0.0};
    for (int n = 0; n < nmode; ++n) {
      const double xt[2] = {xcm[n*g.nx1 + i], xsm[n*g.nx1 + i]};
      const double yt[2] = {ycm[n*g.nx2 + j], ysm[n*g.nx2 + j]};
      const double zt[2] = {zcm[n*g.nx3 + k], zsm[n*g.nx3 + k]};
      const double *a = amp + 24*n;
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int t = 0; t < 8; ++t)
          f[d] += ((a[8*d + t]*xt[t >> 2])*yt[(t >> 1) & 1])*zt[t & 1];
    }
    const int kk = k + g.ks, jj = j + g.js, ii = i + g.is;
    const double den = u0[ix5(g.nvar, g.N3, g.N2, g.N1, m, AKMI_IDN, kk, jj, ii)];
    for (int d = 0; d < 3; ++d) ftmp[ix5(3, g.N3, g.N2, g.N1, m, d, kk, jj, ii)] = f[d];
    acc[0] += den;
    acc[1] += den*f[0];
    acc[2] += den*f[1];
    acc[3] += den*f[2];
  }
  block_sum<4>(acc, tiles + (size_t)blockIdx.x*4);
}

__global__ void __launch_bounds__(NT)
k_turb_moments(TurbGeo g, double t0, double t1, double t2, double t3, const double *__restrict__ u0,
               double *__restrict__ ftmp, double *__restrict__ tiles) {
  const int m = blockIdx.x/g.ntile, tile = blockIdx.x - m*g.ntile;
  double acc[2] = {0.0, 0.0};
  for (int p = 0; p < PER; ++p) {
    const int c = tile*TILE + p*NT + threadIdx.x;
    if (c >= g.ncell) break;
    int k, j, i;
    cell_of(g, c, k, j, i);
    k += g.ks; j += g.js; i += g.is;
    const size_t f0 = ix5(3, g.N3, g.N2, g.N1, m, 0, k, j, i), fs = (size_t)g.N3*g.N2*g.N1;
    const double v1 = ftmp[f0] - t1/t0, v2 = ftmp[f0 + fs] - t2/t0, v3 = ftmp[f0 + 2*fs] - t3/t0;
    ftmp[f0] = v1; ftmp[f0 + fs] = v2; ftmp[f0 + 2*fs] = v3;
    const size_t u = ix5(g.nvar, g.N3, g.N2, g.N1, m, AKMI_IDN, k, j, i);
    const double den = u0[u], mom1 = u0[u + fs], mom2 = u0[u + 2*fs], mom3 = u0[u + 3*fs];
    acc[0] += den*(v1*v1 + v2*v2 + v3*v3);
    acc[1] += mom1*v1 + mom2*v2 + mom3*v3;
  }
  block_sum<2>(acc, tiles + (size_t)blockIdx.x*2);
}

__global__ void __launch_bounds__(NT)
k_turb_force(TurbGeo g, double fcorr, double gcorr, double s, double dt, const double *__restrict__ ftmp,
             double *__restrict__ force, double *__restrict__ u0, double *__restrict__ tiles) {
  const int m = blockIdx.x/g.ntile, tile = blockIdx.x - m*g.ntile;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = 0; p < PER; ++p) {
    const int c = tile*TILE + p*NT + threadIdx.x;
    if (c >= g.ncell) break;
    int k, j, i;
    cell_of(g, c, k, j, i);
    k += g.ks; j += g.js; i += g.is;
    const size_t fs = (size_t)g.N3*g.N2*g.N1, f0 = ix5(3, g.N3, g.N2, g.N1, m, 0, k, j, i);
    const size_t u = ix5(g.nvar, g.N3, g.N2, g.N1, m, AKMI_IDN, k, j, i);
    const double den = u0[u];
    double mom[3];
    for (int d = 0; d < 3; ++d) {
      // force_tmp *= s (turb_driver.cpp:806-810) kept unstored: the same product at every use
      const double v = fcorr*force[f0 + d*fs] + gcorr*(ftmp[f0 + d*fs]*s);
      force[f0 + d*fs] = v;
      mom[d] = u0[u + (d + 1)*fs] + den*v*dt;
      u0[u + (d + 1)*fs] = mom[d];
    }
    acc[0] += den;
    acc[1] += mom[0];
    acc[2] += mom[1];
    acc[3] += mom[2];
  }
  block_sum<4>(acc, tiles + (size_t)blockIdx.x*4);
}

__global__ void __launch_bounds__(NT)
k_turb_netmom(TurbGeo g, double t0, double t1, double t2, double t3, double *__restrict__ u0) {
  const int m = blockIdx.x/g.ntile, tile = blockIdx.x - m*g.ntile;
  for (int p = 0; p < PER; ++p) {
    const int c = tile*TILE + p*NT + threadIdx.x;
    if (c >= g.ncell) break;
    int k, j, i;
    cell_of(g, c, k, j, i);
    k += g.ks; j += g.js; i += g.is;
    const size_t fs = (size_t)g.N3*g.N2*g.N1, u = ix5(g.nvar, g.N3, g.N2, g.N1, m, AKMI_IDN, k, j, i);
    const double den = u0[u];
    u0[u + fs] -= den*t1/t0;
    u0[u + 2*fs] -= den*t2/t0;
    u0[u + 3*fs] -= den*t3/t0;
  }
}

}  // namespace akmi

using namespace akmi;

extern "C" {

double akmi_rng_uniform(akmi_rng_state *st) { return ran_uniform(st); }
double akmi_rng_gaussian(akmi_rng_state *st) { return ran_gaussian(st); }
int akmi_rng_state_bytes(void) { return (int)sizeof(akmi_rng_state); }

int akmi_turb_mode_count(int nlow, int nhigh, int driving_type) {
  if (!turb_args_ok(nlow, nhigh, driving_type)) return AKMI_FAIL;
  int n = 0;
  for (int nkx = 0; nkx <= nhigh; nkx++)
    for (int nky = 0; nky <= nhigh; nky++)
      for (int nkz = 0; nkz <= nhigh; nkz++)
        if (mode_selected(nkx, nky, nkz, nlow, nhigh, driving_type)) ++n;
  return n;
}

int akmi_turb_amplitudes(int nlow, int nhigh, int driving_type, double expo, double exp_prp, double exp_prl,
                         double lx, double ly, double lz, akmi_rng_state *rstate, double *kvec, double *amp) {
  if (!turb_args_ok(nlow, nhigh, driving_type)) return AKMI_FAIL;
  const double dkx = 2.0*M_PI/lx, dky = 2.0*M_PI/ly, dkz = 2.0*M_PI/lz;
  int nmode = 0;
  for (int nkx = 0; nkx <= nhigh; nkx++) {
    for (int nky = 0; nky <= nhigh; nky++) {
      for (int nkz = 0; nkz <= nhigh; nkz++) {
        if (!mode_selected(nkx, nky, nkz, nlow, nhigh, driving_type)) continue;
        const double kx = dkx*nkx, ky = dky*nky, kz = dkz*nkz;
        if (kvec) { kvec[3*nmode] = kx; kvec[3*nmode + 1] = ky; kvec[3*nmode + 2] = kz; }
        if (!amp) { ++nmode; continue; }
        double *a = amp + 24*nmode;
        // a[0..7] x, a[8..15] y, a[16..23] z; per component ccc ccs csc css scc scs ssc sss
        double &xccc = a[0], &xccs = a[1], &xcsc = a[2], &xcss = a[3], &xscc = a[4], &xscs = a[5], &xssc = a[6],
               &xsss = a[7];
        double &yccc = a[8], &yccs = a[9], &ycsc = a[10], &ycss = a[11], &yscc = a[12], &yscs = a[13],
               &yssc = a[14], &ysss = a[15];
        double &zccc = a[16], &zccs = a[17], &zcsc = a[18], &zcss = a[19], &zscc = a[20], &zscs = a[21],
               &zssc = a[22], &zsss = a[23];
        for (int q = 0; q < 24; ++q) a[q] = 0.0;
        akmi_rng_state *rs = rstate;
        double norm = 0.0;
        if (driving_type == 0) {                               // turb_driver.cpp:413-516
          const double kiso = std::sqrt(kx*kx + ky*ky + kz*kz);
          norm = (kiso > 1e-16) ? 1.0/std::pow(kiso, (expo + 2.0)/2.0) : 0.0;
          if (nkz != 0) {
            const double ikz = 1.0/(dkz*((double)nkz));
            xccc = ran_gaussian(rs);
            xccs = ran_gaussian(rs);
            xcsc = (nky == 0) ? 0.0 : ran_gaussian(rs);
            xcss = (nky == 0) ? 0.0 : ran_gaussian(rs);
            xscc = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            xscs = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            xssc = (nkx == 0 || nky == 0) ? 0.0 : ran_gaussian(rs);
            xsss = (nkx == 0 || nky == 0) ? 0.0 : ran_gaussian(rs);
            yccc = ran_gaussian(rs);
            yccs = ran_gaussian(rs);
            ycsc = (nky == 0) ? 0.0 : ran_gaussian(rs);
            ycss = (nky == 0) ? 0.0 : ran_gaussian(rs);
            yscc = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            yscs = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            yssc = (nkx == 0 || nky == 0) ? 0.0 : ran_gaussian(rs);
            ysss = (nkx == 0 || nky == 0) ? 0.0 : ran_gaussian(rs);
            // incompressibility
            zccc = ikz*(kx*xscs + ky*ycss);
            zccs = -ikz*(kx*xscc + ky*ycsc);
            zcsc = ikz*(kx*xsss - ky*yccs);
            zcss = ikz*(-kx*xssc + ky*yccc);
            zscc = ikz*(-kx*xccs + ky*ysss);
            zscs = ikz*(kx*xccc - ky*yssc);
            zssc = -ikz*(kx*xcss + ky*yscs);
            zsss = ikz*(kx*xcsc + ky*yscc);
          } else if (nky != 0) {
            const double iky = 1.0/(dky*((double)nky));
            xccc = ran_gaussian(rs);
            xcsc = ran_gaussian(rs);
            xscc = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            xssc = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            zccc = ran_gaussian(rs);
            zcsc = ran_gaussian(rs);
            zscc = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            zssc = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            yccc = iky*kx*xssc;
            ycsc = -iky*kx*xscc;
            yscc = -iky*kx*xcsc;
            yssc = iky*kx*xccc;
          } else {
            zccc = ran_gaussian(rs);
            zscc = ran_gaussian(rs);
            yccc = ran_gaussian(rs);
            yscc = ran_gaussian(rs);
          }
        } else {                                               // turb_driver.cpp:517-579
          const double kprl = std::sqrt(kx*kx);
          const double kprp = std::sqrt(ky*ky + kz*kz);
          norm = (kprl > 1e-16 && kprp > 1e-16) ?
              1.0/std::pow(kprp, (exp_prp + 1.0)/2.0)/std::pow(kprl, exp_prl/2.0) : 0.0;
          if (nky != 0) {
            const double iky = 1.0/(dky*((double)nky));
            xccc = ran_gaussian(rs);
            xccs = ran_gaussian(rs);
            xcsc = ran_gaussian(rs);
            xcss = ran_gaussian(rs);
            xscc = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            xscs = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            xssc = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            xsss = (nkx == 0) ? 0.0 : ran_gaussian(rs);
            yccc = iky*(kx*xssc);
            yccs = iky*(kx*xsss);
            ycsc = -iky*(kx*xscc);
            ycss = -iky*(kx*xscs);
            yscc = -iky*(kx*xcsc);
            yscs = -iky*(kx*xcss);
            yssc = iky*(kx*xccc);
            ysss = iky*(kx*xccs);
          } else {
            yccc = ran_gaussian(rs);
            yscc = ran_gaussian(rs);
          }
        }
        for (int q = 0; q < 24; ++q) a[q] *= norm;              // turb_driver.cpp:580-604
        ++nmode;
      }
    }
  }
  return nmode;
}

int akmi_turb_tables(int nmb, int nmode, int nx1, int nx2, int nx3, const double *kvec, const double *bounds,
                     double *xs, double *xc, double *ys, double *yc, double *zs, double *zc) {
  // CellCenterX, src/coordinates/cell_locations.hpp:35-39
  auto ccx = [](int ith, int n, double xmin, double xmax) {
    const double x = ((double)ith + 0.5)/(double)n;
    return (x*xmax - x*xmin) - (0.5*xmax - 0.5*xmin) + (0.5*xmin + 0.5*xmax);
  };
  const int nx[3] = {nx1, nx2, nx3};
  double *s[3] = {xs, ys, zs}, *c[3] = {xc, yc, zc};
  for (int m = 0; m < nmb; ++m)
    for (int n = 0; n < nmode; ++n)
      for (int d = 0; d < 3; ++d)
        for (int i = 0; i < nx[d]; ++i) {
          const size_t o = ((size_t)m*nmode + n)*nx[d] + i;
          if (d > 0 && nx[d] == 1) { s[d][o] = 0.0; c[d][o] = 1.0; continue; }   // collapsed dimension
          const double xv = ccx(i, nx[d], bounds[6*m + 2*d], bounds[6*m + 2*d + 1]);
          const double kv = kvec[3*n + d];
          s[d][o] = std::sin(kv*xv);
          c[d][o] = std::cos(kv*xv);
        }
  return AKMI_COMPLETE;
}

long long akmi_turb_workspace_bytes(const akmi_pack *p) {
  const TurbGeo g = make_tgeo(p);
  return (long long)p->nmb*g.ntile*4*sizeof(double);
}

int akmi_turb_synthesize(const akmi_pack *p, int nmode, const double *amp, const double *xs, const double *xc,
                         const double *ys, const double *yc, const double *zs, const double *zc, const double *u0,
                         double *force_tmp, double *partial, double *work, void *stream) {
  if (!pack_ok(p, "turb_synthesize")) return AKMI_FAIL;
  const TurbGeo g = make_tgeo(p);
  hipStream_t st = (hipStream_t)stream;
  k_turb_synth<<<p->nmb*g.ntile, NT, 0, st>>>(g, nmode, amp, xs, xc, ys, yc, zs, zc, u0, force_tmp, work);
  AKMI_CHECK_LAUNCH("turb_synthesize");
  return finish_partials<4>(g, p->nmb, work, partial, st, "turb_synthesize partials");
}

int akmi_turb_moments(const akmi_pack *p, double t0, double t1, double t2, double t3, const double *u0,
                      double *force_tmp, double *partial, double *work, void *stream) {
  if (!pack_ok(p, "turb_moments")) return AKMI_FAIL;
  const TurbGeo g = make_tgeo(p);
  hipStream_t st = (hipStream_t)stream;
  k_turb_moments<<<p->nmb*g.ntile, NT, 0, st>>>(g, t0, t1, t2, t3, u0, force_tmp, work);
  AKMI_CHECK_LAUNCH("turb_moments");
  return finish_partials<2>(g, p->nmb, work, partial, st, "turb_moments partials");
}

int akmi_turb_add_forcing(const akmi_pack *p, double fcorr, double gcorr, double s, double dt,
                          const double *force_tmp, double *force, double *u0, double *partial, double *work,
                          void *stream) {
  if (!pack_ok(p, "turb_add_forcing")) return AKMI_FAIL;
  const TurbGeo g = make_tgeo(p);
  hipStream_t st = (hipStream_t)stream;
  k_turb_force<<<p->nmb*g.ntile, NT, 0, st>>>(g, fcorr, gcorr, s, dt, force_tmp, force, u0, work);
  AKMI_CHECK_LAUNCH("turb_add_forcing");
  return finish_partials<4>(g, p->nmb, work, partial, st, "turb_add_forcing partials");
}

int akmi_turb_remove_net_mom(const akmi_pack *p, double t0, double t1, double t2, double t3, double *u0,
                             void *stream) {
  if (!pack_ok(p, "turb_remove_net_mom")) return AKMI_FAIL;
  const TurbGeo g = make_tgeo(p);
  k_turb_netmom<<<p->nmb*g.ntile, NT, 0, (hipStream_t)stream>>>(g, t0, t1, t2, t3, u0);
  AKMI_CHECK_LAUNCH("turb_remove_net_mom");
  return AKMI_COMPLETE;
}

}  // extern "C"
