// akmi_c2p.hpp -- the conversion of one cell (conserved -> primitive with floors, floor counters, passive scalars), the
// signal speeds of the CFL scan and the reductions that end it, each written once for every kernel that needs it
// (ConsToPrim and its shell / pairs / SMR forms, the hydro stage kernel, NewTimeStep of the fluid, of diffusion and of the
// source terms).  Device code only, apart from the declaration of fill_fltmax; the arithmetic itself stays in
// akmi_numerics.hpp, which also compiles on the host.  Everything here is __forceinline__ and the build keeps products
// and sums separately rounded (-ffp-contract=off): a caller computes the bits it computed with the body written out.
#ifndef AKMI_C2P_HPP_
#define AKMI_C2P_HPP_
#include "akmi_common.hpp"
#include "akmi_numerics.hpp"

namespace akmi {

// ---------------------------------------------------------------------------------------
// Reductions over the wave: the only __shfl_xor loops of the library (akmi_selftest.hip checks the wave with its own)
AKMI_DEV double wave_min(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  return v;
}
AKMI_DEV double wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
AKMI_DEV double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// *addr = min(*addr, v) for positive doubles, which order like their bit patterns: one 64-bit atomicMin.  One word
// saturates at ~88 atomics/us on this chip: only a caller that can lower the running minimum issues the atomic (the plain
// read is a filter, the atomic decides).
AKMI_DEV void atomic_min_positive(double *addr, double v) {
  if (v < __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMin(reinterpret_cast<unsigned long long *>(addr), (unsigned long long)__double_as_longlong(v));
}

// Minimum (MAX: maximum) over the workgroup: the waves first, then across the nw waves through lds.  tid is the linear
// thread index (wave tid >> 6, lane tid & 63), whatever the shape of the workgroup; every thread has to call, there is
// one barrier inside, and lds must be free to overwrite on entry (wg_reduce: nw doubles, wg_reduce3: 3*nw).
// wg_reduce returns the result in thread 0, wg_reduce3 the result of its value number tid in the threads tid < 3; the
// other threads get a partial result.
template <bool MAX>
AKMI_DEV double reduce2(double a, double b) { return MAX ? fmax(a, b) : fmin(a, b); }
template <bool MAX>
AKMI_DEV double wg_reduce(double v, double *lds, int tid, int nw) {
  v = MAX ? wave_max(v) : wave_min(v);
  if ((tid & 63) == 0) lds[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < nw; ++q) v = reduce2<MAX>(v, lds[q]);
  }
  return v;
}
template <bool MAX>
AKMI_DEV double wg_reduce3(double a, double b, double c, double *lds, int tid, int nw) {
  if constexpr (MAX) { a = wave_max(a); b = wave_max(b); c = wave_max(c); }
  else { a = wave_min(a); b = wave_min(b); c = wave_min(c); }
  const int w = tid >> 6;
  if ((tid & 63) == 0) { lds[w] = a; lds[nw + w] = b; lds[2*nw + w] = c; }
  __syncthreads();
  if (tid < 3) {
    a = lds[tid*nw];
    for (int q = 1; q < nw; ++q) a = reduce2<MAX>(a, lds[tid*nw + q]);
  }
  return a;
}

// The end of a CFL scan: mv1..3 the largest signal speed of this thread's cells per direction (0: none), dx_of_m the three
// cell sizes of the workgroup's MeshBlock, dt3 the three running minima.  One division per workgroup and direction:
// min over cells of fl(dx/a) == fl(dx/max a), a correctly rounded division being monotone.  Arguments as wg_reduce3.
AKMI_DEV void cfl_from_max(double mv1, double mv2, double mv3, const double *__restrict__ dx_of_m,
                           double *__restrict__ dt3, double *lds, int tid, int nw) {
  const double v = wg_reduce3<true>(mv1, mv2, mv3, lds, tid, nw);
  if (tid < 3 && v > 0.0) atomic_min_positive(&dt3[tid], dx_of_m[tid]/v);
}

// |v| + the fast (hydro: sound) speed of one cell along the three directions: hydro_newdt.cpp:97-118,
// mhd_newdt.cpp:123-144; the only place with the rotations of fast_speed.  The field is not read without MHD, we not
// for an isothermal gas.  The mv are assigned: a caller that scans several cells per thread keeps its running fmax
// around the call.  max_speeds_ideal: for the kernels that only ever see an ideal gas (the pairs kernel, the hydro stage
// kernel, which has no register left for the constants of the other branch).
template <bool MHD>
AKMI_DEV void max_speeds_ideal(double gamma, double wd, double wvx, double wvy, double wvz, double we, double bx,
                               double by, double bz, double &mv1, double &mv2, double &mv3) {
  const double pr = (gamma - 1.0)*we;
  if constexpr (MHD) {
    mv1 = fabs(wvx) + fast_speed(gamma, wd, pr, bx, by, bz);
    mv2 = fabs(wvy) + fast_speed(gamma, wd, pr, by, bz, bx);
    mv3 = fabs(wvz) + fast_speed(gamma, wd, pr, bz, bx, by);
  } else {
    const double cs_ = sqrt(gamma*pr/wd);
    mv1 = fabs(wvx) + cs_; mv2 = fabs(wvy) + cs_; mv3 = fabs(wvz) + cs_;
  }
}
template <bool MHD>
AKMI_DEV void max_speeds(const Eos &eos, double wd, double wvx, double wvy, double wvz, double we, double bx, double by,
                         double bz, double &mv1, double &mv2, double &mv3) {
  if (eos.is_ideal) {
    max_speeds_ideal<MHD>(eos.gamma, wd, wvx, wvy, wvz, we, bx, by, bz, mv1, mv2, mv3);
  } else if constexpr (MHD) {
    mv1 = fabs(wvx) + fast_speed_iso(eos.iso_cs, wd, bx, by, bz);
    mv2 = fabs(wvy) + fast_speed_iso(eos.iso_cs, wd, by, bz, bx);
    mv3 = fabs(wvz) + fast_speed_iso(eos.iso_cs, wd, bz, bx, by);
  } else {
    mv1 = fabs(wvx) + eos.iso_cs; mv2 = fabs(wvy) + eos.iso_cs; mv3 = fabs(wvz) + eos.iso_cs;
  }
}

// ---------------------------------------------------------------------------------------
// The cell-centred field from the six faces of the cell, through bcc_from_faces (akmi_numerics.hpp)
AKMI_DEV void cell_bcc(double x_lo, double x_hi, double y_lo, double y_hi, double z_lo, double z_hi, double &bx,
                       double &by, double &bz) {
  bx = bcc_from_faces(x_lo, x_hi); by = bcc_from_faces(y_lo, y_hi); bz = bcc_from_faces(z_lo, z_hi);
}
// ... of cell (m, k, j, i) of the three face arrays of a pack
AKMI_DEV void cell_bcc(const Geo &g, const double *__restrict__ bx1f, const double *__restrict__ bx2f,
                       const double *__restrict__ bx3f, int m, int k, int j, int i, double &bx, double &by, double &bz) {
  cell_bcc(bx1f[ix4(g.N3, g.N2, g.N1 + 1, m, k, j, i)], bx1f[ix4(g.N3, g.N2, g.N1 + 1, m, k, j, i + 1)],
           bx2f[ix4(g.N3, g.N2 + 1, g.N1, m, k, j, i)], bx2f[ix4(g.N3, g.N2 + 1, g.N1, m, k, j + 1, i)],
           bx3f[ix4(g.N3 + 1, g.N2, g.N1, m, k, j, i)], bx3f[ix4(g.N3 + 1, g.N2, g.N1, m, k + 1, j, i)], bx, by, bz);
}

// c2p_hyd / c2p_mhd by the template parameter (the pairs kernel converts an ideal gas only and calls this directly)
template <bool MHD>
AKMI_DEV void c2p_ideal(const Eos &eos, double &ud, double umx, double umy, double umz, double &ue, double bx,
                        double by, double bz, double &wd, double &wvx, double &wvy, double &wvz, double &we, bool &dfl,
                        bool &efl, bool &tfl) {
  if constexpr (MHD) c2p_mhd(eos, ud, umx, umy, umz, ue, bx, by, bz, wd, wvx, wvy, wvz, we, dfl, efl, tfl);
  else c2p_hyd(eos, ud, umx, umy, umz, ue, wd, wvx, wvy, wvz, we, dfl, efl, tfl);
}

// The conversion of one cell.  Ideal gas: SingleC2P_IdealHyd / _IdealMHD (c2p_hyd / c2p_mhd).  Isothermal gas:
// SingleC2P_IsothermalHyd / _IsothermalMHD (isothermal_hyd.cpp:30-45, isothermal_mhd.cpp:32-47; density floor
// fmax(dfloor, b^2/sigma_max) :104-106) -- no energy variable: ue is not read, we is 0 and efl / tfl stay false.
// ud and ue come back floored; what to do with that is the caller's business (c2p_commit).
template <bool MHD>
AKMI_DEV void c2p_convert(const Eos &eos, double &ud, double umx, double umy, double umz, double &ue, double bx,
                          double by, double bz, double &wd, double &wvx, double &wvy, double &wvz, double &we, bool &dfl,
                          bool &efl, bool &tfl) {
  if (eos.is_ideal) {
    c2p_ideal<MHD>(eos, ud, umx, umy, umz, ue, bx, by, bz, wd, wvx, wvy, wvz, we, dfl, efl, tfl);
  } else {
    double dfloor_ = eos.dfloor;
    if constexpr (MHD) dfloor_ = fmax(eos.dfloor, (sqr(bx) + sqr(by) + sqr(bz))/eos.sigma_max);
    if (ud < dfloor_) { ud = dfloor_; dfl = true; }
    wd = ud;
    double di;
    vel_from_cons(ud, umx, umy, umz, di, wvx, wvy, wvz);
    we = 0.0;
  }
}

// The five fluid variables of the cell at c (variable stride cs), converted: loads, c2p_convert.
template <bool MHD>
AKMI_DEV void c2p_convert_at(const Eos &eos, const double *__restrict__ u0, size_t c, size_t cs, double &ud, double &ue,
                             double bx, double by, double bz, double &wd, double &wvx, double &wvy, double &wvz,
                             double &we, bool &dfl, bool &efl, bool &tfl) {
  ud = u0[c];
  ue = eos.is_ideal ? u0[c + 4*cs] : 0.0;
  c2p_convert<MHD>(eos, ud, u0[c + cs], u0[c + 2*cs], u0[c + 3*cs], ue, bx, by, bz, wd, wvx, wvy, wvz, we, dfl, efl, tfl);
}

// What ConsToPrim leaves in memory for the cell at c: the floored density / energy back into u0 and one count per floor
// that acted (never on the hot path), the primitives -- w0[0..3] unless DROP (mask of AKMI_DROP_*, ideal gas only) says that
// the caller's next sweeps take them from u0 -- and the passive scalars: ideal gas from variable 5 with their zero floor
// (ideal_hyd.cpp:94-101), isothermal gas from variable 4 without (isothermal_*.cpp).  The cell-centred field is stored by
// the caller, next to cell_bcc.
template <int DROP = 0>
AKMI_DEV void c2p_commit(const Geo &g, const Eos &eos, double *__restrict__ u0, double *__restrict__ w0,
                         int *__restrict__ counters, size_t c, size_t cs, double ud, double ue, double wd, double wvx,
                         double wvy, double wvz, double we, bool dfl, bool efl, bool tfl) {
  if (dfl) { u0[c] = ud; atomicAdd(&counters[0], 1); }
  if (efl) { u0[c + 4*cs] = ue; atomicAdd(&counters[1], 1); }
  if (tfl) { u0[c + 4*cs] = ue; atomicAdd(&counters[2], 1); }
  if constexpr (!(DROP & AKMI_DROP_W03)) { w0[c] = wd; w0[c + cs] = wvx; w0[c + 2*cs] = wvy; w0[c + 3*cs] = wvz; }
  if (eos.is_ideal) {
    w0[c + 4*cs] = we;
    for (int n = 5; n < g.nvar; ++n) {
      double us = u0[c + n*cs];
      if (us < 0.0) { us = 0.0; u0[c + n*cs] = 0.0; }
      w0[c + n*cs] = us/ud;
    }
  } else {
    for (int n = 4; n < g.nvar; ++n) w0[c + n*cs] = u0[c + n*cs]/ud;
  }
}

// The other way for the cell at c: SingleP2C_IdealHyd / _IdealMHD (src/eos/ideal_c2p_hyd.hpp:76-83,
// ideal_c2p_mhd.hpp:75-84; mhd: (bx, by, bz) is the cell-centred field) and, without an energy variable, their
// isothermal forms with the passive scalars from variable 4.
AKMI_DEV void p2c_at(int nvar, bool is_ideal, bool mhd, const double *__restrict__ w, double *__restrict__ u, size_t c,
                     size_t cs, double bx, double by, double bz) {
  const double d = w[c], vx = w[c + cs], vy = w[c + 2*cs], vz = w[c + 3*cs];
  u[c] = d; u[c + cs] = d*vx; u[c + 2*cs] = d*vy; u[c + 3*cs] = d*vz;
  if (is_ideal) {
    if (mhd) u[c + 4*cs] = w[c + 4*cs] + 0.5*(d*(sqr(vx) + sqr(vy) + sqr(vz)) + (sqr(bx) + sqr(by) + sqr(bz)));
    else u[c + 4*cs] = w[c + 4*cs] + 0.5*d*(sqr(vx) + sqr(vy) + sqr(vz));
  }
  for (int n = is_ideal ? 5 : 4; n < nvar; ++n) u[c + n*cs] = d*w[c + n*cs];
}

// x[0..n) = FLT_MAX, n <= 64: where a running minimum starts (akmi_stage_c2p.hip)
void fill_fltmax(double *x, int n, hipStream_t st);

}  // namespace akmi
#endif
