// akmi_stage_march_x2.hip -- the marches along x2 (k_sweep_update<1, ..>) and the 1-D tile kernel (k_sweep_update_1d),
// instantiated from akmi_stage_march.hpp, and the passive scalars of a fused stage (k_scalar_update).
//
// k_scalar_update stands in this unit, ahead of the marches, on purpose: it and the hydro k_sweep_update_1d kernels
// inline the same index and RK-store helpers, and the compiler's result for the latter depends on where those helpers
// stand in the module.  With the scalars first, as they stood in the single unit this one was cut from, the 1-D kernels
// compile to the machine code they had there (tools/stage_split_isa.py, profiles/stage_split_isa.txt).
#include "akmi_stage.hpp"

namespace akmi {

// ---------------------------------------------------------------------------------------
// Passive scalars of the fused stage (hydro_fluxes.cpp:135-147, mhd_fluxes.cpp:153-166 + RKUpdate): a
// scalar's flux is the mass flux times its upwind reconstructed value, so the Riemann kernels only
// have to leave the mass fluxes behind (the MHD sweeps store them anyway, for CornerE); this kernel
// reconstructs each scalar at the six faces of a cell, forms the divergence in the reference's order
// and applies the RK update, CopyCons folded in.  Same operations as the task-granular kernels.
template <int RECON>
__global__ void __launch_bounds__(SX*SY)
k_scalar_update(Geo g, FaceEos eos, const double *__restrict__ w0, const double *__restrict__ m1,
                const double *__restrict__ m2, const double *__restrict__ m3, UpdArgs u, int k0, int nk,
                int nf) {
  // nf: number of fluid variables (5 ideal gas, 4 isothermal); the scalars follow them
  const long p = ((long)blockIdx.x*SY + threadIdx.y)*SX + threadIdx.x;   // rows [js,je] x N1
  const int jj = (int)(p/g.N1);
  const int i = (int)(p - (long)jj*g.N1);
  const int j = g.js + jj;
  const int m = blockIdx.z/nk;
  const int k = k0 + (blockIdx.z - m*nk);
  if (i < g.is || i > g.ie || j > g.je) return;
  const double dx1 = g.dx[3*m], dx2 = g.dx[3*m + 1], dx3 = g.dx[3*m + 2];
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const double bdt = beta_dt_of(u.beta_dt, u.dtp);
  const double f1l = m1[ix5(g.nvar, g.N3, g.N2, g.N1 + 1, m, 0, k, j, i)];
  const double f1h = m1[ix5(g.nvar, g.N3, g.N2, g.N1 + 1, m, 0, k, j, i + 1)];
  double f2l = 0.0, f2h = 0.0, f3l = 0.0, f3h = 0.0;
  if (g.multi_d) {
    f2l = m2[ix5(g.nvar, g.N3, g.N2 + 1, g.N1, m, 0, k, j, i)];
    f2h = m2[ix5(g.nvar, g.N3, g.N2 + 1, g.N1, m, 0, k, j + 1, i)];
  }
  if (g.three_d) {
    f3l = m3[ix5(g.nvar, g.N3 + 1, g.N2, g.N1, m, 0, k, j, i)];
    f3h = m3[ix5(g.nvar, g.N3 + 1, g.N2, g.N1, m, 0, k + 1, j, i)];
  }
  const long s2 = g.N1, s3 = (long)g.N1*g.N2;
  for (int n = nf; n < g.nvar; ++n) {
    const size_t c = ix5(g.nvar, g.N3, g.N2, g.N1, m, n, k, j, i);
    const double *q = w0 + c;
    double sl, sr;
    face_states<RECON, 0>(q, 1, eos, sl, sr);
    const double a_lo = f1l*((f1l >= 0.0) ? sl : sr);
    face_states<RECON, 0>(q + 1, 1, eos, sl, sr);
    const double a_hi = f1h*((f1h >= 0.0) ? sl : sr);
    double divf = (a_hi - a_lo)/dx1;
    if (g.multi_d) {
      face_states<RECON, 0>(q, s2, eos, sl, sr);
      const double b_lo = f2l*((f2l >= 0.0) ? sl : sr);
      face_states<RECON, 0>(q + s2, s2, eos, sl, sr);
      const double b_hi = f2h*((f2h >= 0.0) ? sl : sr);
      divf += (b_hi - b_lo)/dx2;
    }
    if (g.three_d) {
      face_states<RECON, 0>(q, s3, eos, sl, sr);
      const double c_lo = f3l*((f3l >= 0.0) ? sl : sr);
      face_states<RECON, 0>(q + s3, s3, eos, sl, sr);
      const double c_hi = f3h*((f3h >= 0.0) ? sl : sr);
      divf += (c_hi - c_lo)/dx3;
    }
    const double u0v = u.u0[c];
    const double u1v = u.copy_u1 ? u0v : u.u1[c];
    rk_store(u.u0, u.u1, u.copy_u1, c, u0v, u.gam0*u0v + u.gam1*u1v - bdt*divf);
  }
}

// passive scalars of the planes [k0, k0+nk-1] (after the sweeps that left the mass fluxes of these cells)
int launch_scalars(const Geo &g, const Scheme &sc, const double *w0, const double *m1,
                   const double *m2, const double *m3, const UpdArgs &u, int k0, int nk,
                   hipStream_t st) {
  const int nf = sc.iso ? 4 : 5;
  dim3 grid((unsigned)(((long)(g.je - g.js + 1)*g.N1 + SX*SY - 1)/(SX*SY)), 1, nk*g.nmb), block(SX, SY);
  return dispatch_recon(sc.recon, [&](auto R) {
    k_scalar_update<decltype(R)::value><<<grid, block, 0, st>>>(g, sc.eos, w0, m1, m2, m3, u, k0, nk, nf);
    AKMI_CHECK_LAUNCH("scalar_update");
    return AKMI_COMPLETE;
  });
}

}  // namespace akmi

#include "akmi_stage_march.hpp"

namespace akmi {

AKMI_INST_MARCH(0, true, 0, false)     // 1-D
AKMI_INST_MARCH(0, false, 0, false)
AKMI_INST_MARCH(1, true, 0, false)     // 2-D: the last direction, finishes the update
AKMI_INST_MARCH(1, false, 0, false)
AKMI_INST_MARCH(1, true, 1, false)     // 3-D, generic sequence: leaves acc for the x3 march
AKMI_INST_MARCH(1, false, 1, false)
AKMI_INST_MARCH(1, true, 2, false)     // task-granular path: stores the fluxes
AKMI_INST_MARCH(1, false, 2, false)

}  // namespace akmi
