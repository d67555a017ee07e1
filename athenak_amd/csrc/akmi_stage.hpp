// akmi_stage.hpp -- what more than one unit of the fused stage needs (internal; not part of the C ABI).
// The kernels of the stage are compiled per family, each unit with its launchers:
//   akmi_stage_sweeps.hip    k_sweep (thread-per-face x1 / x2 / x3 sweeps)
//   akmi_stage_march_x2.hip  k_scalar_update; k_sweep_update along x2, k_sweep_update_1d   } the marches of both
//   akmi_stage_march_x3.hip  k_sweep_update along x3                                       } over akmi_stage_march.hpp
//   akmi_stage_mhd.hip       k_sweep12s, k_corner_ct, k_ct_copy
//   akmi_stage_hydro.hip     k_hydro_stage3d2 (akmi_hydro_stage3d2.hpp)
//   akmi_stage_c2p.hip       ConsToPrim + CFL scan, with the entry points that need nothing else
//   akmi_c2p.hpp             the conversion of one cell, the signal speeds and the reductions of a CFL scan, for these two
//                            units and the task-granular ones (akmi_tasks, akmi_diffusion, akmi_srcterms, akmi_smr)
//   akmi_stage.hip           the plan of a stage, stage_update and the remaining entry points: no kernel
// The launchers are templates declared at the end of this file; each is instantiated explicitly in the unit that
// defines it, for exactly the combinations the callers use -- a missed one is a link error.
// A tuning macro that one unit reads stays in that unit; the ones below are read by several, so a -D flag for them has
// to reach every unit (tools/build_variant.sh does that by default).
#ifndef AKMI_STAGE_HPP_
#define AKMI_STAGE_HPP_
#include <cstdlib>
#include "akmi_common.hpp"
#include "akmi_c2p.hpp"

namespace akmi {

constexpr int SX = 64, SY = 4;     // plain flux kernels: one wave per row, 4 rows
constexpr int TX = 64;             // 1-D tile width

struct SweepArgs {
  const double *w0, *bcc0, *bxf;
  double *flx, *ey, *ez;          // this direction's flux (face-shaped) and face EMFs
  double *ecc1, *ecc2, *ecc3;     // cell-centred EMFs (x1 sweep only)
  int il, iu, jl, ju, kl, ku;     // face ranges of this sweep
  int f3, f2, f1;
  const double *bt1 = nullptr, *bt2 = nullptr;     // x3 march in its face form: b0.x1f and b0.x2f
  unsigned char *mfb = nullptr;   // byte form of the mass-flux sign (AKMI_MF_BYTES): one byte per face of this direction
};

// Sign of the mass flux as a byte.  On the fused 3-D MHD paths without passive scalars k_corner_ct is the only reader of the
// three mass fluxes, and all it takes from each is `>= 0.0` (the upwind choice of GS05/07): the sweeps store that bit as
// one byte per face instead of the double, the corner kernel tests the byte.  Same comparison as before, made by the
// producer: -0.0 counts as non-negative, NaN as negative (not the sign bit).  The bytes live in the workspace regions of
// the doubles they replace, face-shaped like them: byte offset = double offset / 8, block m at m*(faces of a block).
// 0: doubles everywhere (A/B builds, tools/build_variant.sh).
#ifndef AKMI_MF_BYTES
#define AKMI_MF_BYTES 1
#endif
__device__ __forceinline__ void st_mfs(unsigned char *__restrict__ base, unsigned ob, double fd) {
  base[ob >> 3] = (unsigned char)(fd >= 0.0);
}
__device__ __forceinline__ bool ld_mfs(const unsigned char *__restrict__ base, unsigned ob) { return base[ob >> 3] != 0; }

#ifndef AKMI_POW2DX
#define AKMI_POW2DX 1           // cell sizes that are powers of two: x/dx as one v_ldexp_f64 (wave-uniform choice at run time)
#endif
struct UpdArgs {
  double gam0, gam1, beta_dt;
  double *u0, *u1;
  const double *flx1, *flx2;      // fluxes of the earlier sweeps (face-shaped)
  int copy_u1;
  double *acc;                    // partial divergence (written by the x2 march, read by x3)
  const double *dtp;              // non-null: beta_dt holds the RK weight beta and dt is read from
                                  // device memory (a captured cycle replayed with a new time step)
};
// copy_u1 / copy_b1: 0 = the second register (u1, b1) holds the state of the start of the cycle;
// 1 = first stage, CopyCons folded in: the register receives the old state, u0 / b0 the new one;
// 2 = first stage OUT OF PLACE: u0 / b0 are only read, the new state goes to u1 / b1 and the caller
//     swaps the two registers afterwards -- the copy (5 + 3 arrays written) disappears.  Only the cells /
//     faces the update touches are written: the ghost zones of the new register are filled by the halo
//     exchange and the boundary conditions that follow every stage.
// 3 = LAST stage of a cycle OUT OF PLACE (MHD, the k_sweep12s + x3 march sequence only): u0 and u1 are read, the new state
//     goes to u1's buffer, whose old content (the state at the start of the cycle) nothing reads any more, and the caller
//     swaps the two registers.  The face field stays in place (k_corner_ct sees copy_b1 == 0).
// A stage that does not write the array it reads may run the x3 march in its u0 form (AKMI_COPY_X3_U0, sweep_update_body).
__device__ __forceinline__ bool rk_reads_u1(int copy) { return copy == 0 || copy == 3; }
__device__ __forceinline__ void rk_store(double *__restrict__ u0, double *__restrict__ u1, int copy, size_t c,
                                         double old, double res) {
  if (copy == 2) { u1[c] = res; return; }
  if (copy) u1[c] = old;
  u0[c] = res;
}
// beta*dt: the product the host forms in RKUpdate (hydro_update.cpp:35), same operands, same rounding
__device__ __forceinline__ void rk_store_u(double *__restrict__ u0, double *__restrict__ u1, int copy, unsigned ob,
                                           double old, double res) {
  if (copy >= 2) { stu(u1, ob, res); return; }
  if (copy) stu(u1, ob, old);
  stu(u0, ob, res);
}
__device__ __forceinline__ double beta_dt_of(double beta_dt, const double *dtp) {
  return dtp ? beta_dt*(*dtp) : beta_dt;
}

#ifndef AKMI_ML
#define AKMI_ML 32
#endif
constexpr int ML = AKMI_ML;            // faces marched per thread (chunk length), full-size packs

// chunk length of a marching kernel: ML when that still gives several workgroups per CU, shorter
// marches (more, smaller chunks; one face per chunk is recomputed) for small packs, which would
// otherwise leave most of the 256 CUs idle behind a few long serial chains.  Results do not
// depend on the chunking.
inline int march_len(long col_blocks, int ncells, int nmb, int lmax, int wgs_per_cu = 0) {
  const long want = 2048;                       // workgroups per launch (scan: profiles/r01_small_packs.txt)
  long ml = col_blocks*(long)ncells*nmb/want;
  if (ml > lmax) ml = lmax;
  if (ml < 4) ml = 4;
  static const int tail = getenv("AKMI_TAIL") ? atoi(getenv("AKMI_TAIL")) : 1;
  // tail == 1: the rule below for every launch that asks for it (round 3: with the residency the kernel really
  // has -- two workgroups per CU for the x3 march -- full-length marches gain too: 256^3 x3 march 965 -> 907-914 us
  // at 14 instead of 32 faces, 8 chunks x 263 workgroups being 4.1 rounds of 512; profiles/r03_ab2.txt);
  // tail == 2: the round-2 behaviour (short marches only)
  // (packs of many blocks keep the plain rule: with tens of rounds the fill of the last one does not matter and
  //  every extra chunk costs its priming -- 960 blocks of 32^3, PPM4: x2/x3 marches 1750 -> 2330 us with two
  //  chunks of 17 instead of 32 + 1, profiles/r03_config5.txt)
  const double rounds_plain = (double)(col_blocks*((ncells + ml - 1)/ml)*nmb)/(256.0*(wgs_per_cu > 0 ? wgs_per_cu : 1));
  if (wgs_per_cu > 0 && tail && (ml < lmax || (tail == 1 && rounds_plain < 8.0))) {
    // equal-length workgroups run in rounds of (256 CUs x resident workgroups): pick the chunk
    // length whose last round is fullest, charging the face each chunk recomputes.  Used by the
    // x2/x3 marches of small packs (128^3: -7 % per march); full-length marches, k_corner_ct and
    // the one-kernel hydro stage measured no better than the plain rule (profiles/r01_v14_tail_ab.txt)
    const double resident = 256.0*wgs_per_cu;
    double best = -1.0;
    long best_ml = ml;
    for (long c = (ml < lmax ? lmax : lmax + lmax/4); c >= 4; --c) {
      if (ml < lmax && c > lmax) continue;
      const long nch = (ncells + c - 1)/c;
      const double rounds = (double)(col_blocks*nch*nmb)/resident;
      const double full = rounds <= 1.0 ? 1.0 : rounds/(double)(long)(rounds + 0.999999);
      // below one round the launch is latency-bound: prefer more, shorter chunks up to a round
      const double fill = rounds < 1.0 ? rounds : 1.0;
      const double score = full*fill/(1.0 + 1.0/(double)c);
      if (score > best) { best = score; best_ml = c; }
    }
    ml = best_ml;
  }
  return (int)ml;
}

// ---------------------------------------------------------------------------------------
// face flux from the cell stencil (registers only).  Returns flux in sweep-aligned order.
template <int DIR, int RECON, bool MHD, int RS>
__device__ __forceinline__ void face_flux(const Geo &g, const FaceEos &eos,
    const double *__restrict__ w0, const double *__restrict__ bcc0,
    const double *__restrict__ bxf, int f3, int f2, int f1, int m, int k, int j, int i,
    double &fd, double &fx, double &fy, double &fz, double &fe, double &fby, double &fbz) {
  constexpr int ivx = 1 + DIR, ivy = 1 + (DIR + 1)%3, ivz = 1 + (DIR + 2)%3;
  const long s = (DIR == 0) ? 1 : (DIR == 1 ? (long)g.N1 : (long)g.N1*g.N2);
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  // wave-uniform bases (m comes from blockIdx) + one 32-bit in-variable offset per lane
  const double *q = w0 + (size_t)m*g.nvar*cs;
  const unsigned off = (((unsigned)k*(unsigned)g.N2 + (unsigned)j)*(unsigned)g.N1 + (unsigned)i)*8u;   // bytes
  double ld, lx, ly, lz, le, rd, rx, ry, rz, re;
  // every stencil (and the face field) requested before the first reconstruction: the limiters branch, so with the
  // loads inside face_states_u each variable waited for its own (see sweep_x1_shared)
  constexpr int W = stencil_w<RECON>(), LO = stencil_lo<RECON>();
  constexpr int NVs = MHD ? 7 : 5;
  double sq[NVs][W];
  const double *bq = MHD ? bcc0 + (size_t)m*3*cs : nullptr;
  const double *vb[7] = {q, q + ivx*cs, q + ivy*cs, q + ivz*cs, q + 4*cs,
                         MHD ? bq + ((DIR + 1)%3)*cs : nullptr, MHD ? bq + ((DIR + 2)%3)*cs : nullptr};
#pragma unroll
  for (int n = 0; n < NVs; ++n) {
    if (rs_iso<RS>() && n == 4) continue;
#pragma unroll
    for (int d = 0; d < W; ++d) sq[n][d] = ldu(vb[n] + (long)(d - LO)*s, off);
  }
  [[maybe_unused]] double bxi_g = 0.0;
  if constexpr (MHD) bxi_g = ldu(bxf + (size_t)m*f3*f2*f1,
                                 (((unsigned)k*(unsigned)f2 + (unsigned)j)*(unsigned)f1 + (unsigned)i)*8u);
  __builtin_amdgcn_sched_barrier(0);
  face_states_v<RECON, 1>(sq[0], eos, ld, rd);
  face_states_v<RECON, 0>(sq[1], eos, lx, rx);
  face_states_v<RECON, 0>(sq[2], eos, ly, ry);
  face_states_v<RECON, 0>(sq[3], eos, lz, rz);
  if constexpr (rs_iso<RS>()) { le = re = 0.0; }           // isothermal: no energy variable
  else face_states_v<RECON, 2>(sq[4], eos, le, re);
  if constexpr (MHD) {
    double lby, lbz, rby, rbz;
    face_states_v<RECON, 0>(sq[5], eos, lby, rby);
    face_states_v<RECON, 0>(sq[6], eos, lbz, rbz);
    const double bxi = bxi_g;
    Cons1D fl = riemann_mhd_e<RS>(eos, ld, lx, ly, lz, le, lby, lbz, rd, rx, ry, rz, re, rby, rbz, bxi);
    fd = fl.d; fx = fl.mx; fy = fl.my; fz = fl.mz; fe = fl.e; fby = fl.by; fbz = fl.bz;
  } else {
    riemann_hyd_e<RS>(eos, ld, lx, ly, lz, le, rd, rx, ry, rz, re, fd, fx, fy, fz, fe);
    fby = fbz = 0.0;
  }
}
// ---------------------------------------------------------------------------------------
// The launchers (AKMI_COMPLETE / AKMI_FAIL), by the unit that defines and instantiates them.
// akmi_stage_sweeps.hip
template <int DIR, bool MHD, bool ECC>
int launch_sweep(const Geo &g, const Scheme &sc, const SweepArgs &a, hipStream_t st);
// akmi_stage_march_x2.hip (DIR 0: the 1-D tile kernel, DIR 1), akmi_stage_march_x3.hip (DIR 2)
template <int DIR, bool MHD, int MODE = 0, bool USEACC = false>
int launch_sweep_update(const Geo &g, const Scheme &sc, const SweepArgs &a, const UpdArgs &u, hipStream_t st,
                        bool u0_form = false, bool face_form = false);
// akmi_stage_mhd.hip.  CT of the planes [kA, kB]: the RK weights, the two registers of the face field, copy_b1 as copy_u1
struct CtArgs {
  double gam0, gam1, beta_dt;
  double *b0x1f, *b0x2f, *b0x3f, *b1x1f, *b1x2f, *b1x3f;
  int copy_b1, kA, kB;
  const double *dtp;
};
int launch_sweep12s(const Geo &g, const Scheme &sc, const SweepArgs &a1, const SweepArgs &a2, const UpdArgs &u,
                    hipStream_t st, bool uc = false, bool bf = false, const double *bx3f = nullptr);
// CornerE + CT in one kernel (3-D): efc / ecc the six face and three cell-centred EMFs, mf the three mass fluxes or (mfb)
// the bytes of their signs; launch_ct_copy: CT from the corner EMFs e (1-D / 2-D)
int launch_corner_ct(const Geo &g, double *const *efc, double *const *ecc, bool mfb, const double *const *mf,
                     const CtArgs &c, hipStream_t st);
int launch_ct_copy(const Geo &g, const double *const *e, const CtArgs &c, hipStream_t st);
// (akmi_stage_hydro.hip's launch_hydro_stage3d: akmi_hydro_stage3d2.hpp, beside the types it takes)
// akmi_stage_march_x2.hip: the passive scalars of the planes [k0, k0 + nk)
int launch_scalars(const Geo &g, const Scheme &sc, const double *w0, const double *m1, const double *m2,
                   const double *m3, const UpdArgs &u, int k0, int nk, hipStream_t st);
// akmi_stage_c2p.hip (and fill_fltmax, declared in akmi_c2p.hpp)
template <bool MHD, int DROP = 0>
int launch_c2p(const Geo &g, const Eos &eos, double *u0, const double *bx1f, const double *bx2f, const double *bx3f,
               double *w0, double *bcc0, int do_newdt, int *counters, double *dt3, int il, int iu, int jl, int ju,
               int k0, int nk, hipStream_t st);

}  // namespace akmi
#endif
