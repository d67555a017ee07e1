// akmi_stage.hip -- per-stage fast path of a MeshBlockPack (C ABI: akmi_*_stage_update,
// akmi_*_c2p_newdt).  Results are bit-identical to the task chain of akmi_tasks.hip.
//
// Pass A  (akmi_*_stage_update): flux sweeps with everything memory-bound folded into the
//   VALU-bound Riemann kernels:
//     sweep x1 .. x(D-1): reconstruct + Riemann, write face fluxes (+ face EMFs); the x1 sweep
//                         also emits the cell-centred E = -(v x B) that CornerE needs
//     sweep xD (last)   : reconstruct + Riemann, exchange the normal flux of a tile through
//                         LDS and apply the RK update  u0 = gam0*u0 + gam1*u1 - beta_dt*divF
//                         in the same kernel (stage 1 also stores u1 <- u0: CopyCons folded)
//     corner E + CT     : GS05/07 upwind corner EMFs (select-based, no divergent loads) and the
//                         face-B update in one k-marching kernel in 3-D (stage 1 also stores
//                         b1 <- b0); 1-D/2-D: akmi_mhd_corner_e + k_ct_copy
// Pass B  (akmi_*_c2p_newdt): ConsToPrim over all cells + (last stage) CFL scan in ONE
//   kernel: the three direction maxima of |v|+c_f are reduced per wavefront (DPP shuffles),
//   per workgroup (LDS) and the workgroup's dx/max enters a 64-bit atomicMin.  Division is
//   monotone, so min_cells fl(dx/a) == fl(dx/max_cells a): identical to the reference scan.
//
// This unit holds no kernel: the workspace, the plan of a stage (plan_stage), stage_update and the entry points.  The
// kernels and their launchers live in one unit per family (akmi_stage.hpp lists them).
#include "akmi_stage.hpp"
#include "akmi_hydro_stage3d2.hpp"      // HydTile / hyd_tile, Mass3, HydC2P, launch_hydro_stage3d

using namespace akmi;

namespace akmi {

struct StageWs {
  double *flx1, *flx2, *flx3;
  double *efc[6];
  double *ecc[3];
  double *e1, *e2, *e3;
  double *acc;                    // dF1/dx1 + dF2/dx2 per cell and variable (3-D path)
  size_t total;
};

static StageWs carve(const Geo &g, int is_mhd, void *ws) {
  StageWs w;
  double *p = (double *)ws;
  size_t nmb = g.nmb, nv = g.nvar;
  size_t n1 = nmb*nv*g.N3*g.N2*(g.N1 + 1), n2 = nmb*nv*g.N3*(g.N2 + 1)*g.N1,
         n3 = nmb*nv*(g.N3 + 1)*g.N2*g.N1;
  size_t off = 0;
  auto take = [&](size_t n) { double *r = p ? p + off : nullptr; off += (n + 31) & ~(size_t)31; return r; };
  w.flx1 = take(n1); w.flx2 = take(n2); w.flx3 = take(n3);
  w.acc = take(nmb*nv*g.N3*g.N2*g.N1);
  for (int q = 0; q < 6; ++q) w.efc[q] = nullptr;
  for (int q = 0; q < 3; ++q) w.ecc[q] = nullptr;
  w.e1 = w.e2 = w.e3 = nullptr;
  if (is_mhd) {
    size_t nc = nmb*g.N3*g.N2*g.N1;
    for (int q = 0; q < 6; ++q) w.efc[q] = take(nc);
    for (int q = 0; q < 3; ++q) w.ecc[q] = take(nc);
    if (!g.three_d) {       // 3-D: the corner EMFs never leave k_corner_ct
      w.e1 = take(nmb*(g.N3 + 1)*(g.N2 + 1)*g.N1);
      w.e2 = take(nmb*(g.N3 + 1)*g.N2*(g.N1 + 1));
      w.e3 = take(nmb*g.N3*(g.N2 + 1)*(g.N1 + 1));
    }
  }
  w.total = off*sizeof(double);
  return w;
}

#ifndef AKMI_SMALL_FACE_SWEEPS
#define AKMI_SMALL_FACE_SWEEPS 700000   // task path: packs up to this many cells take thread-per-face x2/x3 sweeps (0: never); the crossover
                                        // measured in round 3 (88^3 = 681 k cells still faster per face, profiles/r03_small_packs.txt); the HOSTS switch
                                        // small MHD packs to the task chain at AKMI_SMALL_PACK_CELLS (include/akmi.h)
#endif

// ---------------------------------------------------------------------------------------
// The flux kernels of the task-granular entry points (akmi_hydro_fluxes / akmi_mhd_fluxes: the path of
// refined meshes and of everything the fused stage does not cover) by the sweeps of the fused stage:
// the x1 sweep with the reconstruction of a cell shared between its two faces, the x2/x3 marches in
// MODE 2.  Same outputs (all five flux components + the two face EMFs per direction, same ranges:
// hydro_fluxes.cpp:95-104, mhd_fluxes.cpp:117-248), same arithmetic per face.
template <bool MHD>
static int sweeps_store_fluxes_t(const akmi_pack *p, int recon, int rsolver, const double *w0,
                                 const double *bcc0, const double *bx1f, const double *bx2f, const double *bx3f,
                                 double *flx1, double *flx2, double *flx3, int fsh, double *e3x1, double *e2x1,
                                 double *e1x2, double *e3x2, double *e2x3, double *e1x3, hipStream_t st) {
  Geo g = make_geo(p);
  if ((size_t)(g.N3 + 1)*(g.N2 + 1)*(g.N1 + 1)*sizeof(double) >= ((size_t)1 << 32)) return -1;   // caller falls back
  const Scheme sc{recon, rsolver, make_face_eos(p), !p->is_ideal};
  SweepArgs a1{w0, bcc0, bx1f, flx1, e3x1, e2x1, nullptr, nullptr, nullptr,
               g.is, g.ie + 1, g.js, g.je, g.ks, g.ke, g.N3, g.N2, g.N1 + fsh};
  SweepArgs a2{w0, bcc0, bx2f, flx2, e1x2, e3x2, nullptr, nullptr, nullptr,
               g.is, g.ie, g.js, g.je + 1, g.ks, g.ke, g.N3, g.N2 + fsh, g.N1};
  SweepArgs a3{w0, bcc0, bx3f, flx3, e2x3, e1x3, nullptr, nullptr, nullptr,
               g.is, g.ie, g.js, g.je, g.ks, g.ke + 1, g.N3 + fsh, g.N2, g.N1};
  if (MHD) {
    if (g.multi_d) { a1.jl = g.js - 1; a1.ju = g.je + 1; }
    if (g.three_d) { a1.kl = g.ks - 1; a1.ku = g.ke + 1; }
    a2.il = g.is - 1; a2.iu = g.ie + 1;
    if (g.three_d) { a2.kl = g.ks - 1; a2.ku = g.ke + 1; }
    a3.il = g.is - 1; a3.iu = g.ie + 1; a3.jl = g.js - 1; a3.ju = g.je + 1;
  }
  const UpdArgs u{};
  int rc = launch_sweep<0, MHD, false>(g, sc, a1, st);
#if AKMI_SMALL_FACE_SWEEPS
  // small packs (the deck-size mesh of BASELINE config 5): a march is a chain of dependent steps per thread and a
  // few hundred workgroups; one thread per face has no chain at all
  static const int tf_env = getenv("AKMI_FACE_SWEEPS") ? atoi(getenv("AKMI_FACE_SWEEPS")) : -1;
  const long ncell = (long)g.nmb*g.nx1*g.nx2*g.nx3;
  // ... and, since the face sweeps run their lanes over the flattened planes (x3: over (j; k; i)), packs of MeshBlocks of up
  // to 96 cells per side at any size: x2 / x3 of 960 blocks of 32^3 (PPM4) 1 712 / 1 641 -> 1 563 / 1 622 us, 64 blocks of
  // 64^3 (PLM) 752 / 720 -> 659 / 655, 8 blocks of 96^3 322 / 314 -> 306 / 285; 8 blocks of 128^3 even (642 / 673 against
  // 664 / 668), one block of 256^3 the marches by 13 % (602 / 583 against 679 / 702) -- profiles/r06_lane_mapping.txt
  const int nmax = g.nx1 > g.nx2 ? (g.nx1 > g.nx3 ? g.nx1 : g.nx3) : (g.nx2 > g.nx3 ? g.nx2 : g.nx3);
  if (g.three_d && (tf_env == 1 || (tf_env != 0 && (ncell <= (long)AKMI_SMALL_FACE_SWEEPS || nmax <= 96)))) {
    if (rc == AKMI_COMPLETE) rc = launch_sweep<1, MHD, false>(g, sc, a2, st);
    if (rc == AKMI_COMPLETE) rc = launch_sweep<2, MHD, false>(g, sc, a3, st);
    return rc;
  }
#endif
  if (rc == AKMI_COMPLETE && g.multi_d) rc = launch_sweep_update<1, MHD, 2, false>(g, sc, a2, u, st);
  if (rc == AKMI_COMPLETE && g.three_d) rc = launch_sweep_update<2, MHD, 2, false>(g, sc, a3, u, st);
  return rc;
}
int sweeps_store_fluxes(const akmi_pack *p, int recon, int rsolver, const double *w0, const double *bcc0,
                        const double *bx1f, const double *bx2f, const double *bx3f, double *flx1, double *flx2,
                        double *flx3, int face_shaped, double *e3x1, double *e2x1, double *e1x2, double *e3x2,
                        double *e2x3, double *e1x3, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (bcc0)
    return sweeps_store_fluxes_t<true>(p, recon, rsolver, w0, bcc0, bx1f, bx2f, bx3f, flx1, flx2, flx3, 1,
                                       e3x1, e2x1, e1x2, e3x2, e2x3, e1x3, st);
  return sweeps_store_fluxes_t<false>(p, recon, rsolver, w0, nullptr, nullptr, nullptr, nullptr, flx1, flx2,
                                      flx3, face_shaped ? 1 : 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, st);
}

// forms (AKMI_FORM_*) of the last stage call of this thread that ran sweeps: akmi_stage_last_forms
static thread_local int last_forms = 0;

// ---------------------------------------------------------------------------------------
// Which kernels a stage runs: a function of the pack, the scheme and the environment switches alone.  The phases of a
// split stage arrive in separate calls and must agree, and the hosts size their arrays at construction from the two
// eligibility answers (akmi_mhd_u0_sweeps_eligible, akmi_hydro_stage_w_eligible) -- everything that asks, asks plan_stage.
enum class Sweeps {
  LowDim,       // 1-D / 2-D: plain sweep (+ x2 march)
  HydroOne,     // hydro DC / PLM: k_hydro_stage3d2
  Sweep12sX3,   // MHD PLM + HLLD, ideal gas: k_sweep12s + x3 march (the sequence that knows copy_u1 == 3 and the u0 forms)
  Generic       // x1 sweep + x2 / x3 marches
};
struct StagePlan {
  Sweeps sweeps;
  HydTile tile;         // HydroOne: the tile of k_hydro_stage3d2
  bool mf_bytes;        // the mass-flux signs travel as bytes (k_corner_ct<true>)
  bool c2p_inside;      // HydroOne may convert the cells it finishes (k_hydro_stage3d2<.., C2P>): ideal gas, no passive scalars
};
static StagePlan plan_stage(bool mhd, const Geo &g, const Scheme &sc) {
  // the A/B switches, read once per process (tile and chunk overrides stay with their tile functions)
  static const auto on = [](const char *e, bool dflt) { return e ? atoi(e) != 0 : dflt; };
  static const bool hydro_one = on(getenv("AKMI_HYDRO_ONE_KERNEL"), true);   // 0: the generic sequence also for hydro DC / PLM
  static const bool fuse_c2p = on(getenv("AKMI_FUSE_C2P"), true);            // 0: ConsToPrim as a pass of its own
  StagePlan pl{Sweeps::Generic, HydTile{0, 0, 0, 0, 0}, false, false};
  if (!g.three_d) {
    pl.sweeps = Sweeps::LowDim;
  } else if (!mhd) {
    if (hydro_one && sc.recon <= 1) pl.tile = hyd_tile(g.nx1, g.nx2);
    if (pl.tile.tw > 0) pl.sweeps = Sweeps::HydroOne;
    pl.c2p_inside = pl.tile.tw > 0 && fuse_c2p && !sc.iso && g.nvar == 5;
  } else {
    if (sc.recon == 1 && !sc.iso && sc.rsolver == AKMI_RS_HLLD && g.nvar == 5) pl.sweeps = Sweeps::Sweep12sX3;
    // bytes where k_corner_ct is the only reader of the mass fluxes: no passive scalars (k_scalar_update reads doubles)
    pl.mf_bytes = AKMI_MF_BYTES && g.nvar == (sc.iso ? 4 : 5);
  }
  return pl;
}

// One stage call: what every entry point has, in the order in which the C ABI passes it, through the constructor; every
// other field has a default, and an entry point sets what it has.
struct StageCall {
  StageCall(const akmi_pack *p_, int recon_, int rsolver_, double gam0_, double gam1_, double beta_dt_, int copy_arg_,
            void *ws_, void *stream)
      : p(p_), recon(recon_), rsolver(rsolver_), gam0(gam0_), gam1(gam1_), beta_dt(beta_dt_), copy_arg(copy_arg_), ws(ws_),
        st((hipStream_t)stream) {}
  const akmi_pack *p;
  int recon, rsolver;
  double gam0, gam1, beta_dt;                         // RK weights
  int copy_arg;                                       // copy_u1 | AKMI_COPY_* form flags
  void *ws;
  hipStream_t st;
  const double *dt_dev = nullptr;                     // set: beta_dt is the weight beta, the kernels multiply it with *dt_dev
  int phases = AKMI_PHASE_ALL;
  const double *w0 = nullptr, *bcc0 = nullptr;        // (ConsToPrim of the active cells writes them)
  double *u0 = nullptr, *u1 = nullptr;
  double *b0x1f = nullptr, *b0x2f = nullptr, *b0x3f = nullptr, *b1x1f = nullptr, *b1x2f = nullptr, *b1x3f = nullptr;
  int c2p = 0, do_newdt = 0, *counters = nullptr;     // ConsToPrim of the active cells (+ CFL scan) at the end of the call
  double *dt3 = nullptr;
  double *w_out = nullptr;                            // hydro: where a stage kernel that converts its cells puts the new
  int *wrote_new = nullptr;                           // primitives; *wrote_new = 1 when it did
};

// Pass A (+ optionally the interior part of pass B) of one stage, in stream order: the Riemann sweeps with the RK update,
// CornerE + CT, ConsToPrim of the active cells.  `phases` selects the parts, so that a rank with off-rank neighbours can
// post its halo messages in between.
template <bool MHD>
static int stage_update(const StageCall &c) {
  const akmi_pack *p = c.p;
  hipStream_t st = c.st;
  if (c.phases <= 0 || c.phases > AKMI_PHASE_ALL) { set_error("stage_phase: bad phase mask"); return AKMI_FAIL; }
  if (check_scheme(p, c.recon, "stage") != AKMI_COMPLETE) return AKMI_FAIL;
  const int copy_arg = c.copy_arg, copy_u1 = copy_arg & AKMI_COPY_MASK;
  const bool want_x3_u0 = (copy_arg & AKMI_COPY_X3_U0) != 0;
  const bool want_x12_u0 = (copy_arg & AKMI_COPY_X12_U0) != 0, want_bf = (copy_arg & AKMI_COPY_BCC_FACES) != 0;
  constexpr int form_flags = AKMI_COPY_X3_U0 | AKMI_COPY_X12_U0 | AKMI_COPY_BCC_FACES;
  if (copy_u1 > 3 || (copy_arg & ~(AKMI_COPY_MASK | form_flags))) { set_error("stage: bad copy_u1 = %d", copy_arg); return AKMI_FAIL; }
  if ((want_x12_u0 || want_bf) && !want_x3_u0) {
    set_error("stage: AKMI_COPY_X12_U0 / AKMI_COPY_BCC_FACES come on top of AKMI_COPY_X3_U0");
    return AKMI_FAIL;
  }
  if (want_x3_u0 && copy_u1 < 2) {
    set_error("stage: the u0 form of the x3 march needs a stage that does not write the array it reads (copy_u1 2 or 3)");
    return AKMI_FAIL;
  }
  // phases: a caller that exchanges halos between the parts of a stage (multi-rank runs) asks
  // for them one at a time; the parts communicate through u0/b0 and the workspace only
  const bool do_sweeps = (c.phases & AKMI_PHASE_SWEEPS) != 0;
  const bool do_emf = MHD && (c.phases & AKMI_PHASE_EMF_CT) != 0;
  const bool do_c2p = c.c2p && (c.phases & AKMI_PHASE_C2P) != 0;
  const Geo g = make_geo(p);
  const Eos eos = make_eos(p);
  const Scheme sc{c.recon, c.rsolver, make_face_eos(p), !p->is_ideal};
  const StagePlan plan = plan_stage(MHD, g, sc);
  if ((copy_u1 == 3 || want_x3_u0) && do_sweeps && plan.sweeps != Sweeps::Sweep12sX3) {
    set_error("stage: copy_u1 = 3 and the form flags AKMI_COPY_X3_U0 / _X12_U0 / _BCC_FACES exist for the k_sweep12s + x3 march "
              "sequence only (MHD, 3-D, PLM + HLLD, ideal gas)");
    return AKMI_FAIL;
  }
  if (do_sweeps) last_forms = 0;
  // the sweeps address one variable of one MeshBlock with a 32-bit byte offset per lane
  if ((size_t)(g.N3 + 1)*(g.N2 + 1)*(g.N1 + 1)*sizeof(double) >= ((size_t)1 << 32)) {
    set_error("stage: a MeshBlock of %d x %d x %d cells (with ghosts) exceeds 4 GB per variable; use smaller "
              "MeshBlocks", g.N1, g.N2, g.N3);
    return AKMI_FAIL;
  }
  StageWs w = carve(g, MHD ? 1 : 0, c.ws);
  UpdArgs u{c.gam0, c.gam1, c.beta_dt, c.u0, c.u1, w.flx1, w.flx2, copy_u1, w.acc, c.dt_dev};
  // copy_u1 == 2 (out-of-place first stage): the new state lands in u1 / b1, which is what the c2p
  // of the active cells has to read
  double *un = copy_u1 >= 2 ? c.u1 : c.u0;
  const double *n1f = copy_u1 == 2 ? c.b1x1f : c.b0x1f, *n2f = copy_u1 == 2 ? c.b1x2f : c.b0x2f,
               *n3f = copy_u1 == 2 ? c.b1x3f : c.b0x3f;
  int rc = AKMI_COMPLETE;
  // sweep ranges: hydro_fluxes.cpp:95-104 (no FOFC) / mhd_fluxes.cpp:117-248 (CT-extended)
  SweepArgs a1{c.w0, c.bcc0, c.b0x1f, w.flx1, w.efc[0], w.efc[1], w.ecc[0], w.ecc[1], w.ecc[2],
               g.is, g.ie + 1, g.js, g.je, g.ks, g.ke, g.N3, g.N2, g.N1 + 1};
  SweepArgs a2{c.w0, c.bcc0, c.b0x2f, w.flx2, w.efc[2], w.efc[3], nullptr, nullptr, nullptr,
               g.is, g.ie, g.js, g.je + 1, g.ks, g.ke, g.N3, g.N2 + 1, g.N1};
  SweepArgs a3{c.w0, c.bcc0, c.b0x3f, w.flx3, w.efc[4], w.efc[5], nullptr, nullptr, nullptr,
               g.is, g.ie, g.js, g.je, g.ks, g.ke + 1, g.N3 + 1, g.N2, g.N1};
  if (MHD) {
    if (g.multi_d) { a1.jl = g.js - 1; a1.ju = g.je + 1; }
    if (g.three_d) { a1.kl = g.ks - 1; a1.ku = g.ke + 1; }
    a2.il = g.is - 1; a2.iu = g.ie + 1;
    if (g.three_d) { a2.kl = g.ks - 1; a2.ku = g.ke + 1; }
    a3.il = g.is - 1; a3.iu = g.ie + 1; a3.jl = g.js - 1; a3.ju = g.je + 1;
  }
  if (do_c2p && c.do_newdt == 1) fill_fltmax(c.dt3, 3, st);       // 2: the caller has reset the minima
  bool c2p_done = false;              // ConsToPrim of the active cells happened inside the sweeps' kernel
  // the bytes of the mass-flux signs: k_sweep12s writes no x1 flux, so they take its place; the generic x1 sweep fills flx1
  // with the five fluxes the x2 march reads, and its bytes go behind those of x2 in the region of flx2, of which only
  // variable 0 is used.
  if (plan.mf_bytes) {
    const size_t nb2 = ((size_t)g.nmb*g.N3*(g.N2 + 1)*g.N1 + 255) & ~(size_t)255;
    a2.mfb = reinterpret_cast<unsigned char *>(w.flx2);
    a1.mfb = plan.sweeps == Sweeps::Sweep12sX3 ? reinterpret_cast<unsigned char *>(w.flx1) : a2.mfb + nb2;
    a3.mfb = reinterpret_cast<unsigned char *>(w.flx3);
  }

  // ---- the VALU-bound sweeps, then the HBM-bound CornerE + CT and ConsToPrim, in stream order.
  // (Cutting the block into k-slabs and running the two groups on two streams one slab apart was built in round 1 and
  //  measured slower at every slab thickness in rounds 1 and 3 -- profiles/r03_slab_ab.txt; it left the source in round 5.)
  const int kA = g.ks, kB = g.ke;
  if (!do_sweeps) {
  } else if (plan.sweeps == Sweeps::LowDim && !g.multi_d) {
    rc = launch_sweep_update<0, MHD>(g, sc, a1, u, st);
  } else if (plan.sweeps == Sweeps::LowDim) {
    // 2-D (and 1-D above): small problems, plain sequence
    rc = MHD ? launch_sweep<0, MHD, MHD>(g, sc, a1, st)
             : launch_sweep<0, MHD, false>(g, sc, a1, st);
    if (rc == AKMI_COMPLETE) rc = launch_sweep_update<1, MHD>(g, sc, a2, u, st);
  } else if (plan.sweeps == Sweeps::HydroOne) {
    // hydro DC/PLM: sweeps + update in one kernel
    if constexpr (!MHD) {
      if (c.w_out && do_c2p && plan.c2p_inside) {
        // (the floor flags of the cells, one byte each, at the start of the workspace: akmi_hydro_ghost_uw reads them there)
        const HydC2P hc{reinterpret_cast<unsigned char *>(c.ws), c.w_out, eos, c.do_newdt, c.counters, c.dt3};
        rc = launch_hydro_stage3d<false>(g, sc, plan.tile, c.w0, u, kA, kB, st, Mass3{nullptr, nullptr, nullptr}, &hc);
        c2p_done = true;
        if (c.wrote_new) *c.wrote_new = 1;
      } else if (g.nvar > (sc.iso ? 4 : 5)) {
        rc = launch_hydro_stage3d<true>(g, sc, plan.tile, c.w0, u, kA, kB, st, Mass3{w.flx1, w.flx2, w.flx3});
      } else {
        rc = launch_hydro_stage3d<false>(g, sc, plan.tile, c.w0, u, kA, kB, st, Mass3{nullptr, nullptr, nullptr});
      }
    }
  } else if (plan.sweeps == Sweeps::Sweep12sX3) {
    // x1 sweep inside the x2 march, cells from the march's window (k_sweep12s); x3 march consumes acc
    // (the other order -- x3 march first, leaving dF3/dx3, k_sweep12s finishing the update -- was built and measured in
    //  round 4: x3 march 891 -> 602 us, k_sweep12s 1130 -> 1374 us, +1 % on the bench; profiles/r04_x3first.txt)
    if (want_bf) { a3.bt1 = c.b0x1f; a3.bt2 = c.b0x2f; }
    if constexpr (MHD) rc = launch_sweep12s(g, sc, a1, a2, u, st, want_x12_u0, want_bf, c.b0x3f);
    if (rc == AKMI_COMPLETE) rc = launch_sweep_update<2, MHD, 0, true>(g, sc, a3, u, st, want_x3_u0, want_bf);
    if (rc == AKMI_COMPLETE && want_x3_u0) last_forms |= AKMI_FORM_X3_U0;
    if (rc == AKMI_COMPLETE && want_x12_u0) last_forms |= AKMI_FORM_X12_U0;
    if (rc == AKMI_COMPLETE && want_bf) last_forms |= AKMI_FORM_BCC_FACES;
  } else {
    rc = MHD ? launch_sweep<0, MHD, MHD>(g, sc, a1, st)
             : launch_sweep<0, MHD, false>(g, sc, a1, st);
    // x2 sweep as a march along j that leaves acc = dF1/dx1 + dF2/dx2; x3 march consumes it
    if (rc == AKMI_COMPLETE) rc = launch_sweep_update<1, MHD, 1, false>(g, sc, a2, u, st);
    if (rc == AKMI_COMPLETE) rc = launch_sweep_update<2, MHD, 0, true>(g, sc, a3, u, st);
  }
  if (rc == AKMI_COMPLETE && do_sweeps && g.nvar > (sc.iso ? 4 : 5))
    rc = launch_scalars(g, sc, c.w0, w.flx1, w.flx2, w.flx3, u, kA, kB - kA + 1, st);
  if (rc != AKMI_COMPLETE) return rc;
  // (k_corner_ct updates the face field in place on a last stage out of place: copy_b1 == 0 for copy_u1 == 3)
  const CtArgs ct{c.gam0, c.gam1, c.beta_dt, c.b0x1f, c.b0x2f, c.b0x3f, c.b1x1f, c.b1x2f, c.b1x3f,
                  plan.sweeps != Sweeps::LowDim && copy_u1 == 3 ? 0 : copy_u1, kA, kB, c.dt_dev};
  if (do_emf && plan.sweeps == Sweeps::LowDim) {
    rc = akmi_mhd_corner_e(p, c.w0, c.bcc0, w.efc[0], w.efc[1], w.efc[2], w.efc[3], w.efc[4], w.efc[5],
                           w.flx1, w.flx2, w.flx3, w.e1, w.e2, w.e3, st);
    if (rc != AKMI_COMPLETE) return rc;
    const double *e[3] = {w.e1, w.e2, w.e3};
    rc = launch_ct_copy(g, e, ct, st);
    if (rc != AKMI_COMPLETE) return rc;
  } else if (do_emf) {
    // CornerE + CT in one kernel
    const bool mfb = plan.mf_bytes;
    const double *mf[3] = {mfb ? reinterpret_cast<const double *>(a1.mfb) : w.flx1,
                           mfb ? reinterpret_cast<const double *>(a2.mfb) : w.flx2,
                           mfb ? reinterpret_cast<const double *>(a3.mfb) : w.flx3};
    rc = launch_corner_ct(g, w.efc, w.ecc, mfb, mf, ct, st);
    if (rc != AKMI_COMPLETE) return rc;
  }
  if (do_c2p && !c2p_done)
    rc = launch_c2p<MHD>(g, eos, un, n1f, n2f, n3f, const_cast<double *>(c.w0),
                         const_cast<double *>(c.bcc0), c.do_newdt, c.counters, c.dt3, g.is, g.ie,
                         g.js, g.je, kA, kB - kA + 1, st);
  return rc;
}

}  // namespace akmi

extern "C" {

const char *akmi_build_flags(void) { return "production"; }

long long akmi_stage_workspace_bytes(const akmi_pack *p, int is_mhd) {
  Geo g = make_geo(p);
  return (long long)carve(g, is_mhd, nullptr).total;
}

int akmi_hydro_stage_update(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                            double beta_dt, int copy_u1, const double *w0, double *u0, double *u1,
                            void *ws, void *stream) {
  StageCall c(p, recon, rsolver, gam0, gam1, beta_dt, copy_u1, ws, stream);
  c.w0 = w0; c.u0 = u0; c.u1 = u1;
  return stage_update<false>(c);
}

int akmi_mhd_stage_update(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                          double beta_dt, int copy_u1, const double *w0, const double *bcc0,
                          double *u0, double *u1, double *b0x1f, double *b0x2f, double *b0x3f,
                          double *b1x1f, double *b1x2f, double *b1x3f, void *ws, void *stream) {
  StageCall c(p, recon, rsolver, gam0, gam1, beta_dt, copy_u1, ws, stream);
  c.w0 = w0; c.bcc0 = bcc0; c.u0 = u0; c.u1 = u1;
  c.b0x1f = b0x1f; c.b0x2f = b0x2f; c.b0x3f = b0x3f; c.b1x1f = b1x1f; c.b1x2f = b1x2f; c.b1x3f = b1x3f;
  return stage_update<true>(c);
}


int akmi_hydro_stage_fused(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                           double beta_dt, int copy_u1, double *w0, double *u0, double *u1,
                           int do_newdt, int *counters, double *dt3, void *ws, void *stream) {
  StageCall c(p, recon, rsolver, gam0, gam1, beta_dt, copy_u1, ws, stream);
  c.w0 = w0; c.u0 = u0; c.u1 = u1;
  c.c2p = 1; c.do_newdt = do_newdt; c.counters = counters; c.dt3 = dt3;
  return stage_update<false>(c);
}

int akmi_hydro_stage_fused_dt(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                              double beta, const double *dt_dev, int copy_u1, double *w0, double *u0,
                              double *u1, int do_newdt, int *counters, double *dt3, void *ws, void *stream) {
  StageCall c(p, recon, rsolver, gam0, gam1, beta, copy_u1, ws, stream);
  c.dt_dev = dt_dev; c.w0 = w0; c.u0 = u0; c.u1 = u1;
  c.c2p = 1; c.do_newdt = do_newdt; c.counters = counters; c.dt3 = dt3;
  return stage_update<false>(c);
}

int akmi_mhd_stage_fused_dt(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                            double beta, const double *dt_dev, int copy_u1, double *w0, double *bcc0,
                            double *u0, double *u1, double *b0x1f, double *b0x2f, double *b0x3f,
                            double *b1x1f, double *b1x2f, double *b1x3f, int do_newdt, int *counters,
                            double *dt3, void *ws, void *stream) {
  StageCall c(p, recon, rsolver, gam0, gam1, beta, copy_u1, ws, stream);
  c.dt_dev = dt_dev; c.w0 = w0; c.bcc0 = bcc0; c.u0 = u0; c.u1 = u1;
  c.b0x1f = b0x1f; c.b0x2f = b0x2f; c.b0x3f = b0x3f; c.b1x1f = b1x1f; c.b1x2f = b1x2f; c.b1x3f = b1x3f;
  c.c2p = 1; c.do_newdt = do_newdt; c.counters = counters; c.dt3 = dt3;
  return stage_update<true>(c);
}

int akmi_mhd_stage_fused(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                         double beta_dt, int copy_u1, double *w0, double *bcc0, double *u0, double *u1,
                         double *b0x1f, double *b0x2f, double *b0x3f, double *b1x1f, double *b1x2f,
                         double *b1x3f, int do_newdt, int *counters, double *dt3, void *ws,
                         void *stream) {
  StageCall c(p, recon, rsolver, gam0, gam1, beta_dt, copy_u1, ws, stream);
  c.w0 = w0; c.bcc0 = bcc0; c.u0 = u0; c.u1 = u1;
  c.b0x1f = b0x1f; c.b0x2f = b0x2f; c.b0x3f = b0x3f; c.b1x1f = b1x1f; c.b1x2f = b1x2f; c.b1x3f = b1x3f;
  c.c2p = 1; c.do_newdt = do_newdt; c.counters = counters; c.dt3 = dt3;
  return stage_update<true>(c);
}

int akmi_hydro_stage_phase(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                           double beta_dt, int copy_u1, double *w0, double *u0, double *u1,
                           int do_newdt, int *counters, double *dt3, int phases, void *ws,
                           void *stream) {
  StageCall c(p, recon, rsolver, gam0, gam1, beta_dt, copy_u1, ws, stream);
  c.phases = phases; c.w0 = w0; c.u0 = u0; c.u1 = u1;
  c.c2p = 1; c.do_newdt = do_newdt; c.counters = counters; c.dt3 = dt3;
  return stage_update<false>(c);
}

int akmi_mhd_stage_phase(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                         double beta_dt, int copy_u1, double *w0, double *bcc0, double *u0, double *u1,
                         double *b0x1f, double *b0x2f, double *b0x3f, double *b1x1f, double *b1x2f,
                         double *b1x3f, int do_newdt, int *counters, double *dt3, int phases,
                         void *ws, void *stream) {
  StageCall c(p, recon, rsolver, gam0, gam1, beta_dt, copy_u1, ws, stream);
  c.phases = phases; c.w0 = w0; c.bcc0 = bcc0; c.u0 = u0; c.u1 = u1;
  c.b0x1f = b0x1f; c.b0x2f = b0x2f; c.b0x3f = b0x3f; c.b1x1f = b1x1f; c.b1x2f = b1x2f; c.b1x3f = b1x3f;
  c.c2p = 1; c.do_newdt = do_newdt; c.counters = counters; c.dt3 = dt3;
  return stage_update<true>(c);
}

int akmi_hydro_stage_phase_dt(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1, double beta,
                              const double *dt_dev, int copy_u1, double *w0, double *u0, double *u1, int do_newdt,
                              int *counters, double *dt3, int phases, void *ws, void *stream) {
  StageCall c(p, recon, rsolver, gam0, gam1, beta, copy_u1, ws, stream);
  c.dt_dev = dt_dev; c.phases = phases; c.w0 = w0; c.u0 = u0; c.u1 = u1;
  c.c2p = 1; c.do_newdt = do_newdt; c.counters = counters; c.dt3 = dt3;
  return stage_update<false>(c);
}

int akmi_mhd_stage_phase_dt(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1, double beta,
                            const double *dt_dev, int copy_u1, double *w0, double *bcc0, double *u0, double *u1,
                            double *b0x1f, double *b0x2f, double *b0x3f, double *b1x1f, double *b1x2f, double *b1x3f,
                            int do_newdt, int *counters, double *dt3, int phases, void *ws, void *stream) {
  StageCall c(p, recon, rsolver, gam0, gam1, beta, copy_u1, ws, stream);
  c.dt_dev = dt_dev; c.phases = phases; c.w0 = w0; c.bcc0 = bcc0; c.u0 = u0; c.u1 = u1;
  c.b0x1f = b0x1f; c.b0x2f = b0x2f; c.b0x3f = b0x3f; c.b1x1f = b1x1f; c.b1x2f = b1x2f; c.b1x3f = b1x3f;
  c.c2p = 1; c.do_newdt = do_newdt; c.counters = counters; c.dt3 = dt3;
  return stage_update<true>(c);
}

int akmi_stage_last_forms(void) { return last_forms; }

// the stage takes k_sweep12s + the x3 march: the sequence that knows copy_u1 == 3 and the u0 forms
int akmi_mhd_u0_sweeps_eligible(const akmi_pack *p, int recon, int rsolver) {
  const Scheme sc{recon, rsolver, make_face_eos(p), !p->is_ideal};
  return plan_stage(true, make_geo(p), sc).sweeps == Sweeps::Sweep12sX3 ? 1 : 0;
}

// akmi_hydro_stage_w converts the cells it finishes (wrote_new = 1 when the caller asks for ConsToPrim)
int akmi_hydro_stage_w_eligible(const akmi_pack *p, int recon, int rsolver) {
  const Scheme sc{recon, rsolver, make_face_eos(p), !p->is_ideal};
  return (rsolver == AKMI_RS_LLF || rsolver == AKMI_RS_HLLE || rsolver == AKMI_RS_HLLC || rsolver == AKMI_RS_ROE) &&
         plan_stage(false, make_geo(p), sc).c2p_inside ? 1 : 0;
}

int akmi_hydro_stage_w(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1, double beta,
                       const double *dt_dev, int copy_u1, double *w0, double *w0_new, double *u0, double *u1,
                       int do_newdt, int *counters, double *dt3, void *ws, void *stream, int *wrote_new) {
  if (wrote_new) *wrote_new = 0;
  StageCall c(p, recon, rsolver, gam0, gam1, beta, copy_u1, ws, stream);
  c.dt_dev = dt_dev; c.w0 = w0; c.u0 = u0; c.u1 = u1;
  c.c2p = 1; c.do_newdt = do_newdt; c.counters = counters; c.dt3 = dt3;
  c.w_out = w0_new; c.wrote_new = wrote_new;
  return stage_update<false>(c);
}


}  // extern "C"
