/* akmi.h -- C ABI of the MI355X-native MeshBlock finite-volume update (AthenaK hot path).
 *
 * AthenaK has no FFI layer; the seam this library replaces is the *task member function*
 *     TaskStatus (Hydro|MHD)::Name(Driver *pdriver, int stage)
 * (reference: src/tasklist/task_list.hpp:178-185, src/hydro/hydro.hpp:124-154,
 * src/mhd/mhd.hpp:155-199).  Each entry point below is the body of one such task, taking
 * what the task reads from pmy_pack as plain pointers and scalars.  See INTEGRATION.md for
 * the one-line binding a maintainer adds inside each reference task.
 *
 * Conventions
 *  - All field pointers are DEVICE pointers (HBM) to IEEE fp64 in the reference's
 *    LayoutRight order (src/athena.hpp:111,127-128):
 *        cell array   (nmb, nvar, N3, N2, N1)            i fastest, no padding
 *        x1-face      (nmb, [nvar,] N3,   N2,   N1+1)    (src/athena.hpp:178-196)
 *        x2-face      (nmb, [nvar,] N3,   N2+1, N1  )
 *        x3-face      (nmb, [nvar,] N3+1, N2,   N1  )
 *        x1-edge      (nmb, N3+1, N2+1, N1  )            (src/athena.hpp:223-231)
 *        x2-edge      (nmb, N3+1, N2,   N1+1)
 *        x3-edge      (nmb, N3,   N2+1, N1+1)
 *    with N1 = nx1+2*ng, N2 = nx2>1 ? nx2+2*ng : 1, N3 likewise
 *    (src/hydro/hydro.cpp:283-288, src/mhd/mhd.cpp:148-160).
 *  - The library never allocates, frees or reallocates a caller's array.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls enqueue
 *    work and return; only functions documented as synchronous block.
 *  - Return value mirrors TaskStatus (src/tasklist/task_list.hpp:30):
 *        AKMI_COMPLETE 0, AKMI_INCOMPLETE 1, AKMI_FAIL <0 (message via akmi_last_error()).
 */
#ifndef AKMI_H_
#define AKMI_H_

#ifdef __cplusplus
extern "C" {
#endif

#define AKMI_COMPLETE    0
#define AKMI_INCOMPLETE  1
#define AKMI_FAIL       -1

/* variable indices, src/athena.hpp:65-67 */
enum { AKMI_IDN = 0, AKMI_IM1 = 1, AKMI_IM2 = 2, AKMI_IM3 = 3, AKMI_IEN = 4 };
enum { AKMI_IBX = 0, AKMI_IBY = 1, AKMI_IBZ = 2 };

/* ReconstructionMethod, src/athena.hpp (enum class) ; only dc/plm/ppm4 are on the path */
enum { AKMI_RECON_DC = 0, AKMI_RECON_PLM = 1, AKMI_RECON_PPM4 = 2, AKMI_RECON_PPMX = 3,
       AKMI_RECON_WENOZ = 4, AKMI_RECON_TENO = 5 };
/* Hydro_RSolver / MHD_RSolver */
enum { AKMI_RS_LLF = 0, AKMI_RS_HLLE = 1, AKMI_RS_HLLC = 2, AKMI_RS_HLLD = 3, AKMI_RS_ROE = 4,
       AKMI_RS_ADVECT = 5 /* kinematic runs (<time>/evolution = kinematic), task-granular entries only */ };
/* BoundaryFlag, src/mesh/mesh.hpp */
enum { AKMI_BC_BLOCK = -1, AKMI_BC_PERIODIC = 0, AKMI_BC_OUTFLOW = 1, AKMI_BC_REFLECT = 2,
       AKMI_BC_USER = 3 /* left to the caller's user function */, AKMI_BC_INFLOW = 4, AKMI_BC_DIODE = 5,
       AKMI_BC_VACUUM = 6 };

/* MeshBlockPack descriptor: RegionIndcs (src/mesh/mesh.hpp:35-41), mb_size.dx1..3
 * (src/mesh/mesh.hpp:25-29) and EOS_Data (src/eos/eos.hpp:27-34) by value. */
typedef struct akmi_pack {
  int nmb;               /* nmb_thispack: MeshBlocks looped over                        */
  int nvar;              /* nhydro|nmhd (+ nscalars): 5 ideal gas, 4 isothermal         */
  int nx1, nx2, nx3;     /* active cells per MeshBlock                                  */
  int ng;                /* ghost cells                                                 */
  const double *dx;      /* [nmb][3] dx1,dx2,dx3 per block, same memory space as fields */
  double gamma;          /* EOS_Data::gamma (ideal gas)                                 */
  double dfloor, pfloor, tfloor, sfloor;   /* default FLT_MIN, src/eos/eos.cpp:22-25    */
  double sigma_max;      /* default FLT_MAX, src/eos/ideal_mhd.cpp:22                   */
  double iso_cs;         /* EOS_Data::iso_cs (isothermal sound speed)                   */
  int is_ideal;          /* EOS_Data::is_ideal: 1 ideal gas (nvar 5), 0 isothermal (nvar 4:
                          * no energy variable, src/eos/isothermal_hyd.cpp:20-23)        */
} akmi_pack;

/* MHD packs of up to this many cells count as "small": both hosts run the task-granular chain instead of the fused stage
 * for such 3-D packs (unless the deck sets mhd/fused_stage itself or small_pack_tasks = false) -- measured crossover 72^3
 * (64^3: chain 1 113 against 1 042 Mcell-updates/s, 80^3: 1 392 against 1 494; PPM4 the same).  Hydro packs always take the
 * fused stage: its one-kernel form wins at every size (64^3: 2 838 against 1 854, 32^3: 485 against 303).  INTEGRATION.md. */
#define AKMI_SMALL_PACK_CELLS 375000

const char *akmi_last_error(void);
int akmi_version(void);
/* "production", or "experiments: ..." for a library built with -DAKMI_EXPERIMENTS (timing experiments that change
 * results; __graft_entry__.build() never defines it and tests/test_capi_symbols.py refuses such a library) */
const char *akmi_build_flags(void);

/* ---- Hydro tasks ------------------------------------------------------------------ */
/* Hydro::CopyCons (src/hydro/hydro_tasks.cpp:130-152): u1 <- u0 */
int akmi_copy_cons(const akmi_pack *p, const double *u0, double *u1, void *stream);
/* Hydro::Fluxes with <hydro>/fofc = true (src/hydro/hydro_fluxes.cpp:92-101): the same fluxes over
 * ranges extended by one face / one transverse cell, as Hydro::FOFC needs them */
int akmi_hydro_fluxes_fofc(const akmi_pack *p, int recon, int rsolver, const double *w0,
                           double *flx1, double *flx2, double *flx3, int face_shaped, void *stream);
/* Hydro::FOFC (src/hydro/hydro_fofc.cpp:30-371, Newtonian): trial update of the cells
 * [is-1,ie+1] x [js-1,je+1] x [ks-1,ke+1], flag those whose conversion to primitives would need a
 * floor (ConsToPrim(..., only_testfloors=true), src/eos/ideal_hyd.cpp:67-72), replace the fluxes on
 * the faces of flagged cells by first-order LLF fluxes (SingleStateLLF_Hyd), reset the flags.
 * fofc = Hydro::fofc as unsigned char [nmb][N3][N2][N1], zero on entry and on exit (caller-owned);
 * nfofc = device int, incremented by the number of flagged cells (EventCounters::nfofc). */
int akmi_hydro_fofc(const akmi_pack *p, double gam0, double gam1, double beta_dt, const double *w0,
                    const double *u0, const double *u1, double *flx1, double *flx2, double *flx3,
                    int face_shaped, unsigned char *fofc, int *nfofc, void *stream);
/* MHD::Fluxes with <mhd>/fofc = true (src/mhd/mhd_fluxes.cpp:100-105): face-normal ranges extended
 * by one face on both sides (ideal gas, no scalars) */
int akmi_mhd_fluxes_fofc(const akmi_pack *p, int recon, int rsolver, const double *w0,
                         const double *bcc0, const double *bx1f, const double *bx2f,
                         const double *bx3f, double *flx1, double *flx2, double *flx3, double *e3x1,
                         double *e2x1, double *e1x2, double *e3x2, double *e2x3, double *e1x3,
                         void *stream);
/* MHD::FOFC (src/mhd/mhd_fofc.cpp:30-493, Newtonian ideal gas): as akmi_hydro_fofc, with the trial
 * cell-centred field bcctest = gam0*bcc0 + gam1*avg(b1) -/+ dt/dx * d(face EMFs) (:88-107) in the
 * floor test, and the face EMFs of flagged cells replaced together with the fluxes. */
int akmi_mhd_fofc(const akmi_pack *p, double gam0, double gam1, double beta_dt, const double *w0,
                  const double *bcc0, const double *b0x1f, const double *b0x2f, const double *b0x3f,
                  const double *b1x1f, const double *b1x2f, const double *b1x3f, const double *u0,
                  const double *u1, double *flx1, double *flx2, double *flx3, double *e3x1,
                  double *e2x1, double *e1x2, double *e3x2, double *e2x3, double *e1x3,
                  unsigned char *fofc, int *nfofc, void *stream);
/* Hydro::NewTimeStep / MHD::NewTimeStep with <time>/evolution = kinematic (src/hydro/hydro_newdt.cpp:55-72,
 * src/mhd/mhd_newdt.cpp:56-73): dt3[d] = min over the active cells of dx_d/|v_d| */
int akmi_kinematic_newdt(const akmi_pack *p, const double *w0, double *dt3, void *stream);

/* ---- diffusion hooks of the Fluxes / EField tasks (src/hydro/hydro_tasks.cpp:183-189,
 * src/mhd/mhd_tasks.cpp:198-206,381-383); constant coefficients ---------------------------- */
/* Viscosity::AddViscousFluxIso (src/diffusion/viscosity.cpp:64-229): momentum and energy fluxes of
 * the isotropic Navier-Stokes stress subtracted from flx on the faces of the active cells */
int akmi_viscous_fluxes(const akmi_pack *p, double nu_iso, const double *w0, double *flx1,
                        double *flx2, double *flx3, int face_shaped, void *stream);
/* Conduction::AddHeatFluxIso (src/diffusion/conduction.cpp:106-152): q = -alpha*d*grad((gamma-1)e/d) */
int akmi_heat_fluxes(const akmi_pack *p, double alpha_iso, const double *w0, double *flx1,
                     double *flx2, double *flx3, int face_shaped, void *stream);
/* Conduction::NewTimeStep (src/diffusion/conduction.cpp:314-377): *dtmin (device) = min over the
 * active cells of SQR(dx)/alpha*d/(gamma-1); the caller multiplies by fac = 1/2, 1/4, 1/6 */
int akmi_conduction_newdt(const akmi_pack *p, double alpha_iso, const double *w0, double *dtmin,
                          void *stream);
/* Resistivity::AddEMFConstantResist (src/diffusion/resistivity.cpp:78-177): efld += eta_ohm*J, J from
 * CurrentDensity (src/diffusion/current_density.hpp:30-57) */
int akmi_resistive_emfs(const akmi_pack *p, double eta_ohm, const double *bx1f, const double *bx2f,
                        const double *bx3f, double *e1, double *e2, double *e3, void *stream);
/* Resistivity::AddFluxConstantResist (src/diffusion/resistivity.cpp:185-272): Poynting flux of the
 * resistive field added to the energy component of the face-shaped MHD fluxes */
int akmi_resistive_fluxes(const akmi_pack *p, double eta_ohm, const double *bx1f, const double *bx2f,
                          const double *bx3f, double *flx1, double *flx2, double *flx3, void *stream);
/* Resistivity::AddEMFConstantAmbipolar (src/diffusion/ambipolar.cpp:66-246): efld += eta_ad*(B^2 J -
 * (J.B) B) with J (EdgeJ1/2/3) and B (faces, bcc0) averaged to each edge. */
int akmi_ambipolar_emfs(const akmi_pack *p, double eta_ad, const double *bcc0, const double *bx1f,
                        const double *bx2f, const double *bx3f, double *e1, double *e2, double *e3,
                        void *stream);
/* Resistivity::AddFluxConstantAmbipolar (src/diffusion/ambipolar.cpp:254-494): Poynting flux of the
 * ambipolar field added to the energy component of the face-shaped MHD fluxes (ideal gas) */
int akmi_ambipolar_fluxes(const akmi_pack *p, double eta_ad, const double *bcc0, const double *bx1f,
                          const double *bx2f, const double *bx3f, double *flx1, double *flx2,
                          double *flx3, void *stream);
/* Resistivity::NewTimeStep with eta_ad != 0 (src/diffusion/resistivity.cpp:313-345): *dtmin (device) =
 * min over the active cells of SQR(dx)/(eta_ohm + eta_ad*B^2); the caller multiplies by fac */
int akmi_resistive_newdt(const akmi_pack *p, double eta_ohm, double eta_ad, const double *bcc0,
                         double *dtmin, void *stream);

/* Hydro::CopyCons, stages 2..4 of integrator rk4 (src/hydro/hydro_tasks.cpp:134-148): the second
 * register of the 2S scheme, u1 += delta*u0 on the active cells */
int akmi_rk4_copy_cons(const akmi_pack *p, double delta, const double *u0, double *u1, void *stream);

/* Hydro::Fluxes -> CalculateFluxes<hllc> (src/hydro/hydro_fluxes.cpp:77-229): reconstruct
 * w0 (recon), solve Riemann problem at faces i in [is,ie+1] (x1), j in [js,je+1] (x2),
 * k in [ks,ke+1] (x3).  flx arrays are cell-shaped (nmb,nvar,N3,N2,N1) as Hydro::uflx
 * (src/hydro/hydro.cpp:290-292) when face_shaped==0, or face-shaped as MHD::uflx when 1. */
int akmi_hydro_fluxes(const akmi_pack *p, int recon, int rsolver, const double *w0,
                      double *flx1, double *flx2, double *flx3, int face_shaped,
                      void *stream);

/* Hydro::RKUpdate / MHD::RKUpdate (src/hydro/hydro_update.cpp:23-83,
 * src/mhd/mhd_update.cpp:24-84):  u0 = gam0*u0 + gam1*u1 - beta_dt*divF */
int akmi_rk_update(const akmi_pack *p, double gam0, double gam1, double beta_dt,
                   double *u0, const double *u1, const double *flx1, const double *flx2,
                   const double *flx3, int face_shaped, void *stream);

/* First stage OUT OF PLACE on the task-granular path: CopyCons (u1 := u0, src/hydro/hydro_tasks.cpp:130-152)
 * followed by RKUpdate in one pass.  u0 is only read; u1 receives, in EVERY cell, what CopyCons + akmi_rk_update would
 * have left in u0 (active cells: gam0*u0 + gam1*u0 - beta_dt*divF, same operands and order; ghost cells: u0).
 * Afterwards the caller swaps the two registers: the old u0 buffer IS the copy CopyCons would have made.
 * akmi_mhd_ct_oop: the same for CopyCons of the face fields + CT (src/mhd/mhd_ct.cpp:23-80). */
int akmi_rk_update_oop(const akmi_pack *p, double gam0, double gam1, double beta_dt, const double *u0, double *u1,
                       const double *flx1, const double *flx2, const double *flx3, int face_shaped, void *stream);
int akmi_mhd_ct_oop(const akmi_pack *p, double gam0, double gam1, double beta_dt, const double *e1, const double *e2,
                    const double *e3, const double *b0x1f, const double *b0x2f, const double *b0x3f, double *b1x1f,
                    double *b1x2f, double *b1x3f, void *stream);

/* IdealHydro::ConsToPrim (src/eos/ideal_hyd.cpp:29-115) over [il,iu]x[jl,ju]x[kl,ku];
 * counters = device int[3] (dfloor,efloor,tfloor), incremented (not reset). */
int akmi_hydro_c2p(const akmi_pack *p, double *u0, double *w0, int il, int iu, int jl,
                   int ju, int kl, int ku, int *counters, void *stream);

/* Hydro::NewTimeStep (src/hydro/hydro_newdt.cpp:30-139): dt3 = device double[3] receiving
 * min over active cells of dx1/(|vx|+cs), dx2/(|vy|+cs), dx3/(|vz|+cs); initial value
 * FLT_MAX as in the reference. */
int akmi_hydro_newdt(const akmi_pack *p, const double *w0, double *dt3, void *stream);

/* ---- MHD tasks -------------------------------------------------------------------- */
/* MHD::Fluxes -> CalculateFluxes<hlld> (src/mhd/mhd_fluxes.cpp:84-266).  flx face-shaped
 * (src/mhd/mhd.cpp:341-343); face EMFs e3x1,e2x1,e1x2,e3x2,e2x3,e1x3 cell-shaped
 * (src/mhd/mhd.cpp:349-354).  Ranges are the reference's CT-extended ranges. */
int akmi_mhd_fluxes(const akmi_pack *p, int recon, int rsolver, const double *w0,
                    const double *bcc0, const double *bx1f, const double *bx2f,
                    const double *bx3f, double *flx1, double *flx2, double *flx3,
                    double *e3x1, double *e2x1, double *e1x2, double *e3x2, double *e2x3,
                    double *e1x3, void *stream);

/* MHD::CornerE (src/mhd/mhd_corner_e.cpp:26-417), Newtonian 1D/2D/3D branches. */
int akmi_mhd_corner_e(const akmi_pack *p, const double *w0, const double *bcc0,
                      const double *e3x1, const double *e2x1, const double *e1x2,
                      const double *e3x2, const double *e2x3, const double *e1x3,
                      const double *flx1, const double *flx2, const double *flx3,
                      double *e1, double *e2, double *e3, void *stream);

/* MHD::CT (src/mhd/mhd_ct.cpp:23-80) */
int akmi_mhd_ct(const akmi_pack *p, double gam0, double gam1, double beta_dt,
                const double *e1, const double *e2, const double *e3, double *b0x1f,
                double *b0x2f, double *b0x3f, const double *b1x1f, const double *b1x2f,
                const double *b1x3f, void *stream);

/* IdealMHD::ConsToPrim (src/eos/ideal_mhd.cpp:30-134) */
int akmi_mhd_c2p(const akmi_pack *p, double *u0, const double *bx1f, const double *bx2f,
                 const double *bx3f, double *w0, double *bcc0, int il, int iu, int jl,
                 int ju, int kl, int ku, int *counters, void *stream);

/* MHD::NewTimeStep (src/mhd/mhd_newdt.cpp:31-174) */
int akmi_mhd_newdt(const akmi_pack *p, const double *w0, const double *bcc0, double *dt3,
                   void *stream);

/* ---- Boundary values (same-level) -------------------------------------------------- */
/* Neighbour table: int nghbr[nmb][27], direction d = (ox3+1)*9 + (ox2+1)*3 + (ox1+1)
 * (the reference's NeighborBlock table, src/mesh/mesh.hpp:47-52, reduced to the
 * same-level case).  Entry >= 0: local index of the neighbour MeshBlock in this pack
 * (same-rank path, src/bvals/bvals_cc.cpp:122-135).  Entry == -1: no neighbour (physical
 * boundary, filled later by akmi_*_bcs).  Entry <= -2: neighbour on another rank; the
 * ghost region is filled from receive-buffer segment  s = -(entry+2)  whose start offset
 * (in doubles) is seg_off[s]. */

/* MeshBoundaryValuesCC::PackAndSendCC + RecvAndUnpackCC, same-rank part
 * (src/bvals/bvals_cc.cpp:42-447; index ranges src/bvals/buffs_cc.cpp:28-70,150-190). */
int akmi_bvals_cc_local(const akmi_pack *p, int nvar, const int *nghbr, double *u,
                        void *stream);
/* off-rank part: send_tab[nsend][2] = {local block m, direction d towards the receiver};
 * send_off[nsend] = start offset (doubles) of that segment in sendbuf. A segment holds
 * [n][k][j][i] of the ng innermost active layers the receiver needs. */
int akmi_bvals_cc_pack(const akmi_pack *p, int nvar, int nsend, const int *send_tab,
                       const long long *send_off, const double *u, double *sendbuf,
                       void *stream);
int akmi_bvals_cc_unpack(const akmi_pack *p, int nvar, const int *nghbr,
                         const long long *seg_off, const double *recvbuf, double *u,
                         void *stream);
/* number of doubles in the CC segment for direction d (per variable) */
long long akmi_bvals_cc_segsize(const akmi_pack *p, int d);

/* MeshBoundaryValuesFC::PackAndSendFC + RecvAndUnpackFC (src/bvals/bvals_fc.cpp:63,289;
 * ranges src/bvals/buffs_fc.cpp:29-110,396-431): shared faces are never exchanged. */
int akmi_bvals_fc_local(const akmi_pack *p, const int *nghbr, double *bx1f, double *bx2f,
                        double *bx3f, void *stream);
int akmi_bvals_fc_pack(const akmi_pack *p, int nsend, const int *send_tab,
                       const long long *send_off, const double *bx1f, const double *bx2f,
                       const double *bx3f, double *sendbuf, void *stream);
int akmi_bvals_fc_unpack(const akmi_pack *p, const int *nghbr, const long long *seg_off,
                         const double *recvbuf, double *bx1f, double *bx2f, double *bx3f,
                         void *stream);
/* doubles in the FC segment for direction d (x1f+x2f+x3f parts, in that order) */
long long akmi_bvals_fc_segsize(const akmi_pack *p, int d);

/* MeshBoundaryValues::HydroBCs / BFieldBCs (src/bvals/physics/hydro_bcs.cpp:28-...,
 * src/bvals/physics/bfield_bcs.cpp:25-...).  bcs = device int[nmb][6] of AKMI_BC_* for
 * inner_x1,outer_x1,inner_x2,outer_x2,inner_x3,outer_x3 (mb_bcs). */
int akmi_hydro_bcs(const akmi_pack *p, int nvar, const int *bcs, double *u, void *stream);
int akmi_bfield_bcs(const akmi_pack *p, const int *bcs, double *bx1f, double *bx2f,
                    double *bx3f, void *stream);
/* the same with the inflow states of MeshBoundaryValues::u_in / b_in (src/bvals/bvals.cpp:323-326):
 * u_in = device double[nvar][6], b_in = device double[3][6], indexed [variable][BoundaryFace].
 * Flags handled: reflect, outflow, inflow, diode (normal velocity clipped to point outwards;
 * field as outflow), vacuum (zeros; field as outflow); AKMI_BC_USER faces are left alone. */
int akmi_hydro_bcs_inflow(const akmi_pack *p, int nvar, const int *bcs, const double *u_in, double *u,
                          void *stream);
int akmi_bfield_bcs_inflow(const akmi_pack *p, const int *bcs, const double *b_in, double *bx1f,
                           double *bx2f, double *bx3f, void *stream);
/* The same with the set of directions that have a physical boundary at all (bit d = direction d; the caller derives it from
 * the flags once): the other directions are not launched.  dirs = 7 equals the entries above; u_in / b_in may be NULL. */
int akmi_hydro_bcs_dirs(const akmi_pack *p, int nvar, const int *bcs, int dirs, const double *u_in, double *u,
                        void *stream);
int akmi_bfield_bcs_dirs(const akmi_pack *p, const int *bcs, int dirs, const double *b_in, double *bx1f, double *bx2f,
                         double *bx3f, void *stream);

/* Same-rank gather AND the physical boundary functions of the pack in ONE launch, for packs without off-rank neighbours
 * (every nghbr entry >= -1): the result equals akmi_bvals_cc_local followed by akmi_hydro_bcs_inflow (resp.
 * akmi_bvals_fc_local followed by akmi_bfield_bcs_inflow) bit for bit.  The reference applies its boundary functions one
 * direction after the other over all transverse indices (hydro_bcs.cpp:69-230, bfield_bcs.cpp:66-300, called from
 * hydro_tasks.cpp:357-375 / mhd_tasks.cpp after the receives); a ghost element therefore holds T3(T2(T1(x))) of ONE source
 * element x, and the kernel fetches that element directly.  u_in / b_in may be NULL when no face is AKMI_BC_INFLOW.
 * dt3_reset (may be NULL): the three CFL minima are set to FLT_MAX by the same launch, so the following
 * akmi_*_c2p_newdt may be called with do_newdt = 2 ("scan, dt3 already reset"). */
int akmi_bvals_cc_local_bcs(const akmi_pack *p, int nvar, const int *nghbr, const int *bcs, const double *u_in, double *u,
                            double *dt3_reset, void *stream);
int akmi_bvals_fc_local_bcs(const akmi_pack *p, const int *nghbr, const int *bcs, const double *b_in, double *bx1f,
                            double *bx2f, double *bx3f, void *stream);

/* ---- SMR/AMR operators between a MeshBlock and its coarse buffer ---------- *
 * Coarse arrays: cnx = nx/2 active cells, the same ng ghost cells, same layout:
 * (nmb,nvar,cN3,cN2,cN1), faces +1 in their own direction (src/mesh/mesh.cpp:286-330).  Index boxes
 * box = {il,iu,jl,ju,kl,ku} are COARSE indices (the iprol boxes of src/bvals/prolongation.cpp);
 * fine index = (coarse - cis)*2 + is.  The mesh tree and the level-aware exchange that drive these
 * operators in the reference are not part of this library yet. */
/* MeshRefinement::RestrictCC (src/mesh/mesh_refinement.cpp:1223-1277) over the active coarse cells */
int akmi_restrict_cc(const akmi_pack *p, int nvar, const double *u, double *cu, void *stream);
/* MeshRefinement::RestrictFC (src/mesh/mesh_refinement.cpp:1283-1382) */
int akmi_restrict_fc(const akmi_pack *p, const double *bx1f, const double *bx2f, const double *bx3f,
                     double *cbx1f, double *cbx2f, double *cbx3f, void *stream);
/* the same for the MeshBlocks m with mask[m] != 0 only (mask on the device, NULL = all).  On a statically refined
 * mesh only a block with a coarser neighbour reads its coarse buffer (sends to that neighbour, prolongation
 * stencils): akmi_smr::needs_coarse is that mask. */
int akmi_restrict_cc_masked(const akmi_pack *p, int nvar, const unsigned char *mask, const double *u, double *cu,
                            void *stream);
int akmi_restrict_fc_masked(const akmi_pack *p, const unsigned char *mask, const double *bx1f, const double *bx2f,
                            const double *bx3f, double *cbx1f, double *cbx2f, double *cbx3f, void *stream);
/* Conservation at fine/coarse faces: what a fine MeshBlock hands to a coarser neighbour.
 * akmi_restrict_flux_cc: the 2x2 (2-D: 2, 1-D: 1) fine face fluxes of direction `dir` behind each coarse
 * face of `box` (coarse indices il,iu,jl,ju,kl,ku; one face thick along dir), in the buffer order of
 * MeshBoundaryValuesCC::PackAndSendFluxCC (src/bvals/flux_correct_cc.cpp:78-148):
 * out[m][(t1-t1l) + n1*((t2-t2l) + n2*v)], (t1,t2) = (j,k) | (i,k) | (i,j).  flx is face-shaped
 * (nmb,nvar,N3(+1),N2(+1),N1(+1)).
 * akmi_restrict_emf: the two fine edges behind each coarse edge of component comp (x1e,x2e,x3e shapes of
 * akmi_mhd_corner_e), MeshBoundaryValuesFC::PackAndSendFluxFC (src/bvals/flux_correct_fc.cpp:84-360):
 * out[m][(i-il) + ni*((j-jl) + nj*(k-kl))]. */
int akmi_restrict_flux_cc(const akmi_pack *p, int nvar, int dir, const int *box, const double *flx,
                          double *out, void *stream);
int akmi_restrict_emf(const akmi_pack *p, int comp, const int *box, const double *e, double *out,
                      void *stream);
/* Primitive -> conserved over the fine cells of `box` (il,iu,jl,ju,kl,ku): SingleP2C_IdealHyd/_IdealMHD/
 * _Isothermal* (src/eos/ideal_c2p_hyd.hpp:76-83, ideal_c2p_mhd.hpp:75-84; scalars u = d*s), the step
 * MeshBoundaryValuesCC::PrimToConsFineBndry performs after primitives were prolongated
 * (src/bvals/prolong_prims.cpp:190-300,465-...).  bcc = NULL for hydro. */
int akmi_prim2cons(const akmi_pack *p, const int *box, const double *w, const double *bcc, double *u,
                   void *stream);
/* ProlongCC (src/mesh/prolongation.hpp:19-63): min-mod limited linear interpolation */
int akmi_prolong_cc(const akmi_pack *p, int nvar, const int *box, const double *cu, double *u,
                    void *stream);
/* ProlongFCSharedX1Face/X2Face/X3Face (src/mesh/prolongation.hpp:69-160): component comp = 0,1,2 */
int akmi_prolong_fc_shared(const akmi_pack *p, int comp, const int *box, const double *cb, double *b,
                           void *stream);
/* ProlongFCInternal (src/mesh/prolongation.hpp:166-230; Toth & Roe 2002), after the shared faces */
int akmi_prolong_fc_internal(const akmi_pack *p, const int *box, double *bx1f, double *bx2f,
                             double *bx3f, void *stream);

/* ---- boundary values of a statically refined pack --------------------------
 * The reference keeps, per MeshBoundaryValues object, 56 MeshBoundaryBuffers with the index ranges
 * of every slot (src/bvals/bvals.hpp:62-107, buffs_cc.cpp, buffs_fc.cpp) and the NeighborBlock table
 * of every MeshBlock (src/mesh/mesh.hpp:47-52).  A caller hands the same information over as flat
 * device tables; the entry points below are the bodies of PackAndSend* / RecvAndUnpack* /
 * FillCoarseInBndry* / Prolongate* / *FluxCC / *FluxFC for neighbours that live in the same pack.
 *   nghbr   [nmb][56][3]   {index of the neighbour block in this pack or -1, its level, dest slot}
 *   mblev   [nmb]          level of each block
 *   cc_tab, fc_tab [2][6][56][3][6]  (send|recv) x (isame, icoar, ifine, iprol, iflux_same,
 *                          iflux_coar) x slot x component x {bis,bie,bjs,bje,bks,bke}; cell-centred
 *                          tables use component 0 only
 *   ndat    [2][56][2][5]  (cc|fc) x slot x (send|recv) x {isame,icoar,ifine,iflxs,iflxc}_ndat
 *   layout  [4][56][2]     (cc vars, cc flux, fc vars, fc flux) x slot x {offset, per-block stride}
 *                          of the receive buffers inside the buffer the caller passes (doubles)
 *   slot_ox [56][3]        offsets (ox1,ox2,ox3) of each slot (inverse of NeighborIndex,
 *                          src/mesh/nghbr_index.hpp:28-54) */
typedef struct akmi_smr {
  int nnghbr;             /* 8 / 24 / 56: src/mesh/meshblock.cpp:145-147 */
  int multilevel;
  const int *nghbr, *mblev, *cc_tab, *fc_tab, *ndat, *slot_ox;
  const long long *layout;
  /* ranks: [4][nmb][56] offsets (doubles) inside the buffer of each class at which block m WRITES
   * the segment of its slot n (soff: the receive segment of a neighbour in this pack, or a place in
   * the message to another rank) and READS the segment it receives (roff).  NULL: everything is
   * in this pack and layout[] alone addresses the buffers.  With them an off-rank neighbour is
   * marked in nghbr by any index >= 0 (it is only tested for existence then). */
  const long long *soff, *roff;
  /* != 0: cell-centred ghost zones whose neighbour has the SAME level and lives in this pack are not packed /
   * unpacked by akmi_smr_*_cc: the caller fills them with akmi_bvals_cc_local (one gather straight from the
   * neighbour's active cells, no buffer round trip; the regions of different slots are disjoint for cell-centred
   * data, so the order does not matter).  0 (a zero-initialised descriptor): every slot goes through the buffers. */
  int direct_same;
  /* [nmb] or NULL: != 0 for blocks with at least one coarser neighbour.  FillCoarseInBndryCC/FC write ghost zones
   * of the COARSE arrays, which only ProlongateCC/FC of such a block ever read; with the table the fill skips the
   * other blocks (NULL: every block, as the reference does; the fine arrays come out the same either way). */
  const unsigned char *needs_coarse;
  /* Work lists (optional; NULL / zero-initialised: every entry point launches over all (MeshBlock, slot) pairs).
   * lists = device array of AKMI_SMR_NLISTS lists of (m, n) int pairs, list l at lists + l*2*nmb*56, list_cnt[l]
   * pairs each, filled by akmi_smr_build_lists once after the tables above are in place.  The entry points then
   * launch over the pairs of the list that covers their own test (existing neighbour; coarser; finer; same level of
   * a block that prolongates; faces and edges that average their EMFs) instead of nmb*56 pairs of which a few per
   * cent do anything.  Results cannot depend on the lists: every kernel still applies its own test. */
  const int *lists;
  int list_cnt[6];
} akmi_smr;
#define AKMI_SMR_NLISTS 6
/* lists: device, 2*nmb*56*AKMI_SMR_NLISTS ints; counts: HOST, AKMI_SMR_NLISTS ints (copy them into list_cnt).
 * Set-up call: synchronises `stream`.  direct_same and needs_coarse of *t must already have their final values. */
int akmi_smr_build_lists(const akmi_pack *p, const akmi_smr *t, int *lists, int *counts, void *stream);
/* RestrictU is akmi_restrict_cc / akmi_restrict_fc above.  SendU+RecvU (PackAndSendCC +
 * RecvAndUnpackCC, src/bvals/bvals_cc.cpp:42-447): u ghost cells from same-level and finer neighbours,
 * coarse buffer cu from coarser ones.  buf: receive buffers (layout[0]) */
int akmi_smr_exchange_cc(const akmi_pack *p, const akmi_smr *t, int nvar, double *u, double *cu,
                         double *buf, void *stream);
/* SendB+RecvB (src/bvals/bvals_fc.cpp:63-436): slots unpacked in order, active faces never
 * overwritten by same-level / finer data.  buf: layout[2] */
int akmi_smr_exchange_fc(const akmi_pack *p, const akmi_smr *t, double *b1, double *b2, double *b3,
                         double *cb1, double *cb2, double *cb3, double *buf, void *stream);
/* FillCoarseInBndryCC / FC (src/bvals/prolongation.cpp:366-462,556-644) */
int akmi_smr_fill_coarse_cc(const akmi_pack *p, const akmi_smr *t, int nvar, const double *u, double *cu,
                            void *stream);
int akmi_smr_fill_coarse_fc(const akmi_pack *p, const akmi_smr *t, const double *b1, const double *b2,
                            const double *b3, double *cb1, double *cb2, double *cb3, void *stream);
/* ProlongateCC / ProlongateFC (src/bvals/prolongation.cpp:470-546,650-785; the latter with the
 * owned-face rule of :90-147) */
int akmi_smr_prolong_cc(const akmi_pack *p, const akmi_smr *t, int nvar, const double *cu, double *u,
                        void *stream);
int akmi_smr_prolong_fc(const akmi_pack *p, const akmi_smr *t, const double *cb1, const double *cb2,
                        const double *cb3, double *b1, double *b2, double *b3, void *stream);
/* <mesh_refinement>/prolong_primitives = true: the two conversions MHD::Prolongate / Hydro::Prolongate put
 * round ProlongateCC (src/mhd/mhd_tasks.cpp:539-544, src/hydro/hydro_tasks.cpp:388-392).
 * ConsToPrimCoarseBndry (src/bvals/prolong_prims.cpp:35-186, 303-461): coarse conserved -> coarse primitive
 * variables on the cells the prolongation of every slot with a coarser neighbour reads (iprol widened by one);
 * cb1..3 = coarse face fields (NULL: hydro); cu is only modified where a passive scalar is negative.
 * PrimToConsFineBndry (:190-296, 465-575): the prolongated fine ghost cells of w back to conserved variables
 * in u; b1..3 = fine face fields after ProlongateFC (NULL: hydro).  Ideal gas only, as in the reference. */
int akmi_smr_c2p_coarse(const akmi_pack *p, const akmi_smr *t, int nvar, double *cu, const double *cb1,
                        const double *cb2, const double *cb3, double *cw, void *stream);
int akmi_smr_p2c_fine(const akmi_pack *p, const akmi_smr *t, int nvar, const double *w, const double *b1,
                      const double *b2, const double *b3, double *u, void *stream);
/* SendFlux+RecvFlux (PackAndSendFluxCC + RecvAndUnpackFluxCC, src/bvals/flux_correct_cc.cpp:29-304):
 * the fluxes on faces shared with finer neighbours are replaced by the restricted fine fluxes.
 * face_shaped: MHD flux arrays (N+1 along their direction), 0: hydro (cell-shaped).  buf: layout[1] */
int akmi_smr_flux_cc(const akmi_pack *p, const akmi_smr *t, int nvar, int face_shaped, double *flx1,
                     double *flx2, double *flx3, double *buf, void *stream);
/* SendE+RecvE (PackAndSendFluxFC + RecvAndUnpackFluxFC, src/bvals/flux_correct_fc.cpp:29-1034): edge
 * EMFs on block surfaces summed over same-level owners, replaced by the restricted EMFs of finer
 * neighbours, averaged.  nflx [nmb][48]: contributions per block edge (the counting of
 * SumBoundaryFluxes / ZeroFluxesAtBoundaryWithFiner, a function of the neighbour table).  buf: layout[3] */
int akmi_smr_emf_exchange(const akmi_pack *p, const akmi_smr *t, const int *nflx, double *e1, double *e2,
                          double *e3, double *buf, void *stream);
/* The four exchanges cut at the point where the reference posts its MPI messages: *_pack_* = the
 * PackAndSend* half (fills the segments soff names), *_unpack_* = the RecvAndUnpack* half (reads the
 * segments roff names; for the EMFs: sum, zero, sum, average).  A caller with off-rank neighbours
 * moves the per-rank slices of buf between the two calls. */
int akmi_smr_pack_cc(const akmi_pack *p, const akmi_smr *t, int nvar, const double *u, const double *cu,
                     double *buf, void *stream);
int akmi_smr_unpack_cc(const akmi_pack *p, const akmi_smr *t, int nvar, const double *buf, double *u,
                       double *cu, void *stream);
int akmi_smr_pack_fc(const akmi_pack *p, const akmi_smr *t, const double *b1, const double *b2,
                     const double *b3, const double *cb1, const double *cb2, const double *cb3, double *buf,
                     void *stream);
int akmi_smr_unpack_fc(const akmi_pack *p, const akmi_smr *t, const double *buf, double *b1, double *b2,
                       double *b3, double *cb1, double *cb2, double *cb3, void *stream);
int akmi_smr_pack_flux_cc(const akmi_pack *p, const akmi_smr *t, int nvar, int face_shaped, const double *flx1,
                          const double *flx2, const double *flx3, double *buf, void *stream);
int akmi_smr_unpack_flux_cc(const akmi_pack *p, const akmi_smr *t, int nvar, int face_shaped, const double *buf,
                            double *flx1, double *flx2, double *flx3, void *stream);
int akmi_smr_pack_emf(const akmi_pack *p, const akmi_smr *t, const double *e1, const double *e2,
                      const double *e3, double *buf, void *stream);
int akmi_smr_unpack_emf(const akmi_pack *p, const akmi_smr *t, const int *nflx, const double *buf, double *e1,
                        double *e2, double *e3, void *stream);

/* The face-field exchange of a refined mesh as one list of element copies.  PackAndSendFC + RecvAndUnpackFC
 * (src/bvals/bvals_fc.cpp:63-289, :300-436) only move values: which face of which array a ghost face receives -- with
 * the precedence of the reference's slot-by-slot unpack where slots overlap, and never a face the block owns -- depends
 * on the mesh alone.  akmi_smr_fc_map (set-up call, synchronises `stream`) finds the copies by running
 * akmi_smr_pack_fc [+ akmi_smr_unpack_fc] once on scratch arrays whose elements hold their own index, and returns their
 * number (-1: failure); map == NULL: count only; otherwise map receives (destination, source) pairs of 32-bit indices
 * into the concatenation [b1 | b2 | b3 | cb1 | cb2 | cb3 | buf], sorted by destination (cap = pairs it has room for).
 *   which = 0: what the unpack does (sources: arrays of this pack, or the part of buf other ranks fill);
 *   which = 1: the outgoing messages, buf[send_lo, send_hi) <- arrays (ranks only; 0 pairs on one rank).
 * The reference packs every message before it unpacks any, so a copy reads the value its source had BEFORE the exchange;
 * the few copies whose source is itself a destination (surface faces of a fine block's coarse array) are the last *ntail
 * pairs of the list -- akmi_smr_fc_copy performs them first, in a launch of their own -- and their place in the ordered
 * part holds a no-op (destination == source).
 * buf (the class-2 buffer of the exchange, buf_doubles long) is used as scratch and zeroed.  akmi_smr_fc_copy performs
 * a list: one rank -- the which = 0 list in place of akmi_smr_pack_fc + akmi_smr_unpack_fc; ranks -- the which = 1
 * list, the transfer, the which = 0 list. */
long long akmi_smr_fc_map(const akmi_pack *p, const akmi_smr *t, double *buf, long long buf_doubles, long long send_lo,
                          long long send_hi, int which, int *map, long long cap, long long *ntail, void *stream);
int akmi_smr_fc_copy(const akmi_pack *p, const int *map, long long npairs, long long ntail, long long buf_doubles,
                     double *b1, double *b2, double *b3, double *cb1, double *cb2, double *cb3, double *buf,
                     void *stream);

/* The same for the cell-centred variables (PackAndSendCC + RecvAndUnpackCC, src/bvals/bvals_cc.cpp:42-447, as this
 * library performs them: akmi_smr_pack_cc + akmi_smr_unpack_cc across levels, then the direct same-level gather
 * akmi_bvals_cc_local with the [nmb][27] table same27): the copies of the nvar variables of a cell are one copy nvar times,
 * so the list holds the pairs of variable 0 in the index space [u | cu] and akmi_smr_cc_copy applies it to every variable.
 * One rank only (returns -1 when akmi_smr::soff / roff are set: the caller keeps the three calls then). */
long long akmi_smr_cc_map(const akmi_pack *p, const akmi_smr *t, int nvar, const int *same27, double *buf,
                          long long buf_doubles, int *map, long long cap, long long *ntail, void *stream);
int akmi_smr_cc_copy(const akmi_pack *p, int nvar, const int *map, long long npairs, long long ntail, double *u,
                     double *cu, void *stream);

/* ---- Fused fast path ("one kernel sequence per MeshBlockPack stage") ----------------- *
 * Must produce results identical to the task chain above.  ws = device workspace of
 * akmi_stage_workspace_bytes() bytes owned by the caller. */
long long akmi_stage_workspace_bytes(const akmi_pack *p, int is_mhd);

/* Hydro: Fluxes + RKUpdate fused (stage 1 reads u0 as u1 when u1==NULL is not allowed;
 * CopyCons semantics are folded in when copy_u1 != 0: u1 <- u0 before the update).
 * copy_u1 == 2: the first stage OUT OF PLACE -- u0 (and b0) are only read, the new state is written
 * to u1 (and b1), and the caller swaps the two registers (pointers) after the call; the copy of
 * Hydro::CopyCons / MHD::CopyCons (5 + 3 arrays written) disappears.  Only the cells and faces the update
 * touches are written; the ghost zones of the new register are filled by the halo exchange and the
 * boundary conditions that follow every stage.  With akmi_*_stage_phase the swap of u follows the
 * SWEEPS part and the swap of b the EMF_CT part (the C2P part is passed the swapped pointers).
 * copy_u1 == 3 (MHD, 3-D PLM + HLLD ideal gas: akmi_mhd_u0_sweeps_eligible): the LAST stage of a cycle OUT OF PLACE --
 * u0 and u1 are read, the new state is written to u1's buffer (the state of the start of the cycle, which nothing
 * reads any more) and the caller swaps u0/u1 afterwards; b0 is updated in place, b0/b1 are not swapped.
 * AKMI_COPY_X3_U0, or-ed into copy_u1 == 2 or 3 by a caller whose w0 is ConsToPrim of u0 in every cell, ghost zones
 * included: the x3 march reads density and momentum once, from u0, instead of w0[0..3] for its window and u0[0..3]
 * again for the update (bit-identical results; refused for a stage that writes the array it reads).
 * AKMI_COPY_X12_U0, or-ed in beside AKMI_COPY_X3_U0 under the same precondition: k_sweep12s reads density and momentum from
 * u0 instead of w0[0..3] (it runs before the x3 march of the stage writes anything, in stream order).
 * AKMI_COPY_BCC_FACES, likewise: k_sweep12s and the x3 march form the cell-centred field from b0's faces instead of reading
 * bcc0.  A stage called with AKMI_COPY_X3_U0 | AKMI_COPY_X12_U0 reads w0[4] alone of w0, with AKMI_COPY_BCC_FACES on top
 * nothing of bcc0: the conversion before it may drop those arrays (akmi_mhd_c2p_newdt_lean).
 * akmi_stage_last_forms(): which forms the last stage call of this thread that ran sweeps took, a mask of AKMI_FORM_*. */
enum { AKMI_COPY_X3_U0 = 0x100, AKMI_COPY_X12_U0 = 0x200, AKMI_COPY_BCC_FACES = 0x400, AKMI_COPY_MASK = 0xff };
enum { AKMI_FORM_X3_U0 = 1,     /* x3 march read u0 for its window and parked it for the update */
       AKMI_FORM_X12_U0 = 2,    /* k_sweep12s read u0 instead of w0[0..3] */
       AKMI_FORM_LEAN_C2P = 4,  /* the sweeps ran on primitives a lean conversion left (set by the host that ran that
                                   conversion: akmi_sim_stage_forms; a stage call cannot know) */
       AKMI_FORM_BCC_FACES = 8 };/* k_sweep12s and the x3 march formed the cell-centred field from the faces */
int akmi_stage_last_forms(void);
int akmi_mhd_u0_sweeps_eligible(const akmi_pack *p, int recon, int rsolver);
int akmi_hydro_stage_update(const akmi_pack *p, int recon, int rsolver, double gam0,
                            double gam1, double beta_dt, int copy_u1, const double *w0,
                            double *u0, double *u1, void *ws, void *stream);
/* MHD: Fluxes + CornerE + RKUpdate + CT fused */
int akmi_mhd_stage_update(const akmi_pack *p, int recon, int rsolver, double gam0,
                          double gam1, double beta_dt, int copy_u1, const double *w0,
                          const double *bcc0, double *u0, double *u1, double *b0x1f,
                          double *b0x2f, double *b0x3f, double *b1x1f, double *b1x2f,
                          double *b1x3f, void *ws, void *stream);
/* ConsToPrim + (optionally, last stage) NewTimeStep fused.  do_newdt: 0 no scan, 1 reset dt3 and scan, 2 scan only (dt3 was
 * reset earlier in stream order, e.g. by akmi_bvals_cc_local_bcs) */
int akmi_hydro_c2p_newdt(const akmi_pack *p, double *u0, double *w0, int do_newdt,
                         int *counters, double *dt3, void *stream);
int akmi_mhd_c2p_newdt(const akmi_pack *p, double *u0, const double *bx1f,
                       const double *bx2f, const double *bx3f, double *w0, double *bcc0,
                       int do_newdt, int *counters, double *dt3, void *stream);

/* Lean conversion: akmi_mhd_c2p_newdt that computes everything as before -- floors, write-back to u0, counters, CFL
 * scan -- but does not STORE the arrays named by drop (a mask of AKMI_DROP_*), which are functions of u0 and the faces
 * alone.  For a caller whose next stage call carries the form flags that cover what is dropped.  drop == 0 is
 * akmi_mhd_c2p_newdt.  akmi_mhd_prims_fill writes exactly the dropped arrays from u0 and the faces (no floors, w0[4]
 * untouched): lean conversion + fill == full conversion, in all eight arrays.  (Converting twice is not the same where a
 * floor binds: the second pass would count the floored cells again.) */
enum { AKMI_DROP_W03 = 1,       /* w0[0..3]: density and velocity */
       AKMI_DROP_BCC = 2 };     /* bcc0 */
int akmi_mhd_c2p_newdt_lean(const akmi_pack *p, double *u0, const double *bx1f, const double *bx2f,
                            const double *bx3f, double *w0, double *bcc0, int do_newdt, int *counters,
                            double *dt3, int drop, void *stream);
int akmi_mhd_prims_fill(const akmi_pack *p, const double *u0, const double *bx1f, const double *bx2f,
                        const double *bx3f, double *w0, double *bcc0, int drop, void *stream);
/* 1 where akmi_mhd_c2p_newdt of this pack takes its two-cells-per-thread kernel, the one that is bound by its stores */
int akmi_mhd_c2p_takes_pairs(const akmi_pack *p);

/* Whole stage in one call: pass A (as akmi_*_stage_update) + ConsToPrim of the ACTIVE cells
 * (+ the CFL scan when do_newdt) in the same call.  w0/bcc0 are read (old primitives) and
 * rewritten for the active cells.  After the halo exchange / physical BCs the caller converts
 * the ghost shell with akmi_*_c2p_shell; together they equal akmi_*_c2p_newdt over all cells
 * (ConToPrim covers ghosts: src/hydro/hydro_tasks.cpp:404-412). */
int akmi_hydro_stage_fused(const akmi_pack *p, int recon, int rsolver, double gam0,
                           double gam1, double beta_dt, int copy_u1, double *w0, double *u0,
                           double *u1, int do_newdt, int *counters, double *dt3, void *ws,
                           void *stream);
int akmi_mhd_stage_fused(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                         double beta_dt, int copy_u1, double *w0, double *bcc0, double *u0,
                         double *u1, double *b0x1f, double *b0x2f, double *b0x3f,
                         double *b1x1f, double *b1x2f, double *b1x3f, int do_newdt,
                         int *counters, double *dt3, void *ws, void *stream);
/* The same with the time step in DEVICE memory: the kernels form beta*(*dt_dev) themselves (the
 * product RKUpdate forms on the host, hydro_update.cpp:35 -- same operands, same rounding).  No
 * argument of the call changes from cycle to cycle then, so a whole cycle can be captured into a
 * hipGraph once and replayed (the C++ host does: akmi_host.cpp Driver::Execute). */
int akmi_hydro_stage_fused_dt(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                              double beta, const double *dt_dev, int copy_u1, double *w0, double *u0,
                              double *u1, int do_newdt, int *counters, double *dt3, void *ws,
                              void *stream);
int akmi_mhd_stage_fused_dt(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                            double beta, const double *dt_dev, int copy_u1, double *w0, double *bcc0,
                            double *u0, double *u1, double *b0x1f, double *b0x2f, double *b0x3f,
                            double *b1x1f, double *b1x2f, double *b1x3f, int do_newdt, int *counters,
                            double *dt3, void *ws, void *stream);
/* The same stage cut into its parts for callers that post halo messages in between (a rank
 * with off-rank neighbours sends u0 after SWEEPS and b0 after EMF_CT, so the transfers run
 * under CornerE/CT and under the c2p of the active cells, in the order of the reference's
 * task list: RKUpdate -> SendU -> EField -> CT -> SendB, src/mhd/mhd_tasks.cpp:48-75).
 * phases is a mask of AKMI_PHASE_*; the parts must be called in increasing order within a
 * stage with identical arguments; AKMI_PHASE_ALL equals akmi_*_stage_fused. */
enum { AKMI_PHASE_SWEEPS = 1,   /* reconstruct + Riemann x1..x3 + RK update of u0 (+ face EMFs) */
       AKMI_PHASE_EMF_CT = 2,   /* CornerE + CT of b0 (MHD only; ignored for hydro)            */
       AKMI_PHASE_C2P    = 4,   /* ConsToPrim of the active cells (+ CFL scan if do_newdt)     */
       AKMI_PHASE_ALL    = 7 };
int akmi_hydro_stage_phase(const akmi_pack *p, int recon, int rsolver, double gam0,
                           double gam1, double beta_dt, int copy_u1, double *w0, double *u0,
                           double *u1, int do_newdt, int *counters, double *dt3, int phases,
                           void *ws, void *stream);
int akmi_mhd_stage_phase(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1,
                         double beta_dt, int copy_u1, double *w0, double *bcc0, double *u0,
                         double *u1, double *b0x1f, double *b0x2f, double *b0x3f,
                         double *b1x1f, double *b1x2f, double *b1x3f, int do_newdt,
                         int *counters, double *dt3, int phases, void *ws, void *stream);
/* the parts with dt read from device memory (beta = the RK weight alone, as in akmi_*_stage_fused_dt): for callers that
 * enqueue a cycle before the previous cycle's new time step has reached the host */
int akmi_hydro_stage_phase_dt(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1, double beta,
                              const double *dt_dev, int copy_u1, double *w0, double *u0, double *u1, int do_newdt,
                              int *counters, double *dt3, int phases, void *ws, void *stream);
int akmi_mhd_stage_phase_dt(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1, double beta,
                            const double *dt_dev, int copy_u1, double *w0, double *bcc0, double *u0, double *u1,
                            double *b0x1f, double *b0x2f, double *b0x3f, double *b1x1f, double *b1x2f, double *b1x3f,
                            int do_newdt, int *counters, double *dt3, int phases, void *ws, void *stream);
/* Hydro, the whole stage with ConsToPrim of the active cells INSIDE the update kernel (3-D, DC / PLM, ideal gas, no passive
 * scalars: akmi_hydro_stage_w_eligible returns 1): the kernel that finishes a cell holds its new conserved state in registers,
 * so the conversion (src/eos/ideal_c2p_hyd.hpp:22-66, floors and counters included) and, with do_newdt, the CFL scan
 * (src/hydro/hydro_newdt.cpp:97-118) cost five stores there instead of a pass that reads u0 back.  Other workgroups still
 * read w0 while one finishes, so the new primitives of the ACTIVE cells go to w0_new, an array of w0's shape, and
 * *wrote_new = 1: the caller uses w0_new as w0 from then on (swap the two) and fills the ghost cells of u0 and of it with
 * akmi_hydro_ghost_uw (NOT by converting the ghost copies of the floored u0 again: see there).  Where the kernel does not apply the call is akmi_hydro_stage_fused[_dt]
 * (active cells converted in place in w0, *wrote_new = 0).  beta: the RK weight when dt_dev != NULL (dt read from device
 * memory), beta*dt otherwise.  do_newdt: 0 no scan, 1 reset dt3 and scan, 2 scan (the caller has reset dt3). */
int akmi_hydro_stage_w_eligible(const akmi_pack *p, int recon, int rsolver);
int akmi_hydro_stage_w(const akmi_pack *p, int recon, int rsolver, double gam0, double gam1, double beta,
                       const double *dt_dev, int copy_u1, double *w0, double *w0_new, double *u0, double *u1,
                       int do_newdt, int *counters, double *dt3, void *ws, void *stream, int *wrote_new);
int akmi_hydro_c2p_shell(const akmi_pack *p, double *u0, double *w0, int *counters,
                         void *stream);
/* What is left of a hydro stage after akmi_hydro_stage_w on a pack without off-rank neighbours: the ghost zones of u0 AND of
 * the new primitive array, one launch, no conversion.  The reference converts every cell after the ghost fill
 * (hydro_tasks.cpp:357-375,404-412), so a ghost cell's (u, w) equals its source cell's under the boundary's value rule
 * (copy for neighbour / periodic / outflow, sign of the normal momentum and velocity for reflect) -- floors included, whereas
 * converting the copy of an already floored u a second time would not reproduce it.  bcs: device int[nmb][6]; bcs_host: the
 * same flags in host memory -- a pack with a diode, vacuum, inflow or user face is refused (AKMI_FAIL): keep
 * akmi_bvals_cc_local_bcs + akmi_hydro_c2p_newdt (no akmi_hydro_stage_w) there.  ws: the workspace akmi_hydro_stage_w was
 * given (it leaves one floor-flag byte per cell at its start); counters: the three floor counters -- every ghost image of a
 * cell a floor acted on is counted, as the reference's ConsToPrim over all cells counts it. */
int akmi_hydro_ghost_uw(const akmi_pack *p, const int *nghbr, const int *bcs, const int *bcs_host, double *u0, double *w0,
                        const void *ws, int *counters, void *stream);
int akmi_mhd_c2p_shell(const akmi_pack *p, double *u0, const double *bx1f, const double *bx2f,
                       const double *bx3f, double *w0, double *bcc0, int *counters,
                       void *stream);

/* History sums (HistoryOutput::LoadHydroHistoryData / LoadMHDHistoryData,
 * src/outputs/history.cpp:78-160,272-374): out[0..7] = volume sums over the active cells of
 * d, M1, M2, M3, E, and the kinetic energies 0.5*Mi^2/d; MHD adds out[8..10] = the magnetic
 * energies 0.25*(B_face^2 + B_face+1^2) per direction.  out is a device array of 8 (11)
 * doubles; it is zeroed by the call. */
int akmi_history_sums(const akmi_pack *p, int is_mhd, const double *u0, const double *bx1f,
                      const double *bx2f, const double *bx3f, double *out, void *stream);

/* ---- native host driver (C++ mirror of Mesh/MeshBlockPack/TaskList/Driver/Hydro/MHD) ----- *
 * athenak_amd/csrc/akmi_host.{hpp,cpp}: the reference's operator surface for this path in
 * C++, every task body one call of the entries above.  One process per GPU: with akmi_comm_init_*
 * called first the Z-ordered MeshBlock list is cut into one pack per rank (Mesh::LoadBalance,
 * src/mesh/load_balance.cpp:38-88) and the arrays of akmi_sim_array are those of THIS rank's pack
 * (blocks akmi_sim_gids .. +akmi_sim_nmb_thisrank-1); without it: one rank, all MeshBlocks in one
 * pack on the current GPU.  deck_text is an athinput deck (src/parameter_input.cpp grammar).  Initial conditions are written by the caller into the arrays returned by
 * akmi_sim_array (device pointers, layouts as above) before akmi_sim_initialize, which performs
 * Driver::Initialize (src/driver/driver.cpp:314-371); tlim_override > 0 replaces <time>/tlim
 * (the linear-wave generator rescales it).  akmi_sim_execute runs Driver::Execute for at most
 * max_cycles (<0: until tlim/nlim) and returns the number of cycles done; both return with the
 * device work finished.  stream = NULL: the simulation runs on a stream of its own (the legacy null
 * stream cannot be captured into a hipGraph) and waits for the device at entry.  On one rank with
 * the fused stage a cycle can be captured once and replayed as a hipGraph with dt read from device
 * memory: <time>/cycle_graph = auto (default: 1-D packs, where it pays) | true | false;
 * AKMI_CYCLE_GRAPH=0/1 overrides the deck.
 * Pointers returned by akmi_sim_array stay valid for the lifetime of the simulation: inside a cycle the
 * driver trades its two registers (u0/u1, b0/b1) after the out-of-place first stage, and
 * akmi_sim_execute copies the state back into the register of that name before it returns whenever
 * an odd number of trades has happened (one device-to-device copy per call, not per cycle).
 * akmi_sim_profile(sim, 1): from now on a HIP event pair is recorded on the launch stream around every
 * akmi_*_stage_fused / akmi_*_stage_phase call (the dominant launch group of a stage);
 * akmi_sim_profile_read waits for the recorded events, returns their summed duration in ms and their
 * number, and clears the record (bench.py: roofline.ms_per_launch measured inside the timed loop). */
void *akmi_sim_create(const char *deck_text, void *stream);
int akmi_sim_initialize(void *sim, double tlim_override);
int akmi_sim_execute(void *sim, int max_cycles);
int akmi_sim_profile(void *sim, int on);
int akmi_sim_profile_read(void *sim, double *ms_total, long long *calls);
void akmi_sim_destroy(void *sim);
double akmi_sim_time(void *sim);
double akmi_sim_dt(void *sim);
double akmi_sim_tlim(void *sim);
int akmi_sim_ncycle(void *sim);
/* forms (AKMI_FORM_* mask) the given stage (1-based) took in the last cycle run; -1 when no such stage has run */
int akmi_sim_stage_forms(void *sim, int stage);
/* the three floor counters of the fluid's conversions (density, energy, temperature), as they stand on the device */
int akmi_sim_counters(void *sim, int *out3);
int akmi_sim_nmb(void *sim);
void *akmi_sim_array(void *sim, const char *name, long long *count);
const int *akmi_sim_lloc(void *sim);
int akmi_sim_gids(void *sim);            /* first global block id of this rank's pack */
int akmi_sim_nmb_thisrank(void *sim);

/* ---- ranks (global_variable::my_rank/nranks + the MPI calls of the reference's hot path:
 * one Isend/Irecv per peer rank and variable class, src/bvals/bvals.cpp:134-310,
 * bvals_cc.cpp:247-303; MPI_Allreduce(MIN) of dt, src/mesh/mesh.cpp:634-637) ------------------- *
 * akmi_comm_init_rccl: RCCL over xGMI, one GPU per rank (hipSetDevice before the call).  id = the
 * 128 bytes rank 0 obtained from akmi_comm_unique_id and handed to every rank by whatever launched
 * the job (MPI_Bcast, a torch.distributed store, a file).  Messages are ncclSend/ncclRecv pairs
 * grouped per variable class on the communicator's own stream, ordered against the compute stream
 * with events; dt is reduced with ncclAllReduce(ncclMin).  akmi_comm_init_env does the same for a
 * job started with RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment (the torchrun
 * convention): rank 0 serves the id on MASTER_PORT+1 over TCP.
 * akmi_comm_init_callbacks: any other transport.  exchange() receives HOST buffers (the library
 * stages device data through pinned memory) and returns when all npeer receives are complete;
 * allreduce_min() reduces n host doubles in place over all ranks.
 * All return AKMI_COMPLETE or AKMI_FAIL (akmi_last_error()).  akmi_comm_finalize releases the
 * communicator; akmi_sim_create reads the rank layout at the time it is called. */
typedef int (*akmi_comm_exchange_fn)(void *user, int npeer, const int *peers,
                                     const double *const *sendptr, const long long *sendcount,
                                     double *const *recvptr, const long long *recvcount);
typedef int (*akmi_comm_allreduce_min_fn)(void *user, double *vals, int n);
int akmi_comm_unique_id(char id[128]);
int akmi_comm_init_rccl(int rank, int nranks, const char id[128]);
int akmi_comm_init_env(void);
int akmi_comm_init_callbacks(int rank, int nranks, akmi_comm_exchange_fn exchange,
                             akmi_comm_allreduce_min_fn allreduce_min, void *user);
int akmi_comm_finalize(void);
/* min over all ranks of n <= 8 host doubles, in place (RCCL: ncclAllReduce on `stream`) */
int akmi_comm_allreduce_min(double *vals, int n, void *stream);
int akmi_comm_rank(void);
int akmi_comm_nranks(void);
/* Where a multi-rank stage spends its exchange (src/bvals/bvals_cc.cpp:108-135,247-258 pack / send / receive / unpack,
 * src/mesh/mesh.cpp:634-637 the dt reduction): akmi_comm_profile(1) starts recording HIP event pairs on the compute stream
 * round (0) the pack kernels of the off-rank segments, (1) the point where the compute stream waits for the receives of a
 * channel -- the time it really stalls there, zero when the transfer finished under the kernels enqueued before it --,
 * (2) the unpack kernels, (3) the dt all-reduce + read-back of a cycle.  akmi_comm_profile_read waits for the recorded
 * events, clears the record and fills out[0..11] = {pack_ms, pack_calls, exposed_wait_ms, wait_calls, unpack_ms,
 * unpack_calls, dt_reduce_ms, dt_calls, bytes_sent, posts, peers (most per post), ranks the communicator reports
 * (ncclCommCount; 0 without RCCL)}.  n = capacity of out (>= 12). */
int akmi_comm_profile(int on);
int akmi_comm_profile_read(double *out, int n);
/* The exchange plan rank `rank` of `nranks` derives from the deck alone -- host code only, no
 * device needed (tests/test_host_plan.py compares it with the Python host's plan).  fc = 0: the
 * cell-centred channel with nvar variables, 1: the face-centred channel.  out (capacity cap,
 * long long) receives: npeer, peers[npeer], {send_a, send_b, recv_a, recv_b}[npeer], nmb,
 * tab[nmb*27], nsend, send_tab[nsend*2], send_off[nsend], nseg, seg_off[nseg].  Returns the
 * number of entries needed (call again with a larger buffer if > cap), or -1 on error. */
long long akmi_host_exchange_plan(const char *deck_text, int rank, int nranks, int nvar, int fc,
                                  long long *out, long long cap);
/* Bytes of device memory the host's arrays (akmi_sim_*) hold in this process; 0 once every simulation is destroyed. */
long long akmi_host_device_bytes(void);

/* ---- measurement utility ------------------------------------------------------------ *
 * dst[i] = src[i] for n doubles with the library's own access pattern (8 B per lane,
 * 512 B per wave, grid-stride): a kernel of KNOWN traffic (8n read + 8n written) used to
 * calibrate the rocprofv3 FETCH_SIZE/WRITE_SIZE counters on gfx950 (tools/pmc.sh). */
int akmi_calib_copy(double *dst, const double *src, long long n, void *stream);

/* ---- arithmetic self-test ------------------------------------------------------------- *
 * The stage kernels evaluate sqrt(x), 1/x and x/dx (dx a power of two) with shorter instruction
 * sequences than the compiler's expansions (csrc/akmi_numerics.hpp: sqrt_x, rcp_x; pow2_shift);
 * these must return the same bits, because the path is bit-comparable with the reference's CPU
 * build (src/eos/eos.hpp:49-57, src/mhd/rsolvers/hlld_mhd.hpp:120-160, src/mhd/mhd_update.cpp:57-80
 * are the expressions concerned).  mode 0: sqrt, 1: reciprocal, 2: division by a power of two.
 * n operands (random in- and out-of-window patterns + a fixed edge table) are evaluated both ways on
 * the device; *mismatch receives the number of operands whose results differ in any bit,
 * *shortform_waves (may be NULL) the number of wave-iterations that really ran the short form. */
int akmi_selftest_fp64(int mode, long long n, unsigned long long seed, long long *mismatch,
                       long long *shortform_waves, void *stream);

/* ---- driven turbulence, <turb_driving> (src/srcterms/turb_driver.cpp) -------------------- *
 * csrc/akmi_turb.hip.  Host-only entries (no GPU needed): the random generator, the mode list and
 * amplitude table of InitializeModes, the sin/cos tables at cell centres.  Device entries, per cycle:
 *   akmi_turb_synthesize      force_tmp = sum over modes (one pass), partial[m][4] = sum rho, sum rho*f1..3
 *   akmi_turb_moments         force_tmp -= (t1,t2,t3)/t0, partial[m][2] = sum rho|f|^2, sum m.f
 *   akmi_turb_add_forcing     force = fcorr*force + gcorr*(s*force_tmp); m += rho*f*dt (rho from u0);
 *                             partial[m][4] = sum rho, sum m1..3 after the push
 *   akmi_turb_remove_net_mom  m -= rho*t_c/t0
 * force and force_tmp are (nmb, 3, N3, N2, N1) device arrays; only active cells are written.  partial[m][K]
 * are per-MeshBlock sums over the active cells by a fixed-shape tree (no floating-point atomics); the caller
 * sums them over all MeshBlocks in gid order.  work: akmi_turb_workspace_bytes() of device memory. */
#define AKMI_RNG_NTAB 32
/* RNG_State (src/utils/random.hpp:26-34); the cached second Gaussian deviate is iset/gset of the state */
typedef struct akmi_rng_state {
  long long idum, idum2, iy;
  long long iv[AKMI_RNG_NTAB];
  int iset;
  double gset;
} akmi_rng_state;
/* ran2 (L'Ecuyer + Bays-Durham shuffle): uniform deviate in (0,1); idum < 0 (re)initialises */
double akmi_rng_uniform(akmi_rng_state *st);
/* Marsaglia polar Box-Muller on akmi_rng_uniform: standard normal deviate */
double akmi_rng_gaussian(akmi_rng_state *st);
int akmi_rng_state_bytes(void);            /* sizeof(akmi_rng_state): 296 */
/* number of modes of (nlow, nhigh, driving_type 0|1), or AKMI_FAIL */
int akmi_turb_mode_count(int nlow, int nhigh, int driving_type);
/* one draw of InitializeModes (turb_driver.cpp:389-604): kvec[n][3] = (kx,ky,kz) and amp[n][24] (x, y, z
 * components, each ccc ccs csc css scc scs ssc sss for the x-, y-, z-trig factors), normalised; either may be
 * NULL (amp NULL: no deviates drawn).  lx, ly, lz: mesh extents.  Returns the mode count or AKMI_FAIL. */
int akmi_turb_amplitudes(int nlow, int nhigh, int driving_type, double expo, double exp_prp, double exp_prl,
                         double lx, double ly, double lz, akmi_rng_state *rstate, double *kvec, double *amp);
/* host tables x?(m,n,i) [nmb][nmode][nx1], y? [..][nx2], z? [..][nx3] of sin/cos(k*x) at the cell centres of
 * the active cells; bounds[m][6] = x1min x1max x2min x2max x3min x3max of each block; a collapsed dimension
 * gets sin 0, cos 1 (turb_driver.cpp:226-270) */
int akmi_turb_tables(int nmb, int nmode, int nx1, int nx2, int nx3, const double *kvec, const double *bounds,
                     double *xs, double *xc, double *ys, double *yc, double *zs, double *zc);
long long akmi_turb_workspace_bytes(const akmi_pack *p);
int akmi_turb_synthesize(const akmi_pack *p, int nmode, const double *amp, const double *xs, const double *xc,
                         const double *ys, const double *yc, const double *zs, const double *zc, const double *u0,
                         double *force_tmp, double *partial, double *work, void *stream);
int akmi_turb_moments(const akmi_pack *p, double t0, double t1, double t2, double t3, const double *u0,
                      double *force_tmp, double *partial, double *work, void *stream);
int akmi_turb_add_forcing(const akmi_pack *p, double fcorr, double gcorr, double s, double dt,
                          const double *force_tmp, double *force, double *u0, double *partial, double *work,
                          void *stream);
int akmi_turb_remove_net_mom(const akmi_pack *p, double t0, double t1, double t2, double t3, double *u0,
                             void *stream);

/* ---- physical source terms, <hydro_srcterms> / <mhd_srcterms> (src/srcterms/srcterms.cpp) ---------- *
 * csrc/akmi_srcterms.hip.  The parameters of the enabled terms in one plain struct; the three unit factors are
 * formed on the host with the reference's expressions (srcterms.cpp:149-154) from <units>:
 *   temp_unit    = temperature_cgs()
 *   cooling_unit = pressure_cgs()/time_cgs()/n_unit/n_unit,   n_unit = density_cgs()/mu()/atomic_mass_unit_cgs
 *   heating_unit = pressure_cgs()/time_cgs()/n_unit
 * They are read only with ism_cooling != 0. */
typedef struct akmi_srcterms {
  int const_accel;         /* constant acceleration on/off */
  int const_accel_dir;     /* 1, 2 or 3 */
  int ism_cooling;         /* optically thin ISM cooling + heating on/off (ideal gas only) */
  int reserved;
  double const_accel_val;  /* g */
  double hrate;            /* heating rate [erg/s] */
  double gamma;            /* adiabatic index of the EOS */
  double temp_unit, cooling_unit, heating_unit;
} akmi_srcterms;
/* SourceTerms::ApplySrcTerms (srcterms.cpp:93-101): one launch applies the enabled terms to the active cells of all
 * MeshBlocks, reading the OLD primitives w0 and updating u0 in place, constant acceleration first, then cooling, each
 * value with the reference's sequence of roundings.  bdt = beta*dt with dt read from dt_dev[0] when dt_dev is not
 * NULL (the form of akmi_*_stage_phase_dt: run-ahead cycles and captured cycle graphs), else the argument dt.
 * Ghost zones are not touched.  Nothing enabled: no launch. */
int akmi_srcterms_apply(const akmi_pack *p, const akmi_srcterms *s, double beta, double dt, const double *dt_dev,
                        const double *w0, double *u0, void *stream);
/* SourceTerms::NewTimeStep (srcterms_newdt.cpp:25-72): *dtmin (device) = min over the active cells of
 * eint/(FLT_MIN + |rho*(rho*lambda - gamma_heating)|), starting from (double)FLT_MAX (which is what it stays at
 * without ism_cooling). */
int akmi_srcterms_newdt(const akmi_pack *p, const akmi_srcterms *s, const double *w0, double *dtmin, void *stream);
/* Host-only (no GPU needed): how the C++ host reads the source-term block of `fluid` ("hydro" or "mhd") of a deck --
 * keys, defaults and the unit factors from <units>.  Returns 1 and fills *out when the deck holds <fluid_srcterms>,
 * 0 when it does not; a deck the host refuses ends the process with "### FATAL ERROR", as akmi_sim_create does. */
int akmi_srcterms_from_deck(const char *deck_text, const char *fluid, akmi_srcterms *out);

/* ---- derived output variables (BaseTypeOutput::ComputeDerivedVariable, src/outputs/derived_variables.cpp) ---- *
 * csrc/akmi_derived.hip.  `which` selects the variable; every one of them has one component.  Centred differences of
 * w0 (vorticity) or bcc0 (current, curvature), face differences of the field (div B). */
enum { AKMI_DV_TEMPERATURE = 0,  /* eint/dens of w0 (ideal gas only)                        derived_variables.cpp:98   */
       AKMI_DV_WZ = 1,           /* hydro_wz, mhd_wz       z-vorticity                                          :119  */
       AKMI_DV_W2 = 2,           /* hydro_w2, mhd_w2       vorticity squared                                    :139  */
       AKMI_DV_JZ = 3,           /* mhd_jz                 z-current from bcc0                                  :167  */
       AKMI_DV_J2 = 4,           /* mhd_j2                 current squared                                      :185  */
       AKMI_DV_CURV = 5,         /* mhd_curv               |(B.grad B).(I - bb)|/B^2                            :212  */
       AKMI_DV_K_JXB = 6,        /* mhd_k_jxb              |j x B|/B^2                                          :781  */
       AKMI_DV_CURV_PERP = 7,    /* mhd_curv_perp          |j x B/B^2 - b.grad b|                               :819  */
       AKMI_DV_BMAG = 8,         /* mhd_bmag               |bcc0|                                               :929  */
       AKMI_DV_DIVB = 9 };       /* mhd_divb               from the face fields, ghost cells included           :1046 */
/* number of components of the variable (1 for all of the above), -1 for an unknown `which` */
int akmi_derived_ncomp(int which);
/* out = (nmb, ncomp_out, N3, N2, N1) in the pack's layout, ncomp_out = akmi_derived_ncomp(which).  One launch for all
 * MeshBlocks writes EVERY element of out: the variable over the index range of the reference's loop (the active cells;
 * the whole array for div B), zero elsewhere -- what the reference's freshly allocated array holds there.  Each value
 * carries the reference's sequence of roundings.  The arrays a variable does not read may be NULL (w0 for 0-2, bcc0 for
 * 3-8, the face fields for 9); u0 is not read by the present variables.  On 1-D / 2-D meshes the two curvature
 * variables take the differences across the missing directions as zero (the reference reads out of bounds there). */
int akmi_derived_var(const akmi_pack *p, int which, const double *w0, const double *u0, const double *bcc0,
                     const double *bx1f, const double *bx2f, const double *bx3f, double *out, int ncomp_out,
                     void *stream);
/* the same on the arrays of a simulation of the C++ host, on its stream: `out` is a device array of
 * nmb_thisrank * N3 * N2 * N1 doubles; the call returns when it is written. */
int akmi_sim_derived(void *sim, int which, double *out);

/* ---- run-time statistics: turbulence history columns and pdf outputs -------------------------------------------- *
 * csrc/akmi_stats.hip; the per-cell arithmetic in csrc/akmi_stats.hpp.
 *
 * akmi_turb_history: the eleven sums of TurbulentHistory (src/pgen/fluids/turb.cpp:247-396) over the active cells of an
 * MHD pack, as per-MeshBlock partials partial[m][11] in the order
 *   Bx By Bz B^2 B^4 dB^2 BdB^2 |BxJ|^2 |B.J|^2 U^2 dU
 * (the first three are sums of the bare components, NOT weighted by the cell volume: turb.cpp:294-296).  The sums are
 * deterministic: fixed-shape trees over tiles of 1024 cells and over the tiles of a MeshBlock, no atomics; the caller adds
 * the partials over all MeshBlocks in gid order.  Reads one ghost layer of bcc0 and w0 (filled by ConToPrim, the last task
 * of a stage).  On 1-D / 2-D meshes the cell-centred neighbour in a direction the mesh does not have is the cell itself.
 * work: akmi_turb_history_workspace_bytes() of device memory. */
#define AKMI_TURB_NHIST 11
long long akmi_turb_history_workspace_bytes(const akmi_pack *p);
int akmi_turb_history(const akmi_pack *p, const double *w0, const double *bcc0, const double *bx1f, const double *bx2f,
                      const double *bx3f, double *partial, double *work, void *stream);
/* the same on the arrays of a simulation of the C++ host (MHD only), on its stream: sums[11] (host) are the sums over ALL
 * MeshBlocks of the mesh in gid order; with ranks, the partials travel as an 11 x nmb_total array reduced with
 * all-reduce(min) against +inf, so every rank adds the same numbers in the same order. */
int akmi_sim_turb_history(void *sim, double *sums);

/* akmi_pdf: volume- or mass-weighted 1-D / 2-D histogram of the active cells (PDFOutput::LoadOutputData,
 * src/outputs/pdf.cpp:244-287).  One axis: the variable as (device array of nvar variables per MeshBlock in the pack's
 * layout, component), nbin bins, the first and the last edge bins(0), bins(nbin) as the host formed them (pdf.cpp:82-93) and
 * the step (pdf.cpp:100-102).  A value below bin_lo goes to bin 0, one >= bin_hi to bin nbin+1, any other to
 * int((x - bin_lo)/step) + 1, or int(log10(x/bin_lo)/step) + 1 with logscale. */
typedef struct akmi_pdf_axis {
  const double *array;
  int nvar, comp;
  int nbin, logscale;
  double bin_lo, bin_hi, step;
} akmi_pdf_axis;
/* y may be NULL (1-D).  counts and weights: device arrays [(y->nbin+2) | 1][x->nbin+2], cleared by the call; the weight of
 * a cell is dx1*dx2*dx3 of its MeshBlock, times u0_mass(m, IDN, k, j, i) when u0_mass (the conserved array of the pack,
 * nvar variables) is not NULL.  A cell with a NaN value belongs to no bin: it is dropped and counted in *nan_count (device).
 * While the histogram has at most AKMI_PDF_LDS_BINS entries every workgroup accumulates a private copy in LDS and adds its
 * non-zero bins to the result at the end; larger histograms, or force_global != 0 (or AKMI_PDF_FORCE_GLOBAL=1 in the
 * environment, for A/B runs), add every cell to the result in global memory.  Counts are exact; the fp64 weights are sums
 * in arrival order and can differ in their last bits from run to run. */
#define AKMI_PDF_LDS_BINS 4096
int akmi_pdf(const akmi_pack *p, const akmi_pdf_axis *x, const akmi_pdf_axis *y, const double *u0_mass,
             unsigned long long *counts, double *weights, unsigned long long *nan_count, int force_global,
             void *stream);
int akmi_pdf_lds_bins(void);      /* AKMI_PDF_LDS_BINS of the library */
/* the same on the arrays of a simulation of the C++ host, on its stream, for THIS rank's MeshBlocks.  An axis with
 * array == NULL names a stored array by nvar: 0 = u0, 1 = w0, 2 = bcc0 (comp the variable); mass_weighted != 0 weights
 * with u0(IDN).  The call returns when the three outputs are written. */
int akmi_sim_pdf(void *sim, const akmi_pdf_axis *x, const akmi_pdf_axis *y, int mass_weighted,
                 unsigned long long *counts, double *weights, unsigned long long *nan_count, int force_global);

/* ---- coarsened binary outputs (file_type = cbin) ------------------------------------------------------------------ *
 * csrc/akmi_coarsen.hip; the per-cell arithmetic in csrc/akmi_coarsen.hpp.
 *
 * akmi_coarsen: the mean over factor^3 fine cells of every variable of the table, for every MeshBlock of the pack, in one
 * launch (CoarsenedBinaryOutput::LoadOutputData, src/outputs/coarsened_binary.cpp:174-290); with moments != 0 also the
 * means of x*x, (x*x)*x and ((x*x)*x)*x.  A variable is (device array of nvar variables per MeshBlock in the pack's
 * layout (nmb, nvar, N3, N2, N1), component); a derived scratch array is nvar = 1. */
typedef struct akmi_coarsen_var {
  const double *array;
  int nvar, comp;
} akmi_coarsen_var;
/* lo = {ois, ojs, oks}: the first fine cell of the output range in the array; nc = {nc1, nc2, nc3}: the coarse extents
 * (lo[d] >= 0 and lo[d] + nc[d]*factor <= N[d] are checked).  out = (nvars*nmom, nmb, nc3, nc2, nc1) in fp64, nmom = 1 or
 * 4: the moments of a variable are adjacent, then the MeshBlock (the reference's outarray).  Every element is written.
 * The value of coarse cell (kc, jc, ic) is bit-defined: accumulators start at +0.0 and take the fine cells
 * (lo3 + kc*f + kk, lo2 + jc*f + jj, lo1 + ic*f + ii) in ascending kk, then jj, then ii, and are divided by (double)(f*f*f).
 * staged = 0: one thread per coarse cell reads global memory at stride f; 1: the workgroup stages fine row segments in LDS
 * with contiguous loads; < 0: AKMI_COARSEN_STAGED of the environment (0|1, for A/B runs), else the library's default.
 * Both forms give the same bits. */
#define AKMI_COARSEN_DEFAULT_STAGED 1
int akmi_coarsen(const akmi_pack *p, const akmi_coarsen_var *vars, int nvars, int factor, int moments, const int *lo,
                 const int *nc, double *out, int staged, void *stream);
int akmi_coarsen_default_staged(void);      /* AKMI_COARSEN_DEFAULT_STAGED of the library */
/* the same on the arrays of a simulation of the C++ host, on its stream, for THIS rank's MeshBlocks.  A variable with
 * array == NULL names a stored array by nvar: 0 = u0, 1 = w0, 2 = bcc0 (comp the variable).  The call returns when out is
 * written. */
int akmi_sim_coarsen(void *sim, const akmi_coarsen_var *vars, int nvars, int factor, int moments, const int *lo,
                     const int *nc, double *out, int staged);

/* ---- adaptive mesh refinement (akmi_amr.hip) ------------------------------------------------
 * Refinement criteria, RefinementCriteria::CheckMinMax / CheckSlope / CheckSecondDeriv
 * (src/mesh/refinement_criteria.cpp:177-338): one launch per criterion, one workgroup per MeshBlock.  q is one
 * variable of a device array in the pack's layout; MeshBlock m starts at q + m*mstride and holds (N3, N2, N1)
 * doubles.  The extremum over the ACTIVE cells of q (min_max), 0.5*sqrt(sum_d (q+ - q-)^2)/q (slope) or
 * |sum_d (q+ - 2q + q-)|/q (second_deriv) is compared on the device and flags[m] (device, nmb ints) updated as the
 * reference does, so criteria applied one after the other compose: max > value_max -> 1; max < value_max and
 * flag == 0 -> -1; equality leaves the flag.  value_max >= FLT_MAX: not checked.  min_max only: value_min > -FLT_MAX
 * checks the MINIMUM the same way (min < value_min -> 1; min > value_min and flag == 0 -> -1), after the maximum. */
#define AKMI_AMR_MIN_MAX 0
#define AKMI_AMR_SLOPE 1
#define AKMI_AMR_SECOND_DERIV 2
int akmi_amr_check(const akmi_pack *p, int method, const double *q, long long mstride, double value_min,
                   double value_max, int *flags, void *stream);
/* Regrid, out of place: the arrays of the new pack from those of the old one (same MeshBlock sizes, other nmb).
 * plan (device): one row of three ints per NEW MeshBlock, {kind, old, octant}.
 *   kind  0: the whole block, ghost zones included, is a copy of old block `old` (MeshRefinement::CopyCC/FC);
 *   kind -1: the active region (faces: its upper plane included) is the restriction of the nleaf old blocks
 *            old .. old+nleaf-1, child l into octant l (RestrictCC/FC + DerefineCC/FCSameRank,
 *            src/mesh/mesh_refinement.cpp:696-810,1223-1382); a plane shared by two octants takes the higher one's;
 *   kind +1: the active region is the prolongation of octant `octant` (ox1 + 2*ox2 + 4*ox3) of old block `old`,
 *            whose cells around the octant (its ghost zones where the octant ends at the block's edge) are the
 *            coarse stencil (CopyForRefinementCC/FC + RefineCC/FC, :919-1182): slope-limited for cells; for
 *            faces the shared faces first, then the internal ones by the Toth & Roe operator (1-D: the mean).
 * Everything else of the new arrays is left as it is.  A row that points outside the old pack writes nothing. */
int akmi_amr_regrid_cc(const akmi_pack *old_pack, const akmi_pack *new_pack, int nvar, const int *plan,
                       const double *u_old, double *u_new, void *stream);
int akmi_amr_regrid_fc(const akmi_pack *old_pack, const akmi_pack *new_pack, const int *plan, const double *b_old1,
                       const double *b_old2, const double *b_old3, double *b_new1, double *b_new2, double *b_new3,
                       void *stream);
/* MeshRefinement::RepairAMRFC (:1189-1220): the internal faces of every MeshBlock m with repair[m] > 0 (device,
 * nmb ints, 0 or 1; a negative entry is not a flag) recomputed from its present shared faces */
int akmi_amr_repair_fc(const akmi_pack *p, const int *repair, double *bx1f, double *bx2f, double *bx3f,
                       void *stream);

/* ---- two-fluid (ion-neutral) MHD, implicit part of the ImEx integrators (akmi_ionn.hip) -----
 * IonNeutral::ImpRKUpdate, src/ion-neutral/ion-neutral_tasks.cpp:144-292, in ONE launch over every cell of the pack
 * (ghost zones included).  ui = ion (MHD) u0, (nmb, nvar_i, ncell); un = neutral (hydro) u0, (nmb, nvar_n, ncell);
 * ru = Driver::impl_src, (nimp_stages, nmb, 8, ncell); ncell = N1*N2*N3 of a MeshBlock.  Only the planes IDN, IM1..IM3
 * of ui / un are read or written.  istage = estage + 2 = 1 .. nimp_stages+1.  Per cell, in this order:
 *  (a) for s = 0 .. istage-2, ascending: the eight values += adt[s]*ru[s] (adt: HOST array of istage-1 doubles,
 *      a_twid[istage-2][s]*dt; may be NULL for istage = 1).  An s with adt[s] == 0.0 exactly is skipped: its slab is
 *      not read (the reference adds 0.0*ru[s]; the results compare equal, a -0.0 keeps its sign);
 *  (b) do_solve != 0 (the reference's estage < nexp_stages): the analytic solution of the implicit equations with
 *      gamma_adt, xi_adt, alpha_adt (the sqrt branch iff alpha_adt > 0);
 *  (c) do_solve != 0: ru[istage-1] = R(U) of the values of (b), with drag_coeff, ionization_coeff, recombination_coeff.
 * Every other plane of ui / un and every other slab of ru is left as it is.  A call with nothing to do (do_solve == 0
 * and all coefficients zero) launches nothing. */
int akmi_ionn_imp_update(int nmb, long long ncell, int nvar_i, int nvar_n, int nimp_stages, int istage, int do_solve,
                         const double *adt, double gamma_adt, double xi_adt, double alpha_adt, double drag_coeff,
                         double ionization_coeff, double recombination_coeff, double *ui, double *un, double *ru,
                         void *stream);

/* ---- self-gravity: multigrid Poisson solver and its source term (akmi_mg.hip) ------------------
 * One MG level is an array (nmb, 1, nz+2, ny+2, nx+2) of doubles: (nz, ny, nx) active cells and ONE ghost layer
 * (mg_nghost = 1).  The MeshBlock levels have nz = ny = nx; the root grid is the same with nmb = 1.  dx is the cell
 * width OF THAT LEVEL (block_rdx * 2^ll, multigrid.hpp:638).  Every operator keeps the roundings of the reference
 * lines named with it and writes nothing but what is said. */
/* Multigrid::Smooth + GravityStencil (multigrid.hpp:622-647, mg_gravity.hpp:25-36): the active cells with
 * i = 1 + c, 3 + c, ..., c = ((color ^ coffset) + k + j) & 1 (k, j: array indices): u -= (lap - src*dx^2)*(omega/6) */
int akmi_mg_smooth(int nmb, int nz, int ny, int nx, double dx, double omega, int color, int coffset, double *u,
                   const double *src, void *stream);
/* CalculateDefect / CalculateFASRHS (multigrid.hpp:271-312), active cells: def = src - lap*(1/(dx*dx));
 * src += lap*(1/(dx*dx)) */
int akmi_mg_defect(int nmb, int nz, int ny, int nx, double dx, const double *u, const double *src, double *def,
                   void *stream);
int akmi_mg_fas_rhs(int nmb, int nz, int ny, int nx, double dx, const double *u, double *src, void *stream);
/* (nz, ny, nx) are the active cells of the COARSE level in the next three; the fine level has twice as many.
 * Restrict (multigrid.cpp:874-894): coarse active cells; ProlongateAndCorrect, trilinear (:1053-1092): fine active
 * cells +=, reads the coarse ghosts; FMGProlongate, tricubic (:1116-1218): fine active cells =, reads coarse ghosts */
int akmi_mg_restrict(int nmb, int nz, int ny, int nx, const double *fine, double *coarse, void *stream);
int akmi_mg_prolongate_correct(int nmb, int nz, int ny, int nx, const double *coarse, double *fine, void *stream);
int akmi_mg_fmg_prolongate(int nmb, int nz, int ny, int nx, const double *coarse, double *fine, void *stream);
/* StoreOldData (uold = u), ComputeCorrection (u -= uold), ZeroClearData, CopySourceToData (u = src): all n cells */
int akmi_mg_store_old(long long n, double *uold, const double *u, void *stream);
int akmi_mg_correction(long long n, double *u, const double *uold, void *stream);
int akmi_mg_zero_clear(long long n, double *u, void *stream);
int akmi_mg_copy_source(long long n, double *u, const double *src, void *stream);
/* LoadSource (multigrid.cpp:289-320): src(all cells, ghosts included) = u0(variable 0)*fac, u0 (nmb, nvar, n+2ng..);
 * LoadFinestData (:261-281): u(active) = phi; RetrieveResult (:420-451): phi(n+2 cells per direction) = u.
 * phi: (nmb, 1, nz+2ng, ny+2ng, nx+2ng) */
int akmi_mg_load_source(int nmb, int nz, int ny, int nx, int ng, int nvar, double fac, const double *u0, double *src,
                        void *stream);
int akmi_mg_load_finest(int nmb, int nz, int ny, int nx, int ng, const double *phi, double *u, void *stream);
int akmi_mg_retrieve(int nmb, int nz, int ny, int nx, int ng, const double *u, double *phi, void *stream);
/* The sums have one order: a row (m, k, j) ascending in i, the rows of a plane ascending in j, the planes of a block
 * ascending in k, the blocks ascending in m.  scratch: akmi_mg_reduce_scratch_doubles() doubles; out: one double.
 * CalculateAverage (multigrid.cpp:763-818): sum(a*dx^3)/(nmb*len^3), len = edge of a block as the reference forms it;
 * SubtractAverage (:824-852): a[0..n) -= *ave; defect norm, l2 (:683-757, multigrid_driver.cpp:908-937):
 * sqrt(sum(def^2)/vol) */
long long akmi_mg_reduce_scratch_doubles(int nmb, int nz, int ny, int nx);
int akmi_mg_average(int nmb, int nz, int ny, int nx, double dx, double len, const double *a, double *scratch,
                    double *out, void *stream);
int akmi_mg_subtract_average(long long n, double *a, const double *ave, void *stream);
int akmi_mg_defect_norm(int nmb, int nz, int ny, int nx, double vol, const double *def, double *scratch, double *out,
                        void *stream);
/* periodic ghost exchange of one level, one launch: every ghost cell (faces, edges, corners) = the active cell it is
 * the image of in MeshBlock nghbr[m*27 + (ox3+1)*9 + (ox2+1)*3 + (ox1+1)] (device ints; the block itself where it is
 * its own neighbour; < 0: left alone).  MGRootBoundary for periodic faces is the same with the grid as its own
 * neighbour everywhere (multigrid_driver.cpp:1835-1930). */
int akmi_mg_exchange(int nmb, int nz, int ny, int nx, const int *nghbr, double *u, void *stream);
int akmi_mg_root_boundary(int nz, int ny, int nx, double *u, void *stream);
/* Boundary types of the non-periodic faces of the mesh, <gravity>/mg_bc */
#define AKMI_MGBC_NONE 0
#define AKMI_MGBC_ZEROFIXED 1
#define AKMI_MGBC_ZEROGRAD 2
#define AKMI_MGBC_MULTIPOLE 3
/* akmi_mg_exchange plus MultigridDriver::PhysicalBoundary (multigrid_tasks.cpp:129-360) in the same launch.  A block
 * has a physical face where the FACE entry of its neighbour table is < 0.  zerofixed / zerograd: a ghost cell is
 * mirrored in every direction in which it lies beyond a physical face, takes the neighbour's image in the others, and
 * is multiplied by -1 per mirrored direction under zerofixed (the composite of the reference's x1, x2, x3 sweeps over
 * the full extent).  multipole: a face ghost over active cells = 2*phis - interior, phis = EvalMultipolePhi
 * (multigrid.hpp:680-708) at the face and the cell centres of THIS level, from the block extents xlim (device,
 * nmb*6: x1min, x1max, x2min, ...) and mp (device, 28 doubles: 25 scaled coefficients, then the origin x, y, z); edge
 * and corner ghosts that touch a physical face are left alone.  bc_type none: physical-face ghosts are left alone.
 * mp and xlim may be NULL for the mirror types.  Reads active cells, writes ghost cells. */
int akmi_mg_exchange_bc(int nmb, int nz, int ny, int nx, const int *nghbr, int bc_type, int mporder, const double *mp,
                        const double *xlim, double *u, void *stream);
/* MGRootBoundary (multigrid_driver.cpp:1835-2026) in one launch: periodic[f] != 0 (host; ix1, ox1, ix2, ox2, ix3, ox3)
 * = periodic face, the others have bc_type.  The mirror types equal the reference's x1, x2, x3 sequence; multipole
 * faces use mesh_ext (host: x1min, x1max, ...) and the cell count of this level, and edge and corner ghosts that touch
 * a multipole face are left alone. */
int akmi_mg_root_boundary_bc(int nz, int ny, int nx, int bc_type, const int periodic[6], int mporder, const double *mp,
                             const double mesh_ext[6], double *u, void *stream);
/* CalculateCenterOfMass (auto_origin != 0: mp[25..27] = 1/m0 * (m3, m1, m2); otherwise mp[25..27] is read) and
 * CalculateMultipoleCoefficients + ScaleMultipoleCoefficients (multigrid_driver.cpp:2213-2434) of the active cells of
 * src: mp[0..8] (mporder 2) or mp[0..24] (4).  Sums in the order of akmi_mg_average; scratch: 25 *
 * akmi_mg_reduce_scratch_doubles() doubles.  4 launches, 8 with auto_origin; nothing is read back. */
int akmi_mg_multipole_moments(int nmb, int nz, int ny, int nx, int mporder, int nodipole, int auto_origin,
                              const double *xlim, const double *src, double *scratch, double *mp, void *stream);
/* Multigrid::ApplyMask (multigrid.cpp:360-388): src = 0 on the active cells with r^2 > mask_radius^2 about
 * (ox, oy, oz), cell centres by CellCenterX from xlim; mask_radius <= 0 launches nothing */
int akmi_mg_mask(int nmb, int nz, int ny, int nx, const double *xlim, double mask_radius, double ox, double oy, double oz,
                 double *src, void *stream);
/* TransferFromBlocksToRoot (multigrid_driver.cpp:479-548) / SetFromRootGrid (multigrid.cpp:617-676): (nz, ny, nx) the
 * root grid, lloc device ints (lx1, lx2, lx3) per block; the blocks' arrays are those of the 1-cell level (27 doubles
 * per block).  initflag: the source alone; folddata: uold too */
int akmi_mg_blocks_to_root(int nmb, int nz, int ny, int nx, const int *lloc, int initflag, const double *bsrc,
                           const double *bu, double *rsrc, double *ru, void *stream);
int akmi_mg_set_from_root(int nmb, int nz, int ny, int nx, const int *lloc, int folddata, const double *ru,
                          const double *ruold, double *bu, double *buold, void *stream);
/* SourceTerms::SelfGravity (srcterms.cpp:215-310), one launch, per cell x1 then x2 then x3.  phi: (nmb, 1, cells of
 * the pack); flx*: the mass fluxes are variable 0 of the flux arrays of the task-granular path, face_shaped != 0:
 * (.., n1+1) / (.., n2+1, n1) / (n3+1, ..); read for the ideal gas only */
int akmi_mg_selfgravity(const akmi_pack *p, int face_shaped, double bdt, const double *w0, const double *phi,
                        const double *flx1, const double *flx2, const double *flx3, double *u0, void *stream);

#define AKMI_MG_NNORMS 42
/* one rank, uniform mesh: the MeshBlocks tile the root grid nrx1 x nrx2 x nrx3 */
typedef struct akmi_mg_plan {
  int nmb, nxb;                        /* MeshBlocks of the pack; edge of a MeshBlock (power of two) */
  int nrx1, nrx2, nrx3;                /* root grid */
  int nmblevel, nrootlevel;            /* multigrid.cpp:100-145 */
  int ng, nvar;                        /* ghost cells and variables of the fluid's u0 (phi: same ng) */
  int npresmooth, npostsmooth, niter, full_multigrid, fmg_ncycle, subtract_average, show_defect;
  double rdx, root_dx;                 /* cell width of the finest block level / of the finest root level */
  double omega, four_pi_G, eps, vol;   /* eps: threshold (< 0: niter V-cycles); vol: volume of the mesh */
  const int *nghbr;                    /* device, nmb*27, as akmi_mg_exchange */
  const int *lloc;                     /* device, nmb*3 */
  double *ws;                          /* device, akmi_mg_workspace_doubles(); keeps u between calls */
  /* physical faces; all zero: six periodic faces, as before these fields existed */
  int mg_bc;                           /* AKMI_MGBC_*: the type of every non-periodic face */
  int periodic[6];                     /* ix1, ox1, ix2, ox2, ix3, ox3: != 0 = periodic face (read when mg_bc != none) */
  int mporder, nodipole, auto_mporigin;
  double mesh_ext[6];                  /* x1min, x1max, x2min, x2max, x3min, x3max of the mesh */
  double mporigin[3];                  /* the origin of the expansion unless auto_mporigin */
  double mask_radius, mask_origin[3];  /* > 0: the source is zeroed outside this radius */
  const double *xlim;                  /* device, nmb*6: extents of every MeshBlock (multipole, mask) */
} akmi_mg_plan;
long long akmi_mg_workspace_doubles(const akmi_mg_plan *plan);
/* offset (doubles) into ws of array `which` (0 u, 1 src, 2 def, 3 uold) of MeshBlock level / root level `level` */
long long akmi_mg_level_offset(const akmi_mg_plan *plan, int is_root, int level, int which);
/* MGGravityDriver::Solve (mg_gravity.cpp:177-245) enqueued as a whole: LoadSource(-four_pi_G), ApplyMask, the initial
 * guess from phi unless full_multigrid, SubtractAverage, under multipole the centre of mass and the scaled moments (on
 * the device, into ws), SolveFMG / SolveMG, RetrieveResult into phi.  With mg_bc != none every exchange and root
 * boundary is the _bc form, one launch each as before.  *coffset: the red-black offset, carried
 * from call to call.  norms (host, AKMI_MG_NNORMS doubles, -1 = not computed): [0] initial defect, [1 + n] after
 * V-cycle n of SolveMG (threshold >= 0, or show_defect >= 2), [41] final (show_defect >= 1).  *ncycles: V-cycles of
 * SolveMG; 40 with the last norm above eps = the reference's "Failed to converge".  The stream is synchronised only
 * where a norm is read. */
int akmi_mg_solve(const akmi_mg_plan *plan, const double *u0, double *phi, int *coffset, double *norms, int *ncycles,
                  void *stream);
/* offset (doubles) into ws of the 28 doubles akmi_mg_solve keeps under multipole: coefficients, then the origin */
long long akmi_mg_multipole_offset(const akmi_mg_plan *plan);
/* kernel launches this unit has enqueued since the last reset */
long long akmi_mg_launch_count(int reset);

/* ---- shearing box, cell-centred half (src/shearing_box/) ------------------------------------------------- *
 * csrc/akmi_sbox.hip.  The entries a hydro fluid uses (an MHD fluid uses them for its cell-centred variables); every entry
 * reproduces the reference's roundings in the written order.
 * xlim = device double[nmb][6]: x1min, x1max, x2min, x2max, x3min, x3max of every MeshBlock (mb_size).
 *
 * ShearingBoxCC::SourceTermsCC (shearing_box_srcterms.cpp:27-84) on the active cells: the 3-D branch when nx3 > 1, the
 * 2-D r-z branch otherwise; old primitives w0 in, u0 read-modify-written.  The host forms
 *   coef1 = 2.0*bdt*omega0,  coef2 = (2.0-qshear)*bdt*omega0,  coef3 = bdt*SQR(omega0),  qo = qshear*omega0
 * as the reference writes them.  stratified (3-D only) reads the x3 bounds of xlim (may be NULL otherwise). */
int akmi_sbox_srcterms(const akmi_pack *p, double coef1, double coef2, double coef3, double bdt, double qo, int stratified,
                       const double *xlim, const double *w0, double *u0, void *stream);
/* The shear-periodic x1 boundary of cell-centred variables, ShearingBoxCC::PackAndSendCC / RecvAndUnpackCC
 * (shearing_box_cc.cpp:48-266, :281-391) on one rank, both faces per launch.
 * tab = device int[2][nslot][tab_stride], tab_stride = 2 + nmbx2, per face (0 inner, 1 outer) and boundary MeshBlock:
 *   {local index of the MeshBlock, its lx2, slot of the MeshBlock at lx2 = 0, 1, .., nmbx2-1 on this face and this lx3};
 * nb_in / nb_out of the nslot slots of a face are used.  buf = device double[2][nslot][nvar][N3][nx2][ng].
 * remap_x1: buf(j) = a(j) - (flx(j+1) - flx(j)) for j in [js, je], all k (ghost planes included), of the x1 ghost slab,
 * eps = fmod(yshear, dx2)/dx2, negated on the outer face; the remap flux by recon: dc, plm, anything else PPMX.
 * shift_x1: every x1 ghost cell, all rows j of the MeshBlock, takes buf at global row g - joffset (inner face) /
 * g + joffset (outer face) modulo nmbx2*nx2, g = lx2*nx2 + (j - js); joffset = int(yshear/dx2) >= 0. */
int akmi_sbox_remap_x1(const akmi_pack *p, int recon, int nb_in, int nb_out, int nslot, const int *tab, int tab_stride,
                       double yshear, const double *u0, double *buf, void *stream);
int akmi_sbox_shift_x1(const akmi_pack *p, int nb_in, int nb_out, int nslot, const int *tab, int tab_stride, int nmbx2,
                       int joffset, const double *buf, double *u0, void *stream);
/* OrbitalAdvectionCC::RecvAndUnpackCC (orbital_advection_cc.cpp:215-288) on one rank: the active cells of `out` are u0
 * remapped along x2 by yshear = -qo*x1v*dt of their column (integer shift + conservative remap of the rest); u0 is
 * only read, the ghost cells of `out` are not written.  Rows beyond an x2 edge are the active rows of the x2 neighbour
 * of nghbr (device int[nmb][27], local indices; a MeshBlock may be its own neighbour).  The caller guarantees
 * nghost + maxjshift <= nx2 (checked) and |int(yshear/dx2)| <= maxjshift for every column (indices are clamped into
 * the arrays if it does not hold; the result is then wrong). */
int akmi_sbox_orbital_cc(const akmi_pack *p, int recon, int maxjshift, double qo, double dt, const int *nghbr,
                         const double *xlim, const double *u0, double *out, void *stream);

/* ---- shearing box, MHD and the face-centred half ---------------------------------------------------------- *
 * The MHD form of SourceTermsCC (shearing_box_srcterms.cpp:92-150): as akmi_sbox_srcterms, with the energy term
 * bdt*(mom1*mom2/den - bcc(IBX)*bcc(IBY))*qo (IBZ in the r-z branch); bcc0 = double[nmb][3][N3][N2][N1], read only for an
 * ideal gas. */
int akmi_sbox_srcterms_mhd(const akmi_pack *p, double coef1, double coef2, double coef3, double bdt, double qo,
                           int stratified, const double *xlim, const double *w0, const double *bcc0, double *u0,
                           void *stream);
/* ShearingBoxFC::SourceTermsFC (shearing_box_srcterms.cpp:159-200), 2-D meshes only: for j in [js, je+1], i in [is, ie+1]
 * e1 -= qo*x1v*b2 and e2 += qo*x1f*b1 at k = ks and ke+1, both from b at ks; x1v = CellCenterX, x1f = LeftEdgeX. */
int akmi_sbox_efield_2d(const akmi_pack *p, double qo, const double *xlim, const double *bx1f, const double *bx2f,
                        double *e1, double *e2, void *stream);
/* The shear-periodic x1 boundary of the face-centred field, ShearingBoxFC::PackAndSendFC / RecvAndUnpackFC
 * (shearing_box_fc.cpp) on one rank; tab as for akmi_sbox_remap_x1, buf = device double[2][nslot][3][N3][nx2][ng].
 * Inner face: all three components at ghost index i; outer face: x1f at (ie+2)+i, x2f and x3f at (ie+1)+i.  Planes
 * k in [0, N3) and, in shift_x1_fc, rows j in [0, N2): the last x2f row and the last x3f plane are not touched. */
int akmi_sbox_remap_x1_fc(const akmi_pack *p, int recon, int nb_in, int nb_out, int nslot, const int *tab, int tab_stride,
                          double yshear, const double *bx1f, const double *bx2f, const double *bx3f, double *buf,
                          void *stream);
int akmi_sbox_shift_x1_fc(const akmi_pack *p, int nb_in, int nb_out, int nslot, const int *tab, int tab_stride, int nmbx2,
                          int joffset, const double *buf, double *bx1f, double *bx2f, double *bx3f, void *stream);
/* OrbitalAdvectionFC::RecvAndUnpackFC (orbital_advection_fc.cpp:223-358) on one rank, 3-D meshes, two launches.
 * orbital_emf: emfx (from x3f, x1 = cell centre) and emfz (from x1f, x1 = left edge), double[nmb][N3][N2][N1], for
 * k in [ks, ke+1], j in [js, je+1], i in [is, ie+1]: the remap flux at face j - joffset and the whole cells of the integer
 * shift, yshear = -qo*x1*dt.  Rows beyond an x2 edge are the x2 neighbour's active rows (nghbr as for orbital_cc); the
 * same guarantees on maxjshift.  orbital_ct: the three CT differences, in place on the field. */
int akmi_sbox_orbital_emf(const akmi_pack *p, int recon, int maxjshift, double qo, double dt, const int *nghbr,
                          const double *xlim, const double *bx1f, const double *bx3f, double *emfx, double *emfz,
                          void *stream);
int akmi_sbox_orbital_ct(const akmi_pack *p, const double *emfx, const double *emfz, double *bx1f, double *bx2f,
                         double *bx3f, void *stream);
/* MRIHistory (src/pgen/tests/mri3d.cpp:233-336) over the active cells of a 3-D MHD pack: nhist = 15 (isothermal) or 16
 * (ideal gas) sums, nmhd = 4 or 5 conserved variables first, then 1-KE 2-KE 3-KE 1-ME 2-ME 3-ME 1-bcc 2-bcc 3-bcc dVxVy dBxBy.
 * partial = device double[nmb][nhist]: per-MeshBlock sums by fixed-shape trees (the same bits on every call); the host
 * adds them in gid order.  work: akmi_mri_history_workspace_bytes() of device memory. */
#define AKMI_MRI_NHIST_MAX 16
long long akmi_mri_history_workspace_bytes(const akmi_pack *p);
int akmi_mri_history(const akmi_pack *p, const double *u0, const double *bcc0, const double *bx1f, const double *bx2f,
                     const double *bx3f, double *partial, double *work, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AKMI_H_ */
