// akmi_stage_march.hpp -- the marching kernels of the fused stage (k_sweep_update, k_sweep_update_1d) and their launcher,
// for the two units that instantiate them: akmi_stage_march_x2.hip (the 1-D kernel and the x2 marches) and
// akmi_stage_march_x3.hip (the x3 marches, u0 and face forms included).  Every macro below is read by both.
#ifndef AKMI_STAGE_MARCH_HPP_
#define AKMI_STAGE_MARCH_HPP_
#include "akmi_stage.hpp"

namespace akmi {

// Window sizes of the marching kernels per reconstruction (cells kept per variable)
template <int RECON> struct RollCfg;
template <> struct RollCfg<0> { static constexpr int NW = 1; };   // dc
template <> struct RollCfg<1> { static constexpr int NW = 2; };   // plm
template <> struct RollCfg<2> { static constexpr int NW = 4; };   // ppm4
template <> struct RollCfg<3> { static constexpr int NW = 4; };   // ppmx
template <> struct RollCfg<4> { static constexpr int NW = 4; };   // wenoz
template <> struct RollCfg<5> { static constexpr int NW = 4; };   // teno

// last-direction sweep with the RK update fused, as a MARCH along the sweep direction:
// each thread owns one transverse position (lanes run over the contiguous index, so every
// load/store of a wave is a coalesced row segment), walks ML faces along the sweep, keeps the
// previous face flux in registers and finishes cell (t-1) as soon as face t is known:
//   divf = dF1/dx1; divf += dF2/dx2; divf += dF3/dx3; u0 = gam0*u0 + gam1*u1 - beta_dt*divf
// (hydro_update.cpp:55-80 order).  No LDS, no barrier: waves run free, so the memory-bound
// update of one wave hides under the Riemann arithmetic of the others.  One face per chunk
// (1/ML) is computed twice.
#ifndef AKMI_PREFETCH_UPD
#define AKMI_PREFETCH_UPD 1
#endif
// The x3 march moves the most bytes of the stage and waits on memory 72 % of its wave cycles
// (profiles/r02_v3_valu_counters.txt).  With the register budget of TWO waves per SIMD it can hold the
// update operands u1 (AKMI_PREFETCH_U1) and the cells of the next step (AKMI_PREFETCH_W) in flight across
// the Riemann solve: 1165 -> 907 us at 256^3, 202 VGPRs, no scratch (profiles/r02_prefetch_w.txt).  At three
// waves the same prefetches spill (x3 march 1.07 -> 1.20-1.35 ms), and the x2 march loses at two waves.
#ifndef AKMI_PREFETCH_U1
#define AKMI_PREFETCH_U1 1
#endif
#ifndef AKMI_MARCH_WAVES
#define AKMI_MARCH_WAVES 3
#endif
#ifndef AKMI_PREFETCH_W
#define AKMI_PREFETCH_W 1       // x3 PLM march: load the cells of step t+1 during step t (2*NV more VGPRs)
#endif
#ifndef AKMI_PPM_WREG
#define AKMI_PPM_WREG 1         // marches with five-point reconstructions keep their window in registers
#endif
#ifndef AKMI_PREFETCH_W2
#define AKMI_PREFETCH_W2 0      // the same in the x2 march
#endif
#ifndef AKMI_X3_WAVES
#define AKMI_X3_WAVES 2         // register budget of the x3 march (waves per SIMD)
#endif
#ifndef AKMI_X2_WAVES
#define AKMI_X2_WAVES AKMI_MARCH_WAVES
#endif
#ifndef AKMI_PREFETCH_X1
#define AKMI_PREFETCH_X1 0
#endif
#ifndef AKMI_PREFETCH_WP2
#define AKMI_PREFETCH_WP2 1     // five-point schemes (two waves per SIMD): next cells prefetched in the x2 march,
#endif
#ifndef AKMI_PREFETCH_WP3
#define AKMI_PREFETCH_WP3 1     // ... in the x3 march,
#endif
#ifndef AKMI_PREFETCH_X1P
#define AKMI_PREFETCH_X1P 1     // ... the x1 flux difference fetched before the solve in the x2 march
#endif
#ifndef AKMI_MARCH_FM
#define AKMI_MARCH_FM 0        // ... in the marches: loses (registers, basic blocks), profiles/r03_ab1.txt
#endif
#ifndef AKMI_X2_EO
#define AKMI_X2_EO 0            // wave-uniform early-outs of HLLD in the x2 / x3 march (registers!)
#endif
#ifndef AKMI_X3_EO
#define AKMI_X3_EO 0
#endif

// MODE 2: no update at all, the five flux components of every face are stored (the flux kernels of the
// task-granular entry points, sweeps_store_fluxes below).
// MODE 0: last direction -- finish the RK update.  MODE 1 (x2 sweep of 3-D runs): store the
// partial divergence acc = dF1/dx1 + dF2/dx2 for the x3 march, which then needs one array
// instead of two face pairs per variable (USEACC).  Rounding sequence unchanged.
// U0F (x3 march of an MHD PLM stage that is out of place, copy_u1 2 or 3): every cell's conserved state is read ONCE.  The
// window takes density and momentum from u0 -- the velocities are formed with vel_from_cons, which is what ConsToPrim
// stored in w0[1..3], bit for bit -- and only the internal energy from w0[4]; the density and the momentum of the cell a
// face finishes are the ones the window loaded two steps earlier (momenta parked in registers), so the update fetches
// u0[4] alone: four streams fewer per cell.  NOT for a stage in place: the priming loads of a chunk read the last two
// cells of the chunk below, which such a stage has overwritten in u0 by then.
// BF (on top of U0F, AKMI_COPY_BCC_FACES): slots 5 and 6 (Bx, By here) are bcc_from_faces of b0.x1f at i, i+1 and b0.x2f at
// j, j+1 instead of bcc0[0..1] -- the priming loads and the one-step-ahead prefetch alike; the prefetched faces stay as
// loaded until the step that consumes them.
template <int DIR, int RECON, bool MHD, int MODE, bool USEACC, int RS, bool P2, bool U0F = false, bool BF = false>
__device__ __forceinline__ void sweep_update_body(const Geo &g, const FaceEos &eos, const SweepArgs &a,
                                                  const UpdArgs &u, int ml, double *sm) {
  static_assert(DIR == 1 || DIR == 2, "marching kernel is for the x2/x3 sweeps");
  static_assert(!U0F || (DIR == 2 && MHD && RECON == 1 && MODE == 0 && USEACC && !rs_iso<RS>() && AKMI_PREFETCH_W &&
                         AKMI_PREFETCH_UPD), "u0 form: x3 march of MHD PLM with the update");
  static_assert(!BF || U0F, "face form: on top of the u0 form");
  constexpr bool STORE = MODE == 2;                                  // all flux components of every face go to memory
  int i, j, k, m, s0;
  bool lane_ok;
  // lanes over the flattened (row, i).  The storing marches (MODE 2: refined meshes, small MeshBlocks) run them over the
  // columns of the sweep only -- [il, iu] instead of the N1 of the row: with four ghost cells a 32^3 block has 40 columns
  // of which 34 carry a face, and nothing couples the lanes of a march.  The other modes keep the N1 rows (at 256^3
  // 258 of 260 lanes carry a face).
  const int row_w = STORE ? a.iu - a.il + 1 : g.N1, row_0 = STORE ? a.il : 0;
  if constexpr (DIR == 2) {
    const long p = ((long)blockIdx.x*SY + threadIdx.y)*SX + threadIdx.x;   // rows [jl,ju] x row_w
    const int jj = (int)(p/row_w);
    i = row_0 + (int)(p - (long)jj*row_w);
    j = a.jl + jj;
    m = blockIdx.z;
    s0 = a.kl + blockIdx.y*ml;
    k = s0;
    lane_ok = (j <= a.ju) && (i >= a.il) && (i <= a.iu);
  } else {
    const long p = ((long)blockIdx.x*SY + threadIdx.y)*SX + threadIdx.x;   // planes [kl,ku] x row_w
    const int kk = (int)(p/row_w);
    i = row_0 + (int)(p - (long)kk*row_w);
    k = a.kl + kk;
    m = blockIdx.z;
    s0 = a.jl + blockIdx.y*ml;
    j = s0;
    lane_ok = (k <= a.ku) && (i >= a.il) && (i <= a.iu);
  }
  if (!lane_ok) return;
  constexpr int ivx = 1 + DIR, ivy = 1 + (DIR + 1)%3, ivz = 1 + (DIR + 2)%3;
  constexpr int iby = (DIR + 1)%3, ibz = (DIR + 2)%3;
  constexpr int NV = MHD ? 7 : 5;
  constexpr bool ISO = rs_iso<RS>();       // slot 4 (energy) of the variable arrays unused
  constexpr int NW = RollCfg<RECON>::NW;
  constexpr int NT = SX*SY;
  // marching state of this thread, parked in LDS ("LDS as an extension of the register file":
  // slot s of thread t lives at sm[s*NT + t], consecutive lanes -> consecutive banks):
  //   W(n,c)  last NW cells of variable n       PL(n)  pending left state of the next face
  //   FP(n)   flux of the previous face
  // Keeping it out of the VGPRs lets the kernel run at the occupancy of the plain Riemann
  // kernel while every cell is loaded from HBM exactly once per sweep.
  double *my = sm + threadIdx.y*SX + threadIdx.x;
  // five-point reconstructions (NW = 4) run with the register budget of two waves per SIMD: their
  // window stays in registers (WREG) and only PL/FP are parked -- 12 instead of 40 LDS slots per thread,
  // 24 KB instead of 80 KB per workgroup, i.e. two workgroups per CU instead of one
  constexpr bool WREG = (RECON >= 2) && AKMI_PPM_WREG;
  constexpr int WB = WREG ? 0 : NV*NW;               // LDS slots taken by the window
  double Wr[WREG ? NV : 1][WREG ? NW : 1];
#define W_(n, c) (*(WREG ? &Wr[WREG ? (n) : 0][WREG ? (c) : 0] : &my[((n)*NW + (c))*NT]))
#define PL_(n) my[(WB + (n))*NT]
#define FP_(n) my[(WB + NV + (n))*NT]
  const int shi = (DIR == 1) ? a.ju : a.ku;           // last face along the sweep
  // beta*dt once per thread, in scalar registers (inside the update loop a device-resident dt was re-read,
  // and waited for, once per variable and step)
  const double bdt = (MODE == 0) ? to_sgpr(beta_dt_of(u.beta_dt, u.dtp)) : 0.0;
  const bool col_active = (i >= g.is) && (i <= g.ie) &&
                          ((DIR == 1) ? (k >= g.ks && k <= g.ke) : (j >= g.js && j <= g.je));
  const int clo = (DIR == 1) ? g.js : g.ks, chi = (DIR == 1) ? g.je : g.ke;
  const double dx1 = g.dx[3*m], dx2 = g.dx[3*m + 1], dx3 = g.dx[3*m + 2];
  const bool p2 = P2 && is_pow2(dx1) && is_pow2(dx2) && is_pow2(dx3);      // wave-uniform: x/dx == ldexp(x, n) bit for bit
  const int n1 = pow2_shift(dx1), n2 = pow2_shift(dx2), n3 = pow2_shift(dx3);
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const long st = (DIR == 1) ? (long)g.N1 : (long)g.N1*g.N2;
  // wave-uniform variable bases in sweep-aligned order d, vx, vy, vz, e, (by, bz) + one
  // per-lane element offset that advances by st per step
  // (addresses = uniform base on the scalar unit + 32-bit byte offset of the lane: global_load v, v_off,
  // s[base]; a block-variable is below 4 GB, checked at launch)
  const double *wb = a.w0 + (size_t)m*g.nvar*cs;
  const double *bb = MHD ? a.bcc0 + (size_t)m*3*cs : nullptr;
  unsigned off = (((unsigned)k*(unsigned)g.N2 + (unsigned)j)*(unsigned)g.N1 + (unsigned)i)*8u;   // cell s
  const unsigned st8 = (unsigned)st*8u;
  const double *cb = U0F ? u.u0 + (size_t)m*g.nvar*cs : wb;      // U0F: slots 0-3 hold density and MOMENTUM
  auto base = [&](int n) -> const double * {
    return n == 0 ? cb : n == 1 ? cb + ivx*cs : n == 2 ? cb + ivy*cs : n == 3 ? cb + ivz*cs
         : n == 4 ? wb + 4*cs : n == 5 ? bb + iby*cs : bb + ibz*cs;
  };
  double mprev[3] = {0.0, 0.0, 0.0}, mcur[3] = {0.0, 0.0, 0.0};     // U0F: momenta (sweep order) of cells s-1 and s
  // BF: x1 faces (N3, N2, N1+1) i, i+1 and x2 faces (N3, N2+1, N1) j, j+1 of cell s, advancing with the march
  const double *bt1m = BF ? a.bt1 + (size_t)m*g.N3*g.N2*(g.N1 + 1) : nullptr;
  const double *bt2m = BF ? a.bt2 + (size_t)m*g.N3*(g.N2 + 1)*g.N1 : nullptr;
  unsigned ox = (((unsigned)k*(unsigned)g.N2 + (unsigned)j)*(unsigned)(g.N1 + 1) + (unsigned)i)*8u;
  unsigned oy = (((unsigned)k*(unsigned)(g.N2 + 1) + (unsigned)j)*(unsigned)g.N1 + (unsigned)i)*8u;
  const long sx = (long)g.N2*(g.N1 + 1), sy = (long)(g.N2 + 1)*g.N1;          // their strides along k
  auto ldf = [&](long r, double (&f)[4]) {              // the four faces of the cell r steps beyond cell s, as loaded
    f[0] = ldu(bt1m + r*sx, ox); f[1] = ldu(bt1m + r*sx + 1, ox);
    f[2] = ldu(bt2m + r*sy, oy); f[3] = ldu(bt2m + r*sy + g.N1, oy);
  };
  if constexpr (BF) {
    double fa[4], fb[4], fc[4];
    ldf(-2, fa); ldf(-1, fb); ldf(0, fc);
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const double qa = bcc_from_faces(fa[2*n], fa[2*n + 1]), qb = bcc_from_faces(fb[2*n], fb[2*n + 1]),
                   qc = bcc_from_faces(fc[2*n], fc[2*n + 1]);
      double pl, dummy;
      plm(qa, qb, qc, pl, dummy);
      W_(5 + n, 0) = qb; W_(5 + n, 1) = qc; PL_(5 + n) = pl;
    }
  }
  // prime the window: left state of the first face comes from cell s0-1
  if constexpr (U0F) {
    double qd[3], qm[3][3], qv[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      qd[c] = ldu(base(0) - (2 - c)*st, off);
#pragma unroll
      for (int n = 0; n < 3; ++n) qm[n][c] = ldu(base(1 + n) - (2 - c)*st, off);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double di;
      vel_from_cons(qd[c], qm[0][c], qm[1][c], qm[2][c], di, qv[0][c], qv[1][c], qv[2][c]);
    }
    double pl, dummy;
    plm(qd[0], qd[1], qd[2], pl, dummy);
    W_(0, 0) = qd[1]; W_(0, 1) = qd[2]; PL_(0) = pl;
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      plm(qv[n][0], qv[n][1], qv[n][2], pl, dummy);
      W_(1 + n, 0) = qv[n][1]; W_(1 + n, 1) = qv[n][2]; PL_(1 + n) = pl;
      mprev[n] = qm[n][1]; mcur[n] = qm[n][2];
    }
  }
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    if (ISO && n == 4) continue;
    if (U0F && n < 4) continue;
    if (BF && n >= 5) continue;
    const double *q = base(n);
    double pl, dummy;
    if constexpr (RECON == 1) {
      const double qa = ldu(q - 2*st, off), qb = ldu(q - st, off), qc = ldu(q, off);
      plm(qa, qb, qc, pl, dummy);
      W_(n, 0) = qb; W_(n, 1) = qc;
    } else if constexpr (RECON >= 2) {
      const double qa = ldu(q - 3*st, off), qb = ldu(q - 2*st, off), qc = ldu(q - st, off), qd = ldu(q, off),
                   qe = ldu(q + st, off);
      recon5<RECON>(qa, qb, qc, qd, qe, pl, dummy);
      if (n == 0) floor_lr<RECON, 1>(eos, pl, dummy);
      if (n == 4) floor_lr<RECON, 2>(eos, pl, dummy);
      W_(n, 0) = qb; W_(n, 1) = qc; W_(n, 2) = qd; W_(n, 3) = qe;
    } else {
      pl = ldu(q - st, off);
      W_(n, 0) = ldu(q, off);
    }
    PL_(n) = pl;
  }
  // face (k,j,i) of this direction's face-shaped arrays (f3,f2,f1), advancing with the march
  const size_t fs = (size_t)a.f3*a.f2*a.f1;
  unsigned foff = (((unsigned)k*(unsigned)a.f2 + (unsigned)j)*(unsigned)a.f1 + (unsigned)i)*8u;
  const unsigned fst8 = ((DIR == 1) ? (unsigned)a.f1 : (unsigned)a.f1*(unsigned)a.f2)*8u;
  const double *bxm = MHD ? a.bxf + (size_t)m*fs : nullptr;
  double *mfm = a.flx ? a.flx + (size_t)m*g.nvar*fs : nullptr;       // variable 0: the mass flux
  // its sign as a byte instead (wave-uniform; the u0 form exists on the k_sweep12s path only, which always takes bytes)
  const bool mf_bytes = AKMI_MF_BYTES && MHD && !STORE && (U0F || a.mfb != nullptr);
  unsigned char *mbm = mf_bytes ? a.mfb + (size_t)m*fs : nullptr;
  // x1 fluxes (N3,N2,N1+1) of the cell row the step finishes (x2 march without acc)
  const size_t fs1 = (size_t)g.N3*g.N2*(g.N1 + 1);
  unsigned o1 = (((unsigned)k*(unsigned)g.N2 + (unsigned)j)*(unsigned)(g.N1 + 1) + (unsigned)i)*8u;
  const unsigned st18 = (unsigned)(g.N1 + 1)*8u;
  constexpr bool PW = (RECON == 1 && ((AKMI_PREFETCH_W && DIR == 2) || (AKMI_PREFETCH_W2 && DIR == 1))) ||
                      (RECON >= 2 && ((AKMI_PREFETCH_WP3 && DIR == 2) || (AKMI_PREFETCH_WP2 && DIR == 1)));
  constexpr int LA = RECON == 1 ? 1 : 2;            // the cell a step loads is LA cells ahead of cell s
  double nx[NV];                         // PW: cells s+1 of the coming step, loaded one step ahead
  // (the face field of the next face prefetched as well: measured, the x3 march loses 865 -> 942 us,
  //  profiles/r03_ab2.txt; requested before the update operands: no effect, profiles/r03_ab4.txt -- both removed)
  double nf[4] = {0.0, 0.0, 0.0, 0.0};   // BF: the faces behind nx[5], nx[6]
  if constexpr (PW) {
#pragma unroll
    for (int n = 0; n < NV; ++n) nx[n] = ((ISO && n == 4) || (BF && n >= 5)) ? 0.0 : ldu(base(n) + LA*st, off);
    if constexpr (BF) ldf(LA, nf);
  }
  for (int t = 0; t <= ml; ++t) {
    const int s = s0 + t;
    if (s > shi) break;
    if constexpr (DIR == 1) j = s; else k = s;
    double nx2[NV];
    if constexpr (PW) {
      const bool more = (t < ml) && (s < shi);           // a next step exists: its cell s+2 is inside the array
#pragma unroll
      for (int n = 0; n < NV; ++n) nx2[n] = (more && !(ISO && n == 4) && !(BF && n >= 5)) ? ldu(base(n) + (LA + 1)*st, off) : 0.0;
    }
    double nf2[4] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (BF) {
      if ((t < ml) && (s < shi)) ldf(LA + 1, nf2);
      nx[5] = bcc_from_faces(nf[0], nf[1]); nx[6] = bcc_from_faces(nf[2], nf[3]);
    }
    double L[NV], R[NV];
    double vnx[3] = {0.0, 0.0, 0.0}, dsc = 0.0;          // U0F: velocities of cell s+1, density of the cell this face finishes
    if constexpr (U0F) {
      double di;
      vel_from_cons(nx[0], nx[1], nx[2], nx[3], di, vnx[0], vnx[1], vnx[2]);
    }
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      if (ISO && n == 4) { L[n] = R[n] = 0.0; continue; }      // isothermal: no energy variable
      const double *q = base(n);
      double qln;
      L[n] = PL_(n);
      if constexpr (RECON == 1) {
        double qp;
        if constexpr (U0F) qp = (n >= 1 && n <= 3) ? vnx[n >= 1 && n <= 3 ? n - 1 : 0] : nx[n];
        else if constexpr (PW) qp = nx[n]; else qp = ldu(q + st, off);
        const double w0 = W_(n, 0), w1 = W_(n, 1);
        if (U0F && n == 0) dsc = w0;
        plm(w0, w1, qp, qln, R[n]);
        W_(n, 0) = w1; W_(n, 1) = qp;
      } else if constexpr (RECON >= 2) {
        double qp;
        if constexpr (PW) qp = nx[n]; else qp = ldu(q + 2*st, off);
        const double w0 = W_(n, 0), w1 = W_(n, 1), w2 = W_(n, 2), w3 = W_(n, 3);
        recon5<RECON>(w0, w1, w2, w3, qp, qln, R[n]);
        if (n == 0) floor_lr<RECON, 1>(eos, qln, R[n]);
        if (n == 4) floor_lr<RECON, 2>(eos, qln, R[n]);
        W_(n, 0) = w1; W_(n, 1) = w2; W_(n, 2) = w3; W_(n, 3) = qp;
      } else {
        const double w0 = W_(n, 0);
        R[n] = w0;
        qln = w0;
        W_(n, 0) = ldu(q + st, off);
      }
      PL_(n) = qln;
    }
    const unsigned oc = off;                            // cell s == face s of the cell-shaped EMF arrays
    const unsigned ocm = off - st8;                     // cell s-1, the one this face finishes
    off += st8;
    if constexpr (BF) { ox += (unsigned)sx*8u; oy += (unsigned)sy*8u; }
    // x3 march: fetch the update operands of the cell this face finishes BEFORE the Riemann solve,
    // so that their latency is covered by ~1000 VALU instructions instead of following them
    // (this kernel moves the most bytes of the stage and runs at 3 waves/SIMD)
    constexpr bool PRE = (DIR == 2) && USEACC && (MODE == 0) && AKMI_PREFETCH_UPD;
    const int sc = s - 1;                               // cell finished by this face
    const bool upd = MODE != 2 && t > 0 && col_active && sc >= clo && sc <= chi;
    double pa[5], pu[5], pu1[5];
    if constexpr (PRE) {
      if (upd) {
        const size_t mb = (size_t)m*g.nvar*cs;
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          if (ISO && n == 4) continue;
          pa[n] = ldu(u.acc + mb + n*cs, ocm);
          if (!U0F || n == 4) pu[n] = ldu(u.u0 + mb + n*cs, ocm);
        }
        if constexpr (U0F) { pu[0] = dsc; pu[ivx] = mprev[0]; pu[ivy] = mprev[1]; pu[ivz] = mprev[2]; }
        if (AKMI_PREFETCH_U1 && rk_reads_u1(u.copy_u1)) {
#pragma unroll
          for (int n = 0; n < 5; ++n) { if (ISO && n == 4) continue; pu1[n] = ldu(u.u1 + mb + n*cs, ocm); }
        }
      }
    }
    // x2 march of 3-D runs: same idea for the x1 flux difference of the finished cell
    constexpr bool PRE1 = (DIR == 1) && (MODE == 1) && !USEACC && (RECON >= 2 ? AKMI_PREFETCH_X1P : AKMI_PREFETCH_X1);
    if constexpr (PRE1) {
      if (upd) {
        const double *f1 = u.flx1 + (size_t)m*g.nvar*fs1 - (g.N1 + 1);       // row sc = s-1
        // the two fluxes stay as loaded until the update below: a subtraction or `p2 ? ldexp : /` here would put a
        // wait (and, through the wave-uniform branch, one basic block per variable: load -> vmcnt(0), five times)
        // in front of the solve that is meant to cover the latency (second audit, profiles/r03_isa_audit.txt)
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          if (ISO && n == 4) continue;
          pu[n] = ldu(f1 + n*fs1 + 1, o1); pa[n] = ldu(f1 + n*fs1, o1);
        }
      }
    }
    double fd, fx, fy, fz, fe;
    if constexpr (MHD) {
      const double bxi = ldu(bxm, foff);
      Cons1D fl = riemann_mhd_e<RS, (DIR == 1 ? AKMI_X2_EO : AKMI_X3_EO) != 0, AKMI_MARCH_FM != 0>(
          eos, L[0], L[1], L[2], L[3], L[4], L[5], L[6], R[0], R[1], R[2], R[3], R[4], R[5], R[6], bxi);
      fd = fl.d; fx = fl.mx; fy = fl.my; fz = fl.mz; fe = fl.e;
      if (t < ml || s == shi) {
        // CornerE needs the sign of the mass flux and the two face EMFs of this direction
        if (mf_bytes) st_mfs(mbm, foff, fd); else stu(mfm, foff, fd);
        stu(a.ey + (size_t)m*cs, oc, -fl.by);
        stu(a.ez + (size_t)m*cs, oc, fl.bz);
      }
    } else {
      riemann_hyd_e<RS>(eos, L[0], L[1], L[2], L[3], L[4], R[0], R[1], R[2], R[3], R[4], fd, fx,
                        fy, fz, fe);
      // passive scalars are advected by the mass flux (k_scalar_update): keep it
      if ((STORE || g.nvar > (ISO ? 4 : 5)) && (t < ml || s == shi)) stu(mfm, foff, fd);
    }
    double fv[5];
    fv[0] = fd; fv[ivx] = fx; fv[ivy] = fy; fv[ivz] = fz; fv[4] = fe;
    if constexpr (STORE) {                // task-granular callers: the whole flux of the face goes to memory
      if (t < ml || s == shi) {
#pragma unroll
        for (int n = 1; n < 5; ++n) { if (ISO && n == 4) continue; stu(mfm + n*fs, foff, fv[n]); }
      }
    }
    foff += fst8;
    if (upd) {
      const int kc = (DIR == 2) ? sc : k, jc = (DIR == 1) ? sc : j;
      const size_t mb = (size_t)m*g.nvar*cs;
      // operands of all variables first (one group of loads, counted waits), then the arithmetic with the
      // power-of-two choice hoisted out of the loop over the variables: with `p2 ? ldexp : /` inside that loop
      // every variable was a basic block of its own with its loads and an s_waitcnt vmcnt(0) at the top
      // (the x3 march with its operands prefetched before the solve keeps the plain loop: nothing is loaded in it, and
      //  the two-copy form costs it 870 -> 940 us, profiles/r03_ab5.txt)
      if constexpr (PRE) {
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          if (ISO && n == 4) continue;
          const double dlast = fv[n] - FP_(n);
          double divf = pa[n];
          divf += p2 ? ldexp(dlast, n3) : dlast/dx3;
          const double u0v = pu[n];
          double u1v;
          if constexpr (AKMI_PREFETCH_U1) u1v = !rk_reads_u1(u.copy_u1) ? u0v : pu1[n];
          else u1v = !rk_reads_u1(u.copy_u1) ? u0v : ldu(u.u1 + mb + n*cs, ocm);
          rk_store_u(u.u0 + mb + n*cs, u.u1 + mb + n*cs, u.copy_u1, ocm, u0v, u.gam0*u0v + u.gam1*u1v - bdt*divf);
        }
      } else {
      double t1[5], t2[5], u0v[5], u1v[5];
#pragma unroll
      for (int n = 0; n < 5; ++n) {
        if (ISO && n == 4) continue;
        t2[n] = 0.0;
        if constexpr (PRE1) {
          t1[n] = pu[n] - pa[n];                          // x1 flux difference, fetched before the solve
        } else if constexpr (PRE) {
          t1[n] = pa[n];                                  // acc, fetched before the solve
        } else if constexpr (USEACC) {
          t1[n] = ldu(u.acc + mb + n*cs, ocm);
        } else if constexpr (DIR == 1) {
          const double *f1 = u.flx1 + (size_t)m*g.nvar*fs1 + n*fs1 - (g.N1 + 1);     // row sc = s-1
          t1[n] = ldu(f1 + 1, o1) - ldu(f1, o1);
        } else {
          t1[n] = u.flx1[ix5(g.nvar, g.N3, g.N2, g.N1 + 1, m, n, kc, jc, i + 1)] -
                  u.flx1[ix5(g.nvar, g.N3, g.N2, g.N1 + 1, m, n, kc, jc, i)];
          t2[n] = u.flx2[ix5(g.nvar, g.N3, g.N2 + 1, g.N1, m, n, kc, jc + 1, i)] -
                  u.flx2[ix5(g.nvar, g.N3, g.N2 + 1, g.N1, m, n, kc, jc, i)];
        }
        if constexpr (MODE != 1) {
          if constexpr (PRE) u0v[n] = pu[n]; else u0v[n] = ldu(u.u0 + mb + n*cs, ocm);
          if constexpr (PRE && AKMI_PREFETCH_U1) u1v[n] = !rk_reads_u1(u.copy_u1) ? u0v[n] : pu1[n];
          else u1v[n] = !rk_reads_u1(u.copy_u1) ? u0v[n] : ldu(u.u1 + mb + n*cs, ocm);
        }
      }
      auto finish = [&](auto P2c) {
        constexpr bool P2v = decltype(P2c)::value;
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          if (ISO && n == 4) continue;
          const double dlast = fv[n] - FP_(n);
          double divf;
          if constexpr ((PRE && !PRE1) || (USEACC && !PRE1)) divf = t1[n];           // acc: already a divergence
          else divf = P2v ? ldexp(t1[n], n1) : t1[n]/dx1;
          if constexpr (DIR == 1) {
            divf += P2v ? ldexp(dlast, n2) : dlast/dx2;
          } else {
            if constexpr (!USEACC) divf += P2v ? ldexp(t2[n], n2) : t2[n]/dx2;
            divf += P2v ? ldexp(dlast, n3) : dlast/dx3;
          }
          if constexpr (MODE == 1) {
            stu(u.acc + mb + n*cs, ocm, divf);
          } else {
            rk_store_u(u.u0 + mb + n*cs, u.u1 + mb + n*cs, u.copy_u1, ocm, u0v[n],
                       u.gam0*u0v[n] + u.gam1*u1v[n] - bdt*divf);
          }
        }
      };
      if (p2) finish(IC<1>{}); else finish(IC<0>{});
      }
    }
#pragma unroll
    for (int n = 0; n < 5; ++n) { if (ISO && n == 4) continue; FP_(n) = fv[n]; }
    o1 += st18;
    if constexpr (U0F) {
#pragma unroll
      for (int n = 0; n < 3; ++n) { mprev[n] = mcur[n]; mcur[n] = nx[1 + n]; }
    }
    if constexpr (PW) {
#pragma unroll
      for (int n = 0; n < NV; ++n) nx[n] = nx2[n];
      if constexpr (BF) { nf[0] = nf2[0]; nf[1] = nf2[1]; nf[2] = nf2[2]; nf[3] = nf2[3]; }
    }
  }
#undef W_
#undef PL_
#undef FP_
}

// the kernel proper: when the cell sizes of the block are powers of two, x/dx == x*(1/dx) bit for
// bit (both are the correctly rounded value of the same real number, and 1/dx is exact), so the
// divisions by dx become products; decided per block, two copies of the loop
template <int DIR, int RECON, bool MHD, int MODE, bool USEACC, int RS, bool U0F = false, bool BF = false>
__global__ void __launch_bounds__(SX*SY, (RECON >= 2 ? 2 : (DIR == 2 ? AKMI_X3_WAVES : AKMI_X2_WAVES)))
k_sweep_update(Geo g, FaceEos eos, SweepArgs a, UpdArgs u, int ml) {
  constexpr int NV = MHD ? 7 : 5;
  __shared__ double sm[(((RECON >= 2) && AKMI_PPM_WREG ? 0 : NV*RollCfg<RECON>::NW) + NV + 5)*SX*SY];
  const int m = blockIdx.z;
  constexpr bool TRY = AKMI_POW2DX != 0;      // power-of-two cell sizes: x/dx by v_ldexp_f64 (wave-uniform run-time choice)
  sweep_update_body<DIR, RECON, MHD, MODE, USEACC, RS, TRY, U0F, BF>(g, eos, a, u, ml, sm);
}


// 1-D problems: the sweep direction is the lane direction, so neighbouring faces are
// exchanged through LDS inside a TX-wide tile (overlap of one face between tiles).
template <int RECON, bool MHD, int RS>
__global__ void __launch_bounds__(TX)
k_sweep_update_1d(Geo g, FaceEos eos, SweepArgs a, UpdArgs u) {
  __shared__ double sF[5][TX];
  const int i = a.il + blockIdx.x*(TX - 1) + threadIdx.x;
  const int j = a.jl, k = a.kl, m = blockIdx.z;
  const bool face_ok = (i <= a.iu);
  double fd = 0, fx = 0, fy = 0, fz = 0, fe = 0, fby = 0, fbz = 0;
  if (face_ok) {
    face_flux<0, RECON, MHD, RS>(g, eos, a.w0, a.bcc0, a.bxf, a.f3, a.f2, a.f1, m, k, j, i, fd, fx,
                                 fy, fz, fe, fby, fbz);
    if constexpr (MHD) {
      a.flx[ix5(g.nvar, a.f3, a.f2, a.f1, m, 0, k, j, i)] = fd;
      const size_t ec = ix4(g.N3, g.N2, g.N1, m, k, j, i);
      a.ey[ec] = -fby;
      a.ez[ec] = fbz;
    } else {
      if (g.nvar > (rs_iso<RS>() ? 4 : 5)) a.flx[ix5(g.nvar, a.f3, a.f2, a.f1, m, 0, k, j, i)] = fd;
    }
  }
  const double fv[5] = {fd, fx, fy, fz, fe};
#pragma unroll
  for (int n = 0; n < 5; ++n) sF[n][threadIdx.x] = fv[n];
  __syncthreads();
  if (threadIdx.x >= TX - 1 || i > g.ie) return;
  const double dx1 = g.dx[3*m];
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const size_t c = ix5(g.nvar, g.N3, g.N2, g.N1, m, 0, k, j, i);
#pragma unroll
  for (int n = 0; n < 5; ++n) {
    if (rs_iso<RS>() && n == 4) continue;            // isothermal: no energy variable
    const double divf = (sF[n][threadIdx.x + 1] - fv[n])/dx1;
    const double u0v = u.u0[c + n*cs];
    const double u1v = u.copy_u1 ? u0v : u.u1[c + n*cs];
    rk_store(u.u0, u.u1, u.copy_u1, c + n*cs, u0v, u.gam0*u0v + u.gam1*u1v - beta_dt_of(u.beta_dt, u.dtp)*divf);
  }
}

template <int DIR, bool MHD, int MODE, bool USEACC>
int launch_sweep_update(const Geo &g, const Scheme &sc, const SweepArgs &a,
                        const UpdArgs &u, hipStream_t st, bool u0_form, bool face_form) {
  int rc;
  if constexpr (DIR == 0) {
    dim3 grid(cdiv(a.iu - a.il + 1, TX - 1), 1, g.nmb), block(TX, 1);
    rc = dispatch_scheme_eos<MHD>(sc, [&](auto R, auto S) {
      k_sweep_update_1d<decltype(R)::value, MHD, decltype(S)::value><<<grid, block, 0, st>>>(
          g, sc.eos, a, u);
      return AKMI_COMPLETE;
    });
  } else {
    dim3 grid, block(SX, SY);
    int ml;
    if (DIR == 2) {
      long np = (long)(a.ju - a.jl + 1)*(MODE == 2 ? a.iu - a.il + 1 : g.N1);          // flattened rows (sweep_update_body)
      const unsigned nb = (unsigned)((np + SX*SY - 1)/(SX*SY));
      const int nc = a.ku - a.kl > 0 ? a.ku - a.kl : 1;
      // resident workgroups per CU: the PLM march is compiled for AKMI_X3_WAVES waves per SIMD, the
      // five-point schemes for two
      const int res3 = (sc.recon >= AKMI_RECON_PPM4) ? 2 : AKMI_X3_WAVES;
      ml = march_len(nb, nc, g.nmb, ML, res3);
      grid = dim3(nb, cdiv(nc, ml), g.nmb);
    } else {
      long np = (long)(a.ku - a.kl + 1)*(MODE == 2 ? a.iu - a.il + 1 : g.N1);          // flattened (k,i)
      const unsigned nb = (unsigned)((np + SX*SY - 1)/(SX*SY));
      const int nc = a.ju - a.jl > 0 ? a.ju - a.jl : 1;
      ml = march_len(nb, nc, g.nmb, ML, (sc.recon >= AKMI_RECON_PPM4) ? 2 : AKMI_X2_WAVES);
      grid = dim3(nb, cdiv(nc, ml), g.nmb);
    }
    constexpr int D = (DIR == 0) ? 1 : DIR;
    if (u0_form) {
      // the x3 march in its u0 form: MHD, PLM, HLLD, ideal gas (what stage_update asks it for)
      if constexpr (MHD && DIR == 2 && MODE == 0 && USEACC) {
        if (sc.iso || sc.recon != 1 || sc.rsolver != AKMI_RS_HLLD) { set_error("x3 march, u0 form: PLM + HLLD, ideal gas"); return AKMI_FAIL; }
        if (face_form && (!a.bt1 || !a.bt2)) { set_error("x3 march, face form: needs the x1 and x2 faces"); return AKMI_FAIL; }
        if (face_form) k_sweep_update<2, 1, true, 0, true, 3, true, true><<<grid, block, 0, st>>>(g, sc.eos, a, u, ml);
        else k_sweep_update<2, 1, true, 0, true, 3, true><<<grid, block, 0, st>>>(g, sc.eos, a, u, ml);
        rc = AKMI_COMPLETE;
      } else {
        set_error("sweep_update: the u0 form exists for the x3 march of MHD only");
        return AKMI_FAIL;
      }
    } else
    rc = dispatch_scheme_eos<MHD>(sc, [&](auto R, auto S) {
      k_sweep_update<D, decltype(R)::value, MHD, MODE, USEACC, decltype(S)::value>
          <<<grid, block, 0, st>>>(g, sc.eos, a, u, ml);
      return AKMI_COMPLETE;
    });
  }
  if (rc != AKMI_COMPLETE) return rc;
  AKMI_CHECK_LAUNCH("sweep_update");
  return AKMI_COMPLETE;
}

// one explicit instantiation of the launcher (the units list what stage_update and sweeps_store_fluxes_t ask for)
#define AKMI_INST_MARCH(DIR, MHD, MODE, USEACC)                                                                   \
  template int launch_sweep_update<DIR, MHD, MODE, USEACC>(const Geo &, const Scheme &, const SweepArgs &, \
                                                           const UpdArgs &, hipStream_t, bool, bool);

}  // namespace akmi
#endif
