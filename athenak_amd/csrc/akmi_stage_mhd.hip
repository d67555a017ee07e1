// akmi_stage_mhd.hip -- the kernels that only the fused MHD stage runs, with their launchers: k_sweep12s (x1 sweep
// inside the x2 march, 3-D PLM + HLLD), k_corner_ct (CornerE + CT in one kernel, 3-D) and k_ct_copy (CT of 1-D / 2-D
// runs).  The unit that tuning work on the MHD headline recompiles.
#include "akmi_stage.hpp"

namespace akmi {

#ifndef AKMI_DPP
#define AKMI_DPP 1            // neighbour lanes by DPP moves instead of ds_bpermute (lane_below / lane_above)
#endif
#if AKMI_DPP
#define AKMI_LANE_BELOW(x) lane_below(x)
#define AKMI_LANE_ABOVE(x) lane_above(x)
#else
#define AKMI_LANE_BELOW(x) __shfl_up(x, 1, 64)
#define AKMI_LANE_ABOVE(x) __shfl_down(x, 1, 64)
#endif
#ifndef AKMI_X12S_FM
#define AKMI_X12S_FM 1         // short sqrt / reciprocal forms (akmi_numerics.hpp) in the two solves of k_sweep12s
#endif

// x1 sweep + x2 march of an MHD pack in one kernel (3-D)
// ---------------------------------------------------------------------------------------
// k_sweep12s: the x1 sweep inside the x2 march (MHD, 3-D, PLM).  While a thread walks along j it also solves
// the x1 face on the low side of its cell in row s-1, the row whose cells the step finishes; the x1 flux
// difference of the cell goes straight into acc = dF1/dx1 + dF2/dx2 (rounding sequence of
// hydro_update.cpp:55-80 unchanged), so the 5-component x1 flux array is never written.  The cells of
// row s-1 are the cells the march loaded one step earlier: they sit in its window (LDS), so the x1
// part issues TWO loads per step (the cell-centred By, which the x2 march does not carry, and the face
// field); the i-1 / i+1 neighbours of the slopes, the left state of the face and the flux of
// face i+1 come from the neighbouring lanes (wave shuffles).  Waves overlap by four lanes: lanes 0 and 63
// only provide cells, lane 1 a left state, lane 62 a face flux; lanes 2..61 own cells.
#ifndef AKMI_X12S_WAVES
#define AKMI_X12S_WAVES 3
#endif
#ifndef AKMI_X12S_EO1
#define AKMI_X12S_EO1 1
#endif
#ifndef AKMI_X12S_EO2
#define AKMI_X12S_EO2 1
#endif
// UC (AKMI_COPY_X12_U0): the window takes density and momentum from u0 and forms the velocities with vel_from_cons where
// the loaded row is consumed (priming, x2 part of the step) -- what ConsToPrim stored in w0[1..3], bit for bit.  u0 is
// still the state of the start of the stage: the x3 march writes it after this kernel, in stream order.
// BF (AKMI_COPY_BCC_FACES): the cell-centred field through bcc_from_faces -- Bz of row s+1 from the x3 faces k and k+1 (the
// one extra stream), Bx of row s+1 from the x1 faces i and i+1 of that row (i+1: the lane above; lanes 0 and 63 and the
// last cell of a row of the array never use their own Bx), By of row s-1 from the x2 faces s-1 (carried) and s.
// All face indices lie inside the face-shaped arrays for k in [ks-1, ke+1] and rows in [js-2, je+2].
template <int RS, bool UC = false, bool BF = false>
__global__ void __launch_bounds__(SX*SY, AKMI_X12S_WAVES)
k_sweep12s(Geo g, FaceEos eos, SweepArgs a1, SweepArgs a2, UpdArgs u, int ml, const double *__restrict__ bx3f) {
  constexpr int NV = 7, NW = 2, NT = SX*SY;
  constexpr int CPW = SX - 4;                              // cells per wave
  __shared__ double sm[(NV*NW + NV + 5)*SX*SY];
  const int lane = threadIdx.x;
  const long wv = (long)blockIdx.x*SY + threadIdx.y;       // wave index over the (k,i) rows
  const long pe = wv*CPW + lane - 2;
  const long np = (long)(a2.ku - a2.kl + 1)*g.N1;
  if (wv*CPW - 2 >= np) return;                            // whole wave beyond the planes
  const long p = pe < 0 ? 0 : (pe > np - 1 ? np - 1 : pe); // clamped lanes compute, never store
  const int kk = (int)(p/g.N1);
  const int i = (int)(p - (long)kk*g.N1);
  const int k = a2.kl + kk;
  const int m = blockIdx.z;
  const int s0 = a2.jl + blockIdx.y*ml;
  const int shi = a2.ju;                                   // last x2 face
  const bool exact = pe == p;
  const bool inner = exact && lane >= 2 && lane <= SX - 3;
  const bool x2_ok = inner && i >= a2.il && i <= a2.iu;    // owns the x2 faces of this column
  const bool x1_ok = inner && i >= a1.il && i <= a1.iu;    // owns the x1 faces of this column
  const bool col_active = inner && i >= g.is && i <= g.ie && k >= g.ks && k <= g.ke;
  double *my = sm + threadIdx.y*SX + threadIdx.x;
#define W_(n, c) my[((n)*NW + (c))*NT]
#define PL_(n) my[(NV*NW + (n))*NT]
#define FP_(n) my[(NV*NW + NV + (n))*NT]
  const double dx1 = g.dx[3*m], dx2 = g.dx[3*m + 1];
  // blocks whose cell sizes are powers of two (the usual case: unit-length domains with 2^n cells, every level
  // of a refined mesh): 1/dx is exact and x/dx == x*(1/dx) bit for bit (both are the correctly rounded value of
  // the same real number), so the ten divisions of a step become products; wave-uniform branch per step
  const bool p2 = AKMI_POW2DX && is_pow2(dx1) && is_pow2(dx2);
  const int n1 = pow2_shift(dx1), n2 = pow2_shift(dx2);
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const long st = (long)g.N1;
  const double *wb = a2.w0 + (size_t)m*g.nvar*cs;
  const double *bb = a2.bcc0 + (size_t)m*3*cs;
  // x2-aligned order of the march: d, vy, vz, vx, e, bz, bx
  auto base2 = [&](int n) -> const double * {
    return n == 0 ? wb : n == 1 ? wb + 2*cs : n == 2 ? wb + 3*cs : n == 3 ? wb + cs
         : n == 4 ? wb + 4*cs : n == 5 ? bb + 2*cs : bb;
  };
  // UC: the conserved variables behind window slots 0-3 (d, m2, m3, m1)
  const double *ub = u.u0 + (size_t)m*g.nvar*cs;
  auto cbase2 = [&](int n) -> const double * { return n == 0 ? ub : n == 1 ? ub + 2*cs : n == 2 ? ub + 3*cs : ub + cs; };
  unsigned off = (((unsigned)k*(unsigned)g.N2 + (unsigned)s0)*(unsigned)g.N1 + (unsigned)i)*8u;    // cell (k, s, i)
  const unsigned st8 = (unsigned)g.N1*8u;
  // face-shaped arrays: x2 faces (f3, f2, f1) = (N3, N2+1, N1), x1 faces (N3, N2, N1+1), x3 faces (N3+1, N2, N1)
  const size_t fs2 = (size_t)a2.f3*a2.f2*a2.f1, fs1 = (size_t)a1.f3*a1.f2*a1.f1;
  unsigned foff2 = (((unsigned)k*(unsigned)a2.f2 + (unsigned)s0)*(unsigned)a2.f1 + (unsigned)i)*8u;   // x2 face s
  const unsigned fst28 = (unsigned)a2.f1*8u;
  unsigned foff1 = (((unsigned)k*(unsigned)a1.f2 + (unsigned)(s0 - 1))*(unsigned)a1.f1 + (unsigned)i)*8u;   // x1 face (k, s-1, i)
  const unsigned fst18 = (unsigned)a1.f1*8u;
  const double *bx2m = a2.bxf + (size_t)m*fs2, *bx1m = a1.bxf + (size_t)m*fs1;
  // x3 face (k, s, i) sits at the byte offset of cell (k, s, i); face k+1 one plane further
  const double *bx3m = BF ? bx3f + (size_t)m*(size_t)(g.N3 + 1)*g.N2*g.N1 : nullptr;
  const long pst = (long)g.N2*g.N1;
  if constexpr (UC) {
    double qd[3], qm[3][3], qv[3][3];                 // rows s0-2, s0-1, s0; momenta / velocities in window order 2, 3, 1
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      qd[c] = ldu(cbase2(0) - (2 - c)*st, off);
#pragma unroll
      for (int n = 0; n < 3; ++n) qm[n][c] = ldu(cbase2(1 + n) - (2 - c)*st, off);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double di;
      vel_from_cons(qd[c], qm[2][c], qm[0][c], qm[1][c], di, qv[2][c], qv[0][c], qv[1][c]);
    }
    double pl, dummy;
    plm(qd[0], qd[1], qd[2], pl, dummy);
    W_(0, 0) = qd[1]; W_(0, 1) = qd[2]; PL_(0) = pl;
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      plm(qv[n][0], qv[n][1], qv[n][2], pl, dummy);
      W_(1 + n, 0) = qv[n][1]; W_(1 + n, 1) = qv[n][2]; PL_(1 + n) = pl;
    }
  }
  if constexpr (BF) {
    double qz[3], qx[3];                              // Bz and Bx of rows s0-2, s0-1, s0
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long r = -(long)(2 - c)*st;
      qz[c] = bcc_from_faces(ldu(bx3m + r, off), ldu(bx3m + r + pst, off));
      const double f = ldu(bx1m + (long)(c - 1)*a1.f1, foff1);
      qx[c] = bcc_from_faces(f, AKMI_LANE_ABOVE(f));
    }
    double pl, dummy;
    plm(qz[0], qz[1], qz[2], pl, dummy);
    W_(5, 0) = qz[1]; W_(5, 1) = qz[2]; PL_(5) = pl;
    plm(qx[0], qx[1], qx[2], pl, dummy);
    W_(6, 0) = qx[1]; W_(6, 1) = qx[2]; PL_(6) = pl;
  }
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    if ((UC && n < 4) || (BF && n >= 5)) continue;
    const double *q = base2(n);
    double pl, dummy;
    const double qa = ldu(q - 2*st, off), qb = ldu(q - st, off), qc = ldu(q, off);
    plm(qa, qb, qc, pl, dummy);
    W_(n, 0) = qb; W_(n, 1) = qc;
    PL_(n) = pl;
  }
#if AKMI_MF_BYTES
  unsigned char *mf2 = a2.mfb + (size_t)m*fs2, *mf1 = a1.mfb + (size_t)m*fs1;
#define ST_MF_ st_mfs
#else
  double *mf2 = a2.flx + (size_t)m*g.nvar*fs2, *mf1 = a1.flx + (size_t)m*g.nvar*fs1;
#define ST_MF_ stu
#endif
  const double *bym = bb + cs;                                                                   // cell-centred By
  const size_t mb = (size_t)m*g.nvar*cs;
  double by_n = BF ? 0.0 : ldu(bym, off - st8), bx1_n = ldu(bx1m, foff1);
  double bx2_p = BF ? ldu(bx2m - a2.f1, foff2) : 0.0;            // BF: x2 face s-1
  for (int t = 0;; ++t) {
    const int s = s0 + t;
    if (s > shi + 1) break;                   // the last chunk ends with the x1 faces of row ju(x1)
    if (t > ml && s <= shi) break;            // the others end with the face they share
    const bool do_x2 = s <= shi;
    const int jr = s - 1;                     // row of the x1 faces of this step
    const bool do_x1 = (t >= 1 || s0 == a2.jl) && jr >= a1.jl && jr <= a1.ju;
    const unsigned orow = off - st8;          // cell (k, jr, i)
    // Every load of the step is unconditional and issued in one group.  (With `do_x2 ? ldu(..) : w1` each of
    // the seven cell loads sat in its own scalar branch followed by s_waitcnt vmcnt(0): eight serialised
    // memory round trips per step, profiles/r03_isa_audit.txt.)  Beyond the last face the address is the
    // row the window already holds, i.e. the value `w1` the old form substituted.
    // BF: the x2 face s is loaded beyond the last face as well (face je+2 exists): By of the last row needs it
    const double bx1 = bx1_n;
    double by_c = by_n;
    if constexpr (!BF) by_n = ldu(bym, off);
    bx1_n = ldu(bx1m + a1.f1, foff1);
    double qn[NV];
    double zlo = 0.0, zhi = 0.0, x1n = 0.0;                 // BF: x3 faces k, k+1 and x1 face i of the row qn holds
    {
      const long stq = do_x2 ? st : 0;
#pragma unroll
      for (int n = 0; n < NV; ++n) {
        if (BF && n >= 5) continue;
        qn[n] = ldu(((UC && n < 4) ? cbase2(n) : base2(n)) + stq, off);
      }
      if constexpr (BF) {
        zlo = ldu(bx3m + stq, off); zhi = ldu(bx3m + stq + pst, off);
        x1n = ldu(bx1m + (do_x2 ? 2 : 1)*(long)a1.f1, foff1);
      }
    }
    const double bx2 = ldu(bx2m, (BF || do_x2) ? foff2 : foff2 - fst28);
    if constexpr (BF) { by_c = bcc_from_faces(bx2_p, bx2); bx2_p = bx2; }
    // ---- x1 face on the low side of cell (k, jr, i): the cell is W_(.,0) of the march
    double f1d, f1x, f1y, f1z, f1e, f1by, f1bz;
    double dF1[5];
    {
      // x1-aligned order d, vx, vy, vz, e, by, bz from the x2-aligned window d, vy, vz, vx, e, bz, bx
      double q0[NV];
      q0[0] = W_(0, 0); q0[1] = W_(3, 0); q0[2] = W_(1, 0); q0[3] = W_(2, 0); q0[4] = W_(4, 0);
      q0[5] = by_c; q0[6] = W_(5, 0);
      const double bxc = W_(6, 0);
      double qln[NV], qr[NV];
#pragma unroll
      for (int n = 0; n < NV; ++n) {
        const double qm = AKMI_LANE_BELOW(q0[n]), qp = AKMI_LANE_ABOVE(q0[n]);
        plm(qm, q0[n], qp, qln[n], qr[n]);
      }
      if (do_x1 && inner && i >= a1.il - 1 && i <= a1.iu) {          // cell-centred E = -(v x B)
        stu(a1.ecc1 + (size_t)m*cs, orow, q0[3]*q0[5] - q0[2]*q0[6]);
        stu(a1.ecc2 + (size_t)m*cs, orow, q0[1]*q0[6] - q0[3]*bxc);
        stu(a1.ecc3 + (size_t)m*cs, orow, q0[2]*bxc - q0[1]*q0[5]);
      }
      double L1[NV];
#pragma unroll
      for (int n = 0; n < NV; ++n) L1[n] = AKMI_LANE_BELOW(qln[n]);
      Cons1D f1 = riemann_mhd_e<RS, AKMI_X12S_EO1 != 0, AKMI_X12S_FM != 0>(eos, L1[0], L1[1], L1[2], L1[3], L1[4], L1[5], L1[6], qr[0],
                                    qr[1], qr[2], qr[3], qr[4], qr[5], qr[6], bx1);
      f1d = f1.d; f1x = f1.mx; f1y = f1.my; f1z = f1.mz; f1e = f1.e; f1by = f1.by; f1bz = f1.bz;
      dF1[0] = AKMI_LANE_ABOVE(f1d) - f1d;
      dF1[1] = AKMI_LANE_ABOVE(f1x) - f1x;
      dF1[2] = AKMI_LANE_ABOVE(f1y) - f1y;
      dF1[3] = AKMI_LANE_ABOVE(f1z) - f1z;
      dF1[4] = AKMI_LANE_ABOVE(f1e) - f1e;
      if (do_x1 && x1_ok) {
        ST_MF_(mf1, foff1, f1d);
        stu(a1.ey + (size_t)m*cs, orow, -f1by);
        stu(a1.ez + (size_t)m*cs, orow, f1bz);
      }
    }
    // ---- x2 face s
    if constexpr (UC) {
      double di;
      const double m2 = qn[1], m3 = qn[2], m1 = qn[3];
      vel_from_cons(qn[0], m1, m2, m3, di, qn[3], qn[1], qn[2]);
    }
    if constexpr (BF) { qn[5] = bcc_from_faces(zlo, zhi); qn[6] = bcc_from_faces(x1n, AKMI_LANE_ABOVE(x1n)); }
    double L[NV], R[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      double qln2;
      L[n] = PL_(n);
      const double w0 = W_(n, 0), w1 = W_(n, 1);
      const double qp = qn[n];
      plm(w0, w1, qp, qln2, R[n]);
      W_(n, 0) = w1; W_(n, 1) = qp;
      PL_(n) = qln2;
    }
    Cons1D f2 = riemann_mhd_e<RS, AKMI_X12S_EO2 != 0, AKMI_X12S_FM != 0>(eos, L[0], L[1], L[2], L[3], L[4], L[5], L[6], R[0], R[1],
                                  R[2], R[3], R[4], R[5], R[6], bx2);
    if (do_x2 && x2_ok && (t < ml || s == shi)) {
      ST_MF_(mf2, foff2, f2.d);
      stu(a2.ey + (size_t)m*cs, off, -f2.by);
      stu(a2.ez + (size_t)m*cs, off, f2.bz);
    }
    // x2 flux in natural component order: d, m1, m2, m3, E  (ivx = 2, ivy = 3, ivz = 1)
    const double fv[5] = {f2.d, f2.mz, f2.mx, f2.my, f2.e};
    const int sc = s - 1;
    if (do_x2 && t > 0 && col_active && sc >= g.js && sc <= g.je) {
      if (p2) {
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          double divf = ldexp(dF1[n], n1);
          divf += ldexp(fv[n] - FP_(n), n2);
          stu(u.acc + mb + n*cs, orow, divf);
        }
      } else {
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          double divf = dF1[n]/dx1;
          divf += (fv[n] - FP_(n))/dx2;
          stu(u.acc + mb + n*cs, orow, divf);
        }
      }
    }
#pragma unroll
    for (int n = 0; n < 5; ++n) FP_(n) = fv[n];
    off += st8; foff2 += fst28; foff1 += fst18;
  }
#undef ST_MF_
#undef W_
#undef PL_
#undef FP_
}

int launch_sweep12s(const Geo &g, const Scheme &sc, const SweepArgs &a1, const SweepArgs &a2,
                    const UpdArgs &u, hipStream_t st, bool uc, bool bf, const double *bx3f) {
  const long np = (long)(a2.ku - a2.kl + 1)*g.N1;          // flattened (k,i) rows
  const long nwaves = (np + (SX - 4) - 1)/(SX - 4);
  const unsigned nb = (unsigned)((nwaves + SY - 1)/SY);
  const int nc = a2.ju - a2.jl > 0 ? a2.ju - a2.jl : 1;
  const int ml = march_len(nb, nc, g.nmb, ML, 3);
  dim3 grid(nb, cdiv(nc, ml), g.nmb), block(SX, SY);
  const int rs = sc.rsolver;
  if (sc.iso || sc.recon != 1 || rs != AKMI_RS_HLLD) { set_error("sweep12s: PLM + HLLD, ideal gas"); return AKMI_FAIL; }
  if (bf && g.ng < 2) { set_error("sweep12s: the face form reads rows js-2 .. je+2"); return AKMI_FAIL; }
  if (uc && bf) k_sweep12s<3, true, true><<<grid, block, 0, st>>>(g, sc.eos, a1, a2, u, ml, bx3f);
  else if (uc) k_sweep12s<3, true, false><<<grid, block, 0, st>>>(g, sc.eos, a1, a2, u, ml, bx3f);
  else if (bf) k_sweep12s<3, false, true><<<grid, block, 0, st>>>(g, sc.eos, a1, a2, u, ml, bx3f);
  else k_sweep12s<3><<<grid, block, 0, st>>>(g, sc.eos, a1, a2, u, ml, bx3f);
  AKMI_CHECK_LAUNCH("sweep12s");
  return AKMI_COMPLETE;
}

// ---------------------------------------------------------------------------------------
// Corner EMFs (mhd_corner_e.cpp:338-414) from face EMFs, cell-centred EMFs and mass-flux
// signs.  All operands are loaded unconditionally and chosen with selects.
__device__ __forceinline__ double upw(bool pos, double fa, double ca, double fb, double cb) {
  return pos ? (fa - ca) : (fb - cb);
}

// ---------------------------------------------------------------------------------------
// CornerE + CT in ONE kernel (3-D).  The corner EMFs never go to memory: a workgroup owns a
// (j,i) tile with a one-column/one-row overlap, marches along k, exchanges the three edge values
// of a plane through LDS (i+1 and j+1 neighbours) and keeps its own previous plane in registers
// (k+1 differences), so that
//     x3-faces of plane k         are updated at step k      (need e1,e2 of plane k),
//     x1-/x2-faces of plane k-1   are updated at step k      (need e3 of plane k-1, e1/e2 of both).
// The k-1 operands of the corner formulas are the previous step's k operands (25 instead of 33
// loads per corner).  Every face is read and written by exactly one thread (the overlap
// column/row only computes edges), so the in-place update of b0 has no cross-workgroup hazard.
// Arithmetic: the expressions of akmi_mhd_corner_e (akmi_tasks.hip) and k_ct_copy, unchanged.
#ifndef AKMI_CKL
#define AKMI_CKL 32
#endif
#ifndef AKMI_CT_XCD_ROWS
#define AKMI_CT_XCD_ROWS 1
#endif
constexpr int CKL = AKMI_CKL;          // cell planes per k-chunk (one plane of edges recomputed)

// The tile of edge positions is tw x th threads (owners: (tw-1) x (th-1)), lanes flattened over
// (ty, tx); the launcher picks the shape that wastes the fewest lanes for the block size (a 64-wide
// tile needs two columns of tiles for the 65 edge columns of a 64^3 MeshBlock, a 34 x 15 tile does
// 33 / 65 / 257 columns in 1 / 2 / 8).
// Tile shape of k_corner_ct for e1 x e2 edge positions, among the shapes of at most 512 threads:
// lanes launched (tiles x padded workgroup size), weighted by what the scan in
// profiles/r01_v12_ct_tiles.txt shows -- short rows cost coalescing (~ 1 + 20/tw per lane), few
// rows re-read the j-1 neighbours more often (~ 1 + 0.6/(th-1)), and a workgroup of 7 waves leaves
// 2 of the 16 wave slots of a CU empty (106 VGPRs: 4 waves per SIMD).
constexpr int CT_THREADS = 512;        // 8 waves: two workgroups per CU hide each other's barriers
struct CtTile { int tw, th, n1, n2, threads; };
static CtTile ct_tile(int e1, int e2) {
  static int f_tw = -1, f_th = 0;
  if (f_tw < 0) {                                    // AKMI_CT_TILE=tw,th pins the shape (experiments)
    const char *e = getenv("AKMI_CT_TILE");
    f_tw = 0;
    if (e && sscanf(e, "%d,%d", &f_tw, &f_th) != 2) f_tw = 0;
    if (f_tw < 2 || f_th < 2 || f_tw*f_th > CT_THREADS) f_tw = 0;
  }
  CtTile best{0, 0, 0, 0, 0};
  double best_cost = -1.0;
  for (int n1 = 1; n1 <= e1; ++n1) {
    const int tw = (e1 + n1 - 1)/n1 + 1;
    if (tw > 130) continue;
    if (tw < 18 && n1 > 1) break;
    for (int th = 3; th <= 32; ++th) {
      if (tw*th > CT_THREADS) break;
      if (f_tw > 0 && (tw != f_tw || th != f_th)) continue;
      const int n2 = (e2 + th - 2)/(th - 1);
      const int threads = (tw*th + 63)/64*64;
      const int waves = threads/64;
      const double cost = (double)n1*n2*threads*(6.3 + 130.0/tw)*(1.0 + 0.6/(th - 1))*16.0/(16/waves*waves);
      if (best_cost < 0 || cost < best_cost) { best = CtTile{tw, th, n1, n2, threads}; best_cost = cost; }
    }
  }
  if (best_cost < 0) {                               // pinned shape not among the candidates
    const int tw = f_tw, th = f_th;
    best = CtTile{tw, th, (e1 + tw - 2)/(tw - 1), (e2 + th - 2)/(th - 1), (tw*th + 63)/64*64};
  }
  return best;
}

// MFB: flx1..3 are the byte arrays of the mass-flux signs (AKMI_MF_BYTES), else the flux arrays whose variable 0 is compared
template <bool P2, bool MFB>
__device__ __forceinline__ void corner_ct_body(const Geo &g, const double *__restrict__ e3x1, const double *__restrict__ e2x1,
            const double *__restrict__ e1x2, const double *__restrict__ e3x2,
            const double *__restrict__ e2x3, const double *__restrict__ e1x3,
            const double *__restrict__ c1, const double *__restrict__ c2,
            const double *__restrict__ c3, const double *__restrict__ flx1,
            const double *__restrict__ flx2, const double *__restrict__ flx3, double gam0,
            double gam1, double beta_dt, double *__restrict__ b0x1f, double *__restrict__ b0x2f,
            double *__restrict__ b0x3f, double *__restrict__ b1x1f, double *__restrict__ b1x2f,
            double *__restrict__ b1x3f, int copy_b1, int kA, int kB, int top, int nchunk,
            int ckl, int tw, int th, const double *dtp) {
  beta_dt = beta_dt_of(beta_dt, dtp);
  extern __shared__ double ct_lds[];     // e1, e2: 2 planes each, e3: 3 planes of th x tw
  const int plane = tw*th;
#define S1(p, y, x) ct_lds[(p)*plane + (y)*tw + (x)]
#define S2(p, y, x) ct_lds[(2 + (p))*plane + (y)*tw + (x)]
#define S3(p, y, x) ct_lds[(4 + (p))*plane + (y)*tw + (x)]
  const int ty = threadIdx.x/tw, tx = threadIdx.x - ty*tw;
  const bool in_tile = ty < th;          // the workgroup is padded to whole waves
  // (xcd_order, which pays in the hydro tile kernel, costs this bandwidth-bound one 2 %: 659 -> 675 us, profiles/r05_mhd_ab.txt)
  // Workgroup -> tile: the tiles of one tile ROW (same j range, same k-chunk: neighbours in x1, whose edge columns and
  // unaligned row ends share 64-/128-byte pieces of every operand row) go to ONE XCD, consecutive rows to consecutive
  // XCDs, so that all eight L2s stream through the same planes at the same time: 625 -> 617 us at 256^3
  // (profiles/r05_corner_ct_xcd_rows.txt; a whole k-chunk per XCD, xcd_order, costs 2 %).
  unsigned bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (AKMI_CT_XCD_ROWS) {
    const unsigned n1 = gridDim.x, nrows = gridDim.y*gridDim.z, full = nrows & ~7u;
    const unsigned b = bx + n1*(by + gridDim.y*bz);
    if (b < n1*full) {                                           // whole groups of eight rows; the rest keeps its place
      const unsigned xcd = b & 7u, slot = b >> 3;
      const unsigned rl = slot/n1;
      bx = slot - rl*n1;
      const unsigned R = rl*8u + xcd;
      bz = R/gridDim.y; by = R - bz*gridDim.y;
    }
  }
  const int i = g.is + bx*(tw - 1) + tx;
  const int j = g.js + by*(th - 1) + ty;
  const int m = bz/nchunk;
  const int ch = bz - m*nchunk;
  const int k0 = kA + ch*ckl;                                   // first cell plane of this chunk
  const int k1 = (k0 + ckl - 1 < kB) ? k0 + ckl - 1 : kB;       // last cell plane
  const bool wtop = top && (k1 == kB);                          // this chunk owns the x3-faces kB+1
  const bool edge_ok = in_tile && (i <= g.ie + 1) && (j <= g.je + 1);
  const bool own = edge_ok && (tx < tw - 1) && (ty < th - 1);
  const double dx1 = g.dx[3*m], dx2 = g.dx[3*m + 1], dx3 = g.dx[3*m + 2];
  // cell sizes that are powers of two: x/dx == x*(1/dx) bit for bit (wave-uniform choice)
  const bool p2 = P2 && is_pow2(dx1) && is_pow2(dx2) && is_pow2(dx3);
  const int ndx1 = pow2_shift(dx1), ndx2 = pow2_shift(dx2), ndx3 = pow2_shift(dx3);
#define DIVX(x, q) (p2 ? ldexp((x), n##q) : (x)/q)
  // addresses: scalar base of (block, array) + a 32-bit byte offset per lane and array shape, advanced by one
  // plane per step (no 64-bit index arithmetic on the vector unit, fewer address registers)
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const long PS = (long)g.N2*g.N1, PS1 = (long)g.N2*(g.N1 + 1), PS2 = (long)(g.N2 + 1)*g.N1;   // plane strides
  unsigned oc = (((unsigned)k0*(unsigned)g.N2 + (unsigned)j)*(unsigned)g.N1 + (unsigned)i)*8u;            // (.., N2, N1)
  unsigned o1 = (((unsigned)k0*(unsigned)g.N2 + (unsigned)j)*(unsigned)(g.N1 + 1) + (unsigned)i)*8u;      // (.., N2, N1+1)
  unsigned o2 = (((unsigned)k0*(unsigned)(g.N2 + 1) + (unsigned)j)*(unsigned)g.N1 + (unsigned)i)*8u;      // (.., N2+1, N1)
  using MF = std::conditional_t<MFB, unsigned char, double>;
  const size_t mfv = MFB ? 1 : (size_t)g.nvar;
  const MF *f1m = reinterpret_cast<const MF *>(flx1) + (size_t)m*mfv*g.N3*PS1,
           *f2m = reinterpret_cast<const MF *>(flx2) + (size_t)m*mfv*g.N3*PS2,
           *f3m = reinterpret_cast<const MF *>(flx3) + (size_t)m*mfv*(g.N3 + 1)*PS;
  auto mf_ge0 = [](const MF *__restrict__ q, unsigned ob) -> bool {        // mass flux >= 0 on the face at byte offset ob / 8 B
    if constexpr (MFB) return ld_mfs(q, ob); else return ldu(q, ob) >= 0.0;
  };
  const double *x31 = e3x1 + (size_t)m*cs, *x21 = e2x1 + (size_t)m*cs, *x12 = e1x2 + (size_t)m*cs,
               *x32 = e3x2 + (size_t)m*cs, *x23 = e2x3 + (size_t)m*cs, *x13 = e1x3 + (size_t)m*cs;
  const double *c1m = c1 + (size_t)m*cs, *c2m = c2 + (size_t)m*cs, *c3m = c3 + (size_t)m*cs;
  double *b01 = b0x1f + (size_t)m*g.N3*PS1, *b02 = b0x2f + (size_t)m*g.N3*PS2, *b03 = b0x3f + (size_t)m*(g.N3 + 1)*PS;
  double *b11 = b1x1f + (size_t)m*g.N3*PS1, *b12 = b1x2f + (size_t)m*g.N3*PS2, *b13 = b1x3f + (size_t)m*(g.N3 + 1)*PS;
  double e1p = 0.0, e2p = 0.0, e3p = 0.0;                       // own edges of the previous plane
  // operands of the corner formulas that belong to plane k-1 (rolled from step to step)
  double x2_km = 0.0, x1_km = 0.0, c1_mm = 0.0, c1_m0 = 0.0, c2_mm = 0.0, c2_m0 = 0.0;
  bool f1_km = false, f2_km = false;          // mass flux >= 0 on the x1 / x2 face of plane k-1
  if (edge_ok) {
    f1_km = mf_ge0(f1m - PS1, o1);
    f2_km = mf_ge0(f2m - PS2, o2);
    x2_km = ldu(x12 - PS, oc);
    x1_km = ldu(x21 - PS, oc);
    c1_mm = ldu(c1m - PS - g.N1, oc); c1_m0 = ldu(c1m - PS, oc);
    c2_mm = ldu(c2m - PS - 1, oc); c2_m0 = ldu(c2m - PS, oc);
  }
  for (int k = k0; k <= k1 + 1; ++k) {
    const int t = k - k0;
    const int pp2 = t & 1, p3 = t % 3;
    double e1 = 0.0, e2 = 0.0, e3 = 0.0;
    if (edge_ok) {
      bool f1_k, f1_jm, f2_k, f2_im, f3_k, f3_jm, f3_im;     // mass flux >= 0 on the faces round the corner
      f1_k = mf_ge0(f1m, o1);
      f1_jm = mf_ge0(f1m - (g.N1 + 1), o1);
      f2_k = mf_ge0(f2m, o2);
      f2_im = mf_ge0(f2m - 1, o2);
      f3_k = mf_ge0(f3m, oc);
      f3_jm = mf_ge0(f3m - g.N1, oc);
      f3_im = mf_ge0(f3m - 1, oc);
      const double c1_0m = ldu(c1m - g.N1, oc), c1_00 = ldu(c1m, oc);
      const double c2_0m = ldu(c2m - 1, oc), c2_00 = ldu(c2m, oc);
      const double x2_k = ldu(x12, oc), x1_k = ldu(x21, oc);
      {  // E1 (mhd_corner_e.cpp:340-363)
        const double x3_jm = ldu(x13 - g.N1, oc), x3_j = ldu(x13, oc);
        double e1_l3 = upw(f2_km, x3_jm, c1_mm, x3_j, c1_m0);
        double e1_r3 = upw(f2_k, x3_jm, c1_0m, x3_j, c1_00);
        double e1_l2 = upw(f3_jm, x2_km, c1_mm, x2_k, c1_0m);
        double e1_r2 = upw(f3_k, x2_km, c1_m0, x2_k, c1_00);
        e1 = 0.25*(e1_l3 + e1_r3 + e1_l2 + e1_r2 + x2_km + x2_k + x3_jm + x3_j);
      }
      {  // E2 (:365-388)
        const double x3_im = ldu(x23 - 1, oc), x3_i = ldu(x23, oc);
        double e2_l3 = upw(f1_km, x3_im, c2_mm, x3_i, c2_m0);
        double e2_r3 = upw(f1_k, x3_im, c2_0m, x3_i, c2_00);
        double e2_l1 = upw(f3_im, x1_km, c2_mm, x1_k, c2_0m);
        double e2_r1 = upw(f3_k, x1_km, c2_m0, x1_k, c2_00);
        e2 = 0.25*(e2_l3 + e2_r3 + e2_l1 + e2_r1 + x3_im + x3_i + x1_km + x1_k);
      }
      {  // E3 (:390-413)
        const double x2_im = ldu(x32 - 1, oc), x2_i = ldu(x32, oc);
        const double x1_jm = ldu(x31 - g.N1, oc), x1_j = ldu(x31, oc);
        const double c_mm = ldu(c3m - g.N1 - 1, oc), c_m0 = ldu(c3m - g.N1, oc);
        const double c_0m = ldu(c3m - 1, oc), c_00 = ldu(c3m, oc);
        double e3_l2 = upw(f1_jm, x2_im, c_mm, x2_i, c_m0);
        double e3_r2 = upw(f1_k, x2_im, c_0m, x2_i, c_00);
        double e3_l1 = upw(f2_im, x1_jm, c_mm, x1_j, c_0m);
        double e3_r1 = upw(f2_k, x1_jm, c_m0, x1_j, c_00);
        e3 = 0.25*(e3_l1 + e3_r1 + e3_l2 + e3_r2 + x2_im + x2_i + x1_jm + x1_j);
      }
      f1_km = f1_k; f2_km = f2_k; x2_km = x2_k; x1_km = x1_k;
      c1_mm = c1_0m; c1_m0 = c1_00; c2_mm = c2_0m; c2_m0 = c2_00;
    }
    if (in_tile) { S1(pp2, ty, tx) = e1; S2(pp2, ty, tx) = e2; S3(p3, ty, tx) = e3; }
    __syncthreads();
    if (own) {
      if (i <= g.ie && j <= g.je && (k <= k1 || wtop)) {          // x3-face of plane k (mhd_ct.cpp:67-77)
        const double b0v = ldu(b03, oc);
        const double b1v = copy_b1 ? b0v : ldu(b13, oc);
        double b = gam0*b0v + gam1*b1v;
        b -= DIVX(beta_dt*(S2(pp2, ty, tx + 1) - e2), dx1);
        b += DIVX(beta_dt*(S1(pp2, ty + 1, tx) - e1), dx2);
        rk_store_u(b03, b13, copy_b1, oc, b0v, b);
      }
      if (k > k0) {
        const int q3 = (t + 2) % 3;                                // the e3 buffer of plane k-1
        if (j <= g.je) {                                           // x1-face (:45-54)
          const double b0v = ldu(b01 - PS1, o1);
          const double b1v = copy_b1 ? b0v : ldu(b11 - PS1, o1);
          double b = gam0*b0v + gam1*b1v;
          b -= DIVX(beta_dt*(S3(q3, ty + 1, tx) - e3p), dx2);
          b += DIVX(beta_dt*(e2 - e2p), dx3);
          rk_store_u(b01 - PS1, b11 - PS1, copy_b1, o1, b0v, b);
        }
        if (i <= g.ie) {                                           // x2-face (:56-65)
          const double b0v = ldu(b02 - PS2, o2);
          const double b1v = copy_b1 ? b0v : ldu(b12 - PS2, o2);
          double b = gam0*b0v + gam1*b1v;
          b += DIVX(beta_dt*(S3(q3, ty, tx + 1) - e3p), dx1);
          b -= DIVX(beta_dt*(e1 - e1p), dx3);
          rk_store_u(b02 - PS2, b12 - PS2, copy_b1, o2, b0v, b);
        }
      }
    }
    e1p = e1; e2p = e2; e3p = e3;
    oc += (unsigned)PS*8u; o1 += (unsigned)PS1*8u; o2 += (unsigned)PS2*8u;
  }
}
#undef DIVX

#ifndef AKMI_CT_WAVES
#define AKMI_CT_WAVES 6         // waves per SIMD the register allocation aims at: 66 VGPRs, three workgroups per CU
#endif                          // (two at the 114 VGPRs the compiler takes when left alone: 640-665 us against 621)
template <bool MFB>
__global__ void __launch_bounds__(CT_THREADS, AKMI_CT_WAVES)
k_corner_ct(Geo g, const double *__restrict__ e3x1, const double *__restrict__ e2x1,
            const double *__restrict__ e1x2, const double *__restrict__ e3x2,
            const double *__restrict__ e2x3, const double *__restrict__ e1x3,
            const double *__restrict__ c1, const double *__restrict__ c2,
            const double *__restrict__ c3, const double *__restrict__ flx1,
            const double *__restrict__ flx2, const double *__restrict__ flx3, double gam0,
            double gam1, double beta_dt, double *__restrict__ b0x1f, double *__restrict__ b0x2f,
            double *__restrict__ b0x3f, double *__restrict__ b1x1f, double *__restrict__ b1x2f,
            double *__restrict__ b1x3f, int copy_b1, int kA, int kB, int top, int nchunk,
            int ckl, int tw, int th, const double *dtp) {
  corner_ct_body<AKMI_POW2DX != 0, MFB>(g, e3x1, e2x1, e1x2, e3x2, e2x3, e1x3, c1, c2, c3, flx1, flx2, flx3, gam0,
                                   gam1, beta_dt, b0x1f, b0x2f, b0x3f, b1x1f, b1x2f, b1x3f, copy_b1, kA, kB, top,
                                   nchunk, ckl, tw, th, dtp);
}

// CT (mhd_ct.cpp:23-80) with CopyCons for B folded in at stage 1 (b1 <- b0 old)
__global__ void __launch_bounds__(SX*SY)
k_ct_copy(Geo g, double gam0, double gam1, double beta_dt, const double *__restrict__ e1,
          const double *__restrict__ e2, const double *__restrict__ e3, double *__restrict__ b0x1f,
          double *__restrict__ b0x2f, double *__restrict__ b0x3f, double *__restrict__ b1x1f,
          double *__restrict__ b1x2f, double *__restrict__ b1x3f, int copy_b1, int k0, int nk,
          int kb, const double *dtp) {
  beta_dt = beta_dt_of(beta_dt, dtp);
  // planes k in [k0, k0+nk-1]; x1f/x2f faces are updated for k <= kb (cells of this slab),
  // x3f faces for every k of the launch (the last slab also owns face ke+1)
  const long p = ((long)blockIdx.x*SY + threadIdx.y)*SX + threadIdx.x;   // rows [js,je+1] x N1
  const int jj = (int)(p/g.N1);
  const int i = (int)(p - (long)jj*g.N1);
  const int j = g.js + jj;
  const int m = blockIdx.z/nk;
  const int k = k0 + (blockIdx.z - m*nk);
  if (i < g.is || i > g.ie + 1 || j > g.je + 1) return;
  const double dx1 = g.dx[3*m], dx2 = g.dx[3*m + 1], dx3 = g.dx[3*m + 2];
#define E1(k, j, i) e1[ix4(g.N3 + 1, g.N2 + 1, g.N1, m, k, j, i)]
#define E2(k, j, i) e2[ix4(g.N3 + 1, g.N2, g.N1 + 1, m, k, j, i)]
#define E3(k, j, i) e3[ix4(g.N3, g.N2 + 1, g.N1 + 1, m, k, j, i)]
  if (j <= g.je && k <= kb) {
    size_t c = ix4(g.N3, g.N2, g.N1 + 1, m, k, j, i);
    const double b0v = b0x1f[c];
    const double b1v = copy_b1 ? b0v : b1x1f[c];
    if (g.multi_d) {
      double b = gam0*b0v + gam1*b1v;
      b -= beta_dt*(E3(k, j + 1, i) - E3(k, j, i))/dx2;
      if (g.three_d) b += beta_dt*(E2(k + 1, j, i) - E2(k, j, i))/dx3;
      rk_store(b0x1f, b1x1f, copy_b1, c, b0v, b);
    } else if (copy_b1) {
      b1x1f[c] = b0v;                  // 1-D: bx is constant; either way the register receives it
    }
  }
  if (i <= g.ie && k <= kb) {
    size_t c = ix4(g.N3, g.N2 + 1, g.N1, m, k, j, i);
    const double b0v = b0x2f[c];
    const double b1v = copy_b1 ? b0v : b1x2f[c];
    double b = gam0*b0v + gam1*b1v;
    b += beta_dt*(E3(k, j, i + 1) - E3(k, j, i))/dx1;
    if (g.three_d) b -= beta_dt*(E1(k + 1, j, i) - E1(k, j, i))/dx3;
    rk_store(b0x2f, b1x2f, copy_b1, c, b0v, b);
  }
  if (i <= g.ie && j <= g.je) {
    size_t c = ix4(g.N3 + 1, g.N2, g.N1, m, k, j, i);
    const double b0v = b0x3f[c];
    const double b1v = copy_b1 ? b0v : b1x3f[c];
    double b = gam0*b0v + gam1*b1v;
    b -= beta_dt*(E2(k, j, i + 1) - E2(k, j, i))/dx1;
    if (g.multi_d) b += beta_dt*(E1(k, j + 1, i) - E1(k, j, i))/dx2;
    rk_store(b0x3f, b1x3f, copy_b1, c, b0v, b);
  }
#undef E1
#undef E2
#undef E3
}

int launch_corner_ct(const Geo &g, double *const *efc, double *const *ecc, bool mfb, const double *const *mf,
                     const CtArgs &c, hipStream_t st) {
  // corner EMFs of the planes [ks, ke+1] stay on chip
  const CtTile tl = ct_tile(g.nx1 + 1, g.nx2 + 1);
  const int ckl = march_len((long)tl.n1*tl.n2, c.kB - c.kA + 1, g.nmb, CKL);
  const int nchunk = cdiv(c.kB - c.kA + 1, ckl);
  dim3 grid(tl.n1, tl.n2, nchunk*g.nmb), block(tl.threads);
  (mfb ? k_corner_ct<true> : k_corner_ct<false>)<<<grid, block, 7*tl.tw*tl.th*sizeof(double), st>>>(
      g, efc[0], efc[1], efc[2], efc[3], efc[4], efc[5], ecc[0], ecc[1], ecc[2], mf[0], mf[1], mf[2], c.gam0, c.gam1,
      c.beta_dt, c.b0x1f, c.b0x2f, c.b0x3f, c.b1x1f, c.b1x2f, c.b1x3f, c.copy_b1, c.kA, c.kB, 1, nchunk, ckl, tl.tw, tl.th,
      c.dtp);
  AKMI_CHECK_LAUNCH("corner_ct");
  return AKMI_COMPLETE;
}

int launch_ct_copy(const Geo &g, const double *const *e, const CtArgs &c, hipStream_t st) {
  const int nkc = c.kB - c.kA + 2;
  long npc = (long)(g.je - g.js + 2)*g.N1;
  dim3 grid((unsigned)((npc + SX*SY - 1)/(SX*SY)), 1, nkc*g.nmb), block(SX, SY);
  k_ct_copy<<<grid, block, 0, st>>>(g, c.gam0, c.gam1, c.beta_dt, e[0], e[1], e[2], c.b0x1f, c.b0x2f, c.b0x3f, c.b1x1f,
                                    c.b1x2f, c.b1x3f, c.copy_b1, c.kA, nkc, c.kB, c.dtp);
  AKMI_CHECK_LAUNCH("ct");
  return AKMI_COMPLETE;
}

}  // namespace akmi
