// akmi_hydro_stage3d2.hpp -- hydro, 3-D, DC/PLM: the three sweeps and the RK update of a stage in ONE kernel
// (k_hydro_stage3d2, its tile chooser and LDS layout; akmi_stage_hydro.hip instantiates the kernel and defines its
// launcher, akmi_stage.hip takes the tile chooser and the argument types for the plan of a stage).
//
// A workgroup owns a tile of (tw-1) x (th-1) cell columns (lanes flattened over the tw x th positions; the last
// column / row of positions only provides the face on its low side) and marches along k.  Per step k (two barriers):
//   (A) planes k-1 and k of the primitives sit in LDS (2-low / 1-high halo in i and j).  Every cell of plane k-1 is
//       reconstructed ONCE per in-plane direction: its position forms the limited slope from the two LDS
//       neighbours, keeps the value at the cell's low face (right state of its own face) and hands the value at
//       the high face to the position above through LDS (that position's left state).  The cells just outside
//       the tile's low sides (one column, one row) are reconstructed by the first th + tw threads.
//   (B) every position solves its low x1 and x2 face; the flux replaces the left state in the same LDS slot
//       (entry (r,t) changes hands only between threads (r,t-1) / (r-1,t) and (r,t) across a barrier, so one array
//       serves both and nothing is double-buffered).  The x3 face below cell k comes from the position's own entries
//       of the two planes and the pending left state in registers.  Plane k+1, loaded during the step, replaces
//       plane k-1 once its readers are past the in-plane reconstruction.
//   (C) cell k-1 is finished: divf = dF1/dx1; divf += dF2/dx2; divf += dF3/dx3 (hydro_update.cpp:55-80
//       order, the same rounding sequence as the three-kernel path; hydro_fluxes.cpp:44-170, hydro_update.cpp:24-84).
// LDS layout: position-major, the five variables of an entry adjacent (stride 5 doubles: conflict-free for 64-bit
// accesses), so that one address register per thread and array serves every variable and the x-neighbours through
// the instruction's immediate offset; the y-neighbours cost one more register per array.
// HBM traffic per cell: w0 once (+halo, L2 hits: neighbouring tiles share an XCD, xcd_order), u0 (+u1) once --
// no flux or partial divergence arrays.  The CT-extended ranges of MHD do not apply (faces is..ie+1 only).
//
// Where the marching state lives and when memory is touched -- the findings of the MHD analogue k_mhd_stage3d (built in
// round 6, slower than the kernels it would replace and removed: profiles/r06_mhd_stage3d.txt) applied to the kernel
// that has the registers for three waves per SIMD:
//   * with both planes in LDS the cells k-1 and k of the position's own column are read from there for the x3 face, so
//     the ten doubles W0 / W1 stay out of the register file -- no scratch (the one-plane kernel of round 5, removed, saved
//     and restored three doubles per step through scratch, each reload an `s_waitcnt vmcnt(0)`);
//   * every global load is unconditional (lanes without a cell read element 0 of the plane, planes are clamped into the
//     array): a load inside a branch turns the wait for it into a wait for everything at the join;
//   * the loads of plane k+1 are issued after the x1 solve and consumed after the x2 solve, the operands of the update
//     after the x2 solve and consumed after the x3 solve; the stores of a step (u0, mass fluxes) all come after its last
//     wait for a load (with loads and stores both outstanding the compiler's wait for a load is `vmcnt(0)`).
#ifndef AKMI_HYDRO_STAGE3D2_HPP_
#define AKMI_HYDRO_STAGE3D2_HPP_
#include "akmi_stage.hpp"

namespace akmi {

struct HydTile { int tw, th, n1, n2, threads; };
constexpr int HS_THREADS = 512;
#ifndef AKMI_HS2_WAVES
#define AKMI_HS2_WAVES 3                   // waves per SIMD the register allocation aims at
#endif

// LDS of a workgroup, in doubles: the two planes with their halo and two face-shaped arrays
constexpr int HS_ES = 5;                   // doubles per LDS entry (a padded 48-byte stride measured slower: profiles/r05_hydro_ab.txt)
inline size_t hyd_lds_doubles(int tw, int th) { return HS_ES*(2*(size_t)(tw + 3)*(th + 3) + 2*(size_t)tw*th); }

inline HydTile hyd_tile(int c1, int c2) {
  // The kernel is bound by the issue of dependent fp64 chains (1 330 VALU instructions per cell, three waves per SIMD), so
  // what a shape costs is the lanes it launches per owned column, not the length of its rows:
  //   cost = lanes launched (tiles x padded workgroup)
  //   x (1 + 0.3 x plane-with-halo / owners)    the LDS plane every step loads: (tw+3)(th+3) entries for (tw-1)(th-1) owners
  //   x (1 + 4/tw)                              short rows (tw = 9: +15 % measured)
  //   / occupancy                               workgroups per CU by LDS x waves per workgroup, against the 12 waves the
  //                                             168 VGPRs allow
  // fitted to the scans in profiles/r04_hydro_tiles.txt and r05_hydro_ab.txt (256^3, the one-plane kernel: 23 x 11 960 us,
  // 28 x 9 964, 18 x 14 990, 21 x 12 990; 384-thread tiles 27 x 14 / 24 x 16: 1 380-1 480 -- six-wave workgroups leave wave
  // slots idle).
  static const int maxt = getenv("AKMI_HS_MAXT") ? atoi(getenv("AKMI_HS_MAXT")) : 256;   // three four-wave workgroups per CU
  static const int maxlds = getenv("AKMI_HS_LDS") ? atoi(getenv("AKMI_HS_LDS")) : 53*1024;
  static int f_tw = -1, f_th = 0;                        // AKMI_HS_TILE=tw,th pins the shape (experiments)
  if (f_tw < 0) {
    const char *e = getenv("AKMI_HS_TILE");                 // "tw,th" or "twxth"
    f_tw = 0;
    if (e && sscanf(e, "%d%*[,x]%d", &f_tw, &f_th) != 2) f_tw = 0;
    if (f_tw < 4 || f_th < 3 || f_tw*f_th > HS_THREADS) f_tw = 0;
  }
  if (f_tw > 0 && 3*(f_tw + 3) + 3*f_th <= f_tw*f_th &&
      hyd_lds_doubles(f_tw, f_th)*sizeof(double) <= 150*1024)
    return HydTile{f_tw, f_th, (c1 + f_tw - 2)/(f_tw - 1), (c2 + f_th - 2)/(f_th - 1), (f_tw*f_th + 63)/64*64};
  HydTile best{0, 0, 0, 0, 0};
  double best_cost = -1.0;
  for (int n1 = 1; n1 <= c1; ++n1) {
    const int tw = (c1 + n1 - 1)/n1 + 1;
    if (tw > 130) continue;
    if (tw < 8 && n1 > 1) break;
    for (int th = 3; th <= 40; ++th) {
      if (tw*th > maxt) break;
      if (3*(tw + 3) + 3*th > tw*th) continue;         // one halo entry per thread at most
      const size_t lds = hyd_lds_doubles(tw, th)*sizeof(double);
      if (lds > (size_t)maxlds) continue;
      const int n2 = (c2 + th - 2)/(th - 1);
      const int threads = (tw*th + 63)/64*64;
      const int waves_cu = (int)(160*1024/lds)*(threads/64);
      const double occ = (waves_cu < 12 ? waves_cu : 12)/12.0;
      const double halo = (double)(tw + 3)*(th + 3)/((double)(tw - 1)*(th - 1));
      const double cost = (double)n1*n2*threads*(1.0 + 0.3*halo)*(1.0 + 4.0/tw)/occ;
      if (best_cost < 0 || cost < best_cost) { best = HydTile{tw, th, n1, n2, threads}; best_cost = cost; }
    }
  }
  return best;
}

// MASS: passive scalars ride along -- leave the three mass fluxes behind for k_scalar_update
struct Mass3 { double *m1, *m2, *m3; };

// C2P: ConsToPrim of the cell the step finishes (+ the CFL scan on the last stage) in the same kernel -- the new conserved
// state is in registers there, so pass B of the active cells costs five stores instead of a kernel that reads u0 back
// (SingleC2P_IdealHyd, src/eos/ideal_c2p_hyd.hpp:22-66 with its floors and counters; hydro_newdt.cpp:97-118).  The new
// primitives go to ANOTHER array of w0's shape (w_out): neighbouring tiles and chunks still read w0 while this one finishes,
// in place is not possible; the caller swaps the two afterwards and converts the ghost shell after the ghost fill
// (akmi_hydro_c2p_shell).  Ideal gas, no passive scalars.
struct HydC2P {
  unsigned char *flags;       // per cell (m, k, j, i): bit 0 / 1 / 2 = the density / energy / temperature floor acted -- the ghost
                              // fill that follows counts the ghost images of such cells (the reference's counters include them)
  double *w_out;
  Eos eos;
  int do_newdt;
  int *counters;
  double *dt3;
};

// the launcher (akmi_stage_hydro.hip).  tl: the tile of the stage's plan; cpa: ConsToPrim of the finished cells inside the
// kernel, nullptr: update only
template <bool MASS>
int launch_hydro_stage3d(const Geo &g, const Scheme &sc, const HydTile &tl, const double *w0, const UpdArgs &u, int kA,
                         int kB, hipStream_t st, Mass3 ms, const HydC2P *cpa = nullptr);

// Workgroup -> tile order.  Workgroup b of a launch runs on XCD b % 8 (observed placement; nothing below depends on
// it for correctness), and each XCD has its own L2.  A tile kernel whose neighbouring tiles re-read each other's edge
// rows wants neighbours on the SAME XCD at about the same time: XCD x takes the x-th contiguous eighth of the tile
// list, in list order.  The map is a bijection of [0, n) for every n.
__device__ __forceinline__ unsigned xcd_order(unsigned b, unsigned n) {
  const unsigned xcd = b & 7u, slot = b >> 3, q = n >> 3, rem = n & 7u;
  return (xcd < rem ? xcd*(q + 1u) : rem*(q + 1u) + (xcd - rem)*q) + slot;
}

template <int RECON, int RS, bool MASS = false, bool C2P = false>
__global__ void __launch_bounds__(HS_THREADS, AKMI_HS2_WAVES)
k_hydro_stage3d2(Geo g, FaceEos eos, const double *__restrict__ w0, UpdArgs u, int kA, int kB,
                 int nchunk, int ckl, int tw, int th, Mass3 ms, HydC2P cp) {
  static_assert(!C2P || (!MASS && RS < 10), "ConsToPrim inside the stage kernel: ideal gas, no passive scalars");
  static_assert(RECON <= 1, "one-kernel hydro stage: DC and PLM");
  constexpr bool ISO = rs_iso<RS>();        // isothermal: variable 4 (energy) does not exist; its slots stay unused
#define ISOSKIP if (ISO && n == 4) continue
  extern __shared__ double hs_lds[];
  const int pw = tw + 3, ph = th + 3;        // plane with halo: cols i0-2..i0+tw, rows j0-2..j0+th
  const int qn = ph*pw, fn = th*tw;
  constexpr int ES = HS_ES;
  const int PLSZ = ES*qn;                    // doubles per plane: two planes, then the two face arrays
  const int tid = threadIdx.x;
  const int r = tid/tw, t = tid - r*tw;
  const bool in_tile = r < th;
  unsigned bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  {                       // tiles of a k-chunk of a block side by side on one XCD (x fastest, then y, then chunk / block)
    const unsigned lin = xcd_order(bx + gridDim.x*(by + gridDim.y*bz), gridDim.x*gridDim.y*gridDim.z);
    const unsigned row = lin/gridDim.x;
    bx = lin - row*gridDim.x; bz = row/gridDim.y; by = row - bz*gridDim.y;
  }
  const int i0 = g.is + (int)bx*(tw - 1), j0 = g.js + (int)by*(th - 1);
  const int i = i0 + t, j = j0 + r;
  const int m = (int)bz/nchunk;
  const int ch = (int)bz - m*nchunk;
  const int k0 = kA + ch*ckl;
  const int k1 = (k0 + ckl - 1 < kB) ? k0 + ckl - 1 : kB;
  const bool cell_ok = in_tile && i < g.N1 && j < g.N2;                // the column exists in memory
  const bool own = in_tile && t < tw - 1 && r < th - 1 && i <= g.ie && j <= g.je;
  const double dx1 = g.dx[3*m], dx2 = g.dx[3*m + 1], dx3 = g.dx[3*m + 2];
  const bool p2 = AKMI_POW2DX && is_pow2(dx1) && is_pow2(dx2) && is_pow2(dx3);      // wave-uniform
  const int n1 = pow2_shift(dx1), n2 = pow2_shift(dx2), n3 = pow2_shift(dx3);
  const double bdt = to_sgpr(beta_dt_of(u.beta_dt, u.dtp));
  const size_t cs = (size_t)g.N3*g.N2*g.N1, ps = (size_t)g.N2*g.N1;
  const double *wb = w0 + (size_t)m*g.nvar*cs;
  // halo entry of this thread: rows 0,1 and ph-1 in full, columns 0,1 and pw-1 of the tile rows
  int hy = -1, hx = 0;
  {
    const int nh = 3*pw + 3*th;
    if (tid < nh) {
      if (tid < 3*pw) { const int q = tid/pw; hy = q < 2 ? q : ph - 1; hx = tid - q*pw; }
      else { const int q = tid - 3*pw; const int rr = q/3, cc = q - rr*3; hy = 2 + rr; hx = cc < 2 ? cc : pw - 1; }
    }
  }
  const int hj = j0 - 2 + hy, hi = i0 - 2 + hx;
  const bool hload = hy >= 0 && hj < g.N2 && hi < g.N1;      // the halo cell exists in memory (i0 - 2, j0 - 2 >= 0: ng >= 2)
  // the cells just outside the tile's low sides: column 1 of the plane (rows of the tile) and row 1 (columns of the tile),
  // reconstructed by the first th + tw threads, one cell each, in the one direction in which a face of the tile needs them
  int ha = -1, hs = 0, hd = 0;                 // entry below the cell, stride to the cell / the entry above, destination
  if (tid < th) { ha = (tid + 2)*pw*ES; hs = ES; hd = 2*PLSZ + tid*tw*ES; }
  else if (tid < th + tw) { const int c = tid - th; ha = (c + 2)*ES; hs = ES*pw; hd = 2*PLSZ + ES*fn + c*ES; }
  // own entries: cell (r+2, t+2) of a plane, position (r, t) of the two face arrays
  const int qo = in_tile ? ((r + 2)*pw + t + 2)*ES : 0, qy = ES*pw;
  const int xo = in_tile ? 2*PLSZ + (r*tw + t)*ES : 2*PLSZ, x2o = xo + ES*fn, xy = ES*tw;
  const int hq = hy >= 0 ? (hy*pw + hx)*ES : -1;
  // scalar base of (block, variable) + a 32-bit byte offset per lane, advanced by one plane per step
  unsigned oc = (cell_ok ? ((unsigned)j*(unsigned)g.N1 + (unsigned)i)*8u : 0u) + (unsigned)(k0 - 1)*(unsigned)ps*8u;      // plane k-1
  unsigned oh = (hload ? ((unsigned)hj*(unsigned)g.N1 + (unsigned)hi)*8u : 0u) + (unsigned)(k0 - 1)*(unsigned)ps*8u;
  const size_t mb = (size_t)m*g.nvar*cs;
  double *u0m = u.u0 + mb, *u1m = u.u1 + mb;
  const double *u1s = u.copy_u1 ? u0m : u1m;             // first stage: the second register is not read (the load repeats u0's)
  // Plane kk lives in slot (kk - k0 + 1) & 1.
  double PL[5], F3p[5];
  {
    double qa[5], qb[5], qc[5], qh[5];
    const long sa = k0 >= 2 ? -(long)ps : 0;             // plane k0-2 (k0-1 where it does not exist: the value is not used)
#pragma unroll
    for (int n = 0; n < 5; ++n) {
      ISOSKIP;
      const double *q = wb + n*cs;
      qa[n] = ldu(q + sa, oc); qb[n] = ldu(q, oc); qc[n] = ldu(q + ps, oc); qh[n] = ldu(q + ps, oh);
    }
#pragma unroll
    for (int n = 0; n < 5; ++n) {
      ISOSKIP;
      if constexpr (RECON == 1) { double dummy; plm(qa[n], qb[n], qc[n], PL[n], dummy); }
      else PL[n] = qb[n];
      if (in_tile) { hs_lds[qo + n] = qb[n]; hs_lds[PLSZ + qo + n] = qc[n]; }      // own entries of planes k0-1 and k0
      if (hq >= 0) hs_lds[PLSZ + hq + n] = qh[n];
    }
  }
#pragma unroll
  for (int n = 0; n < 5; ++n) F3p[n] = 0.0;
  double mv1 = 0.0, mv2 = 0.0, mv3 = 0.0;           // C2P, last stage: running maxima of |v| + c_s over the thread's cells
  double *wom = C2P ? cp.w_out + (size_t)m*g.nvar*cs : nullptr;
  // step k: x3 face k (below cell k); for k > k0 also the x1/x2 faces of plane k-1, which finishes cell k-1;
  // plane k+1 (loaded during the step) replaces plane k-1
  for (int k = k0; k <= k1 + 1; ++k) {
    const bool plane = k > k0;                        // workgroup-uniform
    const long s2 = (k + 1 < g.N3) ? 2*(long)ps : (long)ps;            // plane k+1 relative to plane k-1 (clamped into the array)
    const bool upd = plane && own;
    const int pP = ((k - k0) & 1) ? PLSZ : 0, pC = PLSZ - pP;          // slots of plane k-1 and of plane k
    const int qP = qo + pP, qC = qo + pC;
    double f1[5] = {0, 0, 0, 0, 0}, f2[5] = {0, 0, 0, 0, 0};      // this position's own in-plane fluxes
    double wp[5] = {0, 0, 0, 0, 0}, hv[5] = {0, 0, 0, 0, 0};
    if (!plane) {
#pragma unroll
      for (int n = 0; n < 5; ++n) { ISOSKIP; wp[n] = ldu(wb + n*cs + s2, oc); hv[n] = ldu(wb + n*cs + s2, oh); }
    } else {
      // (A) every cell of plane k-1 once per direction
      double R1[5] = {0, 0, 0, 0, 0}, R2[5] = {0, 0, 0, 0, 0};
      if (in_tile) {
        double W0[5], Wl[5], Wr[5], Wd[5], Wu[5], U1[5] = {0, 0, 0, 0, 0}, U2[5] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          ISOSKIP;
          W0[n] = hs_lds[qP + n];
          if constexpr (RECON == 1) {
            Wl[n] = hs_lds[qP - ES + n]; Wr[n] = hs_lds[qP + ES + n];
            Wd[n] = hs_lds[qP - qy + n]; Wu[n] = hs_lds[qP + qy + n];
          }
        }
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          ISOSKIP;
          if constexpr (RECON == 1) {
            plm(Wl[n], W0[n], Wr[n], U1[n], R1[n]);
            plm(Wd[n], W0[n], Wu[n], U2[n], R2[n]);
          } else {
            R1[n] = W0[n]; R2[n] = W0[n]; U1[n] = W0[n]; U2[n] = W0[n];
          }
        }
        if (t + 1 < tw) {
#pragma unroll
          for (int n = 0; n < 5; ++n) { ISOSKIP; hs_lds[xo + ES + n] = U1[n]; }
        }
        if (r + 1 < th) {
#pragma unroll
          for (int n = 0; n < 5; ++n) { ISOSKIP; hs_lds[x2o + xy + n] = U2[n]; }
        }
      }
      if (ha >= 0) {
        const int hA = ha + pP;
        double ea[5], eb[5], ec[5];              // all three cells requested before the first limiter
#pragma unroll
        for (int n = 0; n < 5; ++n) { ISOSKIP; ea[n] = hs_lds[hA + n]; eb[n] = hs_lds[hA + hs + n]; ec[n] = hs_lds[hA + 2*hs + n]; }
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          ISOSKIP;
          if constexpr (RECON == 1) {
            double up, dummy;
            plm(ea[n], eb[n], ec[n], up, dummy);
            hs_lds[hd + n] = up;
          } else {
            hs_lds[hd + n] = eb[n];
          }
        }
      }
      __syncthreads();
      // (B) the two in-plane faces of this position; the flux takes the place of the left state
      if (in_tile) {
        double fd, fx, fy, fz, fe;
        riemann_hyd_e<RS, true>(eos, hs_lds[xo], hs_lds[xo + 1], hs_lds[xo + 2], hs_lds[xo + 3], ISO ? 0.0 : hs_lds[xo + 4],
                                R1[0], R1[1], R1[2], R1[3], R1[4], fd, fx, fy, fz, fe);
        hs_lds[xo] = fd; hs_lds[xo + 1] = fx; hs_lds[xo + 2] = fy; hs_lds[xo + 3] = fz;
        if constexpr (!ISO) hs_lds[xo + 4] = fe;
        f1[0] = fd; f1[1] = fx; f1[2] = fy; f1[3] = fz; f1[4] = fe;
      }
      __builtin_amdgcn_sched_barrier(0);
      // cell k+1 of the column and of the thread's halo entry: in flight during the x2 solve
#pragma unroll
      for (int n = 0; n < 5; ++n) { ISOSKIP; wp[n] = ldu(wb + n*cs + s2, oc); hv[n] = ldu(wb + n*cs + s2, oh); }
      __builtin_amdgcn_sched_barrier(0);
      if (in_tile) {  // sweep-aligned order (d, vy, vz, vx, e)
        double fd, fx, fy, fz, fe;
        riemann_hyd_e<RS, true>(eos, hs_lds[x2o], hs_lds[x2o + 2], hs_lds[x2o + 3], hs_lds[x2o + 1], ISO ? 0.0 : hs_lds[x2o + 4],
                                R2[0], R2[2], R2[3], R2[1], R2[4], fd, fx, fy, fz, fe);
        hs_lds[x2o] = fd; hs_lds[x2o + 2] = fx; hs_lds[x2o + 3] = fy; hs_lds[x2o + 1] = fz;
        if constexpr (!ISO) hs_lds[x2o + 4] = fe;
        f2[0] = fd; f2[2] = fx; f2[3] = fy; f2[1] = fz; f2[4] = fe;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // x3 face below cell k: sweep-aligned order (d, vz, vx, vy, e).  Cells k-1 and k are the position's entries of the two
    // planes; plane k+1 then takes the place of plane k-1 (every reader of it is past (A))
    double L[5] = {0, 0, 0, 0, 0}, R[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int n = 0; n < 5; ++n) {
      ISOSKIP;
      if constexpr (RECON == 1) {
        double qln;
        L[n] = PL[n];
        plm(hs_lds[qP + n], hs_lds[qC + n], wp[n], qln, R[n]);
        PL[n] = qln;
      } else {
        L[n] = hs_lds[qP + n]; R[n] = hs_lds[qC + n];
      }
    }
    if (in_tile) {
#pragma unroll
      for (int n = 0; n < 5; ++n) { ISOSKIP; hs_lds[qP + n] = wp[n]; }
    }
    if (hq >= 0) {
#pragma unroll
      for (int n = 0; n < 5; ++n) { ISOSKIP; hs_lds[hq + pP + n] = hv[n]; }
    }
    __builtin_amdgcn_sched_barrier(0);
    double pu0[5] = {0, 0, 0, 0, 0}, pu1[5] = {0, 0, 0, 0, 0};
    // operands of the update: in flight during the x3 solve
#pragma unroll
    for (int n = 0; n < 5; ++n) { ISOSKIP; pu0[n] = ldu(u0m + n*cs, oc); pu1[n] = ldu(u1s + n*cs, oc); }
    __builtin_amdgcn_sched_barrier(0);
    double f3[5];
    {
      double fd, fx, fy, fz, fe;
      riemann_hyd_e<RS, true>(eos, L[0], L[3], L[1], L[2], L[4], R[0], R[3], R[1], R[2], R[4], fd, fx, fy, fz, fe);
      f3[0] = fd; f3[3] = fx; f3[1] = fy; f3[2] = fz; f3[4] = fe;
    }
    __syncthreads();
    if (upd) {                                         // (C) finish cell k-1
      double divf[5];
      if (p2) {                                        // one wave-uniform branch for the fifteen quotients
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          ISOSKIP;
          divf[n] = ldexp(hs_lds[xo + ES + n] - f1[n], n1);
          divf[n] += ldexp(hs_lds[x2o + xy + n] - f2[n], n2);
          divf[n] += ldexp(f3[n] - F3p[n], n3);
        }
      } else {
#pragma unroll
        for (int n = 0; n < 5; ++n) {
          ISOSKIP;
          divf[n] = (hs_lds[xo + ES + n] - f1[n])/dx1;
          divf[n] += (hs_lds[x2o + xy + n] - f2[n])/dx2;
          divf[n] += (f3[n] - F3p[n])/dx3;
        }
      }
      double un[5] = {0, 0, 0, 0, 0};
#pragma unroll
      for (int n = 0; n < 5; ++n) { ISOSKIP; un[n] = u.gam0*pu0[n] + u.gam1*pu1[n] - bdt*divf[n]; }
      if constexpr (C2P) {
        double wd, wvx, wvy, wvz, we;
        bool dfl = false, efl = false, tfl = false;
        c2p_hyd<true>(cp.eos, un[0], un[1], un[2], un[3], un[4], wd, wvx, wvy, wvz, we, dfl, efl, tfl);   // floors rewrite un[0] / un[4]
        if (dfl) atomicAdd(&cp.counters[0], 1);
        if (efl) atomicAdd(&cp.counters[1], 1);
        if (tfl) atomicAdd(&cp.counters[2], 1);
        cp.flags[(size_t)m*cs + (oc >> 3)] = (unsigned char)((dfl ? 1 : 0) | (efl ? 2 : 0) | (tfl ? 4 : 0));
        stu(wom, oc, wd); stu(wom + cs, oc, wvx); stu(wom + 2*cs, oc, wvy); stu(wom + 3*cs, oc, wvz); stu(wom + 4*cs, oc, we);
        if (cp.do_newdt) {
          double a1, a2, a3;
          max_speeds_ideal<false>(cp.eos.gamma, wd, wvx, wvy, wvz, we, 0.0, 0.0, 0.0, a1, a2, a3);
          mv1 = fmax(mv1, a1); mv2 = fmax(mv2, a2); mv3 = fmax(mv3, a3);
        }
      }
#pragma unroll
      for (int n = 0; n < 5; ++n) { ISOSKIP; rk_store_u(u0m + n*cs, u1m + n*cs, u.copy_u1, oc, pu0[n], un[n]); }
    }
    if constexpr (MASS) {                              // passive scalars ride on the mass fluxes (k_scalar_update)
      if (plane && in_tile) {
        if (i <= g.ie + 1 && j <= g.je) ms.m1[ix5(g.nvar, g.N3, g.N2, g.N1 + 1, m, 0, k - 1, j, i)] = f1[0];
        if (i <= g.ie && j <= g.je + 1) ms.m2[ix5(g.nvar, g.N3, g.N2 + 1, g.N1, m, 0, k - 1, j, i)] = f2[0];
      }
      if (own) ms.m3[ix5(g.nvar, g.N3 + 1, g.N2, g.N1, m, 0, k, j, i)] = f3[0];
    }
#pragma unroll
    for (int n = 0; n < 5; ++n) { ISOSKIP; F3p[n] = f3[n]; }
    oc += (unsigned)ps*8u; oh += (unsigned)ps*8u;
  }
  if constexpr (C2P) {
    if (cp.do_newdt) {         // uniform across the grid
      __syncthreads();         // the last plane's fluxes have been read: hs_lds is free
      cfl_from_max(mv1, mv2, mv3, g.dx + 3*m, cp.dt3, hs_lds, tid, (int)(blockDim.x >> 6));
    }
  }
#undef ISOSKIP
}

}  // namespace akmi
#endif
