// akmi_stage_sweeps.hip -- the thread-per-face sweeps of the fused stage (k_sweep) and their launcher: the x1 sweep of
// the generic sequence and of 2-D runs, and the x1 / x2 / x3 flux kernels of small packs on the task-granular path
// (sweeps_store_fluxes, akmi_stage.hip).
#include "akmi_stage.hpp"

namespace akmi {

// plain sweep (not the last direction): thread per face.  ECC: also emit e_cc for the right
// cell of every face and for the extra column i = il-1 (mhd_corner_e.cpp:309-317 range
// [is-1,ie+1] x [js-1,je+1] x [ks-1,ke+1] == the CT-extended x1 sweep, right cells).
// x1 sweep with PLM / the five-point schemes: the reconstruction of a cell serves both of its faces
// (ReconCellT, recon.hpp:40-118: cell c-1 writes wl(c), cell c writes wr(c)), so a lane reconstructs
// ITS cell only (PLM: one division per variable instead of two) and takes the left state of its face
// from the lane below through a wave shuffle.  Waves overlap by one lane (lane 0 only
// provides): 63 faces per wave.  Same operands, same operations -> same bits.
#ifndef AKMI_X1_SHARE
#define AKMI_X1_SHARE 1
#endif
template <int DIR, int RECON>
constexpr bool x1_share() { return DIR == 0 && RECON >= 1 && AKMI_X1_SHARE; }
// k_sweep: the planes [kl, ku] flattened into the lane index as well (120 blocks of 16^3, PPM4 + HLLD: x1 sweep 40.7 -> 32,
// x2 sweep 49.4 -> 36 us) -- profiles/r06_lane_mapping.txt

template <int RECON, bool MHD, bool ECC, int RS>
__device__ __forceinline__ void sweep_x1_shared(const Geo &g, const FaceEos &eos, const SweepArgs &a,
                                                int nk) {
  // lanes over the flattened (row, column) with the columns a row needs: cells il-1 .. iu (the first one only provides
  // the left state of face il) -- not the N1 of the row: 34 of the 40 columns of a 32^3 MeshBlock with four ghost cells
  // The flattening runs over the planes [kl, ku] of the MeshBlock as well (a plane of a 16^3 block is 18 x 18 positions:
  // 1.3 workgroups of 252, i.e. two workgroups 64 % full when every plane starts a workgroup of its own).
  const long p = ((long)blockIdx.x*SY + threadIdx.y)*(SX - 1) + (long)threadIdx.x - 1;
  const unsigned pc = p < 0 ? 0u : (unsigned)p;
  const unsigned row_w = (unsigned)(a.iu - a.il + 2), plane = row_w*(unsigned)(a.ju - a.jl + 1);
  const unsigned kk = pc/plane, pr = pc - kk*plane;
  const unsigned jj = pr/row_w;
  const int i = a.il - 1 + (int)(pr - jj*row_w);
  const int j = a.jl + (int)jj;
  const int m = blockIdx.z;
  const int k = a.kl + (int)kk;
  // a lane owns cell i: its stencil (i-1..i+1, five-point schemes i-2..i+2) has to be inside the row
  constexpr int HW = RECON == 1 ? 1 : 2;
  const bool valid = p >= 0 && (int)kk < nk && i >= HW && i <= g.N1 - 1 - HW;
  constexpr int NV = MHD ? 7 : 5;
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  // addresses = wave-uniform base (block m, variable n: scalar unit) + ONE 32-bit byte offset per lane
  // (global_load v, v_off, s[base]): no 64-bit integer multiplies on the vector unit.  A block-variable
  // is below 4 GB (checked at launch).
  const unsigned oc = (((unsigned)k*(unsigned)g.N2 + (unsigned)j)*(unsigned)g.N1 + (unsigned)i)*8u;           // cell (k,j,i)
  const unsigned of = (((unsigned)k*(unsigned)a.f2 + (unsigned)j)*(unsigned)a.f1 + (unsigned)i)*8u;   // face (k,j,i)
  const double *wm = a.w0 + (size_t)m*g.nvar*cs;
  const double *bm = MHD ? a.bcc0 + (size_t)m*3*cs : nullptr;
  double qln[NV], qr[NV];                 // left state of face i+1, right state of face i
#pragma unroll
  for (int n = 0; n < NV; ++n) { qln[n] = 0.0; qr[n] = 0.0; }
  double vx = 0.0, vy = 0.0, vz = 0.0, by = 0.0, bz = 0.0;
  [[maybe_unused]] double bxi_pre = 0.0;
  if (valid) {
    // the five-point reconstructions branch (limiters), so every variable is a basic block of its own and its
    // stencil loads were issued there: load -> s_waitcnt vmcnt(0) -> 43 VALU, seven times over
    // (profiles/r03_isa_audit.txt, second audit).  All stencils are requested first; the waits count down.
    double sq[NV][RECON == 1 ? 3 : 5];
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      if (rs_iso<RS>() && n == 4) continue;
      const double *q = (n < 5) ? wm + n*cs : bm + (n - 4)*cs;
#pragma unroll
      for (int d = 0; d < (RECON == 1 ? 3 : 5); ++d) sq[n][d] = ldu(q + d - (RECON == 1 ? 1 : 2), oc);
    }
    if constexpr (MHD) bxi_pre = ldu(a.bxf + (size_t)m*((size_t)a.f3*a.f2*a.f1), of);   // face (k,j,i) exists for a valid lane
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      if (rs_iso<RS>() && n == 4) continue;             // isothermal: slot 4 (energy) stays unused
      const double *q = (n < 5) ? wm + n*cs : bm + (n - 4)*cs;   // by, bz
      constexpr int C = RECON == 1 ? 1 : 2;
      const double qm = sq[n][C - 1], q0 = sq[n][C], qp = sq[n][C + 1];
      if constexpr (RECON == 1) {
        plm(qm, q0, qp, qln[n], qr[n]);
      } else {
        const double qmm = sq[n][0], qpp = sq[n][4];
        recon5<RECON>(qmm, qm, q0, qp, qpp, qln[n], qr[n]);
        // the floors of recon.hpp:72-103 act on each state separately: per cell == per face
        if (n == 0) floor_lr<RECON, 1>(eos, qln[n], qr[n]);
        if (n == 4) floor_lr<RECON, 2>(eos, qln[n], qr[n]);
      }
      if (n == 1) vx = q0;
      if (n == 2) vy = q0;
      if (n == 3) vz = q0;
      if (n == 5) by = q0;
      if (n == 6) bz = q0;
    }
  }
  double L[NV];
#pragma unroll
  for (int n = 0; n < NV; ++n) L[n] = __shfl_up(qln[n], 1, 64);
  if (!valid) return;
  if constexpr (ECC) {
    if (i >= a.il - 1 && i <= a.iu) {
      const double bx = ldu(bm, oc);
      stu(a.ecc1 + (size_t)m*cs, oc, vz*by - vy*bz);
      stu(a.ecc2 + (size_t)m*cs, oc, vx*bz - vz*bx);
      stu(a.ecc3 + (size_t)m*cs, oc, vy*bx - vx*by);
    }
  }
  if (threadIdx.x == 0 || i < a.il || i > a.iu) return;     // lane 0 only provides
  double fd, fx, fy, fz, fe, fby = 0.0, fbz = 0.0;
  const size_t fs = (size_t)a.f3*a.f2*a.f1;
  if constexpr (MHD) {
    const double bxi = bxi_pre;
    Cons1D fl = riemann_mhd_e<RS, true>(eos, L[0], L[1], L[2], L[3], L[4], L[5], L[6], qr[0], qr[1],
                                        qr[2], qr[3], qr[4], qr[5], qr[6], bxi);
    fd = fl.d; fx = fl.mx; fy = fl.my; fz = fl.mz; fe = fl.e; fby = fl.by; fbz = fl.bz;
  } else {
    riemann_hyd_e<RS>(eos, L[0], L[1], L[2], L[3], L[4], qr[0], qr[1], qr[2], qr[3], qr[4], fd,
                      fx, fy, fz, fe);
  }
  double *f = a.flx + (size_t)m*g.nvar*fs;
  stu(f, of, fd); stu(f + fs, of, fx); stu(f + 2*fs, of, fy); stu(f + 3*fs, of, fz);
  if constexpr (!rs_iso<RS>()) stu(f + 4*fs, of, fe);
  if (AKMI_MF_BYTES && MHD && a.mfb) st_mfs(a.mfb + (size_t)m*fs, of, fd);      // the x2 march still reads the double
  if constexpr (MHD) {
    stu(a.ey + (size_t)m*cs, oc, -fby);
    stu(a.ez + (size_t)m*cs, oc, fbz);
  }
}

template <int DIR, int RECON, bool MHD, bool ECC, int RS>
__global__ void __launch_bounds__(SX*SY)
k_sweep(Geo g, FaceEos eos, SweepArgs a, int nk) {
  if constexpr (x1_share<DIR, RECON>()) {
    sweep_x1_shared<RECON, MHD, ECC, RS>(g, eos, a, nk);
    return;
  }
  // lanes run over the flattened rows [jl,ju] x [0,N1): contiguous in memory, and the few
  // ghost columns outside [il,iu] cost 2-4 idle lanes per 260 instead of a mostly empty wave
  // lanes over the flattened (row, column) with the columns of the sweep only (ECC: one more on the low side), not the
  // N1 of a row: a thread-per-face sweep has no coupling between lanes (18 of 24 columns at 16^3 with four ghost cells)
  // ... and over the planes [kl, ku] of the MeshBlock (a plane of a 16^3 block is 17 x 18 faces: two workgroups 60 % full
  // when every plane starts a workgroup of its own)
  const unsigned p = (blockIdx.x*SY + threadIdx.y)*SX + threadIdx.x;
  const int row_0 = a.il - (ECC ? 1 : 0);
  const unsigned row_w = (unsigned)(a.iu - row_0 + 1), plane = row_w*(unsigned)(a.ju - a.jl + 1);
  unsigned kk, jj, pr;
  if (DIR != 2) {
    kk = p/plane; pr = p - kk*plane;
    jj = pr/row_w; pr -= jj*row_w;
  } else {
    // x3 sweep: (j; k; i) -- the lanes of a wave that are not neighbours in i are neighbours in k, the direction of the
    // stencil, so the rows a wave loads overlap as they do in the x2 sweep (a wave of the (k; j; i) order reads six planes x
    // its own rows and shares nothing: 57 us against 37 for the x2 sweep on 120 blocks of 16^3)
    const unsigned slab = row_w*(unsigned)nk;
    jj = p/slab; pr = p - jj*slab;
    kk = pr/row_w; pr -= kk*row_w;
  }
  const int i = row_0 + (int)pr;
  const int j = a.jl + (int)jj;
  const int m = blockIdx.z;
  const int k = a.kl + (int)kk;
  if ((int)kk >= nk || j > a.ju) return;
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const unsigned oc = (((unsigned)k*(unsigned)g.N2 + (unsigned)j)*(unsigned)g.N1 + (unsigned)i)*8u;   // cell (k,j,i)
  if constexpr (ECC) {
    const double *wm = a.w0 + (size_t)m*g.nvar*cs, *bm = a.bcc0 + (size_t)m*3*cs;
    const double vx = ldu(wm + cs, oc), vy = ldu(wm + 2*cs, oc), vz = ldu(wm + 3*cs, oc);
    const double bx = ldu(bm, oc), by = ldu(bm + cs, oc), bz = ldu(bm + 2*cs, oc);
    stu(a.ecc1 + (size_t)m*cs, oc, vz*by - vy*bz);
    stu(a.ecc2 + (size_t)m*cs, oc, vx*bz - vz*bx);
    stu(a.ecc3 + (size_t)m*cs, oc, vy*bx - vx*by);
    if (i < a.il) return;
  }
  constexpr int ivx = 1 + DIR, ivy = 1 + (DIR + 1)%3, ivz = 1 + (DIR + 2)%3;
  double fd, fx, fy, fz, fe, fby, fbz;
  face_flux<DIR, RECON, MHD, RS>(g, eos, a.w0, a.bcc0, a.bxf, a.f3, a.f2, a.f1, m, k, j, i, fd,
                                 fx, fy, fz, fe, fby, fbz);
  const size_t fs = (size_t)a.f3*a.f2*a.f1;
  const unsigned of = (((unsigned)k*(unsigned)a.f2 + (unsigned)j)*(unsigned)a.f1 + (unsigned)i)*8u;       // face (k,j,i)
  double *f = a.flx + (size_t)m*g.nvar*fs;
  stu(f, of, fd); stu(f + ivx*fs, of, fx); stu(f + ivy*fs, of, fy); stu(f + ivz*fs, of, fz);
  if constexpr (!rs_iso<RS>()) stu(f + 4*fs, of, fe);
  if (AKMI_MF_BYTES && MHD && a.mfb) st_mfs(a.mfb + (size_t)m*fs, of, fd);      // the x2 march still reads the double
  if constexpr (MHD) {
    stu(a.ey + (size_t)m*cs, oc, -fby);
    stu(a.ez + (size_t)m*cs, oc, fbz);
  }
}

template <int DIR, bool MHD, bool ECC>
int launch_sweep(const Geo &g, const Scheme &sc, const SweepArgs &a, hipStream_t st) {
  int nk = a.ku - a.kl + 1;
  dim3 block(SX, SY);
  int rc = dispatch_scheme_eos<MHD>(sc, [&](auto R, auto S) {
    // faces per wave: 63 when the lanes share their slopes (lane 0 of a wave only provides); those kernels run over
    // the columns il-1 .. iu of a row (sweep_x1_shared), the plain one over il (- 1 with ECC) .. iu
    constexpr bool share = x1_share<DIR, decltype(R)::value>();
    const long np = (long)nk*(a.ju - a.jl + 1)*(share ? a.iu - a.il + 2 : a.iu - a.il + 1 + (ECC ? 1 : 0));   // of one MeshBlock
    const long per_wg = (long)(share ? SX - 1 : SX)*SY;
    dim3 grid((unsigned)((np + 1 + per_wg - 1)/per_wg), 1, g.nmb);
    k_sweep<DIR, decltype(R)::value, MHD, ECC, decltype(S)::value><<<grid, block, 0, st>>>(
        g, sc.eos, a, nk);
    return AKMI_COMPLETE;
  });
  if (rc != AKMI_COMPLETE) return rc;
  AKMI_CHECK_LAUNCH("sweep");
  return AKMI_COMPLETE;
}

// what stage_update and sweeps_store_fluxes_t ask for
#define AKMI_INST(DIR, MHD, ECC) \
  template int launch_sweep<DIR, MHD, ECC>(const Geo &, const Scheme &, const SweepArgs &, hipStream_t);
AKMI_INST(0, true, true)
AKMI_INST(0, true, false)
AKMI_INST(0, false, false)
AKMI_INST(1, true, false)
AKMI_INST(1, false, false)
AKMI_INST(2, true, false)
AKMI_INST(2, false, false)
#undef AKMI_INST

}  // namespace akmi
