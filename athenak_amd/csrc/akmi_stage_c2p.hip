// akmi_stage_c2p.hip -- pass B of a stage: ConsToPrim over a box of cells (+ the CFL scan on the last stage) in one
// kernel, the conversion of the ghost shell, the fill of what a lean conversion dropped, and the entry points that need
// nothing else (akmi_*_c2p, akmi_*_c2p_newdt[_lean], akmi_mhd_c2p_takes_pairs, akmi_mhd_prims_fill, akmi_*_c2p_shell).
// The conversion of a cell, the signal speeds and the reduction of the scan: akmi_c2p.hpp.
#include <cfloat>
#include "akmi_stage.hpp"

namespace akmi {

#ifndef AKMI_C2P_PAIRS
#define AKMI_C2P_PAIRS 1
#endif
#ifndef AKMI_C2P_PAIRS_MIN
#define AKMI_C2P_PAIRS_MIN 4000000l
#endif

// cells [il,iu] x [jl,ju] x [k0,k0+nk-1]; lanes over the flattened rows [jl,ju] x N1 of one plane (flat_cells, akmi_common.hpp;
// with the planes flattened too this kernel is slower on small MeshBlocks: 49 -> 60 us on 120 blocks of 16^3).
// DROP (mask of AKMI_DROP_*, ideal gas only): the lean conversion -- w0[0..3] and / or bcc0 are computed as always but not
// stored; a caller whose next sweeps take them from u0 and the faces (AKMI_COPY_X12_U0 / AKMI_COPY_BCC_FACES) asks for it
template <bool MHD, int DROP = 0>
__global__ void __launch_bounds__(SX*SY)
k_c2p_newdt(Geo g, Eos eos, double *__restrict__ u0, const double *__restrict__ bx1f,
            const double *__restrict__ bx2f, const double *__restrict__ bx3f,
            double *__restrict__ w0, double *__restrict__ bcc0, int do_newdt,
            int *__restrict__ counters, double *__restrict__ dt3, int il, int iu, int jl, int ju,
            int k0, int nk) {
  __shared__ double sm[3*SY];
  const Cell3 q = flat_cells(0, g.N1, il, iu, jl, ju - jl + 1, k0, nk);
  const int i = q.i, j = q.j, k = q.k, m = q.m;
  double mv1 = 0.0, mv2 = 0.0, mv3 = 0.0;
  if (q.in) {
    const size_t cs = (size_t)g.N3*g.N2*g.N1;
    const size_t c = ix5(g.nvar, g.N3, g.N2, g.N1, m, 0, k, j, i);
    double ud, ue, wd, wvx, wvy, wvz, we, ubx = 0.0, uby = 0.0, ubz = 0.0;
    bool dfl = false, efl = false, tfl = false;
    if constexpr (MHD) {
      cell_bcc(g, bx1f, bx2f, bx3f, m, k, j, i, ubx, uby, ubz);
      if constexpr (!(DROP & AKMI_DROP_BCC)) {
        const size_t b = ix5(3, g.N3, g.N2, g.N1, m, 0, k, j, i);
        bcc0[b] = ubx; bcc0[b + cs] = uby; bcc0[b + 2*cs] = ubz;
      }
    }
    c2p_convert_at<MHD>(eos, u0, c, cs, ud, ue, ubx, uby, ubz, wd, wvx, wvy, wvz, we, dfl, efl, tfl);
    c2p_commit<DROP>(g, eos, u0, w0, counters, c, cs, ud, ue, wd, wvx, wvy, wvz, we, dfl, efl, tfl);
    if (do_newdt && i >= g.is && i <= g.ie && j >= g.js && j <= g.je && k >= g.ks && k <= g.ke)
      max_speeds<MHD>(eos, wd, wvx, wvy, wvz, we, ubx, uby, ubz, mv1, mv2, mv3);
  }
  if (!do_newdt) return;        // uniform across the grid
  cfl_from_max(mv1, mv2, mv3, g.dx + 3*m, dt3, sm, threadIdx.y*SX + threadIdx.x, SY);
}

// ---------------------------------------------------------------------------------------
// Pass B, two cells per thread (ideal gas, no passive scalars, rows of an even number of cells): every access of
// the cell-centred arrays is one 16-byte non-temporal access -- the streaming form that copies at 6.8 instead of
// 6.2 TB/s on this chip (tools/micro/copy_bw.hip, profiles/r05_copy_bw.txt); the conversion reads each conserved
// value once and its results are not read again before the cache has turned over.  x1 faces have rows of N1 + 1
// (odd) elements: three 8-byte loads, shared with the neighbouring lanes through L1.
typedef double d2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ d2_t ld2nt(const double *p) { return __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(p)); }
__device__ __forceinline__ d2_t ld2(const double *p) { return *reinterpret_cast<const d2_t *>(p); }
__device__ __forceinline__ void st2nt(double *p, double a, double b) {
  d2_t v; v.x = a; v.y = b;
  __builtin_nontemporal_store(v, reinterpret_cast<d2_t *>(p));
}

// (MHD: 88 VGPRs, 94 without the stores of w0[0..3] -- at most 96, five waves per SIMD; held to 80 / 64 registers it spills and runs at 383 / 605 us against 364-389,
//  profiles/r05_c2p_pairs.txt)
template <bool MHD, int DROP = 0>
__global__ void __launch_bounds__(SX*SY)
k_c2p_newdt2(Geo g, Eos eos, double *__restrict__ u0, const double *__restrict__ bx1f,
             const double *__restrict__ bx2f, const double *__restrict__ bx3f,
             double *__restrict__ w0, double *__restrict__ bcc0, int do_newdt,
             int *__restrict__ counters, double *__restrict__ dt3, int il, int iu, int jl, int ju,
             int k0, int nk) {
  // cells [il,iu] x [jl,ju] x [k0,k0+nk-1], il even and iu odd; lanes run over the cell PAIRS of the flattened rows
  __shared__ double sm[3*SY];
  const int hw = g.N1 >> 1;
  const long p = ((long)blockIdx.x*SY + threadIdx.y)*SX + threadIdx.x;
  const int jj = (int)(p/hw);
  const int j = jl + jj;
  const int i = 2*(int)(p - (long)jj*hw);
  const int m = blockIdx.z/nk;
  const int k = k0 + (blockIdx.z - m*nk);
  double mv1 = 0.0, mv2 = 0.0, mv3 = 0.0;
  if (j <= ju && i >= il && i <= iu) {
    const size_t cs = (size_t)g.N3*g.N2*g.N1;
    const size_t c = ix5(5, g.N3, g.N2, g.N1, m, 0, k, j, i);
    double ubx[2] = {0.0, 0.0}, uby[2] = {0.0, 0.0}, ubz[2] = {0.0, 0.0};
    if constexpr (MHD) {
      const double *b1 = bx1f + ix4(g.N3, g.N2, g.N1 + 1, m, k, j, i);
      const double f0 = b1[0], f1 = b1[1], f2 = b1[2];
      ubx[0] = bcc_from_faces(f0, f1); ubx[1] = bcc_from_faces(f1, f2);
      const d2_t y0 = ld2(bx2f + ix4(g.N3, g.N2 + 1, g.N1, m, k, j, i)), y1 = ld2(bx2f + ix4(g.N3, g.N2 + 1, g.N1, m, k, j + 1, i));
      uby[0] = bcc_from_faces(y0.x, y1.x); uby[1] = bcc_from_faces(y0.y, y1.y);
      const d2_t z0 = ld2(bx3f + ix4(g.N3 + 1, g.N2, g.N1, m, k, j, i)), z1 = ld2(bx3f + ix4(g.N3 + 1, g.N2, g.N1, m, k + 1, j, i));
      ubz[0] = bcc_from_faces(z0.x, z1.x); ubz[1] = bcc_from_faces(z0.y, z1.y);
      if constexpr (!(DROP & AKMI_DROP_BCC)) {
        const size_t b = ix5(3, g.N3, g.N2, g.N1, m, 0, k, j, i);
        st2nt(bcc0 + b, ubx[0], ubx[1]); st2nt(bcc0 + b + cs, uby[0], uby[1]); st2nt(bcc0 + b + 2*cs, ubz[0], ubz[1]);
      }
    }
    const d2_t vd = ld2nt(u0 + c), vx = ld2nt(u0 + c + cs), vy = ld2nt(u0 + c + 2*cs), vz = ld2nt(u0 + c + 3*cs),
               ve = ld2nt(u0 + c + 4*cs);
    double ud[2] = {vd.x, vd.y}, ue[2] = {ve.x, ve.y};
    const double umx[2] = {vx.x, vx.y}, umy[2] = {vy.x, vy.y}, umz[2] = {vz.x, vz.y};
    double wd[2], wvx[2], wvy[2], wvz[2], we[2];
    const bool act = do_newdt && j >= g.js && j <= g.je && k >= g.ks && k <= g.ke;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      bool dfl = false, efl = false, tfl = false;
      c2p_ideal<MHD>(eos, ud[q], umx[q], umy[q], umz[q], ue[q], ubx[q], uby[q], ubz[q], wd[q], wvx[q], wvy[q], wvz[q],
                     we[q], dfl, efl, tfl);
      if (dfl) { u0[c + q] = ud[q]; atomicAdd(&counters[0], 1); }
      if (efl) { u0[c + q + 4*cs] = ue[q]; atomicAdd(&counters[1], 1); }
      if (tfl) { u0[c + q + 4*cs] = ue[q]; atomicAdd(&counters[2], 1); }
      if (act && i + q >= g.is && i + q <= g.ie) {
        double a1, a2, a3;
        max_speeds_ideal<MHD>(eos.gamma, wd[q], wvx[q], wvy[q], wvz[q], we[q], ubx[q], uby[q], ubz[q], a1, a2, a3);
        mv1 = fmax(mv1, a1); mv2 = fmax(mv2, a2); mv3 = fmax(mv3, a3);
      }
    }
    if constexpr (!(DROP & AKMI_DROP_W03)) {
      st2nt(w0 + c, wd[0], wd[1]); st2nt(w0 + c + cs, wvx[0], wvx[1]); st2nt(w0 + c + 2*cs, wvy[0], wvy[1]);
      st2nt(w0 + c + 3*cs, wvz[0], wvz[1]);
    }
    st2nt(w0 + c + 4*cs, we[0], we[1]);
  }
  if (!do_newdt) return;        // uniform across the grid
  cfl_from_max(mv1, mv2, mv3, g.dx + 3*m, dt3, sm, threadIdx.y*SX + threadIdx.x, SY);
}

__global__ void k_fill_fltmax(double *x, int n) {
  if ((int)threadIdx.x < n) x[threadIdx.x] = (double)FLT_MAX;
}
void fill_fltmax(double *x, int n, hipStream_t st) { k_fill_fltmax<<<1, 64, 0, st>>>(x, n); }

// ---------------------------------------------------------------------------------------
// c2p on the ghost SHELL only (after the halo exchange): the interior was converted inside
// the slab pipeline.  MODE 0: k-ghost planes (all j,i); 1: j-ghost rows of active planes;
// 2: i-ghost columns of active rows.  Flattened 1-D over the slab so that the 2*ng-wide
// i-slabs do not waste 60 of 64 lanes.
template <bool MHD>
__global__ void __launch_bounds__(256)
k_c2p_shell(Geo g, Eos eos, double *__restrict__ u0, const double *__restrict__ bx1f,
            const double *__restrict__ bx2f, const double *__restrict__ bx3f,
            double *__restrict__ w0, double *__restrict__ bcc0, int *__restrict__ counters) {
  const int MODE = blockIdx.y;                 // slab of the shell, one launch for all three
  const int ng3 = g.three_d ? g.ng : 0, ng2 = g.multi_d ? g.ng : 0;
  int e1, e2, e3;
  if (MODE == 0) { e1 = g.N1; e2 = g.N2; e3 = 2*ng3; }
  else if (MODE == 1) { e1 = g.N1; e2 = 2*ng2; e3 = g.nx3; }
  else { e1 = 2*g.ng; e2 = g.nx2; e3 = g.nx3; }
  const long long per = (long long)e1*e2*e3;
  const long long t = (long long)blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= per*g.nmb) return;
  const int m = (int)(t/per);
  long long r = t - (long long)m*per;
  const int kk = (int)(r/((long long)e1*e2));
  r -= (long long)kk*e1*e2;
  const int jj = (int)(r/e1);
  const int ii = (int)(r - (long long)jj*e1);
  int i, j, k;
  if (MODE == 0) { i = ii; j = jj; k = kk < ng3 ? kk : g.ke + 1 + (kk - ng3); }
  else if (MODE == 1) { i = ii; j = jj < ng2 ? jj : g.je + 1 + (jj - ng2); k = g.ks + kk; }
  else { i = ii < g.ng ? ii : g.ie + 1 + (ii - g.ng); j = g.js + jj; k = g.ks + kk; }
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const size_t c = ix5(g.nvar, g.N3, g.N2, g.N1, m, 0, k, j, i);
  double ud, ue, wd, wvx, wvy, wvz, we, ubx = 0.0, uby = 0.0, ubz = 0.0;
  bool dfl = false, efl = false, tfl = false;
  if constexpr (MHD) {
    cell_bcc(g, bx1f, bx2f, bx3f, m, k, j, i, ubx, uby, ubz);
    const size_t b = ix5(3, g.N3, g.N2, g.N1, m, 0, k, j, i);
    bcc0[b] = ubx; bcc0[b + cs] = uby; bcc0[b + 2*cs] = ubz;
  }
  c2p_convert_at<MHD>(eos, u0, c, cs, ud, ue, ubx, uby, ubz, wd, wvx, wvy, wvz, we, dfl, efl, tfl);
  c2p_commit(g, eos, u0, w0, counters, c, cs, ud, ue, wd, wvx, wvy, wvz, we, dfl, efl, tfl);
}

template <bool MHD>
static int c2p_shell(const akmi_pack *p, double *u0, const double *bx1f, const double *bx2f,
                     const double *bx3f, double *w0, double *bcc0, int *counters, hipStream_t st) {
  Geo g = make_geo(p);
  Eos eos = make_eos(p);
  const long long n0 = g.three_d ? (long long)g.N1*g.N2*2*g.ng*g.nmb : 0;
  const long long n1 = g.multi_d ? (long long)g.N1*2*g.ng*g.nx3*g.nmb : 0;
  const long long n2 = (long long)2*g.ng*g.nx2*g.nx3*g.nmb;
  const long long nmax = n0 > n1 ? (n0 > n2 ? n0 : n2) : (n1 > n2 ? n1 : n2);
  dim3 grid((unsigned)((nmax + 255)/256), 3);
  k_c2p_shell<MHD><<<grid, 256, 0, st>>>(g, eos, u0, bx1f, bx2f, bx3f, w0, bcc0, counters);
  AKMI_CHECK_LAUNCH("c2p_shell");
  return AKMI_COMPLETE;
}

// the cell-centred field and the density / velocity of every cell from u0 and the faces, through the two helpers of
// ConsToPrim (akmi_numerics.hpp): writes what a lean conversion dropped, and nothing else (akmi_mhd_prims_fill)
template <int DROP>
__global__ void __launch_bounds__(SX*SY)
k_prims_fill(Geo g, const double *__restrict__ u0, const double *__restrict__ bx1f, const double *__restrict__ bx2f,
             const double *__restrict__ bx3f, double *__restrict__ w0, double *__restrict__ bcc0) {
  const Cell3 q = flat_cells(0, g.N1, 0, g.N1 - 1, 0, g.N2, 0, g.N3);
  if (!q.in) return;
  const int i = q.i, j = q.j, k = q.k, m = q.m;
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  if constexpr ((DROP & AKMI_DROP_BCC) != 0) {
    const size_t b = ix5(3, g.N3, g.N2, g.N1, m, 0, k, j, i);
    double ubx, uby, ubz;
    cell_bcc(g, bx1f, bx2f, bx3f, m, k, j, i, ubx, uby, ubz);
    bcc0[b] = ubx; bcc0[b + cs] = uby; bcc0[b + 2*cs] = ubz;
  }
  if constexpr ((DROP & AKMI_DROP_W03) != 0) {
    const size_t c = ix5(g.nvar, g.N3, g.N2, g.N1, m, 0, k, j, i);
    double di, wvx, wvy, wvz;
    const double ud = u0[c];
    vel_from_cons(ud, u0[c + cs], u0[c + 2*cs], u0[c + 3*cs], di, wvx, wvy, wvz);
    w0[c] = ud; w0[c + cs] = wvx; w0[c + 2*cs] = wvy; w0[c + 3*cs] = wvz;
  }
}

// the conversion of these cells takes the two-cells-per-thread kernel
static bool c2p_pairs(const Geo &g, const Eos &eos, int il, int iu, int jl, int ju, int nk) {
#if AKMI_C2P_PAIRS
  static const bool pairs_off = getenv("AKMI_C2P_PAIRS") && atoi(getenv("AKMI_C2P_PAIRS")) == 0;       // A/B switch
  // (from ~4 M cells per launch: at 128^3 = 2.3 M the launch is latency-bound and half the threads lose 5 % of a cycle,
  //  at 192^3 = 7.5 M the pairs gain 2.4 %, at 256^3 3.5 %; profiles/r05_c2p_pairs.txt)
  const long ncell = (long)g.nmb*nk*(ju - jl + 1)*g.N1;
  return !pairs_off && ncell >= AKMI_C2P_PAIRS_MIN && eos.is_ideal && g.nvar == 5 && !(g.N1 & 1) && !(il & 1) && (iu & 1);
#else
  return false;
#endif
}

template <bool MHD, int DROP>
int launch_c2p(const Geo &g, const Eos &eos, double *u0, const double *bx1f,
               const double *bx2f, const double *bx3f, double *w0, double *bcc0,
               int do_newdt, int *counters, double *dt3, int il, int iu, int jl, int ju,
               int k0, int nk, hipStream_t st) {
  dim3 grid((unsigned)(((long)(ju - jl + 1)*g.N1 + SX*SY - 1)/(SX*SY)), 1, nk*g.nmb), block(SX, SY);
#if AKMI_C2P_PAIRS
  if (c2p_pairs(g, eos, il, iu, jl, ju, nk)) {
    dim3 grid2((unsigned)(((long)(ju - jl + 1)*(g.N1/2) + SX*SY - 1)/(SX*SY)), 1, nk*g.nmb);
    k_c2p_newdt2<MHD, DROP><<<grid2, block, 0, st>>>(g, eos, u0, bx1f, bx2f, bx3f, w0, bcc0, do_newdt, counters,
                                               dt3, il, iu, jl, ju, k0, nk);
    AKMI_CHECK_LAUNCH("c2p pairs");
    return AKMI_COMPLETE;
  }
#endif
  k_c2p_newdt<MHD, DROP><<<grid, block, 0, st>>>(g, eos, u0, bx1f, bx2f, bx3f, w0, bcc0, do_newdt, counters,
                                           dt3, il, iu, jl, ju, k0, nk);
  AKMI_CHECK_LAUNCH("c2p");
  return AKMI_COMPLETE;
}

// the full conversions stage_update asks for (the lean ones are used below only)
#define AKMI_INST(MHD)                                                                                                   \
  template int launch_c2p<MHD, 0>(const Geo &, const Eos &, double *, const double *, const double *, const double *, \
                                  double *, double *, int, int *, double *, int, int, int, int, int, int, hipStream_t);
AKMI_INST(false)
AKMI_INST(true)
#undef AKMI_INST

}  // namespace akmi

using namespace akmi;

extern "C" {

// ConsToPrim of a box (the task-granular entry points; ideal_hyd.cpp:45-103, ideal_mhd.cpp:47-122): the conversion of
// pass B without its scan
int akmi_hydro_c2p(const akmi_pack *p, double *u0, double *w0, int il, int iu, int jl, int ju,
                   int kl, int ku, int *counters, void *stream) {
  return launch_c2p<false>(make_geo(p), make_eos(p), u0, nullptr, nullptr, nullptr, w0, nullptr, 0, counters, nullptr,
                           il, iu, jl, ju, kl, ku - kl + 1, (hipStream_t)stream);
}

int akmi_mhd_c2p(const akmi_pack *p, double *u0, const double *bx1f, const double *bx2f,
                 const double *bx3f, double *w0, double *bcc0, int il, int iu, int jl, int ju,
                 int kl, int ku, int *counters, void *stream) {
  return launch_c2p<true>(make_geo(p), make_eos(p), u0, bx1f, bx2f, bx3f, w0, bcc0, 0, counters, nullptr,
                          il, iu, jl, ju, kl, ku - kl + 1, (hipStream_t)stream);
}

int akmi_hydro_c2p_newdt(const akmi_pack *p, double *u0, double *w0, int do_newdt, int *counters,
                         double *dt3, void *stream) {
  Geo g = make_geo(p);
  hipStream_t st = (hipStream_t)stream;
  if (do_newdt == 1) fill_fltmax(dt3, 3, st);
  return launch_c2p<false>(g, make_eos(p), u0, nullptr, nullptr, nullptr, w0, nullptr, do_newdt,
                           counters, dt3, 0, g.N1 - 1, 0, g.N2 - 1, 0, g.N3, st);
}

int akmi_mhd_c2p_newdt(const akmi_pack *p, double *u0, const double *bx1f, const double *bx2f,
                       const double *bx3f, double *w0, double *bcc0, int do_newdt, int *counters,
                       double *dt3, void *stream) {
  Geo g = make_geo(p);
  hipStream_t st = (hipStream_t)stream;
  if (do_newdt == 1) fill_fltmax(dt3, 3, st);
  return launch_c2p<true>(g, make_eos(p), u0, bx1f, bx2f, bx3f, w0, bcc0, do_newdt, counters, dt3,
                          0, g.N1 - 1, 0, g.N2 - 1, 0, g.N3, st);
}

int akmi_mhd_c2p_newdt_lean(const akmi_pack *p, double *u0, const double *bx1f, const double *bx2f,
                            const double *bx3f, double *w0, double *bcc0, int do_newdt, int *counters,
                            double *dt3, int drop, void *stream) {
  if (drop < 0 || drop > (AKMI_DROP_W03 | AKMI_DROP_BCC)) { set_error("c2p_newdt_lean: bad drop mask %d", drop); return AKMI_FAIL; }
  if (drop && (!p->is_ideal || p->nvar != 5)) {
    set_error("c2p_newdt_lean: only the sweeps of an ideal gas without scalars can do without the dropped arrays");
    return AKMI_FAIL;
  }
  Geo g = make_geo(p);
  hipStream_t st = (hipStream_t)stream;
  if (do_newdt == 1) fill_fltmax(dt3, 3, st);
  auto go = [&](auto D) {
    return launch_c2p<true, decltype(D)::value>(g, make_eos(p), u0, bx1f, bx2f, bx3f, w0, bcc0, do_newdt, counters, dt3,
                                                0, g.N1 - 1, 0, g.N2 - 1, 0, g.N3, st);
  };
  return drop == 0 ? go(IC<0>{}) : drop == 1 ? go(IC<1>{}) : drop == 2 ? go(IC<2>{}) : go(IC<3>{});
}

int akmi_mhd_c2p_takes_pairs(const akmi_pack *p) {
  Geo g = make_geo(p);
  return c2p_pairs(g, make_eos(p), 0, g.N1 - 1, 0, g.N2 - 1, g.N3) ? 1 : 0;
}

int akmi_mhd_prims_fill(const akmi_pack *p, const double *u0, const double *bx1f, const double *bx2f,
                        const double *bx3f, double *w0, double *bcc0, int drop, void *stream) {
  if (drop < 0 || drop > (AKMI_DROP_W03 | AKMI_DROP_BCC)) { set_error("prims_fill: bad drop mask %d", drop); return AKMI_FAIL; }
  if (drop == 0) return AKMI_COMPLETE;
  Geo g = make_geo(p);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)(((long)g.N2*g.N1 + SX*SY - 1)/(SX*SY)), 1, g.N3*g.nmb), block(SX, SY);
  if (drop == 1) k_prims_fill<1><<<grid, block, 0, st>>>(g, u0, bx1f, bx2f, bx3f, w0, bcc0);
  else if (drop == 2) k_prims_fill<2><<<grid, block, 0, st>>>(g, u0, bx1f, bx2f, bx3f, w0, bcc0);
  else k_prims_fill<3><<<grid, block, 0, st>>>(g, u0, bx1f, bx2f, bx3f, w0, bcc0);
  AKMI_CHECK_LAUNCH("prims_fill");
  return AKMI_COMPLETE;
}

int akmi_hydro_c2p_shell(const akmi_pack *p, double *u0, double *w0, int *counters, void *stream) {
  return c2p_shell<false>(p, u0, nullptr, nullptr, nullptr, w0, nullptr, counters, (hipStream_t)stream);
}

int akmi_mhd_c2p_shell(const akmi_pack *p, double *u0, const double *bx1f, const double *bx2f,
                       const double *bx3f, double *w0, double *bcc0, int *counters, void *stream) {
  return c2p_shell<true>(p, u0, bx1f, bx2f, bx3f, w0, bcc0, counters, (hipStream_t)stream);
}

}  // extern "C"
