// akmi_coarsen.hip -- the coarsened binary output (file_type = cbin, src/outputs/coarsened_binary.cpp:174-290): every
// output variable of every MeshBlock of a pack averaged over f x f x f cells, with moments also <x^2>, <x^3>, <x^4>, in
// ONE launch (the reference: one launch, two device copies and two fences per variable and MeshBlock, atomics into the
// coarse cell).  The per-cell arithmetic and the order of summation are those of akmi_coarsen.hpp: the sum of a coarse
// cell belongs to one thread, which adds its f^3 terms in ascending kk, jj, ii; no atomics, no tree.
//
// Two forms of the same arithmetic, bit-identical (blockIdx.y = MeshBlock, blockIdx.z = variable of the table):
// k_coarsen_direct   one thread per coarse cell, the coarse cells of a block flattened with ic fastest.  A lane reads its f
//                    consecutive doubles of a fine row from global memory: across a wave the addresses are f doubles apart,
//                    so every 128-byte line is touched by f load instructions.
// k_coarsen_staged   a workgroup owns a tile of cw coarse cells in i times R coarse rows (cw*R <= 256, R*cw*f <= 4096
//                    doubles).  For each (kk, jj) it copies the R fine row segments of cw*f doubles into LDS with contiguous
//                    loads (consecutive lanes, consecutive doubles: whole lines), then every thread adds its f consecutive
//                    values from LDS.  The LDS image is padded by one double after every 32, which spreads the stride-f
//                    64-bit reads of a half-wave over all banks for f = 2, 4, 8, 16.
#include "akmi_common.hpp"
#include "akmi_coarsen.hpp"
#include <cstdlib>
#include <vector>

namespace akmi {
namespace {

constexpr int CO_NT = 256;            // threads of a workgroup
constexpr int CO_LDS = 4096;          // doubles of fine data a workgroup stages per (kk, jj)
constexpr int CO_LDS_PAD = CO_LDS + CO_LDS/32;
constexpr int CO_TAB = 24;            // variables of a table passed by value (16 B each)

struct CoarsenVar {
  const double *a;
  int nv, comp;
};
struct TabVal {
  CoarsenVar v[CO_TAB];
  __device__ __forceinline__ CoarsenVar at(int n) const { return v[n]; }
};
struct TabPtr {
  const CoarsenVar *v;
  __device__ __forceinline__ CoarsenVar at(int n) const { return v[n]; }
};

struct CoarsenGeo {
  int nmb, N1, N2, N3;       // array extents of a MeshBlock
  int f, lo1, lo2, lo3;      // factor; first fine cell (ois, ojs, oks)
  int nc1, nc2, nc3;         // coarse extents
  int cw, R, ntile_i;        // staged form: tile of cw coarse cells x R coarse rows; tiles along i
};

__device__ __forceinline__ int lds_pos(int idx) { return idx + (idx >> 5); }

template <bool MOM, class Tab>
__global__ void __launch_bounds__(CO_NT) k_coarsen_direct(CoarsenGeo g, Tab tab, double *__restrict__ out) {
  const int ncc = g.nc3*g.nc2*g.nc1;
  const int t = blockIdx.x*CO_NT + threadIdx.x;
  if (t >= ncc) return;
  const int m = blockIdx.y, v = blockIdx.z;
  const CoarsenVar cv = tab.at(v);
  const int ic = t % g.nc1, r = t/g.nc1, jc = r % g.nc2, kc = r/g.nc2;
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const double *a = cv.a + ((size_t)m*cv.nv + cv.comp)*cs
                    + ((size_t)(g.lo3 + kc*g.f)*g.N2 + (g.lo2 + jc*g.f))*g.N1 + (g.lo1 + ic*g.f);
  const size_t stride = (size_t)g.nmb*ncc;
  double *o = out + ((size_t)v*(MOM ? 4 : 1)*g.nmb + m)*ncc + t;
  coarsen_cell<MOM>(a, (size_t)g.N1, (size_t)g.N2, g.f, o, stride);
}

template <bool MOM, class Tab>
__global__ void __launch_bounds__(CO_NT) k_coarsen_staged(CoarsenGeo g, Tab tab, double *__restrict__ out) {
  __shared__ double s[CO_LDS_PAD];
  const int m = blockIdx.y, v = blockIdx.z;
  const CoarsenVar cv = tab.at(v);
  const int ti = blockIdx.x % g.ntile_i, tr = blockIdx.x/g.ntile_i;
  const int ic0 = ti*g.cw, row0 = tr*g.R;
  const int nrows = g.nc3*g.nc2;
  const int w = (g.nc1 - ic0 < g.cw) ? g.nc1 - ic0 : g.cw;      // coarse cells of this tile along i
  const int fw = w*g.f, seg = g.cw*g.f;                        // fine doubles of a row segment; its place in LDS
  const int rows = (nrows - row0 < g.R) ? nrows - row0 : g.R;
  const int r = threadIdx.x/g.cw, c = threadIdx.x - r*g.cw;
  const bool mine = r < rows && c < w;
  const size_t cs = (size_t)g.N3*g.N2*g.N1;
  const double *a = cv.a + ((size_t)m*cv.nv + cv.comp)*cs;
  CoarsenAcc acc;
  coarsen_init(acc);
  for (int kk = 0; kk < g.f; ++kk)
    for (int jj = 0; jj < g.f; ++jj) {
      __syncthreads();                                          // the previous segment has been read
      for (int e = threadIdx.x; e < rows*fw; e += CO_NT) {
        const int rr = e/fw, cc = e - rr*fw;
        const int row = row0 + rr, kc = row/g.nc2, jc = row - kc*g.nc2;
        const size_t off = ((size_t)(g.lo3 + kc*g.f + kk)*g.N2 + (g.lo2 + jc*g.f + jj))*g.N1 + (g.lo1 + ic0*g.f + cc);
        s[lds_pos(rr*seg + cc)] = a[off];
      }
      __syncthreads();
      if (mine) {
        const int base = r*seg + c*g.f;
        for (int ii = 0; ii < g.f; ++ii) coarsen_add<MOM>(acc, s[lds_pos(base + ii)]);
      }
    }
  if (mine) {
    const int ncc = nrows*g.nc1;
    const int t = (row0 + r)*g.nc1 + ic0 + c;
    coarsen_store<MOM>(acc, (double)(g.f*g.f*g.f), out + ((size_t)v*(MOM ? 4 : 1)*g.nmb + m)*ncc + t, (size_t)g.nmb*ncc);
  }
}

template <class Tab>
void launch(bool staged, bool mom, const CoarsenGeo &g, const Tab &tab, int nvars, double *out, hipStream_t st) {
  if (staged) {
    const dim3 grid((unsigned)(g.ntile_i*cdiv(g.nc3*g.nc2, g.R)), (unsigned)g.nmb, (unsigned)nvars);
    if (mom) k_coarsen_staged<true, Tab><<<grid, CO_NT, 0, st>>>(g, tab, out);
    else k_coarsen_staged<false, Tab><<<grid, CO_NT, 0, st>>>(g, tab, out);
  } else {
    const dim3 grid((unsigned)cdiv(g.nc3*g.nc2*g.nc1, CO_NT), (unsigned)g.nmb, (unsigned)nvars);
    if (mom) k_coarsen_direct<true, Tab><<<grid, CO_NT, 0, st>>>(g, tab, out);
    else k_coarsen_direct<false, Tab><<<grid, CO_NT, 0, st>>>(g, tab, out);
  }
}

}  // namespace
}  // namespace akmi

using namespace akmi;

extern "C" {

int akmi_coarsen_default_staged(void) { return AKMI_COARSEN_DEFAULT_STAGED; }

int akmi_coarsen(const akmi_pack *p, const akmi_coarsen_var *vars, int nvars, int factor, int moments, const int *lo,
                 const int *nc, double *out, int staged, void *stream) {
  if (!p || !vars || !lo || !nc || !out) { set_error("coarsen: null pack, variable table, index range or output"); return AKMI_FAIL; }
  if (p->nmb < 1 || p->nx1 < 1 || p->nx2 < 1 || p->nx3 < 1 || p->ng < 0) {
    set_error("coarsen: pack with nmb %d, nx %d %d %d, ng %d", p->nmb, p->nx1, p->nx2, p->nx3, p->ng);
    return AKMI_FAIL;
  }
  if (nvars < 1 || nvars > 65535 || p->nmb > 65535) {
    set_error("coarsen: %d variables and %d MeshBlocks are outside the launch grid (1 .. 65535 each)", nvars, p->nmb);
    return AKMI_FAIL;
  }
  if (factor < 1 || factor > 1024) { set_error("coarsen: coarsen_factor = %d (1 .. 1024)", factor); return AKMI_FAIL; }
  const Geo geo = make_geo(p);
  const int N[3] = {geo.N1, geo.N2, geo.N3};
  for (int d = 0; d < 3; ++d) {
    // every fine cell a thread reads lies inside the array: lo >= 0 and lo + nc*f <= N
    if (lo[d] < 0 || nc[d] < 1 || (long long)lo[d] + (long long)nc[d]*factor > N[d]) {
      set_error("coarsen: direction %d: %d coarse cells of %d from index %d leave the array extent %d", d + 1, nc[d], factor,
                lo[d], N[d]);
      return AKMI_FAIL;
    }
  }
  if ((long long)nc[0]*nc[1]*nc[2] >= (1ll << 31) - CO_NT) { set_error("coarsen: too many coarse cells in a MeshBlock"); return AKMI_FAIL; }
  for (int n = 0; n < nvars; ++n) {
    if (!vars[n].array || vars[n].nvar < 1 || vars[n].comp < 0 || vars[n].comp >= vars[n].nvar) {
      set_error("coarsen: variable %d: array %p, component %d of %d", n, (const void *)vars[n].array, vars[n].comp, vars[n].nvar);
      return AKMI_FAIL;
    }
  }
  CoarsenGeo g;
  g.nmb = p->nmb; g.N1 = geo.N1; g.N2 = geo.N2; g.N3 = geo.N3;
  g.f = factor; g.lo1 = lo[0]; g.lo2 = lo[1]; g.lo3 = lo[2];
  g.nc1 = nc[0]; g.nc2 = nc[1]; g.nc3 = nc[2];
  g.cw = nc[0] < CO_NT ? nc[0] : CO_NT;
  if (g.cw > CO_LDS/factor) g.cw = CO_LDS/factor;
  g.R = CO_NT/g.cw;
  if (g.R > CO_LDS/(g.cw*factor)) g.R = CO_LDS/(g.cw*factor);
  g.ntile_i = cdiv(g.nc1, g.cw);
  if (staged < 0) {
    static const char *env = std::getenv("AKMI_COARSEN_STAGED");
    staged = env ? (std::atoi(env) != 0) : AKMI_COARSEN_DEFAULT_STAGED;
  }
  hipStream_t st = (hipStream_t)stream;
  if (nvars <= CO_TAB) {
    TabVal tab;
    for (int n = 0; n < CO_TAB; ++n) {
      const akmi_coarsen_var &s = vars[n < nvars ? n : 0];
      tab.v[n] = CoarsenVar{s.array, s.nvar, s.comp};
    }
    launch(staged != 0, moments != 0, g, tab, nvars, out, st);
    AKMI_CHECK_LAUNCH("coarsen");
    return AKMI_COMPLETE;
  }
  // a table that does not fit by value lives in device memory for the one launch
  std::vector<CoarsenVar> host(nvars);
  for (int n = 0; n < nvars; ++n) host[n] = CoarsenVar{vars[n].array, vars[n].nvar, vars[n].comp};
  CoarsenVar *dev = nullptr;
  if (hipMalloc(&dev, sizeof(CoarsenVar)*nvars) != hipSuccess ||
      hipMemcpyAsync(dev, host.data(), sizeof(CoarsenVar)*nvars, hipMemcpyHostToDevice, st) != hipSuccess) {
    set_error("coarsen: variable table of %d entries: %s", nvars, hipGetErrorString(hipGetLastError()));
    if (dev) (void)hipFree(dev);
    return AKMI_FAIL;
  }
  launch(staged != 0, moments != 0, g, TabPtr{dev}, nvars, out, st);
  const hipError_t e = hipGetLastError();
  const hipError_t e2 = hipStreamSynchronize(st);
  (void)hipFree(dev);
  if (e != hipSuccess || e2 != hipSuccess) {
    set_error("coarsen: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return AKMI_FAIL;
  }
  return AKMI_COMPLETE;
}

}  // extern "C"
