// akmi_stats.hip -- statistics of a run while it runs: the turbulence history columns (TurbulentHistory,
// src/pgen/fluids/turb.cpp:247-396) and the histograms of the pdf output (PDFOutput::LoadOutputData, src/outputs/pdf.cpp).
// The per-cell arithmetic lives in akmi_stats.hpp, shared with the CPU build the non-GPU tests use.
//
// k_turb_hist   eleven terms per active cell; a workgroup owns a tile of TILE cells and sums them by the fixed-shape tree
//               of akmi_tile_reduce.hpp, k_tile_sum adds the tiles of a MeshBlock by the second tree: per-MeshBlock
//               partials that depend only on the block's cells.  No floating-point atomics; the caller adds the
//               partials in gid order.
// k_pdf<true>   a workgroup walks over tiles of cells and keeps a private histogram in LDS (32-bit counts, fp64 weights,
//               LDS atomics); at the end it adds its non-zero bins to the result, one 64-bit integer and one fp64 global
//               atomic per bin.  Taken while the histogram has at most PDF_LDS_BINS entries.
// k_pdf<false>  every cell adds to the result in global memory directly (large 2-D histograms).
// Counts are integers: exact whatever the order.  The fp64 weight of a bin is a sum in arrival order, so its last bits
// can differ from run to run (as with the reference's ScatterView and with akmi_history_sums).
#include "akmi_common.hpp"
#include "akmi_tile_reduce.hpp"
#include "akmi_stats.hpp"
#include <cstdlib>
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace akmi {
namespace {

// Entries of the private histogram: 4 B (count) + 8 B (weight) each; with the NaN counter the kernel takes 49 160 B of
// the 160 KiB (163 840 B) of LDS of a compute unit, so
// that three workgroups (twelve waves) fit on one and the static limit of 64 KiB per workgroup is kept.  A 1-D histogram
// of 100 bins has 102 entries, a 2-D one of 62 x 62 bins 4096; 100 x 100 (10 404 entries, 122 KiB) would leave room for
// one workgroup per compute unit and takes the global path.
constexpr int PDF_LDS_BINS = AKMI_PDF_LDS_BINS;
// workgroups of a launch of the LDS path: each walks over many tiles, so that clearing and flushing the private
// histogram is paid once per workgroup and not once per 1024 cells (256 compute units x 3 resident workgroups)
constexpr int PDF_MAX_GROUPS = 768;

DvIn make_dvin(const Geo &g, const double *w0, const double *bcc0, const double *b1, const double *b2, const double *b3) {
  DvIn a;
  a.nvar = g.nvar; a.N1 = g.N1; a.N2 = g.N2; a.N3 = g.N3;
  a.is = g.is; a.ie = g.ie; a.js = g.js; a.je = g.je; a.ks = g.ks; a.ke = g.ke; a.ng = g.ng;
  a.multi_d = g.multi_d; a.three_d = g.three_d;
  a.dx = g.dx; a.w0 = w0; a.bcc0 = bcc0; a.b1 = b1; a.b2 = b2; a.b3 = b3;
  return a;
}

__global__ void __launch_bounds__(NT) k_turb_hist(TurbGeo g, DvIn a, double *__restrict__ tiles) {
  const int m = blockIdx.x/g.ntile, tile = blockIdx.x - m*g.ntile;
  double acc[TURB_NHIST];
  for (int q = 0; q < TURB_NHIST; ++q) acc[q] = 0.0;
  for (int p = 0; p < PER; ++p) {
    const int c = tile*TILE + p*NT + threadIdx.x;
    if (c >= g.ncell) break;
    int k, j, i;
    cell_of(g, c, k, j, i);
    double h[TURB_NHIST];
    turb_hist_cell(a, m, k + g.ks, j + g.js, i + g.is, h);
    for (int q = 0; q < TURB_NHIST; ++q) acc[q] += h[q];
  }
  block_sum<TURB_NHIST>(acc, tiles + (size_t)blockIdx.x*TURB_NHIST);
}

struct PdfOut {
  unsigned long long *counts;    // [(nbin2+2)|1][nbin+2]
  double *weights;               // same shape
  unsigned long long *nan;       // cells dropped because a value is NaN
};

// entry of the cell in the histogram, -1 for a dropped cell; *wgt its weight
__device__ __forceinline__ int pdf_cell(const TurbGeo &g, const PdfAxis &x, const PdfAxis &y, const double *dens,
                                        const double *dx, int m, int c, double *wgt) {
  int k, j, i;
  cell_of(g, c, k, j, i);
  k += g.ks; j += g.js; i += g.is;
  const size_t cs = (size_t)g.N3*g.N2*g.N1, off = ((size_t)k*g.N2 + j)*g.N1 + i;
  const int xb = pdf_bin(x.a[((size_t)m*x.nv + x.comp)*cs + off], x.nbin, x.logscale, x.lo, x.hi, x.step);
  int yb = 0;
  if (y.a) yb = pdf_bin(y.a[((size_t)m*y.nv + y.comp)*cs + off], y.nbin, y.logscale, y.lo, y.hi, y.step);
  double weight = dx[3*m]*dx[3*m + 1]*dx[3*m + 2];
  if (dens) weight *= dens[((size_t)m*g.nvar + AKMI_IDN)*cs + off];
  *wgt = weight;
  return (xb < 0 || yb < 0) ? -1 : yb*(x.nbin + 2) + xb;
}

template <bool LDS>
__global__ void __launch_bounds__(NT)
k_pdf(TurbGeo g, int ntile_all, int nent, PdfAxis x, PdfAxis y, const double *__restrict__ dens,
      const double *__restrict__ dx, PdfOut out) {
  __shared__ unsigned s_cnt[LDS ? PDF_LDS_BINS : 1];
  __shared__ double s_wgt[LDS ? PDF_LDS_BINS : 1];
  __shared__ unsigned s_nan;
  if (LDS) {
    for (int e = threadIdx.x; e < nent; e += NT) { s_cnt[e] = 0u; s_wgt[e] = 0.0; }
  }
  if (threadIdx.x == 0) s_nan = 0u;
  __syncthreads();
  for (int t = blockIdx.x; t < ntile_all; t += gridDim.x) {
    const int m = t/g.ntile, tile = t - m*g.ntile;
    for (int p = 0; p < PER; ++p) {
      const int c = tile*TILE + p*NT + threadIdx.x;
      if (c >= g.ncell) break;
      double w;
      const int e = pdf_cell(g, x, y, dens, dx, m, c, &w);
      if (e < 0) {
        atomicAdd(&s_nan, 1u);
      } else if (LDS) {
        atomicAdd(&s_cnt[e], 1u);
        atomicAdd(&s_wgt[e], w);
      } else {
        atomicAdd(&out.counts[e], 1ull);
        unsafeAtomicAdd(&out.weights[e], w);
      }
    }
  }
  __syncthreads();
  if (LDS) {
    for (int e = threadIdx.x; e < nent; e += NT) {
      const unsigned n = s_cnt[e];
      if (n != 0u) {
        atomicAdd(&out.counts[e], (unsigned long long)n);
        unsafeAtomicAdd(&out.weights[e], s_wgt[e]);
      }
    }
  }
  if (threadIdx.x == 0 && s_nan != 0u) atomicAdd(out.nan, (unsigned long long)s_nan);
}

bool axis_ok(const akmi_pdf_axis *x, const char *who) {
  if (!x->array || x->nvar < 1 || x->comp < 0 || x->comp >= x->nvar) {
    set_error("pdf: %s variable: array %p, component %d of %d", who, (const void *)x->array, x->comp, x->nvar);
    return false;
  }
  if (x->nbin < 1) { set_error("pdf: %s axis with nbin = %d", who, x->nbin); return false; }
  if (!(x->step > 0.0) || !(x->bin_hi > x->bin_lo) || (x->logscale && !(x->bin_lo > 0.0))) {
    set_error("pdf: %s axis: edges %g .. %g, step %g%s", who, x->bin_lo, x->bin_hi, x->step,
              x->logscale ? " (logarithmic bins need a positive first edge)" : "");
    return false;
  }
  return true;
}

PdfAxis make_axis(const akmi_pdf_axis *x) {
  return PdfAxis{x->array, x->nvar, x->comp, x->nbin, x->logscale, x->bin_lo, x->bin_hi, x->step};
}

}  // namespace
}  // namespace akmi

using namespace akmi;

extern "C" {

long long akmi_turb_history_workspace_bytes(const akmi_pack *p) {
  const TurbGeo g = make_tgeo(p);
  return (long long)p->nmb*g.ntile*TURB_NHIST*sizeof(double);
}

int akmi_turb_history(const akmi_pack *p, const double *w0, const double *bcc0, const double *bx1f, const double *bx2f,
                      const double *bx3f, double *partial, double *work, void *stream) {
  if (!p || !pack_ok(p, "turb_history")) return AKMI_FAIL;
  if (!w0 || !bcc0 || !bx1f || !bx2f || !bx3f) {
    set_error("turb_history: needs w0, bcc0 and the three face fields (an MHD pack)");
    return AKMI_FAIL;
  }
  if (!partial || !work) { set_error("turb_history: null partial or work array"); return AKMI_FAIL; }
  const Geo geo = make_geo(p);
  if (geo.ng < 1) { set_error("turb_history: the centred differences need a ghost cell"); return AKMI_FAIL; }
  const TurbGeo g = make_tgeo(p);
  hipStream_t st = (hipStream_t)stream;
  k_turb_hist<<<p->nmb*g.ntile, NT, 0, st>>>(g, make_dvin(geo, w0, bcc0, bx1f, bx2f, bx3f), work);
  AKMI_CHECK_LAUNCH("turb_history");
  return finish_partials<TURB_NHIST>(g, p->nmb, work, partial, st, "turb_history partials");
}

int akmi_pdf(const akmi_pack *p, const akmi_pdf_axis *x, const akmi_pdf_axis *y, const double *u0_mass,
             unsigned long long *counts, double *weights, unsigned long long *nan_count, int force_global,
             void *stream) {
  if (!p || !pack_ok(p, "pdf")) return AKMI_FAIL;
  if (!x || !counts || !weights || !nan_count) { set_error("pdf: null axis or output array"); return AKMI_FAIL; }
  if (!axis_ok(x, "first") || (y && !axis_ok(y, "second"))) return AKMI_FAIL;
  const long long nent = (long long)(y ? y->nbin + 2 : 1)*(x->nbin + 2);
  if (nent >= (1ll << 31)) { set_error("pdf: %lld histogram entries", nent); return AKMI_FAIL; }
  const TurbGeo g = make_tgeo(p);
  const long long ntile_all = (long long)p->nmb*g.ntile;
  if (ntile_all >= (1ll << 31) || ntile_all*TILE >= (1ll << 32)) {
    // (a workgroup's 32-bit private count could not hold every cell either)
    set_error("pdf: a pack of %lld tiles of %d cells is outside the launch grid", ntile_all, TILE);
    return AKMI_FAIL;
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(unsigned long long)*nent, st) != hipSuccess ||
      hipMemsetAsync(weights, 0, sizeof(double)*nent, st) != hipSuccess ||
      hipMemsetAsync(nan_count, 0, sizeof(unsigned long long), st) != hipSuccess) {
    set_error("pdf: clearing the histogram: %s", hipGetErrorString(hipGetLastError()));
    return AKMI_FAIL;
  }
  const PdfAxis ax = make_axis(x);
  const PdfAxis ay = y ? make_axis(y) : PdfAxis{nullptr, 1, 0, 0, 0, 0.0, 1.0, 1.0};
  const PdfOut out{counts, weights, nan_count};
  static const bool env_global = std::getenv("AKMI_PDF_FORCE_GLOBAL") && std::atoi(std::getenv("AKMI_PDF_FORCE_GLOBAL")) != 0;
  if (nent <= PDF_LDS_BINS && !force_global && !env_global) {
    const int groups = ntile_all < PDF_MAX_GROUPS ? (int)ntile_all : PDF_MAX_GROUPS;
    k_pdf<true><<<groups, NT, 0, st>>>(g, (int)ntile_all, (int)nent, ax, ay, u0_mass, p->dx, out);
  } else {
    k_pdf<false><<<(int)ntile_all, NT, 0, st>>>(g, (int)ntile_all, (int)nent, ax, ay, u0_mass, p->dx, out);
  }
  AKMI_CHECK_LAUNCH("pdf");
  return AKMI_COMPLETE;
}

int akmi_pdf_lds_bins(void) { return PDF_LDS_BINS; }

}  // extern "C"
