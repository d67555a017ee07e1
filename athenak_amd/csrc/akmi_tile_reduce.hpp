// akmi_tile_reduce.hpp -- the deterministic sums over the active cells of a pack that akmi_turb.hip and akmi_stats.hip
// share: a workgroup of NT threads owns a tile of TILE cells (PER strided cells per thread), sums its threads' values by
// a fixed-shape tree (block_sum), and the tiles of one MeshBlock are summed by a second fixed-shape tree (k_tile_sum)
// into per-MeshBlock partials.  No floating-point atomics: a partial depends only on the cells of its block.
#ifndef AKMI_TILE_REDUCE_HPP_
#define AKMI_TILE_REDUCE_HPP_
#include "akmi_common.hpp"

namespace akmi {

constexpr int NT = 256;          // threads per workgroup
constexpr int PER = 4;           // cells per thread
constexpr int TILE = NT*PER;     // cells per workgroup (tile)

struct TurbGeo {
  int nx1, nx2, nx3, is, js, ks;
  int N1, N2, N3, nvar;
  int ncell, ntile;
};

inline TurbGeo make_tgeo(const akmi_pack *p) {
  const Geo g = make_geo(p);
  TurbGeo t;
  t.nx1 = g.nx1; t.nx2 = g.nx2; t.nx3 = g.nx3;
  t.is = g.is; t.js = g.js; t.ks = g.ks;
  t.N1 = g.N1; t.N2 = g.N2; t.N3 = g.N3; t.nvar = g.nvar;
  t.ncell = g.nx1*g.nx2*g.nx3;
  t.ntile = cdiv(t.ncell, TILE);
  return t;
}

// sum of v[q] over the NT threads of a workgroup by a fixed-shape tree; thread 0 writes out[q]
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double *out) {
  __shared__ double red[K][NT];
  for (int q = 0; q < K; ++q) red[q][threadIdx.x] = v[q];
  __syncthreads();
  for (int h = NT/2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h)
      for (int q = 0; q < K; ++q) red[q][threadIdx.x] = red[q][threadIdx.x] + red[q][threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    for (int q = 0; q < K; ++q) out[q] = red[q][0];
}

// per-MeshBlock partials: blockIdx.x = m; the ntile tile partials of m summed by threads strided over the tiles,
// then the tree; out[m*K + q]
template <int K>
__global__ void __launch_bounds__(NT) k_tile_sum(int ntile, const double *__restrict__ tiles, double *__restrict__ out) {
  const int m = blockIdx.x;
  double v[K];
  for (int q = 0; q < K; ++q) v[q] = 0.0;
  for (int t = threadIdx.x; t < ntile; t += NT)
    for (int q = 0; q < K; ++q) v[q] += tiles[((size_t)m*ntile + t)*K + q];
  block_sum<K>(v, out + (size_t)m*K);
}

__device__ __forceinline__ void cell_of(const TurbGeo &g, int c, int &k, int &j, int &i) {
  i = c % g.nx1;
  const int r = c/g.nx1;
  j = r % g.nx2;
  k = r/g.nx2;
}

inline bool pack_ok(const akmi_pack *p, const char *who) {
  if (p->nvar < 4 || p->nmb < 1 || p->nx1 < 1 || p->nx2 < 1 || p->nx3 < 1) {
    set_error("%s: pack with nmb %d, nvar %d, nx %d %d %d", who, p->nmb, p->nvar, p->nx1, p->nx2, p->nx3);
    return false;
  }
  return true;
}

template <int K>
inline int finish_partials(const TurbGeo &g, int nmb, const double *tiles, double *partial, hipStream_t st,
                           const char *who) {
  k_tile_sum<K><<<nmb, NT, 0, st>>>(g.ntile, tiles, partial);
  AKMI_CHECK_LAUNCH(who);
  return AKMI_COMPLETE;
}

}  // namespace akmi
#endif
