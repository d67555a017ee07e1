// akmi_stage_hydro.hip -- the one-kernel hydro stage of DC / PLM (k_hydro_stage3d2, akmi_hydro_stage3d2.hpp): its
// instantiations and its launcher.
#include <map>
#include "akmi_hydro_stage3d2.hpp"

namespace akmi {

// dynamic LDS beyond the 64 KB a kernel gets by default: granted once per kernel function and size
static int ensure_lds(const void *kern, size_t lds, const char *who) {
  static std::map<const void *, size_t> granted;
  size_t &gr = granted.emplace(kern, (size_t)64*1024).first->second;
  if (lds <= gr) return AKMI_COMPLETE;
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    set_error("%s: %zu bytes of LDS refused", who, lds);
    return AKMI_FAIL;
  }
  gr = lds;
  return AKMI_COMPLETE;
}

// tl: the tile of the stage's plan (plan_stage); cpa: ConsToPrim of the finished cells inside the kernel (new primitives
// to cpa->w_out), nullptr: update only
template <bool MASS>
int launch_hydro_stage3d(const Geo &g, const Scheme &sc, const HydTile &tl, const double *w0, const UpdArgs &u,
                         int kA, int kB, hipStream_t st, Mass3 ms, const HydC2P *cpa) {
  int ckl = march_len((long)tl.n1*tl.n2, kB - kA + 1, g.nmb, ML);
  static const int ckl_env = getenv("AKMI_HS_CKL") ? atoi(getenv("AKMI_HS_CKL")) : 0;     // experiments: pin the chunk length
  if (ckl_env > 0) ckl = ckl_env;                   // (128^3: the rule's 4 sits on the flat bottom, profiles/r05_hydro_host_ab.txt)
  const int nchunk = cdiv(kB - kA + 1, ckl);
  const size_t lds = hyd_lds_doubles(tl.tw, tl.th)*sizeof(double);
  dim3 grid(tl.n1, tl.n2, nchunk*g.nmb), block(tl.threads);
  int rc = dispatch_scheme_eos<false>(sc, [&](auto R, auto S) {
    constexpr int RV = decltype(R)::value, SV = decltype(S)::value;
    if constexpr (RV <= 1) {
      auto go = [&](auto kern, const HydC2P &cp) {
        if (ensure_lds((const void *)kern, lds, "hydro_stage3d") != AKMI_COMPLETE) return (int)AKMI_FAIL;
        kern<<<grid, block, lds, st>>>(g, sc.eos, w0, u, kA, kB, nchunk, ckl, tl.tw, tl.th, ms, cp);
        return (int)AKMI_COMPLETE;
      };
      if constexpr (!MASS && SV < 10) {
        if (cpa) return go(k_hydro_stage3d2<RV, SV, false, true>, *cpa);
      }
      if (cpa) { set_error("hydro_stage3d: ConsToPrim inside the kernel is for the ideal gas without passive scalars"); return (int)AKMI_FAIL; }
      return go(k_hydro_stage3d2<RV, SV, MASS, false>, HydC2P{});
    } else {
      set_error("hydro_stage3d: DC and PLM only");
      return (int)AKMI_FAIL;
    }
  });
  if (rc != AKMI_COMPLETE) return rc;
  AKMI_CHECK_LAUNCH("hydro_stage3d");
  return AKMI_COMPLETE;
}

template int launch_hydro_stage3d<false>(const Geo &, const Scheme &, const HydTile &, const double *, const UpdArgs &,
                                         int, int, hipStream_t, Mass3, const HydC2P *);
template int launch_hydro_stage3d<true>(const Geo &, const Scheme &, const HydTile &, const double *, const UpdArgs &,
                                        int, int, hipStream_t, Mass3, const HydC2P *);

}  // namespace akmi
