"""Shared by tests/test_stats_host.py (no GPU) and tests/test_gpu_stats.py: the CPU build of the statistics arithmetic
(tests/host_shim/stats_host.cpp), a CPU backend that adds it to the oracle-as-akmi stand-in, the synthetic fields of the
histogram tests and the bounds both suites use."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import stats_restate as S  # noqa: E402

SHIM = os.path.join(ROOT, "tests", "host_shim")
SO = os.path.join(SHIM, "libstats_host.so")
U = 2.0**-53


def build_shim():
    src = os.path.join(SHIM, "stats_host.cpp")
    csrc = os.path.join(ROOT, "athenak_amd", "csrc")
    deps = [src, os.path.join(csrc, "akmi_stats.hpp"), os.path.join(csrc, "akmi_derived.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        # -ffp-contract=off: products and sums rounded separately, as in the device build
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", SHIM, "-I", csrc,
                               src, "-o", SO])
    return C.CDLL(SO)


def install_cpu_backend():
    """tests/cpu_backend.py plus the derived variables, akmi_turb_history and akmi_pdf from the CPU builds"""
    import cpu_backend
    import derived_cases as dc
    from athenak_amd import capi
    H, D = build_shim(), dc.build_shim()

    class Backend(cpu_backend.OracleAsAkmi):
        def akmi_derived_var(self, *args):
            return D.hd_derived_var(*args[:-1])

        def akmi_derived_ncomp(self, which):
            return D.hd_derived_ncomp(which)

        def akmi_turb_history_workspace_bytes(self, pack):
            return 8

        def akmi_turb_history(self, *args):
            return H.hs_turb_history(*args[:7])          # without work and stream

        def akmi_pdf(self, *args):
            return H.hs_pdf(*args[:7])                   # without force_global and stream

    capi._LIB = Backend()
    capi.DEVICE = "cpu"


def uninstall_cpu_backend():
    import cpu_backend
    cpu_backend.uninstall()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def lognormal_field(shape, seed=1234):
    """exp(N(0, 1)), seeded"""
    return np.exp(np.random.default_rng(seed).standard_normal(shape))


def plant(view, seed):
    """into a view of cells: values exactly ON the power-of-two-spaced edges 0, 0.5, ..., 8 of 16 bins on [0, 8], exactly
    representable interior points, -0.0, +-inf and one NaN, at seeded places"""
    rng = np.random.default_rng(seed)
    pick = np.unravel_index(rng.choice(view.size, size=29, replace=False), view.shape)
    special = np.concatenate([np.arange(17)*0.5, np.arange(8)*1.0 + 0.25, [-0.0, np.inf, -np.inf, np.nan]])
    view[pick] = special


def linear_field(shape, seed, lo=-1.0, hi=9.0, planted=True):
    """uniform values around [0, 8): cells below the first edge and at or above the last; with `planted` the values of
    plant() anywhere in the array"""
    a = np.random.default_rng(seed).uniform(lo, hi, shape)
    if planted:
        plant(a, seed + 1)
    return a


def active(bx, a):
    """the active cells of (nmb, N3, N2, N1) in the order the weights list uses: flat over m, k, j, i"""
    return bx.act(a).reshape(-1)


def cell_volumes(bx, dx, nmb):
    n = bx.act(np.zeros((nmb, bx.N3, bx.N2, bx.N1))).shape
    vol = (dx[:, 0]*dx[:, 1])*dx[:, 2]
    return np.broadcast_to(vol[:, None, None, None], n).reshape(-1)


def check_weights(got_w, wl, what, skip=()):
    """every bin within n_b * 2^-53 * sum|w| of math.fsum of the weights the restatement puts there (the bound of a sum
    of n_b terms in ANY order: each of the n_b - 1 additions rounds a partial sum of magnitude at most sum|w|)"""
    worst = 0.0
    for yb, row in enumerate(wl):
        for xb, ws in enumerate(row):
            if (yb, xb) in skip:
                continue
            want = math.fsum(ws)
            bound = 1.0000001*len(ws)*U*math.fsum(abs(w) for w in ws)
            err = abs(float(got_w[yb, xb]) - want)
            if bound > 0:
                worst = max(worst, err/bound)
            assert err <= bound, (what, yb, xb, float(got_w[yb, xb]), want, err, bound)
    return worst


def check_total(got_w, counts, want_total, abs_sum, what, device_sum=False):
    """the total over all bins (added here with math.fsum) against `want_total`: each bin carries the bound above, so the
    total lies within sum_b n_b * 2^-53 * sum|w_b| <= N * 2^-53 * sum|w|.  device_sum: `want_total` is itself a device sum
    over the same N cells in some order (the mass column of akmi_history_sums) and carries the same bound again"""
    n = int(np.asarray(counts).sum())
    tot = math.fsum(np.asarray(got_w).ravel().tolist())
    bound = (2.0 if device_sum else 1.0)*1.0000001*n*U*abs_sum
    print("%s: total %.17g, expected %.17g, |diff| %.3e, bound %.3e" % (what, tot, want_total, abs(tot - want_total), bound))
    assert abs(tot - want_total) <= bound, (what, tot, want_total, bound)


def restated_hist(vals, weights, edges, step, log, vals2=None, edges2=None, step2=None, log2=None):
    """counts and per-bin weight lists of the restatement, and the entries a cell near a log edge could move between (its
    own bin and the neighbours): those are left out of a comparison with the device, whose log10 is not the C library's"""
    counts, wl, nan, _ = S.histogram(vals, weights, edges, step, log, vals2, edges2, step2, log2)
    skip = set()
    v2 = vals2 if vals2 is not None else [0.0]*len(vals)
    for x, y in zip(vals, v2):
        if S.pdf_near_edge(x, edges, step, log) or (vals2 is not None and S.pdf_near_edge(y, edges2, step2, log2)):
            xb = S.pdf_index(x, edges, step, log)
            yb = 0 if vals2 is None else S.pdf_index(y, edges2, step2, log2)
            if xb is not None and yb is not None:
                skip |= {(yb + b, xb + a) for a in (-1, 0, 1) for b in (-1, 0, 1)}
    return counts, wl, nan, skip


def check_hist(got_c, got_w, restated, what):
    """counts equal and weights within the bound of check_weights, over the entries no near-edge cell can reach; at most 1
    cell in 10^4 may be near an edge"""
    counts, wl, nan, skip = restated
    assert len(skip) <= 9*max(1, counts.sum()//10**4), (what, len(skip))
    for yb in range(counts.shape[0]):
        for xb in range(counts.shape[1]):
            if (yb, xb) not in skip:
                assert int(got_c[yb, xb]) == int(counts[yb, xb]), (what, yb, xb, int(got_c[yb, xb]), int(counts[yb, xb]))
    worst = check_weights(got_w, wl, what, skip)
    print("%s: %d entries left out near a log edge, worst weight err/bound %.3f" % (what, len(skip), worst))
