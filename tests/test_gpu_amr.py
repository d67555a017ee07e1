"""gpu: adaptive mesh refinement on the device (csrc/akmi_amr.hip) against the numpy restatement of the reference
(tests/amr_restate.py) and against the same host on the CPU backend, bit for bit:
  * the criteria kernel: flags identical, extremum planted in the last lane of the last partial tile at a block
    corner, loud ghost cells, the equality case, two criteria in sequence;
  * the regrid kernels: every output element identical, untouched elements still the sentinel; repair; div B;
  * whole adaptive runs (leaf lists after every cycle, u0 / b0 / dt at the end), the frozen mesh, outputs.
Nothing here is measured or timed; the figures of DESIGN section 17 come from profiles/."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import amr_cases as ac  # noqa: E402
import amr_restate as ar  # noqa: E402
import amr_runs  # noqa: E402
from athenak_amd import capi  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pack(G, nmb, nvar, dx):
    nx3, nx2, nx1 = G.nx
    return capi.Pack(nmb, nvar, nx1, nx2, nx3, G.ng, dx.data_ptr(), 5.0/3.0, 1e-30, 1e-30, 1e-30, 1e-30, 1e30, 0.0, 1)


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _check(L, pk, method, q, vmin, vmax, flags):
    capi.check(L.akmi_amr_check(C.byref(pk), capi.AMR_METHOD[method], capi._p(q), C.c_longlong(q.stride(0)),
                                capi.d(vmin), capi.d(vmax), capi._p(flags), capi._stream()), "amr_check")


@pytest.mark.parametrize("shape", ac.CHECK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_criteria_kernel_flags_are_the_restatements(shape):
    nx1, nx2, nx3, ng, nmb = shape
    G = ar.Geom(nx1, nx2, nx3, ng)
    L = capi.lib()
    dx = torch.ones((nmb, 3), dtype=torch.float64, device=DEV)
    pk = _pack(G, nmb, 1, dx)
    seen = set()
    for n, method in enumerate(("min_max", "slope", "second_deriv")):
        thr = 2.0 if method == "min_max" else 0.05
        q = ac.planted_field(G, nmb, method, thr, 100 + n, equal_block=0 if method == "min_max" else None)
        want = ar.check(G, method, q, -ar.FLT_MAX, thr, np.zeros(nmb, dtype=np.int32))
        # the plant is what decides: the last block refines, the others would derefine -- except the equality case
        assert want[nmb - 1] == 1 and all(w == -1 for w in want[1:nmb - 1]), (method, want)
        if method == "min_max":
            assert want[0] == 0, want                      # exactly the threshold: the flag stays
        flags = torch.zeros(nmb, dtype=torch.int32, device=DEV)
        _check(L, pk, method, _t(q), -ar.FLT_MAX, thr, flags)
        got = flags.cpu().numpy()
        assert np.array_equal(got, want), (method, got, want)
        seen.update(got.tolist())
    assert seen == {-1, 0, 1}
    # the minimum branch of min_max, and two criteria in sequence on the same flags (an earlier +1 is not lowered, an
    # earlier -1 is raised, a 0 may be lowered)
    rng = np.random.default_rng(7)
    q1 = ac.planted_field(G, nmb, "min_max", 2.0, 11)
    q2 = 1.0e6*np.ones_like(q1)
    (ks, js, is_), (ke, je, ie) = G.s, G.e
    q2[:, ks:ke + 1, js:je + 1, is_:ie + 1] = rng.uniform(3.0, 4.0, size=(nmb,) + G.nx)
    q2[0, ke, je, ie] = 0.5                                 # block 0: minimum below value_min -> refine
    q2[:, ks - 1 if G.on[0] else 0, js - 1 if G.on[1] else 0, is_ - 1] = -1.0e6     # a ghost that would win a min
    want = np.zeros(nmb, dtype=np.int32)
    ar.check(G, "min_max", q1, -ar.FLT_MAX, 2.0, want)
    ar.check(G, "min_max", q2, 1.0, ar.FLT_MAX, want)
    flags = torch.zeros(nmb, dtype=torch.int32, device=DEV)
    _check(L, pk, "min_max", _t(q1), -ar.FLT_MAX, 2.0, flags)
    _check(L, pk, "min_max", _t(q2), 1.0, ar.FLT_MAX, flags)
    assert np.array_equal(flags.cpu().numpy(), want), (flags.cpu().numpy(), want)
    assert want[0] == 1 and want[nmb - 1] == 1


@pytest.mark.parametrize("shape", ac.CHECK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_criteria_kernel_reduces_the_restatements_value_to_the_bit(shape):
    """For each method and each block the restatement's extremum E is taken, and the kernel is run with the threshold
    exactly E (the flag stays 0), one ulp below E and one ulp above E (the flag goes to +1 and -1, or the reverse for
    the minimum): the three answers pin the value the device reduced to the very bit of E, so a dropped stencil arm,
    factor, square root, division or absolute value, or a neighbour read from the wrong cell, fails.  (Square root and
    division are correctly rounded on both sides; products and sums are rounded separately on both.)"""
    nx1, nx2, nx3, ng, nmb = shape
    G = ar.Geom(nx1, nx2, nx3, ng)
    L = capi.lib()
    dx = torch.ones((nmb, 3), dtype=torch.float64, device=DEV)
    pk = _pack(G, nmb, 1, dx)
    (ks, js, is_), (ke, je, ie) = G.s, G.e
    for n, (method, use_min) in enumerate((("min_max", False), ("min_max", True), ("slope", False),
                                           ("second_deriv", False))):
        q = ac.varied_field(G, nmb, 40 + n)
        if method == "min_max":                    # every ghost cell would win the reduction if it were read
            act = np.zeros(q.shape, dtype=bool)
            act[:, ks:ke + 1, js:je + 1, is_:ie + 1] = True
            q[~act] = -1.0e6 if use_min else 1.0e6
        val = ar.criterion_values(G, method, q).reshape(nmb, -1)
        ext = val.min(axis=1) if use_min else val.max(axis=1)
        if method != "min_max":                    # the plants decide in the first and the last block
            assert val[0].argmax() == 0 and val[nmb - 1].argmax() == val.shape[1] - 1
        qd = _t(q)
        for m in range(nmb):
            below, above = np.nextafter(ext[m], -np.inf), np.nextafter(ext[m], np.inf)
            for thr, expect in ((ext[m], 0), (below, -1 if use_min else 1), (above, 1 if use_min else -1)):
                vmin, vmax = (thr, ar.FLT_MAX) if use_min else (-ar.FLT_MAX, thr)
                want = ar.check(G, method, q, vmin, vmax, np.zeros(nmb, dtype=np.int32))
                assert want[m] == expect, (method, m, thr, want)
                flags = torch.zeros(nmb, dtype=torch.int32, device=DEV)
                _check(L, pk, method, qd, vmin, vmax, flags)
                got = flags.cpu().numpy()
                assert np.array_equal(got, want), (method, use_min, m, got, want)


@pytest.mark.parametrize("order", ["first", "last"])
@pytest.mark.parametrize("shape", ac.REGRID_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_regrid_kernels_are_the_restatement_bit_for_bit(shape, order):
    nx1, nx2, nx3, ng = shape
    G = ar.Geom(nx1, nx2, nx3, ng)
    nvar = 2
    old_nmb, plans = ac.regrid_plan(G)
    plan = plans[order]
    new_nmb = len(plan)
    assert sorted(set(plan[:, 0].tolist())) == [-1, 0, 1]
    assert sorted(plan[plan[:, 0] == 1][:, 2].tolist()) == list(range(G.nleaf))
    u, b, dx_old = ac.random_state(G, old_nmb, nvar, 5)
    _, _, dx_new = ac.random_state(G, new_nmb, nvar, 6)
    L = capi.lib()
    dxo, dxn = _t(dx_old), _t(dx_new)
    po, pn = _pack(G, old_nmb, nvar, dxo), _pack(G, new_nmb, nvar, dxn)
    plan_d = _t(plan, torch.int32)
    # --- cell-centred
    want_u = ar.regrid_cc(G, plan, u, np.full((new_nmb, nvar) + G.N, ac.SENTINEL))
    got_u = torch.full((new_nmb, nvar) + G.N, ac.SENTINEL, dtype=torch.float64, device=DEV)
    capi.check(L.akmi_amr_regrid_cc(C.byref(po), C.byref(pn), nvar, capi._p(plan_d), capi._p(_t(u)), capi._p(got_u),
                                    capi._stream()), "amr_regrid_cc")
    got_u = got_u.cpu().numpy()
    assert np.array_equal(got_u, want_u), np.argwhere(got_u != want_u)[:5]
    assert (want_u == ac.SENTINEL).any() and (want_u != ac.SENTINEL).any()
    # the kernel's own output conserves: sum of u*volume before and after, within 8 ulp per coarse cell
    for defect, bound in ac.conservation_defect(G, plan, u, got_u):
        assert defect <= bound, (defect, bound)
    # --- face-centred
    want_b = ar.regrid_fc(G, plan, b, [np.full((new_nmb,) + G.face_shape(d), ac.SENTINEL) for d in range(3)])
    got_b = [torch.full((new_nmb,) + G.face_shape(d), ac.SENTINEL, dtype=torch.float64, device=DEV) for d in range(3)]
    bo = [_t(x) for x in b]
    capi.check(L.akmi_amr_regrid_fc(C.byref(po), C.byref(pn), capi._p(plan_d), capi._p(bo[0]), capi._p(bo[1]),
                                    capi._p(bo[2]), capi._p(got_b[0]), capi._p(got_b[1]), capi._p(got_b[2]),
                                    capi._stream()), "amr_regrid_fc")
    for d in range(3):
        g = got_b[d].cpu().numpy()
        assert np.array_equal(g, want_b[d]), (d, np.argwhere(g != want_b[d])[:5])
        assert (want_b[d] == ac.SENTINEL).any()
    # --- repair on a flag vector with zeros and ones, from fields without sentinels
    rep = np.array([(m % 2) for m in range(new_nmb)], dtype=np.int32)
    assert 0 in rep and 1 in rep
    _, b2, _ = ac.random_state(G, new_nmb, nvar, 9)
    want_r = ar.repair_fc(G, rep, [x.copy() for x in b2])
    got_r = [_t(x) for x in b2]
    capi.check(L.akmi_amr_repair_fc(C.byref(pn), capi._p(_t(rep, torch.int32)), capi._p(got_r[0]), capi._p(got_r[1]),
                                    capi._p(got_r[2]), capi._stream()), "amr_repair_fc")
    for d in range(3):
        assert np.array_equal(got_r[d].cpu().numpy(), want_r[d]), d
    # --- div B of every refined block after regrid + repair: the restatement's, bit for bit.  (Ghost faces of the new
    # blocks are the sentinel's; only active faces enter.)
    refined = np.where(plan[:, 0] == 1)[0]
    repf = (plan[:, 0] != 0).astype(np.int32)
    want_rb = ar.repair_fc(G, repf, [x.copy() for x in want_b])
    capi.check(L.akmi_amr_repair_fc(C.byref(pn), capi._p(_t(repf, torch.int32)), capi._p(got_b[0]), capi._p(got_b[1]),
                                    capi._p(got_b[2]), capi._stream()), "amr_repair_fc")
    got_rb = [x.cpu().numpy() for x in got_b]
    dw = ar.divb(G, want_rb, dx_new)[refined]
    dg = ar.divb(G, got_rb, dx_new)[refined]
    assert np.array_equal(dw, dg) and np.isfinite(dw).all()


@pytest.mark.parametrize("case", sorted(amr_runs.WHOLE_RUNS))
def test_whole_adaptive_run_is_the_cpu_hosts(case):
    """12 cycles on the GPU and on the CPU backend: identical leaf lists after every cycle, u0 / b0 / dt identical
    at the end; the CPU run alone shows a refinement and a derefinement"""
    cpu = amr_runs.run(case, "cpu")
    assert cpu["created"] > 0 and cpu["deleted"] > 0, (cpu["created"], cpu["deleted"])
    gpu = amr_runs.run(case, "cuda")
    assert gpu["leaves"] == cpu["leaves"]
    assert gpu["dt"] == cpu["dt"] and gpu["created"] == cpu["created"] and gpu["deleted"] == cpu["deleted"]
    for k in cpu["arrays"]:
        assert np.array_equal(gpu["arrays"][k], cpu["arrays"][k]), k


def test_frozen_adaptive_mesh_is_the_static_one_on_the_gpu():
    a = amr_runs.run("frozen_adaptive", "cuda")
    s = amr_runs.run("frozen_static", "cuda")
    assert a["created"] == 0 and a["deleted"] == 0 and a["leaves"] == s["leaves"]
    assert a["dt"] == s["dt"]
    for k in s["arrays"]:
        assert np.array_equal(a["arrays"][k], s["arrays"][k]), k


def test_bin_and_hst_outputs_across_a_regrid():
    """a bin file written before and one after a regrid, split by the version-1.1 layout of the reference's reader as
    tests/derived_cases.read_bin restates it (the reference's own reader is checked against recorded output on the CPU,
    tests/test_amr_host.py), hold the old and the new block count; the hst mass is continuous across the regrid within the bound of the
    conservation test (8 ulp per coarse cell of the largest term)"""
    with tempfile.TemporaryDirectory() as d:
        res = amr_runs.outputs_across_regrid(d, "cuda")
    assert res["nmb_files"][0] == res["nmb_before"] and res["nmb_files"][-1] == res["nmb_after"]
    assert res["nmb_before"] != res["nmb_after"]
    # tab files and a derived variable follow the block count too
    rows = res["tab_rows"]
    assert len(rows) == len(res["nmb_files"]) and all(r % res["nx1"] == 0 for r in rows) and rows[-1] > rows[0], rows
    assert res["divb_blocks"] == res["nmb_files"]
    mass = res["hst_mass"]
    assert len(mass) >= 3
    assert np.max(np.abs(np.diff(mass))) <= res["mass_bound"], (mass, res["mass_bound"])
