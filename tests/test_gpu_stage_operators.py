"""gpu: ONE call of a stage entry of the library on an adversarial state against the oracle's task chain, bit for bit.

The fused stage -- k_sweep12s + the x3 march + k_corner_ct, k_hydro_stage3d2 (optionally with ConsToPrim inside), the
generic x1 sweep + x2 / x3 marches, the 1-D / 2-D sequences -- is otherwise checked against the oracle only through whole
runs of smooth decks, where every lane of a wave takes the same Riemann fan and every operand lies inside the exponent
window of the short square roots.  Here the state (tests/stage_cases.py: wild_state) has jumps of many decades between
neighbours, Bx = 0 faces, -0.0 momenta, zero slopes, one cell 2**-701 below its neighbour, floors that bind and mass fluxes
of both signs; tests/test_stage_cases_host.py asserts on the CPU that it reaches all of that.  Every array a call is given
is compared WHOLE with the expected one (np.array_equal: ghost zones and the sentinel of what must stay unwritten included),
the floor counters and the CFL minima exactly.  No deck, no driver: the pack is built directly.
Round the 2**-701 cell a stage leaves speeds that overflow, and they alone fix the CFL minima of those cases (0 for most
MHD ones); the `calm` cases are the same states without that cell, where dt3 is an ordinary number set by ordinary cells.

Shapes (cells per block; nghost 2, 3 for PPM4 / WENOZ) -- the smallest at which these kernels can still go wrong:
  3 x (12, 10, 9)   N1 = 16: k_sweep12s's waves of 60 cells end inside rows and the last one is partly clamped; march_len's
                    minimum of 4 cuts x2 and x3 into three chunks and k_corner_ct's planes into three k-chunks.  Block 0 has
                    dx = (1/16, 1/8, 1/8): the product branch; block 1 (1/12, 1/10, 1/9): the division branch; block 2
                    (1/16, 1/10, 1/8): k_sweep12s and the x2 march need dx1 AND dx2 to be powers of two, k_corner_ct all three.
  1 x (11, 9, 10)   odd rows of 15 cells, rows of the sign bytes unaligned.
  1 x (132, 6, 5)   tile seams along x1.  One tile would be 133 positions wide, more than the 130 hyd_tile and ct_tile allow,
                    so both cut the row whatever their cost functions prefer.  Following the two functions by hand
                    (tw*th <= 256, one halo entry per thread, lowest cost): hyd_tile(132, 6) = 34 x 7 positions, 4 x 1
                    tiles of 33 x 6 cells; ct_tile(133, 7) = 35 x 9 positions, 4 x 1 tiles.
  1 x (6, 40, 5)    tile seams along x2.  A tile of hyd_tile is at most 40 positions = 39 cells high, one of ct_tile 32
                    positions, so 40 rows of cells (41 of edges) need two.  hyd_tile(6, 40) = 7 x 27 positions, 1 x 2 tiles
                    of 6 x 26 cells; ct_tile(7, 41) = 8 x 16 positions, 1 x 3 tiles.
                    (The other shapes are one tile: 13 x 14 / 12 x 10 positions of k_hydro_stage3d2, 14 x 13 / 13 x 14 of
                    k_corner_ct.)  These two shapes run for MHD PLM + HLLD and hydro PLM + HLLC only.
  8 x (12, 10), 64 x (16)   the 2-D and 1-D sequences, with enough blocks for ~1 000 active cells.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stage_cases as sc  # noqa: E402


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(case):
    """the case's stage call on fresh device copies of its inputs; every array back on the host"""
    import torch
    from athenak_amd import capi
    L = capi.lib()
    pk, dx = sc.case_pack(case)
    mhd = case.mhd
    pkd = capi.Pack.from_buffer_copy(bytes(pk))
    dxd = _dev(dx)
    pkd.dx = dxd.data_ptr()
    a = {k: _dev(v) for k, v in sc.stage_inputs(sc.case_state(case), case.copy, mhd).items()}
    a["counters"] = torch.zeros(3, dtype=torch.int32, device="cuda")
    a["dt3"] = torch.full((3,), sc.SENTINEL, dtype=torch.float64, device="cuda")      # do_newdt = 1 resets it itself
    ws = torch.zeros(int(L.akmi_stage_workspace_bytes(C.byref(pkd), 1 if mhd else 0))//8 + 1, dtype=torch.float64,
                     device="cuda")
    g0, g1, beta, dt = sc.WEIGHTS[case.weights]
    rc, rs = capi.RECON[case.recon], capi.RSOLVER[case.rs]
    copy = case.copy | sc.FLAG_SETS[case.flags]
    p = lambda k: capi._p(a[k])
    faces = [p(b + q) for b in ("b0", "b1") for q in sc.BNAMES] if mhd else []
    cells = [p("w0")] + ([p("bcc0")] if mhd else []) + [p("u0"), p("u1")] + faces
    head = [C.byref(pkd), rc, rs, capi.d(g0), capi.d(g1)]
    tail = [capi._p(ws), capi._stream()]
    fluid = case.fluid
    if case.entry == "update":
        rc_ = getattr(L, "akmi_%s_stage_update" % fluid)(*head, capi.d(beta*dt), copy, *cells, *tail)
    elif case.entry == "fused":
        rc_ = getattr(L, "akmi_%s_stage_fused" % fluid)(*head, capi.d(beta*dt), copy, *cells, 1, p("counters"), p("dt3"),
                                                        *tail)
    elif case.entry == "fused_dt":
        a["dt_dev"] = torch.tensor([dt], dtype=torch.float64, device="cuda")
        rc_ = getattr(L, "akmi_%s_stage_fused_dt" % fluid)(*head, capi.d(beta), p("dt_dev"), copy, *cells, 1, p("counters"),
                                                           p("dt3"), *tail)
    else:
        assert case.entry == "w" and not mhd
        a["w0_new"] = torch.full_like(a["w0"], sc.SENTINEL)
        wrote = C.c_int(-1)
        rc_ = L.akmi_hydro_stage_w(*head, capi.d(beta*dt), None, copy, p("w0"), p("w0_new"), p("u0"), p("u1"), 1,
                                   p("counters"), p("dt3"), *tail, C.byref(wrote))
        a["wrote_new"] = torch.tensor([wrote.value])
    capi.check(rc_, case.id())
    forms = L.akmi_stage_last_forms()
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in a.items()}
    out["forms"] = forms
    return out


def _first_difference(name, got, want):
    idx = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return "%s: %d elements differ, first at %s: %r against %r" % (name, len(idx), tuple(idx[0]), got[tuple(idx[0])],
                                                                   want[tuple(idx[0])])


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.id())
def test_stage_call_against_oracle(case):
    exp = sc.case_expected(case)
    got = _call(case)
    g = sc.Geo(sc.case_pack(case)[0])
    names = ["u0", "u1", "w0"] + (["bcc0"] + [b + q for b in ("b0", "b1") for q in sc.BNAMES] if case.mhd else [])
    bad = []
    if case.entry == "w":
        # ConsToPrim inside the update kernel: the new primitives of the ACTIVE cells land in w0_new, w0 stays as it was
        assert got["wrote_new"][0] == 1
        act = (slice(None), slice(None)) + g.active()
        if not np.array_equal(got["w0"], sc.case_state(case)["w0"]):
            bad.append(_first_difference("w0 (must stay unchanged)", got["w0"], sc.case_state(case)["w0"]))
        if not np.array_equal(got["w0_new"][act], exp["w0"][act]):
            bad.append(_first_difference("w0_new (active cells)", got["w0_new"][act], exp["w0"][act]))
        names = ["u0", "u1"]
    for k in names:
        if not np.array_equal(got[k], exp[k]):
            bad.append(_first_difference(k, got[k], exp[k]))
    if case.entry != "update":
        if list(got["counters"]) != list(exp["counters"]):
            bad.append("counters: %s against %s" % (got["counters"], exp["counters"]))
        if not np.array_equal(got["dt3"], exp["dt3"]):
            bad.append("dt3: %r against %r" % (got["dt3"], exp["dt3"]))
    assert not bad, "\n".join(bad)
    if case.fluid == "mhd" and case.recon == "plm" and case.rs == "hlld" and case.ideal and case.nscal == 0 and g.three_d:
        assert got["forms"] == sc.FORMS_OF[sc.FLAG_SETS[case.flags]], got["forms"]
