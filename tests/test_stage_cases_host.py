"""CPU: the conditions that keep test_gpu_stage_operators.py from passing vacuously, asserted on the oracle alone for
every state and every reference the GPU file uses (tests/stage_cases.py: CASES).

  * every output of oracle_stage is finite -- also round the cell whose density is 2**TINY_EXP of its neighbour's;
  * every selection of the Riemann fan (six of HLLD, three regions of HLLC) is taken on at least 1 % of the faces of every
    direction, so lanes of one wave take different selections;
  * mass fluxes of both signs occur in every direction (the sign bytes k_corner_ct reads), and in the MHD pack of three
    blocks one that is exactly zero;
  * with the entries that convert, the density and the pressure floor bind in at least five active cells each (isothermal:
    the density floor, there is no other);
  * the calm companions (no tiny cell) have CFL minima above 1e-9 in every direction, and the entropy floor their packs
    keep binds nowhere.
The census restates the ideal-gas wave speeds only: the isothermal cases (MHD PLM + HLLD, hydro PLM + Roe) rest on the
finiteness, floor and sign conditions alone.
Run with -s to see the census and the floor counts per case.
"""
import numpy as np
import pytest

import stage_cases as sc


def _unique(keyfn, cases):
    seen = {}
    for c in cases:
        seen.setdefault(keyfn(c), c)
    return list(seen.values())


STATES = _unique(lambda c: c.state_key(), sc.CASES)
REFERENCES = _unique(lambda c: c.oracle_key(), sc.CASES)


def _state_id(c):
    return "%s-%s-ng%d%s%s%s" % (c.fluid, c.shape, c.ng, "" if c.ideal else "-iso", "-%dscal" % c.nscal if c.nscal else "",
                                 "-calm" if c.calm else "" if c.tiny_exp == sc.TINY_EXP else "-tiny%d" % c.tiny_exp)


def _ref_id(c):
    return "%s-%s-%s-%s-%s-copy%d" % (_state_id(c), c.recon, c.rs, c.weights, "c2p" if c.entry != "update" else "update",
                                        c.copy)


@pytest.mark.parametrize("case", STATES, ids=_state_id)
def test_state_is_what_a_driver_holds(case):
    """w0 == ConsToPrim(u0) in every cell with no floor left to apply (converting again changes nothing and counts
    nothing, the tiny cell aside), bcc0 the face average, the named cells as described"""
    import ctypes as C
    from oracle import akref
    st = sc.case_state(case)
    pk, dx = sc.case_pack(case)
    g = sc.Geo(pk)
    assert all(np.isfinite(v).all() for v in st.values())
    u, w = st["u0"].copy(), np.zeros_like(st["w0"])
    cnt = np.zeros(3, dtype=np.int32)
    R, P = akref.lib(), akref.ptr
    if case.mhd:
        b = [st["b0" + q].copy() for q in sc.BNAMES]
        bcc = np.zeros_like(st["bcc0"])
        R.akref_mhd_c2p(C.byref(pk), P(u), *[P(x) for x in b], P(w), P(bcc), 0, g.N1 - 1, 0, g.N2 - 1, 0, g.N3 - 1, P(cnt))
        assert (b[0][:, :, :, ::3] == 0.0).mean() > 0.99                 # (the pair of identical cells may fill one)
    else:
        R.akref_hydro_c2p(C.byref(pk), P(u), P(w), 0, g.N1 - 1, 0, g.N2 - 1, 0, g.N3 - 1, P(cnt))
    # A second conversion finds the density floor applied everywhere but in the tiny cell, which it lifts, and returns the
    # density and the velocities the sweeps' u0 form derives from u0.  (The energy is left out: where the pressure floor
    # has bound, E - e_k - e_m of the stored E lands an ulp on either side of the floor, so a second pass is not the
    # identity there -- the stage reads w0[4] in every form.)
    nf = 4
    diff = np.argwhere((w[:, :nf] != st["w0"][:, :nf]).any(axis=1))
    if case.calm:
        assert len(diff) == 0 and cnt[0] == 0, (diff, cnt)
    else:
        assert len(diff) == 1 and cnt[0] == 1, (diff, cnt)
        m, k, j, i = diff[0]
        assert st["w0"][m, 0, k, j, i] == 2.0**case.tiny_exp*st["w0"][m, 0, k, j, i - 1]
        assert (k, j, i) == ((g.ks + 3 % g.nx[2]) if g.three_d else 0, (g.js + 3 % g.nx[1]) if g.multi_d else 0, g.is_ + 1)
    if case.mhd:
        assert np.array_equal(bcc, st["bcc0"])
    mom = st["u0"][:, 1:4]
    assert (np.signbit(mom) & (mom == 0.0)).sum() >= 3                                      # the -0.0 momenta


@pytest.mark.parametrize("case", [c for c in STATES if c.ideal], ids=_state_id)
def test_every_fan_selection_has_faces(case):
    census = sc.hlld_census(sc.case_pack(case), sc.case_state(case))
    names = sc.HLLD_SELECTIONS if case.mhd else sc.HLLC_REGIONS
    for q, n in enumerate(census):
        share = n/n.sum()
        print("%s x%d faces=%d %s" % (_state_id(case), q + 1, n.sum(),
                                      " ".join("%s: %d (%.1f%%)" % (s, a, 100*f) for s, a, f in zip(names, n, share))))
        assert (share >= 0.01).all(), (q, dict(zip(names, n)))


@pytest.mark.parametrize("case", REFERENCES, ids=_ref_id)
def test_reference_is_finite_and_reaches_the_floors(case):
    exp = sc.case_expected(case)
    for k, v in exp.items():
        if isinstance(v, np.ndarray):
            assert np.isfinite(v).all(), k
    signs = exp["mass_flux_signs"]
    assert all(p > 0 and n > 0 for p, n in signs), signs
    if case.mhd and case.shape == "3x12x10x9":
        # ... and of neither: an x1 face whose mass flux is exactly +-0.0, which the sign byte must file under `>= 0`
        assert exp["mass_flux_zeros"] >= 1
    if case.entry != "update":
        cnt = exp["counters"]
        print("%s floors: density %d pressure %d; mass-flux signs (+, -) %s; dt3 %s"
              % (_ref_id(case), cnt[0], cnt[1], signs, exp["dt3"]))
        assert cnt[0] >= 5, cnt
        assert cnt[1] >= 5 or not case.ideal, cnt
        assert (exp["dt3"] < sc.FLT_MAX).all()
        if case.calm:
            # The CFL minima of a calm case are ordinary numbers set by ordinary cells: a density at its floor of 1e-3
            # under momenta and fields of order 1e2 bounds every speed by ~1e6, far from an overflow.  (With the tiny cell
            # they are fixed by the few cells round it: 0 = dx/inf for MHD with HLLD or LLF, 1e-21 .. 1e-109 otherwise, so
            # those cases compare the scan's value in one cell only.)
            ndir = sc.Geo(sc.case_pack(case)[0]).dims
            assert (exp["dt3"][:ndir] > 1.0e-9).all(), exp["dt3"]
            # ... and the default entropy floor these packs keep binds in no cell: without it nothing changes
            nmb, nx = sc.SHAPES[case.shape]
            off = sc.make_pack(nmb, nx, case.ng, case.mhd, case.nscal, case.ideal, sfloor=0.0)
            exp0 = sc.oracle_stage(off, (case.recon, case.rs), sc.beta_dt_of(case.weights), case.copy, sc.case_state(case),
                                   True, 1)
            assert np.array_equal(exp0["w0"], exp["w0"]) and list(exp0["counters"]) == list(exp["counters"])
    # a stage changes the state: the comparison of the GPU file is not one of copies
    new = exp["u1"] if case.copy >= 2 else exp["u0"]
    assert not np.array_equal(new, sc.case_state(case)["u0"])


def test_case_table():
    ids = [c.id() for c in sc.CASES]
    assert len(set(ids)) == len(ids)
    assert 140 <= len(ids) <= 170, len(ids)
