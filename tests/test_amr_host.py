"""not gpu: the host side of adaptive mesh refinement (athenak_amd/mesh_refinement.py, mesh_tree.py, mesh.py) --
the tree against an independent construction on sets of leaves, the flag rules, the refusals, the frozen mesh against
its static twin, the reference's own 2-D AMR linear-wave acceptance test, and conservation across one regrid.  The
device entry points are stood in by the numpy restatement (tests/amr_cases.install_cpu_backend)."""
import itertools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import amr_cases as ac  # noqa: E402
import amr_restate as ar  # noqa: E402
import amr_runs  # noqa: E402
from athenak_amd.mesh_tree import BuildTreeFromScratch  # noqa: E402
from athenak_amd.parameter_input import ParameterInput  # noqa: E402


# ---- an independent construction: leaves as a set of (lx1, lx2, lx3, level), no tree ------------------------------
class Leaves:
    def __init__(self, leaves, nroot, root_level, periodic, ndim):
        self.L = list(leaves)                                  # gid order
        self.nroot, self.root_level, self.per, self.ndim = nroot, root_level, periodic, ndim
        self.nleaf = 1 << ndim
        self.nref = self.nder = 0

    def _n(self, d, level):
        return self.nroot[d] << (level - self.root_level)

    def children(self, l):
        return [(2*l[0] + (n & 1), 2*l[1] + ((n >> 1) & 1 if self.ndim > 1 else 0),
                 2*l[2] + ((n >> 2) & 1 if self.ndim > 2 else 0), l[3] + 1) for n in range(self.nleaf)]

    def parent(self, l):
        return (l[0] >> 1, l[1] >> 1, l[2] >> 1, l[3] - 1)

    def covering(self, S, l):
        """the member of S that is l or an ancestor of l (None: l is covered by finer leaves)"""
        while l[3] >= 0:
            if l in S:
                return l
            l = self.parent(l)
        return None

    def neighbours(self, l):
        """locations at l's level that touch l (faces, edges, corners), through periodic boundaries"""
        out = []
        rng = [(-1, 0, 1) if d < self.ndim else (0,) for d in range(3)]
        for o in itertools.product(*rng):
            if o == (0, 0, 0):
                continue
            n, ok = [], True
            for d in range(3):
                x, N = l[d] + o[d], self._n(d, l[3])
                if x < 0 or x >= N:
                    if not self.per[d]:
                        ok = False
                        break
                    x %= N
                n.append(x)
            if ok:
                out.append((tuple(n) + (l[3],), o))
        return out

    def refine(self, S, l):
        if l not in S:
            return
        S.remove(l)
        S.update(self.children(l))
        self.nref += 1
        for n, _ in self.neighbours(l):                        # 2:1: the touching locations exist at l's level
            while True:
                c = self.covering(S, n)
                if c is None or c[3] >= n[3]:
                    break
                self.refine(S, c)

    def derefine(self, S, p):
        kids = self.children(p)
        if not all(k in S for k in kids):
            return
        # vetoed when a leaf two or more levels below p sits in that child of a touching location which touches p
        for n, o in self.neighbours(p):
            for m in S:
                sh = m[3] - p[3]
                if sh >= 2 and (m[0] >> sh, m[1] >> sh, m[2] >> sh) == n[:3] and touch_child(m, o, sh):
                    return
        for k in kids:
            S.remove(k)
        S.add(p)
        self.nder += 1

    def morton(self, l, maxlev):
        sh = maxlev - l[3]
        key = 0
        for b in range(24):
            key |= (((l[0] << sh) >> b) & 1) << (3*b) | (((l[1] << sh) >> b) & 1) << (3*b + 1) \
                | (((l[2] << sh) >> b) & 1) << (3*b + 2)
        return key

    def update(self, flags):
        """flags per gid -> (new leaves, newtoold, oldtonew, nnew, ndel), by the rules of UpdateMeshBlockTree"""
        old = list(self.L)
        S = set(old)
        self.nref = self.nder = 0
        ref = [old[g] for g in range(len(old)) if flags[g] == 1]
        der = [old[g] for g in range(len(old)) if flags[g] == -1]
        if not ref and len(der) < self.nleaf:
            return self._result(old, set(old), 0, 0)
        groups = []
        if len(der) >= self.nleaf:
            ds = set(der)
            for l in der:                                      # gid order of the even-indexed sibling
                if (l[0] & 1) or (l[1] & 1) or (l[2] & 1):
                    continue
                if all(k in ds for k in self.children(self.parent(l))):
                    groups.append(self.parent(l))
        if len(groups) > 1:                                    # the reference sorts all but the last by level
            groups = sorted(groups[:-1], key=lambda l: -l[3]) + groups[-1:]
        for l in ref:
            self.refine(S, l)
        for p in groups:
            self.derefine(S, p)
        return self._result(old, S, (self.nleaf - 1)*self.nref, (self.nleaf - 1)*self.nder)

    def _result(self, old, S, nnew, ndel):
        """(new leaves, newtoold, oldtonew, nnew, ndel, what happened to every old block, regrid plan), all from the
        two sets of leaves"""
        maxlev = max(l[3] for l in S)
        new = sorted(S, key=lambda l: self.morton(l, maxlev))
        oldset = set(old)
        gid_old = {l: g for g, l in enumerate(old)}
        gid_new = {l: g for g, l in enumerate(new)}
        n2o, plan = [], []
        for l in new:
            c = self.covering(oldset, l)
            if c == l:                                         # kept
                n2o.append(gid_old[l])
                plan.append([0, gid_old[l], 0])
            elif c is not None:                                # a child of an old leaf: one level, never more
                assert c == self.parent(l), (c, l)
                n2o.append(gid_old[c])
                plan.append([1, gid_old[c], (l[0] & 1) + 2*(l[1] & 1) + 4*(l[2] & 1)])
            else:                                              # merged from its children, all old leaves
                kids = self.children(l)
                assert all(k in oldset for k in kids)
                assert [gid_old[k] for k in kids] == list(range(gid_old[kids[0]], gid_old[kids[0]] + self.nleaf))
                n2o.append(gid_old[kids[0]])
                plan.append([-1, gid_old[kids[0]], 0])
        o2n, what = [], []
        for l in old:
            c = self.covering(S, l)
            if c is not None:
                o2n.append(gid_new[c])                         # kept, or merged into its parent
                what.append(0 if c == l else -self.nleaf)
            else:
                d = l
                while d not in S:                              # refined: its first descendant leaf
                    d = self.children(d)[0]
                o2n.append(gid_new[d])
                what.append(1)
        self.L = new
        return new, n2o, o2n, nnew, ndel, what, plan


def touch_child(m, o, sh):
    """m, sh >= 2 levels below a location that touches a block p across offset o, lies in the child of that location
    which touches p: along every offset direction, m's ancestor one level below the location sits at the near end"""
    for d in range(3):
        if o[d] == 0:
            continue
        bit = ((m[d] >> (sh - 1)) & 1)
        if bit != (1 if o[d] < 0 else 0):
            return False
    return True


def _deck(nx, mb, per, num_levels, region=None):
    names = ("ix1_bc", "ox1_bc", "ix2_bc", "ox2_bc", "ix3_bc", "ox3_bc")
    t = "<mesh>\nnghost = 2\n"
    for d in range(3):
        t += "nx%d = %d\nx%dmin = 0.0\nx%dmax = 1.0\n" % (d + 1, nx[d], d + 1, d + 1)
    for n in names:
        t += "%s = %s\n" % (n, "periodic" if per else "outflow")
    t += "<meshblock>\n" + "".join("nx%d = %d\n" % (d + 1, mb[d]) for d in range(3))
    t += "<mesh_refinement>\nrefinement = adaptive\nnum_levels = %d\nmax_nmb_per_rank = 100000\n" % num_levels
    if region:
        t += region
    return ParameterInput(text=t)


class HostTree:
    """the product's tree driven through MeshRefinement.UpdateMeshBlockTree / the list building of a regrid"""

    def __init__(self, pin):
        from athenak_amd import mesh_refinement as mr
        self.mr = mr
        self.tree, self.lloc, self.root_level, self.max_level = BuildTreeFromScratch(pin)
        nx = [pin.GetInteger("mesh", "nx%d" % q) for q in (1, 2, 3)]
        self.ndim = 3 if nx[2] > 1 else (2 if nx[1] > 1 else 1)

    def update(self, flags):
        me = self

        class PM:
            ptree, lloc_eachmb, nmb_total = me.tree, me.lloc, len(me.lloc)
            three_d, multi_d = me.ndim == 3, me.ndim >= 2
        m = self.mr.MeshRefinement.__new__(self.mr.MeshRefinement)
        m.pmy_mesh, m.nleaf = PM, 1 << self.ndim
        m.refine_flag = np.array(flags, dtype=np.int32)
        nnew, ndel = m.UpdateMeshBlockTree()
        # the lists of RedistAndRefineMeshBlocks, by the product's own functions
        n2o = []
        new = self.tree.CreateZOrderedLLList(n2o)
        o2n = self.mr.old_to_new(n2o, len(self.lloc), 1 << self.ndim)
        what = self.mr.level_change_flags(self.lloc, new, o2n, 1 << self.ndim)
        plan = self.mr.regrid_plan(n2o, what, new)
        self.lloc = new
        return [tuple(l) for l in new], n2o, o2n, nnew, ndel, what.tolist(), plan.tolist()


CONFIGS = [((8, 1, 1), (2, 1, 1), True, 3), ((8, 1, 1), (2, 1, 1), False, 3), ((16, 8, 1), (4, 4, 1), True, 3),
           ((12, 8, 1), (4, 4, 1), False, 3), ((8, 8, 8), (4, 4, 4), True, 3), ((8, 4, 4), (4, 4, 4), False, 3)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "%dx%dx%d-%s" % (c[0] + ("per" if c[2] else "open",)))
def test_tree_updates_match_an_independent_construction(cfg):
    nx, mb, per, nlev = cfg
    pin = _deck(nx, mb, per, nlev)
    host = HostTree(pin)
    nroot = [nx[d]//mb[d] for d in range(3)]
    ind = Leaves([tuple(l) for l in host.lloc], nroot, host.root_level, [per]*3, host.ndim)
    rng = np.random.default_rng(hash(cfg) % (2**32))
    dragged = vetoed = merged = three = False
    kinds = set()
    for rnd in range(14):
        old = list(ind.L)
        flags = []
        for l in old:
            r = rng.uniform()
            f = 1 if (r < 0.18 and l[3] < host.max_level) else (-1 if (r > 0.45 and l[3] > host.root_level) else 0)
            flags.append(f)
        if rnd < 2:                                # two sure refinements, the second of a block the first made
            flags = [0]*len(old)
            flags[max(range(len(old)), key=lambda g: (old[g][3], g == len(old)//2))] = 1
        got = host.update(flags)
        want = ind.update(flags)
        assert got[0] == want[0], (rnd, flags)
        assert got[1] == want[1] and got[2] == want[2], (rnd, "newtoold / oldtonew")
        assert got[3] == want[3] and got[4] == want[4], (rnd, got[3:5], want[3:5])
        assert got[5] == want[5], (rnd, "flags reset from the level changes")
        assert got[6] == want[6], (rnd, "regrid plan")
        kinds |= {r[0] for r in got[6]}
        assert len(got[0]) == len(old) + got[3] - got[4]
        nflag = sum(1 for f in flags if f == 1)
        dragged |= got[3] > (ind.nleaf - 1)*nflag
        # a fully flagged sibling group that is still there afterwards was vetoed
        oldset, newset, fl = set(old), set(got[0]), dict(zip(old, flags))
        for l in old:
            if fl[l] == -1 and not ((l[0] | l[1] | l[2]) & 1):
                sib = ind.children(ind.parent(l))
                if all(fl.get(s) == -1 for s in sib):
                    vetoed |= all(s in newset for s in sib) and sum(1 for f in flags if f == -1) >= ind.nleaf
                    merged |= ind.parent(l) in newset
        three |= max(l[3] for l in got[0]) == host.root_level + 2     # the third level is reached
    assert dragged and merged and three and kinds == {-1, 0, 1}, (dragged, merged, three, kinds)


def test_a_derefinement_is_vetoed_by_a_refined_neighbour():
    nx, mb = (16, 16, 1), (4, 4, 1)
    host = HostTree(_deck(nx, mb, True, 3))
    ind = Leaves([tuple(l) for l in host.lloc], [4, 4, 1], host.root_level, [True]*3, 2)

    def both(flagged, value):
        flags = [value if tuple(l) in flagged else 0 for l in ind.L]
        got, want = host.update(flags), ind.update(flags)
        assert list(got) == list(want), (got, want)
        return got
    r = host.root_level
    P, N = (1, 1, 0, r), (2, 1, 0, r)
    both({P}, 1)
    both({N}, 1)
    both({(4, 2, 0, r + 1)}, 1)                       # N's child that touches P, refined: leaves two levels below P
    kids = set(ind.children(P))
    before = list(ind.L)
    out = both(kids, -1)
    assert out[0] == before and out[3] == 0 and out[4] == 0          # refused, silently
    both(set(ind.children((4, 2, 0, r + 1))), -1)                    # merge the grandchildren first ...
    out = both(kids, -1)
    assert out[4] == 3 and P in out[0]                               # ... and P's children may go


def test_too_few_flagged_siblings_do_nothing_and_refine_then_derefine_restores_the_leaves():
    pin = _deck((16, 16, 1), (4, 4, 1), True, 3)
    host = HostTree(pin)
    start = [tuple(l) for l in host.lloc]
    flags = [0]*len(start)
    flags[5] = 1
    new, n2o, o2n, nnew, ndel = host.update(flags)[:5]
    assert nnew == 3 and ndel == 0 and len(new) == len(start) + 3
    kids = [g for g, o in enumerate(n2o) if o == 5]
    assert len(kids) == 4 and o2n[5] == kids[0]
    # nleaf-1 flagged siblings: nothing happens, not even with other blocks flagged -1 to reach the count
    flags = [0]*len(new)
    for g in kids[:3]:
        flags[g] = -1
    flags[0] = -1                                  # a root block: four flags in all, no complete group
    again = host.update(flags)
    assert again[0] == new and again[3] == 0 and again[4] == 0
    flags = [0]*len(new)
    for g in kids:
        flags[g] = -1
    back = host.update(flags)
    assert back[0] == start and back[3] == 0 and back[4] == 3
    assert back[1] == [g if g < kids[0] else (g + 3 if g > kids[0] else kids[0]) for g in range(len(start))]


# ---- flag rules, refusals -------------------------------------------------------------------------------------------
@pytest.fixture
def cpu():
    ac.install_cpu_backend()
    yield
    ac.uninstall_cpu_backend()


def _blast(extra="", ov=(), blk="mhd"):
    pin = ParameterInput(text=amr_runs._text("blast_%s_amr.athinput" % blk, extra))
    pin.ModifyFromCmdline(["mesh/nx1=32", "mesh/nx2=32", "meshblock/nx1=8", "meshblock/nx2=8"] + list(ov))
    return pin


def test_flag_rules(cpu):
    from athenak_amd.main import Simulation
    # two criteria in the deck's order: the second (value_max far above the data) asks every block to derefine but
    # may not lower a +1 of the first; blocks on the root level lose their -1, blocks at max_level their +1
    extra = "<amr_criterion1>\nmethod = min_max\nvariable = mhd_u_d\nvalue_max = 1.0e30\n" + amr_runs._region(1, -0.45, -0.3, 2)
    sim = Simulation(_blast(extra, ["mesh_refinement/refinement_interval=1000"]))
    pm, pmr = sim.pmesh, sim.pmesh.pmr
    assert pm.adaptive and pm.multilevel and pm.max_level == pm.root_level + 1
    assert sim.Execute(max_cycles=2) == 2 and pmr.nmb_created == 0      # the density is uniform until the blast moves
    pmr.refinement_interval = 0
    pmr.ncyc_since_ref[:] = 0
    pm.ncycle = 0
    pmr.CheckForRefinement(pm.pmb_pack)
    lev = np.array([l.level for l in pm.lloc_eachmb])
    rf = pmr.refine_flag
    assert (rf[lev == pm.root_level] >= 0).all() and (rf[lev == pm.max_level] <= 0).all()
    assert (rf == 1).any() and (rf[lev == pm.max_level] == -1).all()
    assert (pmr.ncyc_since_ref == 1).all()
    # equality leaves the flag alone: a uniform density equal to value_max
    ph = pm.pmb_pack.pmhd
    ph.u0[:, 0] = 0.75
    ph.w0[:, 0] = 0.75
    pmr.rcrit = [pmr.rcrit[1]]
    pmr.rcrit[0].value_max = 0.75
    pmr.CheckForRefinement(pm.pmb_pack)
    assert (pmr.refine_flag == 0).all()
    pmr.rcrit[0].value_max = 0.5                               # above: refine wherever the level allows
    pmr.CheckForRefinement(pm.pmb_pack)
    assert (pmr.refine_flag[lev == pm.root_level] == 1).all() and (pmr.refine_flag[lev == pm.max_level] == 0).all()
    # refinement_interval: blocks younger than it are left alone; ncycle_check: no check on other cycles, but the
    # age still advances
    pmr.refinement_interval = 10
    pmr.CheckForRefinement(pm.pmb_pack)
    assert (pmr.refine_flag == 0).all() and (pmr.ncyc_since_ref == 4).all()
    pmr.refinement_interval, pmr.ncyc_check_amr, pm.ncycle = 0, 3, 4
    pmr.CheckForRefinement(pm.pmb_pack)
    assert (pmr.refine_flag == 0).all() and (pmr.ncyc_since_ref == 5).all()
    pm.ncycle = 6
    pmr.CheckForRefinement(pm.pmb_pack)
    assert (pmr.refine_flag == 1).any()


def test_location_criterion_and_defaults(cpu):
    from athenak_amd.main import Simulation
    pin = _blast()
    d = pin.blocks["amr_criterion0"]
    d.pop("variable"), d.pop("value_max")
    d.update(method="location", location_x1="0.375", location_x2="0.26", location_rad="0.05")
    sim = Simulation(pin)
    pmr = sim.pmesh.pmr
    assert pmr.ncyc_check_amr == 1 and pmr.refinement_interval == 3
    pmr.refinement_interval = 0
    pmr.CheckForRefinement(sim.pmesh.pmb_pack)
    got = {tuple(sim.pmesh.lloc_eachmb[g])[:2] for g in np.where(pmr.refine_flag == 1)[0]}
    # x1: 0.375 +- 0.05 lies inside the block [0.25, 0.5] alone; x2: 0.26 +- 0.05 holds the edge 0.25 of two blocks
    assert got == {(3, 2), (3, 3)}, got


REFUSALS = [
    ("max_nmb_below_root_grid", "", ["mesh_refinement/max_nmb_per_rank=0"], "Root grid requires more MeshBlocks"),
    ("no_criterion", "", None, "No <amr_criterion> blocks"),
    ("user_method", "", ["amr_criterion0/method=user"], "min_max, slope, second_deriv, location"),
    ("unknown_variable", "", ["amr_criterion0/variable=rad_coord_e"], "hydro_u_d, hydro_w_d, mhd_u_d, mhd_w_d"),
    ("wrong_fluid", "", ["amr_criterion0/variable=hydro_w_d"], "<hydro> not defined"),
    ("region_too_deep", amr_runs._region(2, -0.1, 0.1, 2), [], "level exceeds maximum allowed"),
    ("rst_output", "<output3>\nfile_type = rst\ndt = 0.1\n", [], "file_type = rst"),
    ("turb_driving", "<turb_driving>\ntype = hydro\n", [], "<turb_driving> is not available on refined meshes"),
]


@pytest.mark.parametrize("what,extra,ov,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_are_loud_and_at_construction(cpu, what, extra, ov, msg):
    from athenak_amd.main import Simulation
    pin = _blast(extra, ov or [])
    if what == "no_criterion":
        del pin.blocks["amr_criterion0"]
    with pytest.raises(RuntimeError, match=msg.replace("<", ".").replace(">", ".")):
        Simulation(pin, initialize=False)


def test_more_refusals(cpu):
    from athenak_amd.main import Simulation
    from athenak_amd.mesh import Mesh
    pin = _blast()
    del pin.blocks["mesh_refinement"]["max_nmb_per_rank"]
    with pytest.raises(RuntimeError, match="max_nmb_per_rank"):
        Simulation(pin, initialize=False)
    with pytest.raises(RuntimeError, match="one rank"):
        Mesh(_blast(), my_rank=0, nranks=2)
    # a regrid that would exceed max_nmb_per_rank
    sim = Simulation(_blast("", ["mesh_refinement/max_nmb_per_rank=20"]))
    with pytest.raises(RuntimeError, match="exceeds .mesh_refinement./max_nmb_per_rank = 20"):
        sim.Execute(max_cycles=3)
    # --host native: refused by the Python side before the C++ host sees the deck
    from athenak_amd.native import NativeSimulation
    with pytest.raises(RuntimeError, match="adaptive runs on the Python host only"):
        NativeSimulation(_blast(), initialize=False)
    # -r of an adaptive deck
    with pytest.raises(RuntimeError, match="-r of a deck"):
        Simulation(_blast(), initialize=False, restart=({}, None))


# ---- frozen mesh ---------------------------------------------------------------------------------------------------
def test_frozen_adaptive_mesh_is_its_static_twin_bit_for_bit():
    a = amr_runs.run("frozen_adaptive", "cpu")
    s = amr_runs.run("frozen_static", "cpu")
    assert a["created"] == 0 and a["deleted"] == 0
    assert a["leaves"] == s["leaves"] and len({l[3] for l in a["leaves"][0]}) == 2
    assert a["dt"] == s["dt"] and a["time"] == s["time"]
    assert set(a["arrays"]) == {"mhd_u0", "b0_x1f", "b0_x2f", "b0_x3f"}
    for k in s["arrays"]:
        assert np.array_equal(a["arrays"][k], s["arrays"][k]), k


def test_whole_runs_refine_and_derefine_on_the_cpu_backend():
    for case in sorted(amr_runs.WHOLE_RUNS):
        r = amr_runs.run(case, "cpu")
        assert r["created"] > 0 and r["deleted"] > 0, case
        assert all(np.isfinite(a).all() for a in r["arrays"].values())


def test_hst_tab_and_bin_outputs_follow_the_block_count_across_a_regrid(tmp_path):
    res = amr_runs.outputs_across_regrid(str(tmp_path), "cpu")
    assert res["nmb_files"][0] == res["nmb_before"] and res["nmb_files"][-1] == res["nmb_after"] != res["nmb_before"]
    rows = res["tab_rows"]
    assert len(rows) == len(res["nmb_files"]) and all(r % res["nx1"] == 0 for r in rows) and rows[-1] > rows[0], rows
    assert np.max(np.abs(np.diff(res["hst_mass"]))) <= res["mass_bound"]


def test_the_references_readers_accept_the_files_either_side_of_a_regrid(tmp_path):
    """tests/golden/amr_reference_readers.npz holds what the reference's bin_convert.read_binary and athena_read.hst
    returned for these files (tests/golden/make_amr_fixtures.py); the files are regenerated here and shown to be the
    very bytes that were read, then the record is held against the run"""
    import hashlib
    rec = np.load(os.path.join(ROOT, "tests", "golden", "amr_reference_readers.npz"), allow_pickle=False)
    res = amr_runs.outputs_across_regrid(str(tmp_path), "cpu")
    sha = lambda rel: hashlib.sha256(open(os.path.join(str(tmp_path), rel), "rb").read()).hexdigest()
    assert sha(res["bin_files"][0]) == str(rec["sha256/bin_before"]) and res["bin_files"][0] == str(rec["name/bin_before"])
    assert sha(res["bin_files"][-1]) == str(rec["sha256/bin_after"]) and res["bin_files"][-1] == str(rec["name/bin_after"])
    assert sha(res["hst_file"]) == str(rec["sha256/hst"])
    assert int(rec["bin_before/n_mbs"]) == res["nmb_before"] and int(rec["bin_after/n_mbs"]) == res["nmb_after"]
    assert rec["bin_before/mb_logical"].shape[0] == res["nmb_before"]
    assert rec["bin_after/mb_logical"].shape[0] == res["nmb_after"]
    assert len(set(rec["bin_after/mb_logical"][:, 3].tolist())) == 3          # three levels in the file
    assert [str(v) for v in rec["bin_after/var_names"]][:1] == ["dens"]
    # the reader drops a line whose time does not advance (the final output repeats the time of the last cycle's)
    t, mass = res["hst_time"], res["hst_mass"]
    keep = [n for n in range(len(t)) if n == len(t) - 1 or t[n] < t[n + 1:].min()]
    assert np.array_equal(rec["hst/time"], t[keep]) and np.array_equal(rec["hst/mass"], mass[keep])
    assert len(keep) >= 5 and list(rec["hst/keys"][:3]) == ["time", "dt", "mass"] and "3-ME" in rec["hst/keys"]


# ---- the reference's acceptance test ----------------------------------------------------------------------------------
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "known_answers_amr.json")))


@pytest.mark.parametrize("blk", ["hydro", "mhd"])
def test_reference_lwave2d_amr_acceptance(blk, cpu):
    """tst/test_suite/nr/test_nr_lwave2d_amr_mpicpu.py: rk2 + plm, wave 0, amp = 1e-3, cfl = 0.4, tlim = 1, at 64x32 with
    4x4 blocks and 128x64 with 8x8 blocks; L1-RMS error at 128 and the error ratio within the reference's bounds.
    Measured here: hydro 1.1913e-05 / 0.2845, mhd 1.2945e-05 / 0.2718."""
    from athenak_amd.main import Simulation, load_deck
    k = KNOWN["lwave2d_amr_abs"]["%s_rk2_plm_0" % blk]
    ratio = json.load(open(os.path.join(ROOT, "tests", "golden", "known_answers.json")))["lwave2d_amr_ratio"]
    errs = {}
    for n in (64, 128):
        ov = ["mesh/nx1=%d" % n, "mesh/nx2=%d" % (n//2), "mesh/nx3=1", "meshblock/nx1=%d" % (n//16),
              "meshblock/nx2=%d" % (n//16), "meshblock/nx3=1", "time/tlim=1.0", "time/cfl_number=0.4",
              "time/integrator=rk2", "mesh/nghost=2", "%s/reconstruct=plm" % blk,
              "%s/rsolver=%s" % (blk, k["rsolver"]), "problem/amp=1.0e-3", "problem/wave_flag=0"]
        sim = Simulation(load_deck("linear_wave_%s_amr.athinput" % blk, ov))
        sim.Execute()
        errs[n] = float(sim.pmesh.pgen.pgen_final_func()[0])        # the RMS-L1 error Finalize writes to -errs.dat
        assert sim.pmesh.pmr.nmb_created > 0
    print("lwave2d_amr", blk, errs, errs[128]/errs[64])
    assert errs[128] <= k["max_error"], errs
    rk = [v for kk, v in _flat(ratio) if blk in kk]
    assert rk, ratio
    assert errs[128]/errs[64] <= rk[0], (errs, rk)


def _flat(d, pre=""):
    if isinstance(d, dict):
        for k, v in d.items():
            yield from _flat(v, pre + "/" + str(k))
    elif isinstance(d, (int, float)):
        yield pre, float(d)
    elif isinstance(d, (list, tuple)):
        for n, v in enumerate(d):
            yield from _flat(v, pre + "/" + str(n))


# ---- conservation across one regrid --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 8, 1, 2), (8, 8, 8, 2), (12, 1, 1, 2)], ids=lambda s: "x".join(map(str, s)))
def test_conservation_across_one_regrid(shape):
    """Sum of u*volume over the blocks a regrid touches, before and after, for a plan with all three kinds.

    Bound: 8 ulp of the largest term per coarse cell.  Derivation, per coarse cell of volume V holding nleaf = 2^d fine
    cells of volume V/2^d (the factor is a power of two, so the volumes are exact):
      * restriction: the new value is (1/2^d)*fl(sum of 2^d fine values); the sum of at most 8 terms of magnitude <= M is
        formed with 7 roundings, each at most half an ulp of the running sum (<= 8M): the restricted value times V
        differs from the sum of fine value times V/2^d by at most 7 * ulp(8M)/2 * V/8 < 4 ulp(M) V.
      * prolongation: the children are q -+ d1 -+ d2 -+ d3; in exact arithmetic the 2^d values sum to 2^d q because every
        slope enters as often with + as with -.  Each child is formed with d <= 3 roundings of half an ulp of a number
        of magnitude <= 2M (the limited slopes are at most an eighth of a difference of two values), so the sum of the
        children times V/2^d differs from q V by at most 3 * ulp(2M)/2 * V = 3 ulp(M) V.
    Either way less than 8 ulp(M) V per coarse cell, M the largest |u| and V the coarse cell volume (here nleaf, in units
    of a fine cell).  The sums themselves are exact (math.fsum), so the bound is about the regrid alone.

    Here the regrid is the numpy restatement's (tests/amr_restate.py), which is what the CPU backend runs; the same sums
    over the output of the HIP kernels are asserted in tests/test_gpu_amr.py (test_regrid_kernels_...), which also holds
    the kernels to the restatement bit for bit."""
    nx1, nx2, nx3, ng = shape
    G = ar.Geom(nx1, nx2, nx3, ng)
    old_nmb, plans = ac.regrid_plan(G)
    for order in ("first", "last"):
        plan = plans[order]
        u, _, _ = ac.random_state(G, old_nmb, 3, 21)
        new = ar.regrid_cc(G, plan, u, np.zeros((len(plan), 3) + G.N))
        for defect, bound in ac.conservation_defect(G, plan, u, new):
            assert defect <= bound, (order, defect, bound)
