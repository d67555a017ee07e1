"""TEST INFRASTRUCTURE shared by tests/test_amr_host.py (CPU) and tests/test_gpu_amr.py: the shapes of the kernel
tests, their planted data, and a CPU backend that stands the numpy restatement (tests/amr_restate.py) in for
akmi_amr_* so that the whole adaptive host runs without a GPU."""
import ctypes as C

import numpy as np

import amr_restate as ar

# (nx1, nx2, nx3, ng, nmb)
CHECK_SHAPES = [(4, 4, 1, 2, 5), (8, 8, 8, 2, 3), (12, 6, 4, 2, 3), (132, 1, 1, 2, 2), (130, 6, 4, 4, 2)]
# (nx1, nx2, nx3, ng)
REGRID_SHAPES = [(4, 4, 1, 2), (8, 8, 8, 2), (16, 8, 4, 4), (132, 1, 1, 2), (130, 10, 1, 2), (196, 6, 4, 2)]
SENTINEL = -7.25e300


def _arr(ptr, shape):
    v = ptr.value if hasattr(ptr, "value") else ptr
    n = int(np.prod(shape))
    return np.ctypeslib.as_array(C.cast(C.c_void_p(v), C.POINTER(C.c_double)), (n,)).reshape(shape)


def _iarr(ptr, shape):
    v = ptr.value if hasattr(ptr, "value") else ptr
    n = int(np.prod(shape))
    return np.ctypeslib.as_array(C.cast(C.c_void_p(v), C.POINTER(C.c_int)), (n,)).reshape(shape)


def _geom(byref_pack):
    p = byref_pack._obj
    return ar.Geom(p.nx1, p.nx2, p.nx3, p.ng), p.nmb


def install_cpu_backend():
    import cpu_backend
    from athenak_amd import capi
    methods = {v: k for k, v in ar.METHODS.items()}

    class Backend(cpu_backend.OracleAsAkmi):
        def akmi_amr_check(self, pack, method, q, mstride, vmin, vmax, flags, stream):
            G, nmb = _geom(pack)
            ms = int(getattr(mstride, "value", mstride))
            cells = int(np.prod(G.N))
            qa = _arr(q, (nmb, ms))[:, :cells].reshape((nmb,) + G.N)
            ar.check(G, methods[int(method)], qa, float(vmin.value), float(vmax.value), _iarr(flags, (nmb,)))
            return 0

        def akmi_amr_regrid_cc(self, po, pn, nvar, plan, uo, un, stream):
            G, nold = _geom(po)
            _, nnew = _geom(pn)
            ar.regrid_cc(G, _iarr(plan, (nnew, 3)), _arr(uo, (nold, nvar) + G.N), _arr(un, (nnew, nvar) + G.N))
            return 0

        def akmi_amr_regrid_fc(self, po, pn, plan, o1, o2, o3, n1, n2, n3, stream):
            G, nold = _geom(po)
            _, nnew = _geom(pn)
            bo = [_arr(p, (nold,) + G.face_shape(d)) for d, p in enumerate((o1, o2, o3))]
            bn = [_arr(p, (nnew,) + G.face_shape(d)) for d, p in enumerate((n1, n2, n3))]
            ar.regrid_fc(G, _iarr(plan, (nnew, 3)), bo, bn)
            return 0

        def akmi_amr_repair_fc(self, pack, repair, b1, b2, b3, stream):
            G, nmb = _geom(pack)
            b = [_arr(p, (nmb,) + G.face_shape(d)) for d, p in enumerate((b1, b2, b3))]
            ar.repair_fc(G, _iarr(repair, (nmb,)), b)
            return 0

    capi._LIB = Backend()
    capi.DEVICE = "cpu"


def uninstall_cpu_backend():
    import cpu_backend
    cpu_backend.uninstall()


def regrid_plan(G):
    """plans with every kind: a kept block that moves to a lower index, one that moves to a higher index, a derefined
    group, and a refined block whose nleaf children cover every octant -> (old_nmb, {"first": plan, "last": plan}),
    the refined block's children first resp. last in the new pack.
    first: old pack [P, c0 .. c_{nleaf-1}, K1, K2] -> new [P's children, K2 (lower), derefined, K1 (higher)];
    last:  old pack [K1, K2, c0 .. c_{nleaf-1}, P] -> new [K2 (lower), derefined, K1 (higher), P's children]."""
    nl = G.nleaf
    old_nmb = nl + 3
    first = [(1, 0, o) for o in range(nl)] + [(0, nl + 2, 0), (-1, 1, 0), (0, nl + 1, 0)]
    last = [(0, 1, 0), (-1, 2, 0), (0, 0, 0)] + [(1, nl + 2, o) for o in range(nl)]
    return old_nmb, {"first": np.array(first, dtype=np.int32), "last": np.array(last, dtype=np.int32)}


def random_state(G, nmb, nvar, seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.5, 1.5, size=(nmb, nvar) + G.N)
    b = [rng.uniform(-1.0, 1.0, size=(nmb,) + G.face_shape(d)) for d in range(3)]
    # non-dyadic cell sizes, one set per block
    dx = np.array([[0.1/(3 + m), 0.07/(1 + m), 0.013*(m + 1)] for m in range(nmb)])
    return u, b, dx


def planted_field(G, nmb, method, threshold, seed, equal_block=None):
    """q (nmb, N3, N2, N1) whose criterion value stays well below `threshold` everywhere except in the LAST active
    cell of block nmb-1 (the last lane of the last partial tile, at the block's upper corner, so that every
    ghost-side stencil arm is read), where it exceeds it; the ghost cells elsewhere hold values that would win the
    reduction if a masked or out-of-range lane were read.  equal_block: a block whose extremum is made EXACTLY the
    threshold (min_max only)."""
    rng = np.random.default_rng(seed)
    (ks, js, is_), (ke, je, ie) = G.s, G.e
    q = np.empty((nmb,) + G.N)
    if method == "min_max":
        q[...] = 1.0e6                                              # ghosts: would win a max
        q[:, ks:ke + 1, js:je + 1, is_:ie + 1] = rng.uniform(0.2, 0.8, size=(nmb,) + G.nx)*threshold
        q[nmb - 1, ke, je, ie] = 1.5*threshold
        if equal_block is not None:
            q[equal_block, ke, je, ie] = threshold
    else:
        # smooth and nearly flat everywhere, ghosts included (the stencil legitimately reads one ghost layer) ...
        q[...] = 1.0 + 1e-4*rng.uniform(size=q.shape)
        # ... cells further out than one layer are never read: make them loud
        big = np.full_like(q, 1.0e6)
        inner = tuple(slice(max(s - 1, 0), e + 2) if on else slice(0, 1) for s, e, on in zip(G.s, G.e, G.on))
        big[(slice(None),) + inner] = q[(slice(None),) + inner]
        q = big
        # the extremum lives in the ghost-side arms of the corner cell
        q[nmb - 1, ke, je, ie + 1] = 1.0 + 40.0*threshold
        if G.on[1]:
            q[nmb - 1, ke, je + 1, ie] = 1.0 - 0.9
        if G.on[0]:
            q[nmb - 1, ke + 1, je, ie] = 1.0 + 3.0
    return q


def varied_field(G, nmb, seed):
    """q (nmb, N3, N2, N1) for the exact-threshold tests: random in (0.5, 1.5) over the active cells and the one ghost
    layer the stencils read, 1e6 beyond it (never read).  Block 0 carries its slope / second-derivative extremum in
    the LOWEST active cell through the low-side ghost arms (is-1, js-1, ks-1), the last block in the HIGHEST active
    cell -- the last lane of the last partial tile -- through the high-side ghost arms; in the blocks between, the
    extremum falls where the random numbers put it.  Since the tests pin the reduced value to the bit, every arm,
    factor and operation of every cell that could hold the extremum is checked, not only the planted ones."""
    rng = np.random.default_rng(seed)
    (ks, js, is_), (ke, je, ie) = G.s, G.e
    q = np.full((nmb,) + G.N, 1.0e6)
    inner = tuple(slice(s - 1, e + 2) if on else slice(0, 1) for s, e, on in zip(G.s, G.e, G.on))
    q[(slice(None),) + inner] = rng.uniform(0.5, 1.5, size=q[(slice(None),) + inner].shape)
    q[0, ks, js, is_ - 1] = 8.0 + rng.uniform()
    q[nmb - 1, ke, je, ie + 1] = 8.0 + rng.uniform()
    if G.on[1]:
        q[0, ks, js - 1, is_] = 6.0 + rng.uniform()
        q[nmb - 1, ke, je + 1, ie] = 6.0 + rng.uniform()
    if G.on[0]:
        q[0, ks - 1, js, is_] = 5.0 + rng.uniform()
        q[nmb - 1, ke + 1, je, ie] = 5.0 + rng.uniform()
    return q


def conservation_defect(G, plan, u_old, u_new):
    """per variable (|sum after - sum before|, bound) of u*volume over the active cells of a regrid with one of the
    plans of regrid_plan; sums exact (math.fsum).  Volumes in units of a fine cell: an old block that is refined and a
    new block that was merged are coarse (nleaf), all others fine.  Bound: 8 ulp of the largest |u| times the coarse
    cell volume, per coarse cell of the refined and of the merged block (derived in
    tests/test_amr_host.py::test_conservation_across_one_regrid)."""
    import math
    nl = G.nleaf
    plan = np.asarray(plan)
    (ks, js, is_), (ke, je, ie) = G.s, G.e
    act = (slice(ks, ke + 1), slice(js, je + 1), slice(is_, ie + 1))
    vol_old = np.ones(u_old.shape[0])
    vol_old[plan[plan[:, 0] == 1][:, 1]] = nl
    vol_new = np.where(plan[:, 0] == -1, float(nl), 1.0)
    ncoarse = 2*G.nx[0]*G.nx[1]*G.nx[2]
    out = []
    for v in range(u_old.shape[1]):
        before = math.fsum(float(x)*vol_old[m] for m in range(u_old.shape[0]) for x in u_old[m, v][act].ravel())
        after = math.fsum(float(x)*vol_new[m] for m in range(len(plan)) for x in u_new[m, v][act].ravel())
        out.append((abs(after - before), 8*np.spacing(float(np.abs(u_old[:, v]).max()))*nl*ncoarse))
    return out
