"""ctypes binding of the C ABI in include/akmi.h (athenak_amd/lib/libakmi.so).

PyTorch is used here only as plumbing: device memory (tensor.data_ptr()) and HIP streams
(torch.cuda.current_stream().cuda_stream).  There is NO CPU fallback: if the HIP library is
missing or a call fails, an exception is raised.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# AKMI_LIB: developer override used by tools/kbench.py to A/B kernel variants
LIB_PATH = os.environ.get("AKMI_LIB") or os.path.join(_HERE, "lib", "libakmi.so")
# the one declaration of the C ABI: lib() types every entry from it
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "akmi.h")

RECON = {"dc": 0, "plm": 1, "ppm4": 2, "ppmx": 3, "wenoz": 4, "teno": 5}
RSOLVER = {"llf": 0, "hlle": 1, "hllc": 2, "hlld": 3, "roe": 4, "advect": 5}
BC = {"block": -1, "periodic": 0, "outflow": 1, "reflect": 2, "user": 3, "inflow": 4, "diode": 5,
      "vacuum": 6}

COMPLETE, INCOMPLETE, FAIL = 0, 1, -1


class Pack(C.Structure):
    """struct akmi_pack"""
    _fields_ = [("nmb", C.c_int), ("nvar", C.c_int), ("nx1", C.c_int), ("nx2", C.c_int),
                ("nx3", C.c_int), ("ng", C.c_int), ("dx", C.c_void_p),
                ("gamma", C.c_double), ("dfloor", C.c_double), ("pfloor", C.c_double),
                ("tfloor", C.c_double), ("sfloor", C.c_double), ("sigma_max", C.c_double),
                ("iso_cs", C.c_double), ("is_ideal", C.c_int)]


PHASE_SWEEPS, PHASE_EMF_CT, PHASE_C2P, PHASE_ALL = 1, 2, 4, 7     # AKMI_PHASE_* of include/akmi.h
SMALL_PACK_CELLS = 375000       # AKMI_SMALL_PACK_CELLS of include/akmi.h
# (tests/test_capi_symbols.py compares every constant mirrored here with the header)

AMR_METHOD = {"min_max": 0, "slope": 1, "second_deriv": 2}               # AKMI_AMR_* of include/akmi.h

FORM_X3_U0, FORM_X12_U0, FORM_LEAN_C2P, FORM_BCC_FACES = 1, 2, 4, 8      # AKMI_FORM_* of include/akmi.h
COPY_X3_U0, COPY_X12_U0, COPY_BCC_FACES = 0x100, 0x200, 0x400            # AKMI_COPY_*: or-ed into copy_u1 of a stage call
DROP_W03, DROP_BCC = 1, 2                                                # AKMI_DROP_* of the lean conversion

# AKMI_DV_* of include/akmi.h: `which` of akmi_derived_var
DERIVED = {"temperature": 0, "wz": 1, "w2": 2, "jz": 3, "j2": 4, "curv": 5, "k_jxb": 6, "curv_perp": 7, "bmag": 8,
           "divb": 9}

_LIB = None


class Smr(C.Structure):
    """struct akmi_smr (include/akmi.h)"""
    _fields_ = [("nnghbr", C.c_int), ("multilevel", C.c_int), ("nghbr", C.c_void_p),
                ("mblev", C.c_void_p), ("cc_tab", C.c_void_p), ("fc_tab", C.c_void_p),
                ("ndat", C.c_void_p), ("slot_ox", C.c_void_p), ("layout", C.c_void_p),
                ("soff", C.c_void_p), ("roff", C.c_void_p), ("direct_same", C.c_int), ("needs_coarse", C.c_void_p),
                ("lists", C.c_void_p), ("list_cnt", C.c_int*6)]


class RngState(C.Structure):
    """struct akmi_rng_state (RNG_State, src/utils/random.hpp:26-34): 296 bytes"""
    _fields_ = [("idum", C.c_longlong), ("idum2", C.c_longlong), ("iy", C.c_longlong),
                ("iv", C.c_longlong*32), ("iset", C.c_int), ("gset", C.c_double)]


class SrcTerms(C.Structure):
    """struct akmi_srcterms (include/akmi.h)"""
    _fields_ = [("const_accel", C.c_int), ("const_accel_dir", C.c_int), ("ism_cooling", C.c_int),
                ("reserved", C.c_int), ("const_accel_val", C.c_double), ("hrate", C.c_double),
                ("gamma", C.c_double), ("temp_unit", C.c_double), ("cooling_unit", C.c_double),
                ("heating_unit", C.c_double)]


class PdfAxis(C.Structure):
    """struct akmi_pdf_axis (include/akmi.h)"""
    _fields_ = [("array", C.c_void_p), ("nvar", C.c_int), ("comp", C.c_int), ("nbin", C.c_int), ("logscale", C.c_int),
                ("bin_lo", C.c_double), ("bin_hi", C.c_double), ("step", C.c_double)]


class CoarsenVar(C.Structure):
    """struct akmi_coarsen_var (include/akmi.h)"""
    _fields_ = [("array", C.c_void_p), ("nvar", C.c_int), ("comp", C.c_int)]


class MgPlan(C.Structure):
    """struct akmi_mg_plan (include/akmi.h)"""
    _fields_ = [("nmb", C.c_int), ("nxb", C.c_int), ("nrx1", C.c_int), ("nrx2", C.c_int), ("nrx3", C.c_int),
                ("nmblevel", C.c_int), ("nrootlevel", C.c_int), ("ng", C.c_int), ("nvar", C.c_int),
                ("npresmooth", C.c_int), ("npostsmooth", C.c_int), ("niter", C.c_int), ("full_multigrid", C.c_int),
                ("fmg_ncycle", C.c_int), ("subtract_average", C.c_int), ("show_defect", C.c_int),
                ("rdx", C.c_double), ("root_dx", C.c_double), ("omega", C.c_double), ("four_pi_G", C.c_double),
                ("eps", C.c_double), ("vol", C.c_double), ("nghbr", C.c_void_p), ("lloc", C.c_void_p),
                ("ws", C.c_void_p),
                ("mg_bc", C.c_int), ("periodic", C.c_int*6), ("mporder", C.c_int), ("nodipole", C.c_int),
                ("auto_mporigin", C.c_int), ("mesh_ext", C.c_double*6), ("mporigin", C.c_double*3),
                ("mask_radius", C.c_double), ("mask_origin", C.c_double*3), ("xlim", C.c_void_p)]


MG_NNORMS = 42                  # AKMI_MG_NNORMS of include/akmi.h
MGBC = {"none": 0, "zerofixed": 1, "zerograd": 2, "multipole": 3}        # AKMI_MGBC_* of include/akmi.h
MG_NMPCOEFF = 25                # coefficients of mporder = 4; the origin (x, y, z) follows them in the library's arrays

TURB_NHIST = 11                 # AKMI_TURB_NHIST of include/akmi.h
TURB_HIST_LABELS = ["Bx", "By", "Bz", "B^2", "B^4", "dB^2", "BdB^2", "|BxJ|^2", "|B.J|^2", "U^2", "dU"]   # turb.cpp:249-259


class AkmiError(RuntimeError):
    pass


_CTYPES = {"int": C.c_int, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "double": C.c_double}
_RESTYPES = dict(_CTYPES, **{"void": None, "void *": C.c_void_p, "const char *": C.c_char_p,
                             "const int *": C.POINTER(C.c_int)})
_FN_TYPEDEFS = ("akmi_comm_exchange_fn", "akmi_comm_allreduce_min_fn")
_from_address = C.c_void_p.from_param
_NULL, _TENSOR, _STRUCT, _ADDRESS, _REFUSED = range(5)
_KIND = {type(None): _NULL}     # type of an argument -> how Ptr passes it; _kind() files each new type once


def _kind(tp):
    k = (_STRUCT if issubclass(tp, C.Structure) else _TENSOR if hasattr(tp, "data_ptr")
         else _REFUSED if issubclass(tp, str) else _ADDRESS)
    _KIND[tp] = k
    return k


class Ptr(C.c_void_p):
    """argtype of every pointer parameter: None, a tensor (its data_ptr()), a Structure (by reference), or whatever
    c_void_p takes (an address, bytes, c_void_p, byref(...), ctypes arrays and pointers).  One dictionary look-up on the
    argument's type per argument: this runs for every pointer of every call."""

    @classmethod
    def from_param(cls, a, _get=_KIND.get, _byref=C.byref):
        k = _get(type(a))
        if k is None:
            k = _kind(type(a))
        if k == _TENSOR:
            return _from_address(a.data_ptr())
        if k == _ADDRESS:
            return _from_address(a)
        if k == _STRUCT:
            return _byref(a)
        if k == _NULL:
            return None
        raise TypeError("%r is not a pointer argument" % (a,))


def parse_header(text):
    """{name: (restype, argtypes)} of every function a header in the style of include/akmi.h declares"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M).replace('extern "C" {', "")
    text = re.sub(r"\{[^{}]*\}", "", text)          # struct and enum bodies
    sigs = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not re.search(r"\bakmi_[a-z0-9_]+ ?\(", stmt):
            continue
        m = re.fullmatch(r"([a-z *]+?) ?\b(akmi_[a-z0-9_]+) ?\(([^()]*)\)", stmt)
        ret = m and re.sub(r" ?\* ?", " *", m.group(1)).strip()
        if not m or ret not in _RESTYPES:
            raise AkmiError("include/akmi.h: cannot type the declaration `%s`" % stmt)
        argtypes = []
        for prm in (s.strip() for s in m.group(3).split(",")):
            if prm == "void" and "," not in m.group(3):
                break
            if "*" in prm or "[" in prm or prm.split()[0] in _FN_TYPEDEFS:
                argtypes.append(Ptr)
                continue
            words = [w for w in prm.split() if w != "const"]
            ctype = _CTYPES.get(" ".join(words)) or _CTYPES.get(" ".join(words[:-1]))     # unnamed or named
            if ctype is None:
                raise AkmiError("include/akmi.h: unknown type of parameter `%s` in the declaration of %s"
                                % (prm, m.group(2)))
            argtypes.append(ctype)
        sigs[m.group(2)] = (_RESTYPES[ret], tuple(argtypes))
    return sigs


SIGNATURES = {}      # name -> (restype, argtypes) of every entry include/akmi.h declares; filled by the first lib()


def signatures():
    """SIGNATURES, parsed from include/akmi.h on first use"""
    if not SIGNATURES:
        if not os.path.exists(HEADER_PATH):
            raise AkmiError("header %s not found: it declares the entries of %s" % (HEADER_PATH, LIB_PATH))
        with open(HEADER_PATH) as f:
            SIGNATURES.update(parse_header(f.read()))
    return SIGNATURES


class _StandIn:
    """What lib() returns for an object that was put into _LIB from outside (tests/cpu_backend.py stands CPU code in for
    the library): it does for that object what the typed entries do for libakmi.so.  The plain arguments of a call become
    the ctypes values the C function would receive -- byref(struct), c_void_p(address), c_double(x), c_longlong(n) --
    so a stand-in need not know how the host spells a call.  An int for a C int stays an int: ctypes passes it as one."""

    def __init__(self, target):
        self.target = target

    def __getattr__(self, name):
        fn = getattr(self.target, name)
        if name not in signatures():
            return fn
        argtypes = SIGNATURES[name][1]

        def convert(t, a):
            if t is Ptr:        # a tensor as a c_void_p instance: stand-ins written in Python read its .value
                return _p(a) if hasattr(a, "data_ptr") else Ptr.from_param(a)
            return a if isinstance(a, C._SimpleCData) or (t is C.c_int and type(a) is int) else t(a)

        def call(*args):
            if len(args) != len(argtypes):
                raise TypeError("%s takes %d arguments (%d given)" % (name, len(argtypes), len(args)))
            return fn(*map(convert, argtypes, args))
        return call


_LOADED = None       # the library lib() loaded and typed itself
_STANDIN = None      # the _StandIn around what _LIB holds otherwise


def lib():
    """Load libakmi.so (fails loudly when it has not been built) and type every entry from include/akmi.h."""
    global _LIB, _LOADED, _STANDIN
    if _LIB is not None and _LIB is not _LOADED:
        if _STANDIN is None or _STANDIN.target is not _LIB:
            _STANDIN = _StandIn(_LIB)
        return _STANDIN
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise AkmiError(
                "HIP library %s not found: run `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in signatures().items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _LIB = _LOADED = L
    return _LIB


def _p(t):
    """device pointer of a torch tensor (None -> NULL)"""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


DEVICE = "cuda"      # device of all field tensors; CPU-only unit tests of the host logic
                     # override it together with _LIB (see tests/cpu_backend.py)


def _stream():
    if DEVICE != "cuda":
        return None
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, what):
    if rc < 0:
        raise AkmiError("%s failed: %s" % (what, lib().akmi_last_error().decode()))
    return rc


def d(x):
    return C.c_double(float(x))
