"""not gpu: the C-ABI library loads and exports every symbol include/akmi.h declares, and athenak_amd/capi.py types every
entry from that header: signatures, the pointer argument class, mirrored constants and struct sizes."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "akmi.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(akmi_[a-z0-9_]+)\s*\(", txt)))


needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                 reason="hipcc not available")


@pytest.fixture
def typed_lib(monkeypatch):
    """(capi, the real library as capi.lib() loads and types it)"""
    import __graft_entry__ as g
    from athenak_amd import capi
    g.build()
    monkeypatch.setattr(capi, "_LIB", None)
    monkeypatch.setattr(capi, "_LOADED", None)
    return capi, capi.lib()


def _constants():
    """every AKMI_* #define and enumerator of the header with an integer value"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "akmi.h")).read(), flags=re.S)
    pairs = re.findall(r"#define\s+(AKMI_[A-Z0-9_]+)\s+(-?\w+)\s*$", txt, flags=re.M)
    for body in re.findall(r"\benum\s*\{([^}]*)\}", txt):
        pairs += re.findall(r"(AKMI_[A-Z0-9_]+)\s*=\s*(-?\w+)", body)
    return {k: int(v, 0) for k, v in pairs}


def test_header_symbols_listed_in_binding():
    """the parser misses no declaration"""
    from athenak_amd import capi
    assert len(_declared()) >= 190 and _declared() == sorted(capi.signatures())


@needs_hipcc
def test_every_entry_of_the_loaded_library_is_typed(typed_lib):
    capi, L = typed_lib
    assert _declared() == sorted(capi.SIGNATURES)
    for name, (restype, argtypes) in capi.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and tuple(fn.argtypes) == argtypes, name
        assert all(t in (ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_double, capi.Ptr) for t in argtypes), name


def test_one_signature_of_each_kind():
    from athenak_amd import capi
    i, ll, ull, dbl, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_double, capi.Ptr
    want = {
        "akmi_last_error": (ctypes.c_char_p, ()),
        "akmi_sim_create": (ctypes.c_void_p, (P, P)),
        "akmi_sim_time": (dbl, (P,)),
        "akmi_sim_lloc": (ctypes.POINTER(i), (P,)),
        "akmi_sim_destroy": (None, (P,)),
        "akmi_smr_cc_copy": (i, (P, i, P, ll, ll, P, P, P)),
        "akmi_selftest_fp64": (i, (i, ll, ull, P, P, P)),
        "akmi_comm_init_callbacks": (i, (i, i, P, P, P)),
        "akmi_rk_update": (i, (P, dbl, dbl, dbl, P, P, P, P, P, i, P)),
    }
    sigs = capi.signatures()
    assert {k: sigs[k] for k in want} == want
    assert sum(t is ll for _, argtypes in sigs.values() for t in argtypes) == 21


def test_unknown_parameter_type_is_refused_by_name():
    from athenak_amd import capi
    good = "int akmi_fine(const akmi_pack *p, long long n, double x[3], void *stream);\n"
    assert capi.parse_header(good) == {"akmi_fine": (ctypes.c_int, (capi.Ptr, ctypes.c_longlong, capi.Ptr, capi.Ptr))}
    for bad in ("int akmi_odd(const akmi_pack *p, float x, void *stream);", "int akmi_odd(akmi_pack p);",
                "short akmi_odd(int n);", "int akmi_odd(int (*fn)(int));"):
        with pytest.raises(capi.AkmiError, match="akmi_odd"):
            capi.parse_header(good + bad)


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    from athenak_amd import capi
    monkeypatch.setattr(capi, "SIGNATURES", {})
    monkeypatch.setattr(capi, "HEADER_PATH", str(tmp_path/"nope.h"))
    with pytest.raises(capi.AkmiError, match="nope.h"):
        capi.signatures()


def test_ptr_from_param():
    import torch
    from athenak_amd import capi

    def address(x):
        """the pointer a C function receives for the converted argument"""
        got = []
        ctypes.CFUNCTYPE(ctypes.c_int, capi.Ptr)(lambda p: got.append(p.value or 0) or 0)(x)
        return got[0]

    pack, t, n = capi.Pack(), torch.arange(6, dtype=torch.float64), ctypes.c_longlong(7)
    buf = ctypes.create_string_buffer(16)
    assert capi.Ptr.from_param(None) is None and address(None) == 0
    assert address(0x7f0012345678) == 0x7f0012345678              # an address beyond 32 bits
    assert address(ctypes.c_void_p(0x7f0012345678)) == 0x7f0012345678
    assert address(ctypes.byref(n)) == ctypes.addressof(n)
    assert address(ctypes.byref(pack)) == ctypes.addressof(pack)
    assert address(pack) == ctypes.addressof(pack)
    assert address(t) == t.data_ptr() and address(capi._p(t)) == t.data_ptr()
    assert address(buf) == ctypes.addressof(buf)
    assert address((ctypes.c_int*6)()) != 0 and address(ctypes.pointer(n)) == ctypes.addressof(n)
    assert ctypes.string_at(address(b"deck\0"), 4) == b"deck"
    for bad in (1.5, "deck"):
        with pytest.raises((TypeError, ctypes.ArgumentError)):
            capi.Ptr.from_param(bad)


@needs_hipcc
def test_struct_passed_directly_is_passed_by_reference(typed_lib):
    """host-only entry through the real library: the two spellings of the pack argument"""
    capi, L = typed_lib
    pack = capi.Pack(nmb=1, nvar=5, nx1=8, nx2=4, nx3=2, ng=2)
    sizes = [L.akmi_bvals_cc_segsize(pack, d) for d in range(27)]
    assert sizes == [L.akmi_bvals_cc_segsize(ctypes.byref(pack), d) for d in range(27)]
    assert sizes[13 + 1] == 2*4*2 and sizes[13 + 3] == 8*2*2 and sizes[13 + 9] == 8*4*2 and sizes[26] == 8   # faces, a corner
    assert all(type(n) is int for n in sizes)


def test_stand_in_receives_what_a_typed_entry_would(monkeypatch):
    """an object put into capi._LIB from outside (tests/cpu_backend.py) is called with ctypes values, whichever the spelling"""
    import torch
    from athenak_amd import capi

    class Fake:
        def akmi_smr_cc_copy(self, *args):
            self.got = args
            return 0

        def akmi_not_in_the_header(self, x):
            return x

    fake, pack, m, n = Fake(), capi.Pack(nx1=8), torch.zeros(4, dtype=torch.int32), ctypes.c_longlong(3)
    monkeypatch.setattr(capi, "_LIB", fake)
    L = capi.lib()
    assert L is capi.lib() and L.akmi_not_in_the_header(5) == 5
    for args in ((pack, 5, m, 2**40, 3, None, m, None),
                 (ctypes.byref(pack), 5, capi._p(m), ctypes.c_longlong(2**40), n, None, capi._p(m), None)):
        assert L.akmi_smr_cc_copy(*args) == 0
        p, nvar, mp, npairs, ntail, u, cu, stream = fake.got
        assert p._obj is pack and nvar == 5 and type(nvar) is int and mp.value == m.data_ptr() == cu.value
        assert (type(npairs), npairs.value, type(ntail), ntail.value) == (ctypes.c_longlong, 2**40, ctypes.c_longlong, 3)
        assert u is None and stream is None
    with pytest.raises(TypeError, match="akmi_smr_cc_copy"):
        L.akmi_smr_cc_copy(pack, 5)
    with pytest.raises(AttributeError):
        L.akmi_rk_update


def test_mirrored_constants_equal_the_header():
    from athenak_amd import capi
    H = _constants()

    def group(prefix):
        return {k[len(prefix):].lower(): v for k, v in H.items() if k.startswith(prefix)}

    assert (capi.COMPLETE, capi.INCOMPLETE, capi.FAIL) == (H["AKMI_COMPLETE"], H["AKMI_INCOMPLETE"], H["AKMI_FAIL"])
    assert capi.RECON == group("AKMI_RECON_") and len(capi.RECON) == 6
    assert capi.RSOLVER == group("AKMI_RS_") and len(capi.RSOLVER) == 6
    assert capi.BC == group("AKMI_BC_") and len(capi.BC) == 8
    assert capi.DERIVED == group("AKMI_DV_") and len(capi.DERIVED) == 10
    assert capi.AMR_METHOD == group("AKMI_AMR_") and len(capi.AMR_METHOD) == 3
    flags = [n for n in dir(capi) if n.startswith(("PHASE_", "FORM_", "COPY_", "DROP_"))]
    assert len(flags) == 4 + 4 + 3 + 2
    for n in flags + ["SMALL_PACK_CELLS", "MG_NNORMS", "TURB_NHIST"]:
        assert getattr(capi, n) == H["AKMI_" + n], n


def test_struct_mirrors_have_the_size_of_their_structs(tmp_path):
    from athenak_amd import capi
    exe = str(tmp_path/"capi_sizes")
    subprocess.check_call([shutil.which("cc") or "gcc", "-std=c99", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "capi_sizes_main.c"), "-o", exe])
    sizes = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    mirrors = {"akmi_pack": capi.Pack, "akmi_smr": capi.Smr, "akmi_rng_state": capi.RngState, "akmi_srcterms": capi.SrcTerms,
               "akmi_pdf_axis": capi.PdfAxis, "akmi_coarsen_var": capi.CoarsenVar, "akmi_mg_plan": capi.MgPlan}
    assert {k: int(v) for k, v in sizes.items()} == {k: ctypes.sizeof(m) for k, m in mirrors.items()}


@needs_hipcc
def test_library_builds_and_exports_all_symbols():
    import __graft_entry__ as g
    g.build()
    lib = ctypes.CDLL(g.LIB)
    for s in _declared():
        assert hasattr(lib, s), s
    assert lib.akmi_version() >= 100
    # timing experiments that change results exist only behind -DAKMI_EXPERIMENTS; the library under test is not one
    lib.akmi_build_flags.restype = ctypes.c_char_p
    assert lib.akmi_build_flags() == b"production"


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from athenak_amd import capi
    monkeypatch.setattr(capi, "_LIB", None)
    monkeypatch.setattr(capi, "LIB_PATH", str(tmp_path/"nope.so"))
    with pytest.raises(capi.AkmiError):
        capi.lib()


def test_product_does_not_import_oracle():
    """the product package must never reach into oracle/"""
    pkg = os.path.join(ROOT, "athenak_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "akref" not in src and "oracle" not in src.replace("oracle/", "oracle/") \
                    or f == "__none__", os.path.join(dp, f)
