"""Regenerates tests/golden/outputs/*: the files the output writers (athenak_amd/outputs.py,
pgen.WriteErrorsFile) produce for the cases of tests/output_cases.py, with the product's host
logic driven by the CPU oracle (tests/cpu_backend.py), so the fixtures do not depend on a GPU.
Every file is parsed with the REFERENCE's own readers (vis/python/athena_read.py, bin_convert.py)
before it is committed -- that is what pins the formats: --reference-readers DIR (the reference's
vis/python) records what they return for the fixtures, with the sha256 of every file they read,
in tests/golden/reference_readers.npz; tests/test_outputs_formats.py checks that record.

    python tests/golden/make_output_fixtures.py [--reference-readers DIR]
"""
import hashlib
import os
import shutil
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import cpu_backend
    import output_cases as oc
    cpu_backend.install()
    dst = os.path.join(HERE, "outputs")
    shutil.rmtree(dst, ignore_errors=True)
    os.makedirs(dst)
    for name in ("sod", "ot", "lwave_hydro", "lwave_mhd"):
        with tempfile.TemporaryDirectory() as d:
            files = oc.run_case(name, d, fused=False)
            for rel in files:
                tgt = os.path.join(dst, name, rel)
                os.makedirs(os.path.dirname(tgt), exist_ok=True)
                shutil.copy(os.path.join(d, rel), tgt)
                print(name, rel, os.path.getsize(tgt))
    cpu_backend.uninstall()


# the fixtures the reference's readers parse: (record prefix, reader, file under outputs/)
PARSED = [("tab_sod", "tab", "sod/tab/Sod.hydro_w.00002.tab"),
          ("hst_sod", "hst", "sod/Sod.hydro.hst"),
          ("hst_ot", "hst", "ot/OrszagTang.mhd.hst"),
          ("errs_lwave_hydro", "error_dat", "lwave_hydro/LinWave-errs.dat"),
          ("errs_lwave_mhd", "error_dat", "lwave_mhd/LinWave-errs.dat"),
          ("bin_ot", "read_binary", "ot/bin/OrszagTang.mhd_bcc.00000.bin"),
          ("bin_sod", "read_binary", "sod/bin/Sod.hydro_u.00001.bin")]


def _flatten(prefix, v, rec):
    """a reader's result as npz entries: dicts by key (the key order in <prefix>/keys), lists of arrays stacked"""
    import numpy as np
    if isinstance(v, dict):
        rec[prefix + "/keys"] = np.array([str(k) for k in v])
        for k, x in v.items():
            _flatten("%s/%s" % (prefix, k), x, rec)
    elif isinstance(v, (list, tuple)) and v and all(isinstance(x, str) for x in v):
        rec[prefix] = np.array(v)
    elif isinstance(v, (list, tuple)) and v and all(isinstance(x, np.ndarray) for x in v):
        rec[prefix] = np.stack(v)
    elif v is not None:
        rec[prefix] = np.asarray(v)


def record_reference_readers(readers_dir):
    import numpy as np
    sys.path.insert(0, readers_dir)
    import athena_read
    if "h5py" not in sys.modules:            # bin_convert imports h5py for its athdf writer only;
        try:                                 # read_binary() does not use it
            import h5py  # noqa: F401
        except ImportError:
            sys.modules["h5py"] = types.ModuleType("h5py")
    import bin_convert
    readers = {"tab": athena_read.tab, "hst": athena_read.hst, "error_dat": athena_read.error_dat,
               "read_binary": bin_convert.read_binary}
    rec = {}
    for prefix, reader, rel in PARSED:
        path = os.path.join(HERE, "outputs", rel)
        rec["sha256/" + rel] = np.array(hashlib.sha256(open(path, "rb").read()).hexdigest())
        _flatten(prefix, readers[reader](path), rec)
    # the bin dump of the refined mesh that test_refined_mesh_bin_and_rst_carry_block_levels writes
    import cpu_backend
    import test_outputs_formats as tof
    cpu_backend.install()
    with tempfile.TemporaryDirectory() as d:
        tof._run_smr(d, [])
        path = os.path.join(d, "bin", "LinWave.hydro_u.00001.bin")
        rec["generated_sha256/bin_smr"] = np.array(hashlib.sha256(open(path, "rb").read()).hexdigest())
        _flatten("bin_smr", bin_convert.read_binary(path), rec)
    cpu_backend.uninstall()
    out = os.path.join(HERE, "reference_readers.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out))


if __name__ == "__main__":
    if "--reference-readers" in sys.argv:
        record_reference_readers(sys.argv[sys.argv.index("--reference-readers") + 1])
    else:
        main()
