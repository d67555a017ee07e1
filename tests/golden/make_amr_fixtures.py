"""Records what the REFERENCE's own readers (vis/python/bin_convert.read_binary, athena_read.hst) return for the bin
and hst files an adaptive run writes before and after its regrids, into tests/golden/amr_reference_readers.npz, with
the sha256 of the files read.  tests/test_amr_host.py regenerates the files on the CPU backend, checks that they are
those very bytes, and compares the block counts and the history with the record.

    python tests/golden/make_amr_fixtures.py <directory of the reference's vis/python>

The readers are imported here, at generation time, only; nothing of them is stored."""
import hashlib
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(readers_dir):
    import numpy as np
    import amr_runs
    from make_output_fixtures import _flatten
    sys.path.insert(0, readers_dir)
    import athena_read
    if "h5py" not in sys.modules:            # bin_convert imports h5py for its athdf writer only
        try:
            import h5py  # noqa: F401
        except ImportError:
            sys.modules["h5py"] = types.ModuleType("h5py")
    import bin_convert
    rec = {}
    with tempfile.TemporaryDirectory() as d:
        res = amr_runs.outputs_across_regrid(d, "cpu")
        for tag, rel in (("bin_before", res["bin_files"][0]), ("bin_after", res["bin_files"][-1])):
            path = os.path.join(d, rel)
            rec["sha256/" + tag] = np.array(hashlib.sha256(open(path, "rb").read()).hexdigest())
            rec["name/" + tag] = np.array(rel)
            _flatten(tag, bin_convert.read_binary(path), rec)
        path = os.path.join(d, res["hst_file"])
        rec["sha256/hst"] = np.array(hashlib.sha256(open(path, "rb").read()).hexdigest())
        _flatten("hst", athena_read.hst(path), rec)
    out = os.path.join(HERE, "amr_reference_readers.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), sorted(k for k in rec if "/" not in k or k.count("/") == 1)[:40])


if __name__ == "__main__":
    main(sys.argv[1])
