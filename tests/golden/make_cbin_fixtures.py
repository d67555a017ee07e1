"""Records tests/golden/cbin_fixture.cbin and tests/golden/cbin_reader.npz.

    python tests/golden/make_cbin_fixtures.py <directory of the reference's vis/python>

The file is written by CoarsenedBinaryOutput on CPU tensors (tests/coarsen_cases.write_fixture: 16^3 Orszag-Tang in 8^3
blocks, mhd_bcc, coarsen_factor = 2, compute_moments = true, after two cycles).  The npz holds what the reference's own
reader, bin_convert.read_coarsened_binary, returned for it, and the file's sha256.  The reader is imported here, at
recording time, only: tests/test_coarsen_host.py needs neither it nor this script."""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import coarsen_cases as cc  # noqa: E402


def main(reader_dir):
    sys.path.insert(0, reader_dir)
    if "h5py" not in sys.modules:            # bin_convert imports h5py for its athdf writer only
        try:
            import h5py  # noqa: F401
        except ImportError:
            import types
            sys.modules["h5py"] = types.ModuleType("h5py")
    import bin_convert
    cc.install_cpu_backend()
    try:
        with tempfile.TemporaryDirectory() as d:
            _, path = cc.write_fixture(d)
            shutil.copyfile(path, cc.FIXTURE)
    finally:
        cc.uninstall_cpu_backend()
    fd = bin_convert.read_coarsened_binary(cc.FIXTURE)
    names = list(fd["var_names"])
    np.savez_compressed(
        cc.FIXTURE_NPZ, sha256=np.array(cc.sha256(cc.FIXTURE)), var_names=np.array(names),
        mb_data=np.stack([np.stack(fd["mb_data"][v]) for v in names]), mb_index=fd["mb_index"],
        mb_logical=fd["mb_logical"], mb_geometry=fd["mb_geometry"], number_of_moments=np.array(fd["number_of_moments"]),
        nx_out_mb=np.array([fd["nx1_out_mb"], fd["nx2_out_mb"], fd["nx3_out_mb"]]), n_mbs=np.array(fd["n_mbs"]),
        time=np.array(fd["time"]), cycle=np.array(fd["cycle"]), nvars=np.array(fd["nvars"]),
        nx_mb=np.array([fd["nx1_mb"], fd["nx2_mb"], fd["nx3_mb"]]), Nx=np.array([fd["Nx1"], fd["Nx2"], fd["Nx3"]]))
    print("wrote", cc.FIXTURE, os.path.getsize(cc.FIXTURE), "bytes;", cc.FIXTURE_NPZ, os.path.getsize(cc.FIXTURE_NPZ), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
