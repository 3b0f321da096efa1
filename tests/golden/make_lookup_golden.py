"""Records tests/golden/lookup/parent_bits.npz: what the routes through the (T, log10 P) table look-up give for the cases of
tests/lookup_cases.py (test_gpu_lookup_columns.routes) with the LIBRARY of the commit whose look-up kernels were replaced
(cf4ceda).  The cases and routes() came with the commit after it, so the fixture is re-recorded from THIS tree's tests/ over
that commit's library: build cf4ceda's helios_amd/csrc into a library of its own and name it in HELIOS_HIP_LIB, on an MI355X:

    HELIOS_HIP_LIB=/path/to/cf4ceda/libhelios_hip.so python tests/golden/make_lookup_golden.py [output.npz]

(routes() uses only entry points that commit has.)  Everything is computed twice, in fresh batches; the two recordings must
agree bit for bit.  Arrays are stored as they are, smallest first, as long as the file's raw content stays under BUDGET bytes;
the others as the SHA-256 of their raw bytes under the key "sha256 <name>"."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
BUDGET = 800 * 1024


def main(path):
    import test_gpu_lookup_columns as t
    import test_gpu_lookup_edges as le
    from helios_amd.device import Context
    ctx = Context(0)
    first = t.routes(ctx)
    le._kept.clear()
    second = t.routes(ctx)
    assert set(first) == set(second)
    for key in first:
        le._same_bytes(first[key], second[key], key + ", second recording")
    out, used = {}, 0
    for key in sorted(first, key=lambda k: (first[k].nbytes, k)):
        if used + first[key].nbytes <= BUDGET:
            out[key] = first[key]
            used += first[key].nbytes
        else:
            out["sha256 " + key] = t.digest(first[key])
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print("%d arrays (%d as digests), %d bytes raw, %d bytes on disk: %s"
          % (len(out), sum(k.startswith("sha256 ") for k in out), used, os.path.getsize(path), path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lookup", "parent_bits.npz"))
