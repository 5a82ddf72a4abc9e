"""Pins oracle.vit_oracle.median_filter (and with it the device kernel ocm_op_median_filter) against the real
scipy.ndimage.median_filter the reference calls (eval.py:144,158). scipy IS importable in the build container, so this
post-processing step is pinned rather than restated: run `python oracle/make_golden_median.py` there; the fixtures
tests/golden/median.npz and tests/golden/median_edges.npz hold scipy's outputs only (inputs are regenerated from the
seed). `python oracle/make_golden_median.py edges` (or `median`) writes one of the two and leaves the other alone."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vit_oracle as O  # noqa: E402
from tests.golden_cases import MEDIAN_SIZES as SIZES, median_inputs as inputs  # noqa: E402  (scipy-free, shared with the tests)
from tests.golden_cases import MEDIAN_EDGE_SHAPES, MEDIAN_EDGE_SIZES, median_edge_inputs  # noqa: E402


def write_median():
    from scipy.ndimage import median_filter  # only the fixture writer needs scipy
    x = inputs()
    out = {"seed": np.int64(17)}
    import scipy
    out["scipy_version"] = np.array(scipy.__version__)
    for k in SIZES:
        ref = np.stack([median_filter(x[t], size=k) for t in range(x.shape[0])])
        assert np.array_equal(ref, O.median_filter(x, k)), f"oracle median_filter != scipy at size {k}"
        out[f"size{k}"] = ref
    path = os.path.join(ROOT, "tests", "golden", "median.npz")
    np.savez_compressed(path, **out)
    print(f"median_filter sizes {SIZES} pinned against scipy {scipy.__version__} -> {os.path.relpath(path, ROOT)}")


def write_edges():
    """Maps of height / width 1 and windows wider than the map at sizes up to the kernel's cap (tests/golden_cases.py)."""
    import scipy
    from scipy.ndimage import median_filter
    seed = 23
    out = {"seed": np.int64(seed), "scipy_version": np.array(scipy.__version__)}
    for i, x in enumerate(median_edge_inputs(seed)):
        for k in MEDIAN_EDGE_SIZES:
            ref = np.stack([median_filter(x[t], size=k) for t in range(x.shape[0])])
            assert np.array_equal(ref, O.median_filter(x, k)), f"oracle median_filter != scipy on map {x.shape} at size {k}"
            out[f"map{i}_size{k}"] = ref
    path = os.path.join(ROOT, "tests", "golden", "median_edges.npz")
    np.savez_compressed(path, **out)
    print(f"median_filter maps {MEDIAN_EDGE_SHAPES} x sizes {MEDIAN_EDGE_SIZES} pinned against scipy {scipy.__version__} -> "
          f"{os.path.relpath(path, ROOT)}")


def main(which=()):
    writers = {"median": write_median, "edges": write_edges}
    for name in which or writers:
        writers[name]()


if __name__ == "__main__":
    main(sys.argv[1:])
