"""CPU: the batch residual and compaction entry points answer a NULL handle with a negative status and a message, before
they touch a device (there is none here)."""
import ctypes as C

from spherical_bundle_adjuster_amd import _cabi as cabi


def test_batch_select_entry_points_refuse_a_null_handle():
    lib = cabi.load_library()
    n_kept = (C.c_size_t * 1)()
    calls = {
        "batch_residuals": lambda: lib.sba_batch_residuals(None, 0, None, None, None, None, 1.0, None, None, None, None),
        "batch_compact": lambda: lib.sba_batch_compact(None, None, n_kept, None),
        "batch_keep_inliers": lambda: lib.sba_batch_keep_inliers(None, 0, None, None, None, None, 1.0, n_kept, None),
    }
    for name, call in calls.items():
        rc = call()
        assert rc < 0, name
        assert "null batch handle" in cabi.last_error(lib), name
