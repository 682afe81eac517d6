"""GPU tests of the device's std::sort permutation on its own (ddlo_debug_sort_order,
csrc/voxel_order.hip) against the plain restatement tests/pcl_order_ref.py, which
tests/test_pcl_order_ref_cpu.py pins to std::sort itself: exact equality of the whole
permutation, on lengths around the insertion threshold (16) and the hand-over threshold S the
library reports, on the key patterns that steer the median and the Hoare scan, and on inputs
chosen for the paths they take (depth-limit heap sort, global levels, scale)."""
import numpy as np
import pytest

from dynamic_direct_lidar_odometry_amd import odometry as OD
import pcl_order_ref as PO

pytestmark = pytest.mark.gpu


def threshold():
    return int(OD.sort_order(np.zeros(1, np.uint32))[1].threshold)


def check(keys):
    perm, st = OD.sort_order(keys)
    ref, rst = PO.sort_order(keys)
    np.testing.assert_array_equal(perm, ref)
    assert st.heap_segments == rst["heap_segments"] and st.heap_longest == rst["heap_longest"]
    assert st.levels == rst["levels"]
    return st


def test_threshold_is_the_documented_one():
    assert threshold() == 512


LENGTHS = {"0": lambda S: 0, "1": lambda S: 1, "2": lambda S: 2, "16": lambda S: 16, "17": lambda S: 17,
           "18": lambda S: 18, "33": lambda S: 33, "S-1": lambda S: S - 1, "S": lambda S: S, "S+1": lambda S: S + 1,
           "2S+3": lambda S: 2 * S + 3}


@pytest.mark.parametrize("which", list(LENGTHS))
def test_lengths_and_patterns(which):
    S = threshold()
    n = LENGTHS[which](S)
    if n < 17:
        perm, st = OD.sort_order(np.arange(n)[::-1] // 2)
        np.testing.assert_array_equal(perm, PO.sort_order(np.arange(n)[::-1] // 2)[0])
        assert st.levels == 0 and st.lds_segments == 0
        return
    for name, keys in PO.key_patterns(n).items():
        st = check(keys)
        assert (st.global_levels > 0) == (n > S), name
        assert st.lds_segments > 0, name


def test_heap_path_at_length():
    st = check(PO.heap_keys())
    print(f"heap path: {st.heap_segments} heap-sorted segments, longest {st.heap_longest}, levels {st.levels}, "
          f"global {st.global_levels}, handed over {st.lds_segments}")
    assert st.heap_segments >= 1 and st.heap_longest > 64


def test_global_path():
    S = threshold()
    st = check(np.full(4 * S, 11))
    assert st.global_levels >= 1 and st.lds_segments >= 2


def test_scale():
    keys = np.random.default_rng(5).integers(0, 40000, 131072)
    st = check(keys)
    print(f"scale: levels {st.levels} of a limit of 34, global {st.global_levels}, handed over {st.lds_segments}")
    assert st.heap_segments == 0 and st.levels < 34


def test_errors():
    import ctypes as C
    L = OD._lib()
    out = np.zeros(4, np.int32)
    assert L.ddlo_debug_sort_order(0, None, 4, out.ctypes.data_as(C.c_void_p), None) == 1      # GICP_EINVAL
    k = np.arange(4, dtype=np.uint32)
    assert L.ddlo_debug_sort_order(0, k.ctypes.data_as(C.c_void_p), 4, None, None) == 1
    assert L.ddlo_debug_sort_order(0, k.ctypes.data_as(C.c_void_p), 4, out.ctypes.data_as(C.c_void_p), None) == 0
    assert out.tolist() == [0, 1, 2, 3]
