"""The order-free formulation of the labelling (tests/label_ref.py, DESIGN.md
§11) against the literal restatement oracle/segment_ref.py:label_components,
with no kernel involved: labels and segment count equal, average residuals
within (m + 1) 2^-24 of the oracle's value (m positive float terms summed
sequentially and one float division there, a double sum here).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
import label_ref as LR
from dynamic_direct_lidar_odometry_amd import segmentation as S
from oracle import segment_ref as R


def check(p, rng, z, init, sensor_z, resid):
    olab, oavg, on = R.label_components(p, rng, z, init, sensor_z, resid)
    stats = {}
    lab, avg, n = LR.label_components(p, rng, z, init, sensor_z, resid, stats)
    assert n == on
    assert np.array_equal(lab, olab)
    LR.assert_avg_within_bound(avg, oavg, LR.residual_terms(olab, resid, on))
    return olab, on, stats


@pytest.mark.parametrize("block", range(6))
def test_random_images_match_oracle(block):
    """300 seeds, 50 per case."""
    with_segment = 0
    for seed in range(50 * block, 50 * block + 50):
        _, on, _ = check(*LR.random_case(seed))
        with_segment += on > 0
    assert with_segment >= 45


@pytest.mark.parametrize("name", sorted(LR.hand_cases()))
def test_hand_built_cases(name):
    p, rng, z, init, sensor_z, resid, want = LR.hand_cases()[name]
    olab, on, _ = check(p, rng, z, init, sensor_z, resid)
    assert on == want["segments"]
    for (r, c), l in want.get("labels", {}).items():
        assert olab[r, c] == l, (r, c)


def test_falling_pole_replays_the_whole_component():
    p, rng, z, init, sensor_z, resid, _ = LR.hand_cases()["falling_pole_rejected"]
    stats = {}
    LR.label_components(p, rng, z, init, sensor_z, resid, stats)
    assert stats == {"replayed": 1, "longest_prefix": 59}


def test_plain_maximum_is_not_the_reference():
    """Replacing the prefix rule by the maximum over all non-seed z accepts the 5, 0, 3 push
    sequence that the reference rejects: the inputs discriminate."""
    p, rng, z, init, sensor_z, resid, want = LR.hand_cases()["zero_goes_to_else_rejected"]
    assert want["segments"] == 0
    rest = [z[1, 2], z[2, 1], z[1, 3]]
    assert p.min_delta_z <= max(rest) - min(v for v in rest if v != 0) <= p.max_delta_z


@pytest.mark.parametrize("cols", [130, 300])
def test_serpentine(cols):
    p, rng, z, init, sensor_z, resid = LR.serpentine_case(cols)
    olab, on, _ = check(p, rng, z, init, sensor_z, resid)
    assert on == 1
    assert (olab == 1).sum() == 12 * cols + 11 and (cols < 300 or (olab == 1).sum() >= 3000)
    assert 190 <= (olab == R.REJECTED).sum() <= 215


def test_window_outside_the_columns_is_refused():
    p, rng, z, init, sensor_z, resid = LR.random_case(0)
    p.win_col1 = p.cols
    with pytest.raises(ValueError):
        LR.label_components(p, rng, z, init, sensor_z, resid)


def test_device_labelling_entry_points_without_a_gpu():
    """Exported, declared, bound; argument errors come back before any device is touched."""
    names = ("ddlo_seg_set_labelling", "ddlo_seg_get_labelling", "ddlo_seg_label_device", "ddlo_seg_labelling_stats")
    out = subprocess.run(["nm", "-D", "--defined-only", P.lib_path()], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "ddlo_seg_label.h"' in open(os.path.join(inc, "ddlo_segment.h")).read()   # comes with ddlo_segment.h
    hdr = open(os.path.join(inc, "ddlo_seg_label.h")).read()
    L = S._lib()
    for n in names:
        assert n in exported and n + "(" in hdr and getattr(L, n).argtypes is not None, n
    assert "#define DDLO_SEG_LABEL_HOST   0" in hdr and "#define DDLO_SEG_LABEL_DEVICE 1" in hdr
    assert S.LABELLING == {"host": 0, "device": 1}
    m = C.c_int()
    assert L.ddlo_seg_set_labelling(None, 1) == 1 and L.ddlo_seg_get_labelling(None, C.byref(m)) == 1   # GICP_EINVAL
    assert L.ddlo_seg_labelling_stats(None, None, None) == 1
    # a window that reaches outside the columns, and null images
    p, rng, z, init, sensor_z, resid = LR.random_case(0)
    sp = S.default_seg_params(ground_rows=0, **vars(p))
    seg = C.c_int32()
    avg = np.zeros(4)
    args = lambda q, r: (0, C.byref(q), r, P._ptr(z), None, 0.3, P._ptr(init), P._ptr(avg), avg.size, C.byref(seg))
    assert L.ddlo_seg_label_device(*args(sp.replace(win_col1=sp.cols), P._ptr(rng))) == 1
    assert L.ddlo_seg_label_device(*args(sp.replace(win_col0=-1), P._ptr(rng))) == 1
    assert L.ddlo_seg_label_device(*args(sp, None)) == 1
    assert (init == LR.random_case(0)[3]).all()
