"""The evaluation files (include/ddlo_eval.h, csrc/eval.cpp) through the C-ABI.
No GPU: the writer is host code.

The layout of a pose's whitespace (Eigen's default operator<<) is unpinned:
Eigen is not available to print one.  The tests hold what a parser sees: file
names, one index per line, and per pose record the stamp, sixteen numbers to 6
significant digits in row-major order, and the ';' that ends it; and the
restated layout rules only against themselves (equal cell width, one space).
"""
import ctypes as C
import os

import numpy as np
import pytest

import dynamic_direct_lidar_odometry_amd as P
from dynamic_direct_lidar_odometry_amd import evaluation as E


def six_digits(x):
    """x rounded to 6 significant digits, as %.6g prints a float32 value"""
    return np.array([float("%.6g" % float(v)) for v in np.asarray(x, np.float32).reshape(-1)])


POSES = [
    np.array([[0.36, 0.48, -0.8, 12.5], [-0.8, 0.6, 0.0, -3.25], [0.48, 0.64, 0.6, 1e-7], [0, 0, 0, 1]], np.float32),
    np.array([[1, 0, 0, -123456.789], [0, -1, 0, 0.000123456789], [0, 0, -1, 98765.4321], [0, 0, 0, 1]], np.float32),
    np.eye(4, dtype=np.float32),
]
STAMPS = [1_650_000_000_123_456_789, 1_650_000_000_223_456_789, 2**63 + 5]
INDICES = [np.array([5, 17, 4096, 131071], np.int32), np.zeros(0, np.int32), np.array([0, 1, 2], np.int32)]
SEQS = [7, 12345, 8]


def test_files_records_and_append(tmp_path):
    d = tmp_path / "a" / "b"                      # created with its parent
    ev = E.Evaluation(d)
    for seq, stamp, T, idx in zip(SEQS, STAMPS, POSES, INDICES):
        ev.write(seq, stamp, T, idx)
    assert sorted(os.listdir(d)) == ["0007.txt", "0008.txt", "12345.txt", "poses.txt"]
    # one index per line, nothing else; n == 0 leaves an empty file
    assert (d / "0007.txt").read_text() == "5\n17\n4096\n131071\n"
    assert (d / "12345.txt").read_text() == ""
    assert (d / "0008.txt").read_text() == "0\n1\n2\n"
    # the record structure of poses.txt: stamp line, four rows of four, ';' directly after the last coefficient
    lines = (d / "poses.txt").read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 5 * 3 + 1
    for k in range(3):
        rec = lines[5 * k:5 * k + 5]
        assert rec[0] == str(STAMPS[k])
        assert rec[4].endswith(";") and not rec[4][:-1].endswith(" ") and all(";" not in r for r in rec[:4])
        rows = [r.rstrip(";") for r in rec[1:]]
        got = np.array([[float(t) for t in r.split()] for r in rows])
        assert got.shape == (4, 4)
        np.testing.assert_array_equal(got.reshape(-1), six_digits(POSES[k]))
        # the restated layout: every coefficient right-aligned to the widest, one space between
        width = max(len("%.6g" % float(v)) for v in POSES[k].reshape(-1))
        assert all(len(r) == 4 * width + 3 for r in rows)
        assert rows == [" ".join(("%.6g" % float(v)).rjust(width) for v in row) for row in POSES[k]]
    # negative coefficients and the 1e-7 one came through
    first = np.array([[float(t) for t in r.rstrip(";").split()] for r in lines[1:5]])
    assert first[0, 2] == -0.8 and first[1, 0] == -0.8 and first[2, 3] == 1e-7
    # a second write with the same seq appends to both files
    ev.write(7, 42, POSES[2], np.array([9, 8], np.int32))
    assert (d / "0007.txt").read_text() == "5\n17\n4096\n131071\n9\n8\n"
    ev.close()
    idx, poses = E.read_eval(d)
    assert sorted(idx) == [7, 8, 12345]
    np.testing.assert_array_equal(idx[7], [5, 17, 4096, 131071, 9, 8])
    assert idx[12345].size == 0 and idx[12345].dtype == np.int32
    np.testing.assert_array_equal(idx[8], [0, 1, 2])
    assert [s for s, _ in poses] == STAMPS + [42]
    for (_, T), want in zip(poses, POSES + [POSES[2]]):
        np.testing.assert_array_equal(T.reshape(-1), six_digits(want))


def test_reopen_appends(tmp_path):
    with E.Evaluation(tmp_path) as ev:
        ev.write(1, 10, POSES[0], [3])
    with E.Evaluation(tmp_path) as ev:              # an existing directory is kept as it is
        ev.write(1, 20, POSES[1], [4])
    idx, poses = E.read_eval(tmp_path)
    np.testing.assert_array_equal(idx[1], [3, 4])
    assert [s for s, _ in poses] == [10, 20]


def test_unwritable_directory_and_bad_arguments(tmp_path):
    blocker = tmp_path / "file"
    blocker.write_text("x")
    L = E._lib()
    h = C.c_void_p()
    # a path below a regular file cannot be created, whoever runs the test
    assert L.ddlo_eval_open(os.fsencode(blocker / "sub"), C.byref(h)) == 1 and not h
    assert L.ddlo_eval_open(os.fsencode(blocker), C.byref(h)) == 1 and not h
    assert b"file" in P.load().gicp_last_error()
    with pytest.raises(P.GicpError):
        E.Evaluation(blocker / "sub")
    assert L.ddlo_eval_open(None, C.byref(h)) == 1
    assert L.ddlo_eval_open(os.fsencode(tmp_path / "ok"), None) == 1
    # the directory taken away between open and write: an error status, no crash
    ev = E.Evaluation(tmp_path / "gone")
    os.remove(tmp_path / "gone" / "poses.txt")
    os.rmdir(tmp_path / "gone")
    T = np.eye(4, dtype=np.float32).reshape(16)
    assert L.ddlo_eval_write(ev.h, 1, 1, P._ptr(T), None, 0) == 1
    assert L.ddlo_eval_write(ev.h, 1, 1, None, None, 0) == 1
    assert L.ddlo_eval_write(ev.h, 1, 1, P._ptr(T), None, 3) == 1
    assert L.ddlo_eval_write(None, 1, 1, P._ptr(T), None, 0) == 1
    ev.close()
    assert L.ddlo_eval_close(None) == 0
