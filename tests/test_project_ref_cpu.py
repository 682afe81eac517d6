"""What the restatement of the range-image projection (project_ref.py) alone says about the inputs the GPU
tests use (test_gpu_project.py, test_gpu_project_driver.py), so that their caps are known to hold before any
kernel runs: undecided points <= 1e-3 of the kept points and excluded pixels <= 2 over all geometries used
(here both are 0 on the ray-cast frames), every point of a flattened organized frame lands on the pixel it
came from, and the hand points fall where include/ddlo_seg_project.h says.  No GPU.
"""
import numpy as np
import pytest

import project_ref as PJ


cast = PJ.cast


def ang_bottom(rows):
    return 22.5 if rows <= 64 else 45.0      # scene.lidar_dirs' vertical field of view


# rows, cols: (own pixel, coarse collisions, out of view at half the field of view)
FIGURES = {(16, 256): (4096, 3584, 2048), (64, 2048): (131072, 114688, 65536)}


@pytest.mark.parametrize("rows,cols", sorted(FIGURES))
def test_frames_figures(rows, cols):
    f = cast(rows, cols)
    n = rows * cols
    own, coarse_coll, half_oov = FIGURES[(rows, cols)]
    # a ray-cast frame without blanks would make the figures below trivially n; these scenes are closed
    # (ground, facades), so every pixel has a return
    assert len(f) == n and np.isfinite(f).all()
    proj = PJ.default_projection(rows, ang_bottom(rows))
    a = PJ.analyse(f, proj, rows, cols)
    undecided, kept, excluded = int(a["undecided"].sum()), int(a["kept"].sum()), int(a["excluded"].sum())
    print(rows, cols, "own", int((a["pixel_of_point"] == np.arange(n)).sum()), "undecided", undecided, "kept", kept)
    assert int((a["pixel_of_point"] == np.arange(n)).sum()) == own == n
    assert np.array_equal(a["winner"].ravel(), np.arange(n))
    assert (a["invalid"], a["out_of_view"], a["occupied_pixels"], a["collisions"]) == (0, 0, n, 0)
    assert undecided == 0
    # the coarse image: half the rows, a quarter of the columns, the same field of view
    r2, c2 = rows // 2, cols // 4
    b = PJ.analyse(f, PJ.default_projection(r2, ang_bottom(rows)), r2, c2)
    assert b["occupied_pixels"] == r2 * c2 and b["collisions"] == coarse_coll and b["out_of_view"] == 0
    undecided += int(b["undecided"].sum())
    kept += int(b["kept"].sum())
    excluded += int(b["excluded"].sum())
    # half the field of view at the same resolution: an image of half the rows whose top is at elev_top / 2
    # (the beams then sit a quarter of a row off the rows' centres)
    half = PJ.Projection(proj.elev_top / 2, proj.elev_res)
    c = PJ.analyse(f, half, rows // 2, cols)
    assert c["out_of_view"] == half_oov
    undecided += int(c["undecided"].sum())
    kept += int(c["kept"].sum())
    excluded += int(c["excluded"].sum())
    print("undecided", undecided, "of", kept, "kept; excluded pixels", excluded)
    assert undecided <= 1e-3 * kept and excluded <= 2
    assert (undecided, excluded) == (0, 0)


def test_frame_512_own_pixels():
    f = cast(512, 512)
    a = PJ.analyse(f, PJ.default_projection(512, 45.0), 512, 512)
    assert np.isfinite(f).all()
    assert np.array_equal(a["pixel_of_point"], np.arange(512 * 512)) and int(a["undecided"].sum()) == 0


HAND_GEOMETRIES = [(3, 7, PJ.SMALL_PROJECTION), (16, 256, PJ.default_projection(16, 22.5)),
                   (8, 64, PJ.default_projection(8, 22.5))]


@pytest.mark.parametrize("rows,cols,proj", HAND_GEOMETRIES, ids=["3x7", "16x256", "8x64"])
def test_hand_points(rows, cols, proj):
    hp = PJ.hand_points(proj, rows, cols)
    pts = np.stack([p for _, p, _ in hp])
    a = PJ.analyse(pts, proj, rows, cols)
    valid = PJ.angles(pts)[0]
    seen_half = False
    for i, (name, _, want) in enumerate(hp):
        if want[0] == "undecided":
            assert a["undecided"][i], name
            seen_half = True
            continue
        assert not a["undecided"][i], f"{name} is undecided"
        if want[0] == "invalid":
            assert not valid[i] and a["pixel_of_point"][i] == -1, name
        elif want[0] == "oov":
            assert valid[i] and not a["kept"][i] and a["pixel_of_point"][i] == -1, name
        else:
            assert a["kept"][i], name
            if want[1] is not None:
                assert a["row"][i] == want[1], (name, a["row"][i])
            if want[2] is not None:
                assert a["col"][i] == want[2], (name, a["col"][i])
    assert seen_half == (rows == 3)
    assert a["invalid"] == 3
    if cols == 256:
        cols_of = {n: int(a["col"][i]) for i, (n, _, _) in enumerate(hp)}
        assert [cols_of[k] for k in ("+x", "+y", "-x", "-y")] == [0, 64, 128, 192]


@pytest.mark.parametrize("rows,cols,proj", HAND_GEOMETRIES, ids=["3x7", "16x256", "8x64"])
def test_wrap_and_reversed_azimuth(rows, cols, proj):
    # qc rounds to cols itself -> column 0
    q, p, (row, col) = PJ.wrap_case(proj, rows, cols)
    _, _, qc = PJ.quotients(p, q, rows, cols)
    assert cols - 0.5 < qc[0] < cols
    a = PJ.analyse(p, q, rows, cols)
    assert a["kept"][0] and not a["undecided"][0] and (a["row"][0], a["col"][0]) == (row, col)
    # azim_sign = -1 with azim0 = 90 (the horizontal angle atan2(x, y) of the reference's commented loop):
    # qc = -(a - 90) / w, so +y is column 0, +x a quarter turn on, -y half a turn, -x wraps to three quarters
    r = PJ.Projection(proj.elev_top, proj.elev_res, 90.0, -1)
    axes = np.array([[0, 1, 0], [1, 0, 0], [0, -1, 0], [-1, 0, 0]], np.float32)
    b = PJ.analyse(axes, r, rows, cols)
    assert b["kept"].all() and not b["undecided"].any()
    w = 360.0 / cols
    want = [int(np.floor(-(deg - 90.0) / w + 0.5)) % cols for deg in (90.0, 0.0, -90.0, 180.0)]
    assert b["col"].tolist() == want
    if cols % 4 == 0:
        assert want == [0, cols // 4, cols // 2, 3 * cols // 4]


def test_highest_index_wins_and_counts():
    proj = PJ.default_projection(16, 22.5)
    p = PJ.direction(0.0 + 1.5, 10.0)          # row 7, some column
    pts = np.stack([p, p * 2, np.zeros(3, np.float32), p * 3, np.array([0, 0, 1], np.float32)]).astype(np.float32)
    a = PJ.project(pts, proj, 16, 256)
    pix = a["pixel_of_point"]
    assert pix[0] == pix[1] == pix[3] >= 0 and pix[2] == pix[4] == -1
    assert a["winner"].ravel()[pix[0]] == 3 and int((a["winner"] >= 0).sum()) == 1
    assert (a["points"], a["invalid"], a["out_of_view"], a["occupied_pixels"], a["collisions"]) == (5, 1, 1, 1, 2)
    e = PJ.project(np.zeros((0, 3), np.float32), proj, 16, 256)
    assert (e["winner"] == -1).all() and e["points"] == e["occupied_pixels"] == e["collisions"] == 0


def test_gpu_test_clouds_are_decided():
    """The blanked, shuffled 16 x 256 cloud of test_gpu_project.py in every geometry it is projected into, the
    hand points before and after it: the only undecided points are the two copies of the hand point placed
    exactly between two rows of the 3 x 7 image, and they can change at most 2 pixels."""
    f = PJ.blank(cast(16, 256), 16, 256, (4, 60), 11)
    pts = f[np.isfinite(f).all(axis=1)]
    undecided = kept = excluded = 0
    for rows, cols, proj in HAND_GEOMETRIES + [(8, 256, PJ.Projection(11.25, 3.0))]:
        hp = np.stack([p for _, p, _ in PJ.hand_points(proj, rows, cols)])
        wq, wp, _ = PJ.wrap_case(proj, rows, cols)
        cloud = np.concatenate([hp, pts, hp, wp[None]]).astype(np.float32)
        for q in (proj, wq, PJ.Projection(proj.elev_top, proj.elev_res, proj.azim0 + 90.0, -1)):
            a = PJ.analyse(cloud, q, rows, cols)
            print(rows, cols, q, int(a["undecided"].sum()), int(a["excluded"].sum()))
            assert int(a["undecided"].sum()) == (2 if rows == 3 else 0) and int(a["excluded"].sum()) <= 2
            undecided += int(a["undecided"].sum())
            kept += int(a["kept"].sum())
            excluded = max(excluded, int(a["excluded"].sum()))
    assert undecided <= 1e-3 * kept
