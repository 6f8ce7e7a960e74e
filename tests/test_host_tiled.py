"""CPU: the host half of sliced inference (ultralytics/utils/tiled.py) -- the grid rule, the whole-image record, the refusals, the new
configuration keys -- and the numpy statement of the cross-tile merge (tests/tiled_util.py) on a hand-made border case."""
import numpy as np
import pytest

from tiled_util import merge_reference, planted_case


def test_grids_checked_by_hand():
    from ultralytics.utils.tiled import tile_grid
    assert [r[0] for r in tile_grid(640, 1000, 640, 0.2)] == [0, 360]
    assert [r[0] for r in tile_grid(640, 1152, 640, 0.2)] == [0, 512]
    assert tile_grid(300, 700, 640, 0.2) == [(0, 0, 640, 300), (60, 0, 700, 300)]
    assert tile_grid(640, 640, 640, 0.2) == [(0, 0, 640, 640)]  # exactly one tile
    assert tile_grid(1, 1, 640, 0.2) == [(0, 0, 1, 1)]
    assert len(tile_grid(2160, 3840, 640, 0.2)) == 32 and len(tile_grid(3648, 5472, 640, 0.2)) == 77
    # row-major: y outer, x inner
    assert tile_grid(100, 150, 64, 0.25) == [(0, 0, 64, 64), (48, 0, 112, 64), (86, 0, 150, 64), (0, 36, 64, 100), (48, 36, 112, 100), (86, 36, 150, 100)]


@pytest.mark.parametrize("overlap", [0.0, 0.25, 0.6])
def test_random_grids_cover_the_image(overlap):
    from ultralytics.utils.tiled import tile_grid
    rng = np.random.default_rng(int(overlap * 100))
    for H, W in [(1, 1), (64, 64), (65, 64), (300, 300), *rng.integers(1, 301, (40, 2)).tolist()]:
        grid = tile_grid(H, W, 64, overlap)
        cover = np.zeros((H, W), bool)
        for x1, y1, x2, y2 in grid:
            assert 0 <= x1 < x2 <= W and 0 <= y1 < y2 <= H, (H, W, grid)
            assert x2 - x1 == min(64, W) and y2 - y1 == min(64, H)
            cover[y1:y2, x1:x2] = True
        assert cover.all(), (H, W)
        assert len(set(grid)) == len(grid)
        assert grid == sorted(grid, key=lambda r: (r[1], r[0])), "row-major order"


def test_refusals():
    from ultralytics.utils.tiled import check_tile, tile_grid
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            tile_grid(100, 100, 64, bad)
    for bad in (0, -64, 48, 100, 64.0, "64", True):
        with pytest.raises(ValueError):
            check_tile(bad, 32)
    assert check_tile(64, 32) == 64 and check_tile(640, 32) == 640
    with pytest.raises(ValueError):
        check_tile(96, 64)  # a model with a coarser stride


def test_full_pass_record():
    from ultralytics.utils.tiled import plan_tiles
    plan = plan_tiles([(100, 150), (60, 60)], 64, 0.25)
    assert plan["rec_off"].tolist() == [0, 7, 8]  # 6 tiles + the whole-image pass; one tile and no pass for the image a tile holds
    assert plan["rects"][6].tolist() == [0, 0, 150, 100] and plan["geom"][6].tolist() == [64, 43, 0, 10]
    r = np.float32(64 / 150)
    assert plan["maps"].dtype == np.float32 and plan["maps"][6].tolist() == [0, 0, 0, 10, r, np.float32(1) / r]
    assert plan["rects"][7].tolist() == [0, 0, 60, 60] and plan["geom"][7].tolist() == [60, 60, 0, 0] and plan["maps"][7].tolist() == [0, 0, 0, 0, 1, 1]
    assert plan["maps"][2].tolist() == [86, 0, 0, 0, 1, 1] and plan["geom"][2].tolist() == [64, 64, 0, 0]
    assert plan["tile_img"].tolist() == [0] * 7 + [1]
    assert plan_tiles([(100, 150)], 64, 0.25, full_image=False)["rec_off"].tolist() == [0, 6]


def test_merge_reference_on_an_object_that_straddles_a_border():
    """A 30 x 20 object at x 40..70 of a 128-wide frame.  The tile at x 0 reports it whole; the tile at x 60 sees its last third and
    reports that with a lower score.  The fragment has IoU 1/3 with the whole box but lies inside it: intersection over the smaller
    box is 1, so IoS 0.5 keeps one box where IoU 0.5 keeps two."""
    maps = np.array([[0, 0, 0, 0, 1, 1], [60, 0, 0, 0, 1, 1]], np.float32)
    rows = np.array([[40, 10, 70, 30, 0.9, 0],    # tile 0: the whole object
                     [0, 10, 10, 30, 0.6, 0]],    # tile 1: x 60..70 in the frame, the truncated third, lower score
                    np.float32)
    out, keep, n = merge_reference(rows, [0, 1], maps, 64, 128, 0.5, ios=True)
    assert out[1].tolist() == [60, 10, 70, 30, np.float32(0.6), 0] and n == 2
    assert keep == [0]
    assert merge_reference(rows, [0, 1], maps, 64, 128, 0.5, ios=False)[1] == [0, 1]
    # another label survives unless the merge is class-agnostic; a tie goes to the lower row
    rows[1, 5] = 1
    assert merge_reference(rows, [0, 1], maps, 64, 128, 0.5)[1] == [0, 1]
    assert merge_reference(rows, [0, 1], maps, 64, 128, 0.5, agnostic=True)[1] == [0]
    rows[1, 4] = rows[0, 4]
    assert merge_reference(rows[::-1], [1, 0], maps, 64, 128, 0.5, agnostic=True)[1] == [0]
    # the whole-image pass: (v - pad) / r + 0, clipped; a row inside the pad band clips to nothing and is dropped
    r = np.float32(0.5)
    maps = np.array([[0, 0, 0, 16, r, np.float32(1) / r]], np.float32)
    rows = np.array([[20, 21, 35, 31, 0.5, 0], [5, 2, 30, 14, 0.9, 0], [60, 40, 70, 60, 0.4, 0]], np.float32)
    out, keep, n = merge_reference(rows, [0, 0, 0], maps, 64, 128, 0.5)
    assert out[0, :4].tolist() == [40, 10, 70, 30] and out[1, :4].tolist() == [10, 0, 60, 0] and out[2, :4].tolist() == [120, 48, 128, 64]
    assert keep == [0, 2] and n == 2


def test_planted_cases_exercise_the_sweep():
    for seed in range(6):
        rows, row_tile, maps, (H, W) = planted_case(seed)
        scores = rows[:, 4]
        tied = sum((scores == s).sum() > 1 for s in scores)
        for ios in (False, True):
            _, keep, n = merge_reference(rows, row_tile, maps, H, W, 0.5, ios=ios)
            print(f"seed {seed} ios {ios}: {len(rows)} rows, {n - len(keep)} suppressed, {tied} tied")
            assert n - len(keep) >= 0.25 * len(rows) and tied >= 5, (seed, ios)


def test_cfg_keys():
    from ultralytics.cfg import get_cfg
    a = get_cfg(overrides=dict(tile=640, tile_overlap=0.2))
    assert a.tile == 640 and a.tile_overlap == 0.2 and a.tile_iou == 0.5 and a.tile_metric == "ios" and a.tile_full is True
    assert get_cfg().tile is None  # off by default
    with pytest.raises(TypeError):
        get_cfg(overrides=dict(tile="640"))
    with pytest.raises(ValueError):
        get_cfg(overrides=dict(tile_overlap=1.5))
    with pytest.raises(TypeError):
        get_cfg(overrides=dict(tile_full=1))
    with pytest.raises(SyntaxError):
        get_cfg(overrides=dict(tiles=640))
