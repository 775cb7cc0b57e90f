"""OccupancyGrid configurations away from the two square, clipped grids of gen_golden.py --
TEST INFRASTRUCTURE, plain data: read by oracle/gen_golden_obs.py (which records the reference
OccupancyGridObservation on them, tests/golden/obsref_grid_<scene>.npz) and by the tests that
hold the oracle and the HIP kernels to those fixtures.

Shapes are [F, W, H] with W = floor(x extent / x step), H = floor(y extent / y step); a cell is
grid[f, ix, iy], so W != H tells a transposed index or stride apart.
"""

GRID_CASES = {
    # 32 x 8: C % 4 == 0 with an on_road layer (the vector write-out's road-bit lookup), non-uniform step
    "wide_road": dict(features=["presence", "vx", "on_road", "y"], grid_size=[[-56, 56], [-16, 32]],
                      grid_step=[3.5, 6], features_range=None, clip=True),
    # 20 x 60: ranges for x and vx only, clip off (values outside [-1, 1] survive)
    "tall_noclip": dict(features=["x", "y", "vx", "vy", "heading", "presence"], grid_size=[[-60, 60], [-60, 60]],
                        grid_step=[6, 2], features_range={"x": [-20, 20], "vx": [-5, 5]}, clip=False),
    # 21 x 7 = 147 cells: the scalar write-out with an on_road layer, lane-relative features
    "odd_road": dict(features=["on_road", "presence", "cos_h", "sin_h", "long_off", "lat_off", "ang_off"],
                     grid_size=[[-50, 55], [-14, 28]], grid_step=[5, 6],
                     features_range={"y": [-8, 8], "vy": [-1, 1]}, clip=True),
    # 128 x 128: more than 64 KB of LDS scratch
    "big": dict(features=["presence", "on_road", "vx"], grid_size=[[-64, 64], [-64, 64]], grid_step=[1, 1],
                features_range=None, clip=True),
}
GRID_SHAPES = {"wide_road": (4, 32, 8), "tall_noclip": (6, 20, 60), "odd_road": (7, 21, 7), "big": (3, 128, 128)}

# (kind, vehicles, seed, policy steps) of the gen_golden.py scenes the fixtures are recorded on
GRID_SCENES = [("highway", 32, 0, 4), ("sine", 32, 0, 4), ("arc", 32, 1, 4), ("dense", 16, 0, 2)]


def scene_name(kind: str, n: int, seed: int) -> str:
    return f"{kind}_n{n}_s{seed}"
