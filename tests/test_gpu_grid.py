"""The OccupancyGrid observer on the GPU (grid_observe: the standalone grid_obs_kernel and the
epilogue ttrl_env_step_grid fuses into the step launch) at the shapes and LDS sizes the rest of the
suite does not reach, against the float64 oracle and the reference observer's recorded outputs
(tests/golden/obsref_grid_*.npz, oracle/grid_cases.py).  Run on an MI355X.

  * f64: every comparison is bit for bit (np.array_equal / torch.equal).
  * f32: test_gpu_parity's rule unchanged: a cell may differ by more than F32_TOL only where the
    oracle's float64 cell-floor margin is below F32_MARGIN; at most F32_EXCUSED_CAP of a
    configuration's cells may carry such a margin (counted from the oracle's margins alone, so the
    cap is a property of the test's scenes, not of the kernel).

Grids are not square (a swapped axis or stride shows), take both write-outs with an on_road layer
(C % 4 == 0: the 4-cell groups' road-bit lookup; else the scalar loop), keep values outside
[-1, 1] (clip off), give ranges to some features only, have one row or one column, leave the
observer outside, carry all 14 features, and are coarse enough for several vehicles to contest a
cell (lowest slot wins).  The state edits move the observer out of slot 0, punch absent slots
between present ones and remove the controlled vehicle of one env.  The fused step is taken at
every LDS tier of its launch (ttrl_diag_grid_step_lds names the tier), with the observer moved,
and beyond it (two launches); the caps of both entry points are pinned.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import golden_files, load_golden
from oracle.grid_cases import GRID_CASES, GRID_SCENES, scene_name
from oracle.oracle import HostState, Oracle
from test_gpu_parity import F32_MARGIN, F32_TOL, G7, GR, f32_inputs, to_dev
from topotrafficrl_amd import _abi, _lib
from topotrafficrl_amd.observation import occupancy_grid
from topotrafficrl_amd.road import BatchedRoad, RoadNetwork

pytestmark = pytest.mark.gpu

P = _abi.default_params()
LANES = _abi.straight_lane_table(4)
E_UNSUPPORTED = -3
F32_EXCUSED_CAP = 0.01
GRID_LDS_CAP = 160 * 1024  # ttrl_observe_grid's scratch cap

EXTRA = {
    "row_1x40": dict(features=["presence", "y", "vx"], grid_size=[[-60, 60], [-10.25, 9.75]], grid_step=[120, 0.5]),
    "col_40x1": dict(features=["presence", "x", "on_road"], grid_size=[[-121, 119], [-10, 10]], grid_step=[6, 20]),
    "no_observer": dict(features=["presence", "x", "y", "on_road"], grid_size=[[10, 90], [-6, 10]], grid_step=[4, 4]),
    "all14": dict(features=list(_abi.FEATURES), grid_size=[[-49, 47], [-13.5, 10.5]], grid_step=[4, 3]),
    "coarse": dict(features=["presence", "x", "y", "vx"], grid_size=[[-66, 62], [-14, 14]], grid_step=[8, 4]),
}
CASES = dict(GRID_CASES, **EXTRA)
BATCHES = [(24, 32), (64, 64), (100, 128), (200, 256)]


def cfg_of(name, shift=(0.0, 0.0)):
    """The case's grid, moved by ``shift`` metres."""
    c = dict(CASES[name])
    c["grid_size"] = [[v + d for v in ax] for ax, d in zip(c["grid_size"], shift)]
    return _abi.grid_cfg(**c)


# The float32 runs move every grid by this much.  Unmoved, the cases put cell edges where content
# sits by construction: lane centres lie multiples of 4 m from an observer in the middle of its
# lane, and the on_road waypoints step from -100 m by the smaller cell size, so whole rows and the
# road layer's outline would carry a zero cell-floor margin (7 % of wide_road's cells, the whole
# on_road layer of a one-row grid).  Moved, an edge is at least 0.3 m from such content and a small
# margin is a vehicle that happens to be near an edge.
F32_SHIFT = (0.3, 0.7)


@functools.lru_cache(maxsize=None)
def _batch(n):
    """test_grid_random_batch_vs_oracle's batch: 37 highway scenes of n vehicles after one policy
    step.  Cached: callers take a copy."""
    E = 37
    o = Oracle(LANES, P)
    h = HostState(E, n)
    o.reset_highway(h, _abi.reset_cfg(n, LANES), list(range(500, 500 + E)))
    o.simulate(h, np.random.default_rng(n).integers(0, 5, E).astype(np.int32), 15, 1 / 15)
    return h


def batch(n, envs=None):
    """A copy of the batch (its first ``envs`` envs)."""
    h = _batch(n)
    g = HostState(envs or h.E, n)
    for k in g.a:
        g.a[k][...] = h.a[k][:g.E]
    return g


def move_observer(h, slot):
    """The vehicles of slot 0 (the MDP vehicle reset puts there) and ``slot`` change places."""
    for k, v in h.a.items():
        if v.ndim >= 2 and v.shape[1] == h.N and k != "rng":
            v[:, [0, slot]] = v[:, [slot, 0]]
    assert np.all(h["kind"][:, slot] == _abi.MDP) and np.all(h["kind"][:, 0] != _abi.MDP)


def crowd(h, factor=0.2):
    """Every vehicle pulled towards the controlled one along the road (5 m apart instead of 25 m):
    vehicles of one lane then share the coarse grid's 8 m cells."""
    ex = h["x"][:, :1]
    h["x"][...] = ex + (h["x"] - ex) * factor


def punch_absent(h, seed):
    """A fifth of the slots absent, at random interior positions (never the observer's)."""
    rng = np.random.default_rng(seed)
    for e in range(h.E):
        free = np.nonzero(h["kind"][e, 1:h.N - 1] != _abi.MDP)[0] + 1
        h["kind"][e, rng.choice(free, h.N // 5, replace=False)] = _abi.ABSENT


def contested_cells(h, cfg):
    """(vehicles inside the grid, those that lose their cell to a lower slot), counted on the host
    from the float64 positions (no feature range for x / y in the configurations this is used with)."""
    assert not cfg.has_range[_abi.FEATURE_CODE["x"]] and not cfg.has_range[_abi.FEATURE_CODE["y"]]
    total = losers = 0
    for e in range(h.E):
        ego = np.nonzero(h["kind"][e] == _abi.MDP)[0]
        if not len(ego):
            continue
        on = h["kind"][e] != _abi.ABSENT
        fx = np.floor((h["x"][e][on] - h["x"][e, ego[0]] - cfg.grid_min_x) / cfg.step_x)
        fy = np.floor((h["y"][e][on] - h["y"][e, ego[0]] - cfg.grid_min_y) / cfg.step_y)
        inside = (fx >= 0) & (fx < cfg.shape_x) & (fy >= 0) & (fy < cfg.shape_y)
        _, counts = np.unique(fx[inside] * cfg.shape_y + fy[inside], return_counts=True)
        total += int(inside.sum())
        losers += int((counts - 1).sum())
    return total, losers


def device_grid(h, cfg, device, dtype="f64", pad=None):
    return occupancy_grid(to_dev(h, device, dtype, pad), RoadNetwork(LANES), P, cfg).cpu().numpy()


# ------------------------------------------------------------------ a. the standalone kernel
@pytest.mark.parametrize("case", list(GRID_CASES))
@pytest.mark.parametrize("kind,n,seed,steps", GRID_SCENES, ids=[scene_name(*s[:3]) for s in GRID_SCENES])
def test_grid_cases_on_golden_states_equal_the_reference_observer(kind, n, seed, steps, case, hip_device):
    """f64 grid_obs_kernel == the reference OccupancyGridObservation's recorded output and the
    oracle, bit for bit, on every policy step of the scene (curved roads included)."""
    d = load_golden(golden_files(scene_name(kind, n, seed) + ".npz")[0])
    ref = load_golden(golden_files(f"obsref_grid_{scene_name(kind, n, seed)}.npz")[0])[case]
    lanes = _abi.lane_table_from_arrays(d["lane_table"])
    cfg, net, o = cfg_of(case), RoadNetwork(lanes), Oracle(lanes, P)
    for p in range(steps + 1):
        h = HostState.from_golden(d, 15 * p)
        got = occupancy_grid(to_dev(h, hip_device), net, P, cfg).cpu().numpy()[0]
        assert np.array_equal(got, ref[p]), (p, np.argwhere(got != ref[p])[:5])
        assert np.array_equal(got, o.observe_grid(h, cfg)[0])


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("n,pad", BATCHES)
def test_grid_cases_on_random_batch_equal_the_oracle(n, pad, case, hip_device):
    """f64, slots padded, blocks of 64 / 128 / 256 threads: bit-identical to the oracle.  The
    coarse grid must really have contested cells, the observer-free one a vehicle in view."""
    h, cfg = batch(n), cfg_of(case)
    if case == "coarse":
        crowd(h)
    want = Oracle(LANES, P).observe_grid(h, cfg)
    feats = CASES[case]["features"]
    occupied = int(want[:, feats.index("presence")].sum())
    assert occupied > h.E // 2, "a grid that sees next to nothing checks nothing"
    if case == "coarse":  # the lowest-slot-wins rule decides some cells: the oracle shows fewer than are inside
        inside, losers = contested_cells(h, cfg)
        assert losers > 0 and occupied == inside - losers, (occupied, inside, losers)
    if "on_road" in feats:
        layer = want[:, feats.index("on_road")]
        assert layer.min() == 0 and layer.max() == 1
    got = device_grid(h, cfg, hip_device, pad=pad)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


# ------------------------------------------------------------------ b. state edits
@pytest.mark.parametrize("case", ["wide_road", "tall_noclip", "odd_road", "coarse"])
@pytest.mark.parametrize("edit", ["moved", "absent", "moved+absent"])
@pytest.mark.parametrize("n,pad,slot", [(100, 128, 70), (200, 256, 130)])
def test_grid_after_state_edits_equals_the_oracle(n, pad, slot, edit, case, hip_device):
    """The observer in a slot other than 0 (the tid == ego % nt hand-off through LDS: every launch
    has a thread per slot, so the observer's own thread passes it on -- thread 70 of a 128-thread
    block, thread 130 of 256, neither in the first wave), a fifth of the slots absent between
    present ones, and env 5 without a controlled vehicle (an all-zero grid): f64 bit-identical."""
    h, cfg = batch(n), cfg_of(case)
    if case == "coarse":
        crowd(h)
    if "moved" in edit:
        move_observer(h, slot)
    if "absent" in edit:
        punch_absent(h, n)
    h["kind"][5][h["kind"][5] == _abi.MDP] = _abi.IDM
    want = Oracle(LANES, P).observe_grid(h, cfg)
    assert not want[5].any() and want[4].any() and want[6].any()
    got = device_grid(h, cfg, hip_device, pad=pad)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


# ------------------------------------------------------------------ c. float32
def f32_excused_fraction(h, cfg):
    """(oracle grid on the float32-rounded inputs, its margins, the fraction of cells with a
    float64 cell-floor margin below F32_MARGIN) -- CPU only."""
    want, m = Oracle(LANES, P).observe_grid(f32_inputs(h), cfg, margins=True)
    return want, m, float(np.mean(m < F32_MARGIN))


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("n,pad", BATCHES)
def test_grid_cases_on_random_batch_f32(n, pad, case, hip_device):
    """f32 grid_obs_kernel against the oracle on the float32-rounded state: every cell within
    F32_TOL except where the oracle's float64 cell-floor margin is below F32_MARGIN, and such cells
    are at most F32_EXCUSED_CAP of the configuration's (counted on the CPU before the launch; the
    worst of these batches is 0.09 %, col_40x1 at n = 200)."""
    h, cfg = batch(n), cfg_of(case, F32_SHIFT)
    if case == "coarse":
        crowd(h)
    h = f32_inputs(h)
    want, m, excused = f32_excused_fraction(h, cfg)
    assert excused <= F32_EXCUSED_CAP, excused
    got = device_grid(h, cfg, hip_device, "f32", pad)
    off = np.abs(got - want) > F32_TOL
    bad = off & ~(m < F32_MARGIN)
    assert not np.any(bad), (int(off.sum()), np.argwhere(bad)[:5])


# ------------------------------------------------------------------ d. the fused step
def _diag():
    lib = _lib.load()
    f = lib.ttrl_diag_grid_step_lds
    f.restype, f.argtypes = C.c_long, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
    v = lib.ttrl_diag_view_bytes
    v.restype, v.argtypes = C.c_long, [C.c_int32] * 6
    return f, v


def fused_lds(dtype, slots, cfg, n_veh):
    """LDS bytes of ttrl_env_step_grid's fused launch, 0: it takes two launches."""
    return _diag()[0](_abi.F64 if dtype == "f64" else _abi.F32, slots, C.byref(cfg), n_veh)


def view_bytes(dtype, slots):
    """The sorted straight one-env view the fused launch starts from (STRAIGHT_LANE_CAP = 4 lanes)."""
    return _diag()[1](_abi.F64 if dtype == "f64" else _abi.F32, 1, slots, 4, 0, 1)


def scratch_bytes(cfg, n_veh, real):
    """grid_scratch_bytes (csrc/ttrl_mi355x.hip): winners and road bits, feature values, the observer."""
    c = cfg.shape_x * cfg.shape_y
    return ((4 * c + 4 * ((c + 31) // 32) + 15) & ~15) + ((4 * cfg.n_features * n_veh + 15) & ~15) + 6 * real + 16


def square(w, h=None, features=("presence", "on_road", "vx")):
    """A w x h grid of 1 m cells centred on the observer."""
    h = h or w
    return _abi.grid_cfg(features=list(features), grid_size=[[-w / 2, w / 2], [-h / 2, h / 2]], grid_step=[1, 1])


def widest_fused(dtype, slots, n_veh):
    """The largest W for which a W x 128 grid of 3 features still takes the fused launch."""
    fits = [w for w in range(1, 256) if fused_lds(dtype, slots, square(w, 128), n_veh)]
    assert fits and fits == list(range(1, fits[-1] + 1)) and fits[-1] < 255
    return fits[-1]


def tier_cfg(tier, dtype, slots, n_veh):
    """The grid of an LDS tier, with the tier asserted as the test's precondition."""
    real = 8 if dtype == "f64" else 4
    if tier == "inside the view":
        cfg = G7 if fused_lds(dtype, slots, G7, n_veh) == view_bytes(dtype, slots) else GR
        assert fused_lds(dtype, slots, cfg, n_veh) == view_bytes(dtype, slots)
    elif tier == "grown block":
        cfg = square(64)
        assert view_bytes(dtype, slots) < fused_lds(dtype, slots, cfg, n_veh) <= 64 * 1024
    elif tier == "widest fused":
        cfg = square(widest_fused(dtype, slots, n_veh), 128)
        assert 60 * 1024 < fused_lds(dtype, slots, cfg, n_veh) <= 64 * 1024
    elif tier == "first unfused":
        cfg = square(widest_fused(dtype, slots, n_veh) + 1, 128)
        assert fused_lds(dtype, slots, cfg, n_veh) == 0
    else:
        cfg = cfg_of("big")
        assert tier == "big" and fused_lds(dtype, slots, cfg, n_veh) == 0
        assert 64 * 1024 < scratch_bytes(cfg, n_veh, real) <= GRID_LDS_CAP
    return cfg


def step_once(dev, acts, cfg):
    """One 15-frame env.step on ``dev``: (grid, time, reward, terminated, truncated, components,
    ego speed, ego crashed); cfg None: the Kinematics-free ttrl_env_step, then the grid kernel is
    the caller's."""
    road = BatchedRoad(RoadNetwork(LANES), dev, P)
    time = torch.zeros(dev.n_envs, dtype=torch.float64, device=dev.device)
    obs, _, *outs = road.env_step(torch.from_numpy(acts), 15, 1 / 15, None, _abi.reward_cfg(), time, 1.0,
                                  grid_cfg=cfg)
    return obs, time, outs


TIERS = ["inside the view", "grown block", "widest fused", "first unfused", "big"]
STEP_SHAPES = [(40, 48, 64, 0), (100, 128, 128, 0), (40, 48, 64, 37), (100, 128, 128, 70)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("n,pad,slots,ego", STEP_SHAPES, ids=["64", "128", "64-ego37", "128-ego70"])
def test_fused_step_grid_at_every_lds_tier(n, pad, slots, ego, tier, dtype, hip_device):
    """ttrl_env_step_grid after one 15-frame step with random actions, on straight roads of 64 and
    128 slots, the observer in slot 0 or moved (slot 70 of 128 sits in the second wave of the LDS
    view): the grid == oracle simulate + observe_grid bit for bit (f64) and == the two-launch
    path's bit for bit (both dtypes); state, time, reward, dones, components and info == the
    Kinematics-free ttrl_env_step's."""
    E = 12
    h = batch(n, E)
    if ego:
        move_observer(h, ego)
    if dtype == "f32":
        h = f32_inputs(h)
    cfg = tier_cfg(tier, dtype, slots, pad)
    acts = np.random.default_rng(slots + ego).integers(0, 5, E).astype(np.int32)
    a, b = to_dev(h, hip_device, dtype, pad), to_dev(h, hip_device, dtype, pad)
    grid, time, outs = step_once(a, acts, cfg)
    none, time_b, outs_b = step_once(b, acts, None)
    grid_b = occupancy_grid(b, RoadNetwork(LANES), P, cfg)
    torch.cuda.synchronize()
    assert none.numel() == 0 and tuple(grid.shape) == (E, cfg.n_features, cfg.shape_x, cfg.shape_y)
    assert torch.equal(grid, grid_b)
    for k in a.t:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(time, time_b) and bool((time == 1.0).all())
    for x, y in zip(outs, outs_b):
        assert torch.equal(x, y)
    assert float(grid[:, 0].sum()) >= E  # every observer is in its own grid (presence is layer 0)
    if dtype == "f64":
        o = Oracle(LANES, P)
        o.simulate(h, acts, 15, 1 / 15)
        want = o.observe_grid(h, cfg)
        got = grid.cpu().numpy()
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        assert np.array_equal(a.to_numpy()["lane"][:, :n], h["lane"])


def test_env_with_a_128_x_128_grid_steps_by_default(hip_device):
    """VecHighwayEnv with the `big` OccupancyGrid and the default fuse_grid: env.step runs (two
    launches inside ttrl_env_step_grid) and returns the oracle's observation."""
    from topotrafficrl_amd.envs import VecHighwayEnv
    E, N = 8, 64
    env = VecHighwayEnv({"num_envs": E, "vehicles_count": N, "device": "cuda:0", "dtype": "f64",
                         "observation": dict(GRID_CASES["big"], type="OccupancyGrid")})
    assert env.config["fuse_grid"] and fused_lds("f64", 64, env.observation_type.cfg, N) == 0
    obs, _ = env.reset(seed=40)
    o = Oracle(env.network.table, env.params)
    h = HostState(E, N)
    o.reset_highway(h, env.reset_cfg, [40 + e for e in range(E)])
    cfg = cfg_of("big")
    assert np.array_equal(obs.cpu().numpy(), o.observe_grid(h, cfg))
    acts = np.array([0, 1, 2, 3, 4, 1, 3, 0])
    obs, rew, term, trunc, _ = env.step(torch.from_numpy(acts))
    o.simulate(h, acts.astype(np.int32), 15, 1 / 15)
    assert np.array_equal(obs.cpu().numpy(), o.observe_grid(h, cfg))
    ref_r, ref_term, ref_trunc = o.rewards(h, env.reward_cfg, 1.0)
    assert np.allclose(rew.cpu().numpy(), ref_r, atol=1e-6) and np.array_equal(term.cpu().numpy(), ref_term)


# ------------------------------------------------------------------ e. the caps
def largest_square(n_veh, n_features, real=8):
    """The largest W x W grid whose scratch ttrl_observe_grid accepts (grid_scratch_bytes' formula)."""
    probe = _abi.GridCfg()
    probe.n_features = n_features
    w = 1
    while True:
        probe.shape_x = probe.shape_y = w + 1
        if scratch_bytes(probe, n_veh, real) > GRID_LDS_CAP:
            return w
        w += 1


def test_grid_beyond_the_cap_is_refused_before_anything_runs(hip_device):
    """A grid whose scratch exceeds 160 KB: TTRL_E_UNSUPPORTED from ttrl_observe_grid and from
    ttrl_env_step_grid, which leaves x, time and reward untouched (nothing was launched)."""
    E, n = 8, 100
    h = batch(n, E)
    st = to_dev(h, hip_device, pad_to=128)
    w = largest_square(128, 3)
    cfg = square(w + 1)
    assert scratch_bytes(cfg, 128, 8) > GRID_LDS_CAP >= scratch_bytes(square(w), 128, 8)
    lib = _lib.load()
    R, PP, RC = C.byref(LANES), C.byref(P), C.byref(_abi.reward_cfg())
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((E, 3, w + 1, w + 1), -7.0, device=hip_device)
    assert lib.ttrl_observe_grid(C.byref(st.struct()), R, PP, C.byref(cfg), out.data_ptr(), stream) == E_UNSUPPORTED
    x0 = st["x"].clone()
    time = torch.full((E,), 3.0, dtype=torch.float64, device=hip_device)
    rew, comp = torch.full((E,), -7.0, device=hip_device), torch.zeros((E, 4), device=hip_device)
    te, tr, cr = (torch.zeros(E, dtype=torch.uint8, device=hip_device) for _ in range(3))
    sp = torch.zeros(E, dtype=torch.float64, device=hip_device)
    acts = torch.ones(E, dtype=torch.int32, device=hip_device)
    rc = lib.ttrl_env_step_grid(C.byref(st.struct()), R, PP, acts.data_ptr(), 15, 1 / 15, C.byref(cfg), out.data_ptr(),
                                RC, time.data_ptr(), 1.0, rew.data_ptr(), te.data_ptr(), tr.data_ptr(),
                                comp.data_ptr(), sp.data_ptr(), cr.data_ptr(), None, 0, stream)
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED
    assert torch.equal(st["x"], x0) and bool((time == 3.0).all()) and bool((rew == -7.0).all())
    assert bool((out == -7.0).all())


def test_largest_grid_under_the_cap_equals_the_oracle(hip_device):
    """The largest square grid ttrl_observe_grid accepts for 128 slots and 3 features (just under
    160 KB of dynamic LDS in one workgroup) runs and equals the oracle, f64 bit for bit."""
    E, n = 8, 100
    h = batch(n, E)
    w = largest_square(128, 3)
    cfg = square(w)
    assert cfg.shape_x == cfg.shape_y == w > 190
    want = Oracle(LANES, P).observe_grid(h, cfg)
    assert want[:, 0].sum() >= 3 * E and want[:, 1].min() == 0 and want[:, 1].max() == 1
    got = device_grid(h, cfg, hip_device, pad=128)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
