"""The C-ABI boundary on CPU: the HIP library loads, exports every entry point that
include/ttrl_mi355x.h declares, the ctypes mirror matches the C struct layouts, and
argument errors come back as TTRL_E_ARG before any device work.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from topotrafficrl_amd import _abi, _lib

HEADER = os.path.join(ROOT, "include", "ttrl_mi355x.h")


def declared():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^(?:int|int64_t) (ttrl_\w+)\(", txt, re.M)))


def test_library_loads_and_exports_every_declared_symbol():
    lib = _lib.load()
    assert lib.ttrl_abi_version() == 8
    names = declared()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (ttrl_\w+)", out))
    assert set(names) <= exported
    assert set(_lib.EXPORTS) == set(names)


def test_ctypes_mirror_matches_c_layout(tmp_path):
    structs = {"ttrl_lane_table_t": _abi.LaneTable, "ttrl_params_t": _abi.Params, "ttrl_state_t": _abi.State,
               "ttrl_kin_cfg_t": _abi.KinCfg, "ttrl_grid_cfg_t": _abi.GridCfg, "ttrl_reset_cfg_t": _abi.ResetCfg,
               "ttrl_reward_cfg_t": _abi.RewardCfg, "ttrl_ttc_cfg_t": _abi.TtcCfg, "ttrl_lidar_cfg_t": _abi.LidarCfg,
               "ttrl_ix_cfg_t": _abi.IxCfg}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ttrl_mi355x.h"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                  check=True).stdout.split("\n") if line)
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)


def test_argument_errors_need_no_device():
    lib = _lib.load()
    lanes = _abi.straight_lane_table(4)
    p = _abi.default_params()
    assert lib.ttrl_simulate(None, C.byref(lanes), C.byref(p), None, 15, 1 / 15, None) == -1
    s = _abi.State()  # null buffers
    s.n_envs, s.n_veh, s.dtype = 4, 64, _abi.F64
    assert lib.ttrl_road_act(C.byref(s), C.byref(lanes), C.byref(p), None) == -1
    s.dtype = 7
    assert lib.ttrl_road_step(C.byref(s), C.byref(lanes), C.byref(p), 0.1, None) == -1
    bad = _abi.straight_lane_table(4)
    bad.n_lanes = 99
    s.dtype = _abi.F64
    assert lib.ttrl_neighbours(C.byref(s), C.byref(bad), None, None, None, None) == -1
    # the intersection entry points need the network fields and np_random (state.rng)
    from topotrafficrl_amd.intersection import VecIntersectionEnv, intersection_network, ix_cfg
    net = intersection_network()
    cfg = ix_cfg(net, VecIntersectionEnv.default_config(), p)
    words = (C.c_uint32 * 4)(1, 2, 3, 4)
    assert lib.ttrl_ix_reset(C.byref(s), C.byref(net.table), C.byref(p), C.byref(cfg), words, 1, None, None) == -1
    assert lib.ttrl_ix_clear_spawn(C.byref(s), C.byref(net.table), C.byref(p), C.byref(cfg), None, None) == -1
    kin = _abi.kin_cfg(order="shuffled", shuffle_rng="np_random")
    assert lib.ttrl_observe_kinematics_masked(C.byref(s), C.byref(lanes), C.byref(p), C.byref(kin), None, None,
                                              None, None) == -1


def test_product_refuses_to_run_without_hip_library(tmp_path):
    with pytest.raises(ImportError):
        _lib.load(str(tmp_path / "missing.so"))


def test_product_refuses_cpu_tensors():
    import torch
    from topotrafficrl_amd.road import BatchedRoad, RoadNetwork
    from topotrafficrl_amd.state import BatchState
    st = BatchState(2, 8, device="cpu")
    road = BatchedRoad(RoadNetwork.straight_road_network(4), st)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        road.act()
    with pytest.raises(RuntimeError):
        road.simulate(torch.zeros(2, dtype=torch.int32))


def test_device_seeding_matches_numpy_seedsequence():
    """ttrl_seed_pcg64 (the SeedSequence -> PCG64 seeding the reset kernel runs on the device)
    equals numpy's np.random.PCG64(SeedSequence(entropy)) state for single and multi-word entropy."""
    import numpy as np
    lib = _lib.load()
    rng = np.random.default_rng(0)
    cases = [[0], [1], [12345], [2 ** 32 - 1], [5, 0, 1], [7, 3, 2], list(rng.integers(0, 2 ** 32, 6))]
    cases += [list(rng.integers(0, 2 ** 32, k)) for k in (1, 2, 3, 4, 5, 9)]
    for ent in cases:
        w = np.asarray(ent, dtype=np.uint32)
        out = np.zeros(4, dtype=np.uint64)
        assert lib.ttrl_seed_pcg64(w.ctypes.data, len(w), out.ctypes.data) == 0
        assert np.array_equal(out, _abi.pcg64_states([[int(v) for v in ent]])[0]), ent
    assert lib.ttrl_seed_pcg64(None, 1, None) == -1


def test_view_budgets_fit_the_residency_they_are_sized_for():
    """LDS bytes per workgroup of the simulate kernel's views (ttrl_diag_view_bytes): the straight
    highway's float64 64-slot env fits 16 workgroups per CU (4 waves per SIMD, 160 KB LDS), the
    intersection's float64 road network (2 envs x 32 slots, 20 lanes; capped list rows and float32
    trajectory prefilters) fits 8 (2 waves per SIMD: a 4096-env batch in one round)."""
    lib = _lib.load()
    f = lib.ttrl_diag_view_bytes
    f.restype = C.c_long
    f.argtypes = [C.c_int32] * 6
    assert f(_abi.F64, 1, 64, 4, 0, 1) * 16 <= 160 * 1024
    assert f(_abi.F64, 2, 32, 20, 1, 0) * 8 <= 160 * 1024
    assert f(_abi.F32, 2, 32, 20, 1, 0) * 8 <= 160 * 1024


# ------------------------------------------------------------------ the host layer's return codes
# Every extern "C" entry point under one fault at a time: a valid host-side baseline (every field
# pointer of the states at one dummy host buffer -- validation never dereferences them), one
# mutation, the exact code.  Every expected code but the empty batch's TTRL_OK is non-zero, so a
# case that slipped through to a launch shows as 0 or TTRL_E_LAUNCH.  The table runs in a child
# process (ctypes only) with no visible device.
OK, E_ARG, E_UNSUPPORTED = 0, -1, -3
N_ENVS, N_VEH, SPARE_K = 4, 24, 2
REQUIRED = _abi.REAL_FIELDS + _abi.I32_FIELDS + _abi.U8_FIELDS  # the 18 rows every entry needs

_RUN = ["s", "road", "p"]
_IX = ["s", "net", "p", "cfg"]
_REW = ["reward_cfg", "time", "time_inc", "reward", "terminated", "truncated", "components", "ego_speed",
        "ego_crashed"]
ENTRIES = {
    "ttrl_meta_action": _RUN + ["actions", "stream"],
    "ttrl_road_act": _RUN + ["stream"],
    "ttrl_road_step": _RUN + ["dt", "stream"],
    "ttrl_simulate": _RUN + ["actions", "frames", "dt", "stream"],
    "ttrl_diag_simulate": _RUN + ["actions", "frames", "dt", "ablate", "stream"],
    "ttrl_env_step": _RUN + ["actions", "frames", "dt", "kin", "obs", "obs_ids"] + _REW
                     + ["order", "action_lut", "n_action_lut", "stream"],
    "ttrl_env_step_grid": _RUN + ["actions", "frames", "dt", "grid_cfg", "grid"] + _REW
                          + ["action_lut", "n_action_lut", "stream"],
    "ttrl_neighbours": ["s", "road", "query_lane", "front", "rear", "stream"],
    "ttrl_observe_kinematics": _RUN + ["kin", "obs", "obs_ids", "stream"],
    "ttrl_observe_kinematics_masked": _RUN + ["kin", "mask", "obs", "obs_ids", "stream"],
    "ttrl_observe_grid": _RUN + ["grid_cfg", "grid", "stream"],
    "ttrl_observe_ttc": _RUN + ["ttc", "out", "stream"],
    "ttrl_observe_lidar": _RUN + ["lidar", "out", "stream"],
    "ttrl_reset_highway": _RUN + ["rcfg", "pcg", "stream"],
    "ttrl_reset_highway_seeded": _RUN + ["rcfg", "entropy", "n_words", "mask", "stream"],
    "ttrl_auto_reset_highway": _RUN + ["rcfg", "entropy", "n_words", "episode_word", "terminated", "truncated", "time",
                                       "done", "stream"],
    "ttrl_rewards": ["s", "road", "reward_cfg", "time", "reward", "terminated", "truncated", "stream"],
    "ttrl_rewards_ex": ["s", "road", "reward_cfg", "time", "reward", "terminated", "truncated", "components",
                        "stream"],
    "ttrl_rewards_step": ["s", "road"] + _REW + ["stream"],
    "ttrl_ix_reset": _IX + ["entropy", "n_words", "mask", "stream"],
    "ttrl_ix_reset_parts": _IX + ["parts", "entropy", "n_words", "mask", "mask", "warm_frames", "mask", "stream"],
    "ttrl_ix_clear_spawn": _IX + ["mask", "stream"],
    "ttrl_ix_step_tail": _IX + ["spare", "terminated", "truncated", "spare_parity", "entropy", "spare_entropy",
                                "n_words", "time", "done", "spare_mask", "kin", "obs", "obs_next", "obs_ids",
                                "ids_next", "live_count", "order", "stream"],
    "ttrl_ix_env_step": _IX + ["actions", "frames", "dt", "kin", "obs", "obs_ids", "obs_next", "ids_next"] + _REW
                        + ["spare", "spare_parity", "entropy", "spare_entropy", "n_words", "done", "spare_mask",
                           "order", "action_lut", "n_action_lut", "live_count", "stream"],
}
# ... and the two that take no state / lane table pair
ARGS = dict(ENTRIES, ttrl_copy_envs=["dst", "src", "mask", "stream"], ttrl_seed_pcg64=["entropy", "n_words", "pcg"])
IX_ENTRIES = [e for e, a in ENTRIES.items() if "net" in a]
_INTS = {"frames": 15, "n_action_lut": 5, "n_words": 4, "episode_word": 3, "parts": 7, "warm_frames": 3, "ablate": 0}
_REALS = {"dt": 1 / 15, "time_inc": 1.0}
_DIAG_SIGS = {"ttrl_diag_simulate": [C.c_void_p] * 4 + [C.c_int32, C.c_double, C.c_int32, C.c_void_p]}


def _baseline(blob):
    """A valid argument set for every entry point; ``blob``: the intersection's lane table and
    scene cfg as bytes (built by the parent: the child imports no torch)."""
    buf = (C.c_uint8 * 4096)()
    ptr = C.addressof(buf)

    def state(n_envs):
        s = _abi.State()
        s.n_envs, s.n_veh, s.dtype = n_envs, N_VEH, _abi.F64
        for f in _abi.ALL_FIELDS:
            setattr(s, f, ptr)
        return s

    n = C.sizeof(_abi.LaneTable)
    road = _abi.straight_lane_table(4)
    a = {k: ptr for names in ARGS.values() for k in names}
    a.update(_INTS)
    a.update(_REALS)
    a.update(_keep=buf, stream=None, s=state(N_ENVS), spare=state(SPARE_K * N_ENVS), dst=state(N_ENVS),
             src=state(N_ENVS), road=road, p=_abi.default_params(), net=_abi.LaneTable.from_buffer_copy(blob[:n]),
             cfg=_abi.IxCfg.from_buffer_copy(blob[n:]), kin=_abi.kin_cfg(), grid_cfg=_abi.grid_cfg(),
             rcfg=_abi.reset_cfg(N_VEH, road), reward_cfg=_abi.reward_cfg(), ttc=_abi.ttc_cfg(),
             lidar=_abi.lidar_cfg(), action_lut=(C.c_int32 * 8)(0, 1, 2, 3, 4, 1, 1, 1))
    return a


def _set(obj, field, val, *idx):
    def m(a):
        if not idx:
            return setattr(a[obj], field, val)
        arr = getattr(a[obj], field)
        for i in idx[:-1]:
            arr = arr[i]
        arr[idx[-1]] = val
    return m


def _arg(**kv):
    return lambda a: a.update(kv)


def _lut(q, v):
    return lambda a: a["action_lut"].__setitem__(q, v)


def _n_veh(n):  # the spare scenes follow the state's shape
    return lambda a: (setattr(a["s"], "n_veh", n), setattr(a["spare"], "n_veh", n))


def _both(*ms):
    return lambda a: [m(a) for m in ms]


def _empty(entry):
    """n_envs = 0 with nothing else valid: no rows, no lanes, every other argument null."""
    def m(a):
        road = "net" if entry in IX_ENTRIES else "road"
        s = _abi.State()
        s.n_veh, s.dtype = N_VEH, _abi.F64
        a["s"] = s
        a[road] = _abi.LaneTable()
        for k in ENTRIES[entry]:
            if k not in ("s", road):
                a[k] = 0 if k in _INTS else 0.0 if k in _REALS else None
    return m


def _fault_cases(blob):
    """[(id, entry, mutation, expected code)]"""
    base = _baseline(blob)
    cases = []

    def add(entry, name, m, want=E_ARG):
        cases.append((f"{entry}:{name}", entry, m, want))

    for n, (e, args) in enumerate(ENTRIES.items()):
        ix = e in IX_ENTRIES
        road = "net" if ix else "road"
        has = lambda k: k in args  # noqa: E731

        # ---- the state, the lanes and the roads (check_state)
        add(e, "s null", _arg(s=None))
        add(e, "road null", _arg(**{road: None}))
        add(e, "dtype", _set("s", "dtype", 7))
        for v in (0, 257):
            add(e, f"n_veh {v}", _set("s", "n_veh", v))
        add(e, "n_envs -1", _set("s", "n_envs", -1))
        for v in (0, _abi.MAX_LANES + 1):
            add(e, f"n_lanes {v}", _set(road, "n_lanes", v))
        for v in (0, _abi.MAX_ROADS + 1):
            add(e, f"n_roads {v}", _set(road, "n_roads", v))
        add(e, "regulation_frequency -1", _set(road, "regulation_frequency", -1))
        add(e, "lane 1 of no road", _set(road, "road", -1, 1))
        add(e, "lane 1 of a road past n_roads", _set(road, "road", base[road].n_roads, 1))
        add(e, "lane 1 not at road_first + lane_id", _set(road, "lane_id", 1 if ix else 0, 1))
        add(e, "lane 0 past its road's lanes", _set(road, "road_n", 0, 0))
        fields = REQUIRED if e == "ttrl_simulate" else [REQUIRED[n % len(REQUIRED)]]
        for f in fields:
            add(e, f"{f} null", _set("s", f, None))
        graph = (lambda a: None) if ix else _set(road, "regulation_frequency", 2)
        fields = _abi.NET_FIELDS if ix or e == "ttrl_simulate" else [_abi.NET_FIELDS[n % len(_abi.NET_FIELDS)]]
        for f in fields:
            add(e, f"graph road, {f} null", _both(graph, _set("s", f, None)))

        # ---- the empty batch: TTRL_OK before any other argument is looked at
        first = {"ttrl_meta_action": "actions", "ttrl_ix_reset": "cfg"}.get(e)  # a null check ahead of check_state
        if first:
            add(e, f"empty batch, {first} null", _empty(e))
            add(e, "empty batch", _both(_empty(e), _arg(**{first: base[first]})), OK)
        else:
            add(e, "empty batch", _empty(e), OK)
        for f, v in (("dtype", 7), ("n_veh", 0), ("n_veh", 257)):
            add(e, f"empty batch, {f} {v}", _both(_empty(e), _arg(**{first: base[first]}) if first else _arg(),
                                                  _set("s", f, v)))

        # ---- params
        if has("p"):
            add(e, "p null", _arg(p=None))
        shapes = (N_VEH, 64, 100) if e == "ttrl_env_step_grid" else (N_VEH,)  # two launches; fused 64, 128 slots
        if has("p") and not e.startswith(("ttrl_observe_kin", "ttrl_observe_grid", "ttrl_observe_lidar")):
            for nv in shapes:
                for v in (0, 9):
                    add(e, f"n_veh {nv}, n_target_speeds {v}", _both(_n_veh(nv), _set("p", "n_target_speeds", v)))
        if has("frames") and e != "ttrl_ix_env_step":
            for nv in shapes:
                add(e, f"n_veh {nv}, frames -1", _both(_n_veh(nv), _arg(frames=-1)))
                add(e, f"n_veh {nv}, p null", _both(_n_veh(nv), _arg(p=None)))

        # ---- the action LUT
        if has("action_lut"):
            for nv in shapes:
                w = f"n_veh {nv}, "
                for v in (-1, 9):
                    add(e, w + f"n_action_lut {v}", _both(_n_veh(nv), _arg(n_action_lut=v)))
                add(e, w + "lut null", _both(_n_veh(nv), _arg(action_lut=None)))
                for q, v in ((0, -1), (0, 5), (4, -1), (4, 5)):
                    add(e, w + f"lut[{q}] {v}", _both(_n_veh(nv), _lut(q, v)))

        # ---- the reward and observation arguments
        if has("reward_cfg"):
            for nv in shapes:
                w = f"n_veh {nv}, "
                for k in ("time", "reward", "terminated", "truncated"):
                    add(e, w + f"{k} null", _both(_n_veh(nv), _arg(**{k: None})))
                if has("ego_speed"):
                    add(e, w + "ego_speed alone", _both(_n_veh(nv), _arg(ego_crashed=None)))
                    add(e, w + "ego_crashed alone", _both(_n_veh(nv), _arg(ego_speed=None)))
            if e.startswith("ttrl_rewards") or e == "ttrl_ix_env_step":
                add(e, "reward_cfg null", _arg(reward_cfg=None))
        if has("kin"):
            if e == "ttrl_env_step":
                add(e, "obs_cfg without obs", _arg(obs=None))
                add(e, "obs without obs_cfg", _arg(kin=None))
            elif e != "ttrl_ix_step_tail":
                add(e, "obs_cfg null", _arg(kin=None))
                add(e, "obs null", _arg(obs=None))
            if e in ("ttrl_ix_step_tail", "ttrl_ix_env_step"):
                add(e, "obs_next null", _arg(obs_next=None))
                add(e, "obs_ids alone", _arg(ids_next=None))
                add(e, "ids_next alone", _arg(obs_ids=None))
            if e == "ttrl_ix_step_tail":
                add(e, "obs_in null", _arg(obs=None))
            kin = [("vehicles_count 0", _set("kin", "vehicles_count", 0)), ("n_features 0", _set("kin", "n_features", 0)),
                   ("n_features 15", _set("kin", "n_features", _abi.N_FEATURES + 1)),
                   ("order_shuffled -1", _set("kin", "order_shuffled", -1)),
                   ("order_shuffled 3", _set("kin", "order_shuffled", 3)),
                   ("np_random order without rng", _both(_set("kin", "order_shuffled", 2), _set("s", "rng", None))),
                   ("np_random order of 65 rows", _both(_set("kin", "order_shuffled", 2),
                                                        _set("kin", "vehicles_count", 66))),
                   ("feature -1", _set("kin", "features", -1, 0)),
                   ("feature on_road", _set("kin", "features", _abi.FEATURE_CODE["on_road"], 4))]
            for name, m in kin:
                add(e, name, m)
        if has("grid_cfg"):
            for nv in shapes:
                w = f"n_veh {nv}, "
                grid = [("grid_cfg null", _arg(grid_cfg=None)), ("grid null", _arg(grid=None)),
                        ("n_features 0", _set("grid_cfg", "n_features", 0)),
                        ("n_features 15", _set("grid_cfg", "n_features", _abi.N_FEATURES + 1)),
                        ("shape_x 0", _set("grid_cfg", "shape_x", 0)), ("shape_y 0", _set("grid_cfg", "shape_y", 0)),
                        ("step_x 0", _set("grid_cfg", "step_x", 0.0)), ("step_y -1", _set("grid_cfg", "step_y", -1.0)),
                        ("feature -1", _set("grid_cfg", "features", -1, 0)),
                        ("feature 14", _set("grid_cfg", "features", _abi.N_FEATURES, 3))]
                for name, m in grid:
                    add(e, w + name, _both(_n_veh(nv), m))

    # ---- a grid beyond the LDS cap, 160 KB of scratch: refused by the observer and, before it steps,
    # by the fused step (a grid over the fused launch's 64 KB takes two launches: tests/test_gpu_grid.py)
    add("ttrl_observe_grid", "200 x 200 cells", _both(_set("grid_cfg", "shape_x", 200), _set("grid_cfg", "shape_y", 200)),
        E_UNSUPPORTED)
    for nv in (64, 100):
        add("ttrl_env_step_grid", f"n_veh {nv}, 200 x 200 cells",
            _both(_n_veh(nv), _set("grid_cfg", "shape_x", 200), _set("grid_cfg", "shape_y", 200)), E_UNSUPPORTED)
    add("ttrl_diag_simulate", "ablate in a product build", _arg(ablate=1), E_UNSUPPORTED)
    add("ttrl_diag_simulate", "ablate, s null", _arg(ablate=1, s=None), E_UNSUPPORTED)
    add("ttrl_meta_action", "actions null", _arg(actions=None))
    for e in ("ttrl_neighbours",):
        add(e, "front null", _arg(front=None))
        add(e, "rear null", _arg(rear=None))

    # ---- resets
    resets = ("ttrl_reset_highway", "ttrl_reset_highway_seeded", "ttrl_auto_reset_highway")
    for e in resets:
        add(e, "cfg null", _arg(rcfg=None))
        for v in (0, N_VEH + 1):
            add(e, f"n_vehicles {v}", _set("rcfg", "n_vehicles", v))
        for v in (-1, 4):
            add(e, f"ego_lane {v}", _set("rcfg", "ego_lane", v))
    add(resets[0], "pcg null", _arg(pcg=None))
    for e, top in ((resets[1], 64), (resets[2], 8), ("ttrl_ix_reset", 64), ("ttrl_ix_reset_parts", 64),
                   ("ttrl_ix_step_tail", 65), ("ttrl_ix_env_step", 65)):
        add(e, "entropy null", _arg(entropy=None))
        add(e, "n_words 0", _arg(n_words=0, episode_word=0))
        add(e, f"n_words {top + 1}", _arg(n_words=top + 1))
    for k in ("terminated", "truncated", "time", "done"):
        add(resets[2], f"{k} null", _arg(**{k: None}))
    for v in (-1, 4):
        add(resets[2], f"episode_word {v} of 4", _arg(episode_word=v))
    # 65 words are within the spare-scene entries' bound: the later slot-class refusal is reached
    for e in ("ttrl_ix_step_tail", "ttrl_ix_env_step"):
        add(e, "n_veh 100, n_words 65", _both(_n_veh(100), _arg(n_words=65)), E_UNSUPPORTED)
        add(e, "n_veh 100, n_words 66", _both(_n_veh(100), _arg(n_words=66)))

    # ---- time to collision, lidar
    e = "ttrl_observe_ttc"
    add(e, "cfg null", _arg(ttc=None))
    add(e, "out null", _arg(out=None))
    for v in (0, 65):
        add(e, f"horizon_bins {v}", _set("ttc", "horizon_bins", v))
        add(e, f"raw, horizon_bins {v}", _both(_set("ttc", "obs_lanes", 0), _set("ttc", "obs_speeds", 0),
                                               _set("ttc", "horizon_bins", v)))
    for v in (0.0, -1.0, float("nan")):
        add(e, f"time_quantization {v}", _set("ttc", "time_quantization", v))
    add(e, "lanes window without a speeds window", _set("ttc", "obs_speeds", 0))
    add(e, "speeds window without a lanes window", _set("ttc", "obs_lanes", 0))
    add(e, "obs_lanes -1", _set("ttc", "obs_lanes", -1))
    add(e, "obs_speeds -1", _set("ttc", "obs_speeds", -1))
    e = "ttrl_observe_lidar"
    add(e, "cfg null", _arg(lidar=None))
    add(e, "out null", _arg(out=None))
    for v in (0, 65):
        add(e, f"cells {v}", _set("lidar", "cells", v))
    for v in (0.0, -1.0, float("nan")):
        add(e, f"maximum_range {v}", _set("lidar", "maximum_range", v))

    # ---- the intersection (check_ix)
    net, cfg = base["net"], base["cfg"]
    nd, k = next((i, j) for i in range(_abi.MAX_NODES) for j in range(4) if cfg.path_len[i][j] > 0)
    for e in IX_ENTRIES:
        add(e, "cfg null", _arg(cfg=None))
        add(e, "rng null", _set("s", "rng", None))
        add(e, "n_corners 3", _set("cfg", "n_corners", 3))
        for v in (0, _abi.IX_MAX_INIT + 1):
            add(e, f"initial_vehicle_count {v}", _set("cfg", "initial_vehicle_count", v))
        add(e, "warmup_frames -1", _set("cfg", "warmup_frames", -1))
        for v in (-1, net.n_lanes):
            add(e, f"ego_lane {v}", _set("cfg", "ego_lane", v))
            for c in (0, 3):
                add(e, f"entry_lane[{c}] {v}", _set("cfg", "entry_lane", v, c))
        for v in (-2, 4):
            add(e, f"ego_destination {v}", _set("cfg", "ego_destination", v))
        for v in (-1, _abi.MAX_NODES):
            for r in (0, net.n_roads - 1):
                add(e, f"road_from[{r}] {v}", _set("net", "road_from", v, r))
                add(e, f"road_to[{r}] {v}", _set("net", "road_to", v, r))
        add(e, "a path of ROUTE_MAX roads", _set("cfg", "path_len", _abi.ROUTE_MAX, nd, k))
        for v in (-1, net.n_roads):
            add(e, f"a path over road {v}", _set("cfg", "path_road", v, nd, k, 0))
    e = "ttrl_ix_reset_parts"
    for v in (-1, 8):
        add(e, f"parts {v}", _arg(parts=v))
    add(e, "warm_frames -1", _arg(warm_frames=-1))

    # ---- the spare scenes
    for e in ("ttrl_ix_step_tail", "ttrl_ix_env_step"):
        add(e, "spare null", _arg(spare=None))
        for kk in (1, 17):
            add(e, f"K {kk}", _set("spare", "n_envs", kk * N_ENVS))
        add(e, "spare rows no multiple of n_envs", _set("spare", "n_envs", SPARE_K * N_ENVS + 1))
        add(e, "spare n_veh", _set("spare", "n_veh", N_VEH + 1))
        add(e, "spare dtype", _set("spare", "dtype", _abi.F32))
        for f in REQUIRED + _abi.NET_FIELDS + ["rng"]:
            add(e, f"spare {f} null", _set("spare", f, None))
        for f in ("spare_parity", "spare_entropy", "done", "spare_mask") + (
                ("terminated", "truncated", "time") if e == "ttrl_ix_step_tail" else ()):
            add(e, f"{f} null", _arg(**{f: None}))
        for nv in (65, 100, 200):  # one wavefront per env: the 32 and 64 slot classes only
            add(e, f"n_veh {nv}", _n_veh(nv), E_UNSUPPORTED)
    e = "ttrl_ix_step_tail"  # the slot-class refusal comes with the observation's checks, ahead of their E_ARG
    add(e, "n_veh 100, bad obs_cfg", _both(_n_veh(100), _set("kin", "n_features", 0)), E_UNSUPPORTED)
    add(e, "n_veh 100, obs_out null", _both(_n_veh(100), _arg(obs_next=None)), E_UNSUPPORTED)
    add(e, "n_veh 100, spare dtype", _both(_n_veh(100), _set("spare", "dtype", _abi.F32)))
    e = "ttrl_ix_env_step"  # ... here after every null and range check, ahead of the LUT's codes
    add(e, "n_veh 100, n_action_lut 9", _both(_n_veh(100), _arg(n_action_lut=9)))
    add(e, "n_veh 100, reward null", _both(_n_veh(100), _arg(reward=None)))
    add(e, "n_veh 100, lut[0] 5", _both(_n_veh(100), _lut(0, 5)), E_UNSUPPORTED)

    # ---- ttrl_copy_envs: its own shape checks, then the empty batch, then the rows
    e = "ttrl_copy_envs"
    for k in ("dst", "src", "mask"):
        add(e, f"{k} null", _arg(**{k: None}))
    for side in ("dst", "src"):
        add(e, f"{side} n_envs", _set(side, "n_envs", N_ENVS + 1))
        add(e, f"{side} n_veh", _set(side, "n_veh", N_VEH + 1))
        add(e, f"{side} dtype", _set(side, "dtype", _abi.F32))
        for f in REQUIRED:
            add(e, f"{side} {f} null", _set(side, f, None))
        add(e, f"{side} alone without routes", _set(side, "route_road", None))
        for f in ("route_lane", "route_n", "yielding"):
            add(e, f"{side} {f} null", _set(side, f, None))
    for f, v in (("n_envs", -1), ("n_veh", 0), ("n_veh", 257), ("dtype", 7)):
        add(e, f"both {f} {v}", _both(_set("dst", f, v), _set("src", f, v)))
    empty = _both(_arg(dst=_abi.State(), src=_abi.State()), _set("dst", "n_veh", N_VEH), _set("src", "n_veh", N_VEH))
    add(e, "empty batch", empty, OK)
    add(e, "empty batch, mask null", _both(empty, _arg(mask=None)))
    add(e, "empty batch, n_veh", _both(empty, _set("src", "n_veh", N_VEH + 1)))
    add(e, "empty batch, dtype", _both(empty, _set("src", "dtype", _abi.F64)))
    add(e, "empty batch, n_veh 0", _both(empty, _set("dst", "n_veh", 0), _set("src", "n_veh", 0)))

    # ---- the host seeding helper
    for name, m in (("entropy null", _arg(entropy=None)), ("state null", _arg(pcg=None)), ("n_words 0", _arg(n_words=0)),
                    ("n_words 65", _arg(n_words=65))):
        add("ttrl_seed_pcg64", name, m)
    return cases


def _run_fault_table(blob):
    """The child's side: every case's return code, [[id, code]]."""
    lib = _lib.load()
    for name, sig in _DIAG_SIGS.items():
        getattr(lib, name).argtypes, getattr(lib, name).restype = sig, C.c_int
    out = []
    for cid, entry, mutate, _ in _fault_cases(blob):
        a = _baseline(blob)
        mutate(a)
        args = [C.byref(a[k]) if isinstance(a[k], C.Structure) else a[k] for k in ARGS[entry]]
        out.append([cid, getattr(lib, entry)(*args)])
    return out


def test_every_entry_point_returns_its_code_for_each_fault(tmp_path):
    import json
    import sys
    from topotrafficrl_amd.intersection import VecIntersectionEnv, intersection_network, ix_cfg
    net = intersection_network()
    blob = bytes(net.table) + bytes(ix_cfg(net, VecIntersectionEnv.default_config(), _abi.default_params()))
    (tmp_path / "ix.bin").write_bytes(blob)
    cases = _fault_cases(blob)
    want = {cid: code for cid, _, _, code in cases}
    assert len(want) == len(cases) > 1000  # ids are unique
    assert {cid.split(":")[0] for cid, code in want.items() if code == OK} == set(ENTRIES) | {"ttrl_copy_envs"}
    assert {cid.split(":")[0] for cid in want} == set(ARGS)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")  # a stray launch fails instead of running
    res = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) +
                         [os.path.abspath(__file__), str(tmp_path / "ix.bin")], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    got = dict(json.loads(res.stdout.splitlines()[-1]))
    assert set(got) == set(want)
    wrong = {cid: (got[cid], want[cid]) for cid in want if got[cid] != want[cid]}
    assert not wrong, f"{len(wrong)} of {len(want)} (case: (returned, expected)): {wrong}"


if __name__ == "__main__":  # the child of the test above: argv[1] holds the intersection's structs
    import json
    import sys
    print(json.dumps(_run_fault_table(open(sys.argv[1], "rb").read())))
