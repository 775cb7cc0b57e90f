"""QNetworkPolicy.act through the fused launch (ttrl::mlp_act) against the same network through the
policy's torch path, on the same build: time per call at the two flagship observation shapes.

  python tools/qnet_bench.py [--envs 4096] [--rounds 7] [--calls 200]

Timing: HIP events on the current stream around ``calls`` back-to-back act() calls, after a warm-up
of both paths at the timed shape; ``rounds`` alternating windows per path in one process (the
median and the minimum are reported, and every window).  The torch path is the yardstick.  Launch
counts come from a separate profiler pass over one act() per path, after the timing.  One JSON
line per shape on stdout.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from topotrafficrl_amd.agent import QNetworkPolicy  # noqa: E402

SHAPES = [  # (label, observation shape, model config, actions)
    ("kinematics 15x7, MLP [128, 128]", (15, 7), {"type": "MultiLayerPerceptron", "layers": [128, 128]}, 3),
    ("grid 7x11x11, MLP [48, 48]", (7, 11, 11), {"type": "MultiLayerPerceptron", "layers": [48, 48]}, 3),
]


def window(fn, calls):
    """Microseconds per call over ``calls`` back-to-back calls (device events)."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / calls * 1e3


def launches(fn):
    """Device kernels one call enqueues (profiler pass; None where the profiler reports none)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qnet_bench needs a HIP device")
    dev = torch.device("cuda:0")
    for label, shape, model, n_actions in SHAPES:
        fused = QNetworkPolicy(dev, model, shape, n_actions=n_actions, seed=0)
        eager = QNetworkPolicy(dev, model, shape, n_actions=n_actions, seed=0, fused=False)
        g = torch.Generator(device=dev).manual_seed(1)
        obs = torch.rand((args.envs, *shape), device=dev, generator=g) * 2 - 1
        assert fused.fused_acting(obs) and not eager.fused_acting(obs)
        diff = float((fused.q_values(obs) - eager.q_values(obs)).abs().max())
        paths = {"fused": lambda: fused.act(obs, dtype=torch.int32), "torch": lambda: eager.act(obs, dtype=torch.int32)}
        for fn in paths.values():  # warm-up at the timed shape
            window(fn, 20)
        times = {k: [] for k in paths}
        for _ in range(args.rounds):  # alternating windows
            for k, fn in paths.items():
                times[k].append(window(fn, args.calls))
        row = {"shape": label, "envs": args.envs, "calls_per_window": args.calls, "max_abs_q_diff": diff}
        for k, v in times.items():
            row[k + "_us_median"], row[k + "_us_min"] = statistics.median(v), min(v)
            row[k + "_us_windows"] = [round(t, 2) for t in v]
        row["speedup_median"] = row["torch_us_median"] / row["fused_us_median"]
        for k, fn in paths.items():
            try:
                row[k + "_launches"] = launches(fn)
            except Exception as exc:  # the timing above stands; the count is reported as not measured
                row[k + "_launches"] = None
                row[k + "_launches_error"] = repr(exc)[:200]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
