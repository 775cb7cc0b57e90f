"""Golden-vector generator for the MLP / dueling / convolutional value nets and the DQN update over
an MLP -- TEST INFRASTRUCTURE, runs only in the build container (it needs the reference checkout
that oracle/gen_golden_policy.py imports).

It runs the reference's own ``model_factory`` (models.py:431-441) on its agent configs
(scripts/configs/IntersectionEnv/agents/DQNAgent/baseline.json, grid.json, grid_convnet.json; a
DuelingNetwork with its default empty heads over a [128, 128] base) and its ``DQNAgent``
(deep_q_network/pytorch.py) and writes data only: ``tests/golden/qnet/qnet_*.npz`` (inputs, the
state dict, Q at several batch sizes) and ``tests/golden/dqn_mlp.npz``.  The network fixtures have a
directory of their own: tests/conftest.py's ``golden_files()`` takes every ``tests/golden/*.npz``
whose prefix it does not know for a road-frame scene.

``dqn_mlp.npz`` follows gen_golden_policy.gen_dqn with one difference: the target net's weights
are not stored after every step (nine copies of a 30 k-parameter net pass the size limit of a
committed file); ``s{step}/tw_step`` names the step whose value-net weights the reference's target
net equals bit for bit after that step (-1: the initial weights).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_qnet.py
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden_policy import OUT, R, _Env, agent_config, policy_inputs  # noqa: E402

QOUT = os.path.join(OUT, "qnet")
BATCHES = (1, 15, 16, 17, 37)
DUELING = {"type": "DuelingNetwork",
           "base_module": {"type": "MultiLayerPerceptron", "layers": [128, 128]},
           "value": {"type": "MultiLayerPerceptron", "layers": []},
           "advantage": {"type": "MultiLayerPerceptron", "layers": []}}


def grid_inputs(seed: int = 17, rows: int = 256) -> np.ndarray:
    """[rows, 7, 11, 11] float32 OccupancyGrid-like rows: about 10 % of the cells occupied
    (presence 1, the other features uniform in [-1, 1]), the rest zero; a few rows all zero."""
    rng = np.random.default_rng(seed)
    occ = rng.random((rows, 1, 11, 11)) < 0.1
    x = rng.uniform(-1, 1, size=(rows, 7, 11, 11))
    x[:, 0] = 1.0
    x = np.where(occ, x, 0.0).astype(np.float32)
    x[[3, 100, 255]] = 0.0
    return np.ascontiguousarray(x)


def build(model_cfg: dict, shape, n_actions: int, seed: int, bias_scale: float):
    cfg = copy.deepcopy(model_cfg)
    R.models.size_model_config(_Env(n_actions, shape), cfg)
    torch.manual_seed(seed)
    net = R.models.model_factory(cfg)
    if hasattr(net, "reset"):  # the convolutional net is a plain nn.Module: torch's default init
        net.reset()
    if bias_scale:  # as gen_golden_policy.build_network
        g = torch.Generator().manual_seed(seed + 1000)
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith("bias"):
                    p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bias_scale)
    return net.eval()


def gen_qnets():
    kin, grid = policy_inputs(), grid_inputs()
    variants = [  # (file, model config, inputs, actions, weight seed, bias scale)
        ("qnet_mlp_kin_a3", agent_config("baseline.json")["model"], kin, 3, 41, 0.1),
        ("qnet_mlp_kin_a5", agent_config("baseline.json")["model"], kin, 5, 42, 0.0),
        ("qnet_mlp_grid_a3", agent_config("grid.json")["model"], grid, 3, 43, 0.1),
        ("qnet_dueling_a5", DUELING, kin, 5, 44, 0.1),
        ("qnet_conv_a3", agent_config("grid_convnet.json")["model"], grid, 3, 45, 0.1),
    ]
    for fname, cfg, x, n_actions, seed, bias in variants:
        net = build(cfg, x.shape[1:], n_actions, seed, bias)
        out = {"x": x, "n_actions": np.int32(n_actions)}
        for k, v in net.state_dict().items():
            out["w/" + k] = v.numpy()
        with torch.no_grad():
            for b in BATCHES + (len(x),):
                out[f"q_b{b}"] = net(torch.from_numpy(x[:b])).numpy()
        os.makedirs(QOUT, exist_ok=True)
        path = os.path.join(QOUT, fname + ".npz")
        np.savez_compressed(path, **out)
        q = np.sort(out[f"q_b{len(x)}"], axis=1)
        print(fname, "params", sum(p.numel() for p in net.parameters()), "bytes", os.path.getsize(path),
              "clear share", float(np.mean(q[:, -1] - q[:, -2] > 1e-4)))


def gen_dqn_mlp():
    x = policy_inputs(seed=21)
    rng = np.random.default_rng(6)
    cfg = agent_config("baseline.json")
    cfg.update(device="cpu", double=True, target_update=2)
    torch.manual_seed(33)
    agent = R.dqn.DQNAgent(_Env(3), cfg)
    out = {"double": np.int32(1), "gamma": np.float64(agent.config["gamma"]),
           "lr": np.float64(agent.config["optimizer"]["lr"]), "target_update": np.int32(2)}
    history = {-1: {k: v.numpy().copy() for k, v in agent.value_net.state_dict().items()}}
    for k, v in history[-1].items():
        out["w0/" + k] = v
    B = agent.config["batch_size"]
    for step in range(4):
        idx = rng.choice(len(x), size=B, replace=False)
        nidx = rng.choice(len(x), size=B, replace=False)
        s, s2 = x[idx], x[nidx]
        a = rng.integers(0, 3, size=B)
        r = rng.uniform(0, 1, size=B)
        t = rng.random(B) < 0.25
        batch = R.memory.Transition(tuple(s), tuple(int(v) for v in a), tuple(float(v) for v in r),
                                    tuple(s2), tuple(bool(v) for v in t), tuple({} for _ in range(B)))
        loss, target, _ = agent.compute_bellman_residual(batch)
        agent.step_optimizer(loss)
        agent.update_target_network()
        out[f"s{step}/state"], out[f"s{step}/next_state"] = s, s2
        out[f"s{step}/action"], out[f"s{step}/reward"] = a.astype(np.int64), r.astype(np.float32)
        out[f"s{step}/terminal"] = t
        out[f"s{step}/loss"] = np.float32(loss.item())
        out[f"s{step}/target"] = target.numpy()
        history[step] = {k: v.numpy().copy() for k, v in agent.value_net.state_dict().items()}
        for k, v in history[step].items():
            out[f"s{step}/w/" + k] = v
        tw = {k: v.numpy() for k, v in agent.target_net.state_dict().items()}
        same = [n for n, w in history.items() if all(np.array_equal(w[k], tw[k]) for k in tw)]
        assert len(same) == 1, same
        out[f"s{step}/tw_step"] = np.int32(same[0])
    path = os.path.join(OUT, "dqn_mlp.npz")
    np.savez_compressed(path, **out)
    print("dqn_mlp", [float(out[f"s{i}/loss"]) for i in range(4)], [int(out[f"s{i}/tw_step"]) for i in range(4)],
          "bytes", os.path.getsize(path))


if __name__ == "__main__":
    torch.set_num_threads(1)  # deterministic CPU reductions for the fixtures
    gen_qnets()
    gen_dqn_mlp()
