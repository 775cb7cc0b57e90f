"""The fused MLP / dueling Q-network forward and acting (mlp_q_kernel, ttrl::mlp_q / ttrl::mlp_act)
on the GPU: against the reference's networks (tests/golden/qnet/), against float64 over every
padding path of the kernel, against its C ABI, against ego_attention_act's draws, captured in a
StepGraph and in the training loop.

Tolerance: rtol 1e-4 / atol 1e-5 on Q-values, the project's tolerance for float32 MFMA (an exact
fmaf chain) against the reference or float64.
"""
import itertools

import numpy as np
import pytest
import torch

from test_qnet import BASELINE, BATCHES, FUSED_FIXTURES, GRID, _duel, _mlp, _widths, fixture_network, load_qnet
from topotrafficrl_amd import _lib, ops
from topotrafficrl_amd.agent import EgoAttentionNetwork, QNetworkPolicy
from topotrafficrl_amd.trainer import BatchedDQNAgent, BatchedEvaluation

pytestmark = pytest.mark.gpu
KIN = {"type": "Kinematics", "vehicles_count": 15, "features": ["presence", "x", "y", "vx", "vy", "cos_h", "sin_h"],
       "features_range": {"x": [-100, 100], "y": [-100, 100], "vx": [-20, 20], "vy": [-20, 20]},
       "absolute": False, "order": "sorted"}


@pytest.mark.parametrize("name", FUSED_FIXTURES)
def test_fused_forward_matches_reference_network(name, hip_device):
    z = load_qnet(name)
    net = fixture_network(name, z, hip_device)
    assert net.fused_supported()
    for b in BATCHES + (len(z["x"]),):
        ref = z[f"q_b{b}"]
        q = net.fused_q(torch.from_numpy(z["x"][:b]).to(hip_device)).cpu().numpy()
        print(name, b, "max abs err", float(np.max(np.abs(q - ref))))
        np.testing.assert_allclose(q, ref, rtol=1e-4, atol=1e-5)
        srt = np.sort(ref, axis=1)
        clear = (srt[:, -1] - srt[:, -2]) > 1e-4
        assert (q.argmax(1)[clear] == ref.argmax(1)[clear]).all()


SWEEP_WIDTHS = ([16], [48, 48], [128, 128], [128, 48, 16], [64, 64, 64])


@pytest.mark.parametrize("inp", [1, 3, 4, 105, 847, 1024])
def test_shape_sweep_matches_float64(inp, hip_device):
    """Batch 37 (two full row tiles and a partial one), random weights with non-zero biases: K not a
    multiple of 4, a second staged chunk (in > 512), one / three / eight output tiles, a full
    16-column head and the extra dueling column."""
    g = torch.Generator().manual_seed(inp)
    x = torch.rand(37, inp, generator=g) * 2 - 1
    xd = x.to(hip_device)
    for widths, n_actions, dueling in itertools.product(SWEEP_WIDTHS, (1, 3, 5, 16), (False, True)):
        if dueling and n_actions > 15:
            continue
        net = _duel(n_actions, widths, (inp,)) if dueling else _mlp(widths, (inp,), n_actions)
        net.reset(g)
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith("bias"):
                    p.copy_(torch.rand(p.shape, generator=g) - 0.5)
        assert net.fused_supported(), (widths, n_actions, dueling)
        with torch.no_grad():
            ref = net.double()(x.double()).numpy()
        q = net.float().to(hip_device).fused_q(xd).cpu().numpy()
        np.testing.assert_allclose(q, ref, rtol=1e-4, atol=1e-5, err_msg=str((inp, widths, n_actions, dueling)))


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", ["qnet_mlp_grid_a3", "qnet_dueling_a5"])
def test_ops_equal_the_c_abi(name, hip_device):
    z = load_qnet(name)
    net = fixture_network(name, z, hip_device)
    widths, A, dueling = net.fused_spec()
    x = torch.from_numpy(z["x"][:100]).to(hip_device)
    B, inp = 100, x[0].numel()
    w = net.packed_weights()
    lib = _lib.load()
    cw = _widths(widths)
    q1 = torch.empty((B, A), device=hip_device)
    assert lib.ttrl_mlp_q(x.data_ptr(), B, inp, len(widths), cw, w.data_ptr(), A, int(dueling), q1.data_ptr(),
                          _stream()) == 0
    q2 = ops.T.mlp_q(x, w, widths, A, dueling)
    act1 = torch.empty(B, dtype=torch.int64, device=hip_device)
    act32 = torch.empty(B, dtype=torch.int32, device=hip_device)
    q3 = torch.empty((B, A), device=hip_device)
    assert lib.ttrl_mlp_act(x.data_ptr(), B, inp, len(widths), cw, w.data_ptr(), A, int(dueling), 0.3, None, 77, 5, None,
                            9, q3.data_ptr(), act1.data_ptr(), act32.data_ptr(), _stream()) == 0
    act2, q4 = ops.T.mlp_act(x, w, widths, A, dueling, 0.3, 77, 5, env_offset=9)
    act3, _ = ops.T.mlp_act(x, w, widths, A, dueling, 0.3, 77, 5, int32_actions=True, env_offset=9)
    torch.cuda.synchronize()
    assert torch.equal(q1, q2) and torch.equal(q3, q1) and torch.equal(q4, q1)
    assert torch.equal(act1, act2) and act3.dtype == torch.int32 and torch.equal(act32, act3)
    assert torch.equal(act3.long(), act2)
    assert ops.T.mlp_q(x[:0], w, widths, A, dueling).shape == (0, A)  # the empty batch: no launch
    with pytest.raises(RuntimeError, match="packed weights need"):
        ops.T.mlp_q(x, w[:-1], widths, A, dueling)
    with pytest.raises(RuntimeError, match="does not cover"):
        ops.T.mlp_q(x, w, [20], A, dueling)


@pytest.mark.parametrize("name", ["qnet_mlp_kin_a3", "qnet_dueling_a5"])
def test_fused_epsilon_greedy(name, hip_device):
    z = load_qnet(name)
    net = fixture_network(name, z, hip_device)
    widths, A, dueling = net.fused_spec()
    w = net.packed_weights()
    x = torch.from_numpy(z["x"]).to(hip_device)  # 1000 envs
    act = lambda rows, *a, **k: ops.T.mlp_act(rows, w, widths, A, dueling, *a, **k)  # noqa: E731
    a0, q0 = act(x, 0.0, 3, 1)
    assert torch.equal(q0, net.fused_q(x))
    assert torch.equal(a0, q0.argmax(1))  # first maximum, as np.argmax
    # epsilon 1: the draw alone, the one ego_attention_act makes at the same seed, step, A and batch
    att = EgoAttentionNetwork(A).reset(torch.Generator().manual_seed(0)).to(hip_device)
    kin = torch.from_numpy(load_qnet("qnet_mlp_kin_a3")["x"]).to(hip_device)
    for seed, step, off in ((11, 7, 0), (2 ** 40 + 5, 2 ** 33, 3000)):
        r1, _ = act(x, 1.0, seed, step, env_offset=off)
        e1, _ = ops.T.ego_attention_act(kin, att.packed_weights(), 2, A, 1.0, seed, step, env_offset=off)
        assert torch.equal(r1, e1)
        assert len(torch.unique(r1)) == A
    r1, _ = act(x, 0.5, 11, 7)
    r2, _ = act(x, 0.5, 11, 7)
    r3, _ = act(x, 0.5, 11, 8)
    assert torch.equal(r1, r2) and not torch.equal(r1, r3)
    assert 0.2 < float((r1 != a0).float().mean()) < 0.5 * (1 - 1 / A) + 0.1
    # env e's draw does not depend on the batch it is in
    r4, _ = act(x[:100], 0.5, 11, 7)
    assert torch.equal(r4, r1[:100])
    r5, q5 = act(x[300:555], 0.5, 11, 7, env_offset=300)
    assert torch.equal(r5, r1[300:555]) and torch.equal(q5, q0[300:555])
    r6, _ = act(x, 0.5, 11, 7, int32_actions=True)
    assert r6.dtype == torch.int32 and torch.equal(r6.long(), r1)
    # device scalars override epsilon / step (the captured-graph path)
    eps = torch.tensor(0.5, device=hip_device)
    stp = torch.tensor(7, dtype=torch.int64, device=hip_device)
    r7, _ = act(x, 0.0, 11, 0, eps, stp)
    assert torch.equal(r7, r1)


def test_a_nan_row_wins_the_argmax_and_stays_in_its_row(hip_device):
    z = load_qnet("qnet_mlp_kin_a3")
    net = fixture_network("qnet_mlp_kin_a3", z, hip_device)
    x = torch.from_numpy(z["x"][:37]).to(hip_device).clone()
    x[5, 3, 2] = float("nan")
    widths, A, dueling = net.fused_spec()
    a, q = ops.T.mlp_act(x, net.packed_weights(), widths, A, dueling, 0.0, 1, 1)
    assert bool(torch.isnan(q[5]).all()) and int(a[5]) == 0  # np.argmax: the first NaN
    keep = torch.arange(37, device=hip_device) != 5
    assert torch.equal(q[keep], net.fused_q(torch.from_numpy(z["x"][:37]).to(hip_device))[keep])


def test_policy_acts_in_a_step_graph(hip_device):
    """QNetworkPolicy.act on the GPU is the fused launch; inside a StepGraph the replays draw with
    the schedule's epsilon and a fresh step each time, equal to eager acting bit for bit."""
    from topotrafficrl_amd.envs import VecHighwayEnv
    from topotrafficrl_amd.graph import StepGraph
    cfg = {"num_envs": 64, "vehicles_count": 20, "observation": KIN, "device": hip_device}
    e1, e2 = VecHighwayEnv(cfg), VecHighwayEnv(cfg)
    o1, _ = e1.reset(seed=3)
    o2, _ = e2.reset(seed=3)
    p1 = QNetworkPolicy(hip_device, BASELINE, (15, 7), n_actions=5, seed=0, tau=2.0)
    p2 = QNetworkPolicy(hip_device, BASELINE, (15, 7), n_actions=5, seed=0, tau=2.0)
    assert p1.fused_acting(o1)
    assert torch.equal(p1.q_values(o1), p1.value_net.fused_q(o1))
    np.testing.assert_allclose(p1.q_values(o1).cpu().numpy(), p1.value_net(o1).detach().cpu().numpy(), rtol=1e-4,
                               atol=1e-5)
    sg = StepGraph(e2, o2, p2)
    assert p2.time == 0
    for t in range(3):
        a = p1.act(o1)
        o1, r1, *_ = e1.step(a)
        o2g, r2, *_ = sg.replay()
        assert torch.equal(a, sg.actions), t
        assert torch.equal(o1, o2g) and torch.equal(r1, r2), t
    assert p1.time == p2.time == 3
    slow = QNetworkPolicy(hip_device, BASELINE, (15, 7), n_actions=5, seed=0, fused=False)
    assert not slow.fused_acting(o1) and slow.act(o1).shape == (64,)  # the torch path


def _loop(env, agent, steps):
    ev = BatchedEvaluation(env, agent, num_episodes=1, sim_seed=5)
    rewards = ev.rollout(steps)
    torch.cuda.synchronize()
    assert rewards.shape == (steps, env.num_envs) and bool(torch.isfinite(rewards).all())
    assert agent.policy.time == steps
    lrn = agent.learner
    assert len(lrn.memory) == steps * env.num_envs and lrn.steps >= 1
    assert lrn.last_loss is not None and bool(torch.isfinite(lrn.last_loss))
    return ev


def test_kinematics_mlp_in_the_loop(hip_device):
    from topotrafficrl_amd.intersection import VecIntersectionEnv
    env = VecIntersectionEnv({"num_envs": 8, "device": hip_device, "env_id_offset": 16,
                              "observation": dict(VecIntersectionEnv.default_config()["observation"], **KIN)})
    agent = BatchedDQNAgent.from_env(env, {"model": BASELINE, "batch_size": 16, "memory_capacity": 256}, seed=1)
    pol = agent.policy
    assert isinstance(pol, QNetworkPolicy) and pol.n_actions == 3 and pol.obs_shape == (15, 7)
    assert pol.env_id_offset == 16
    ev = _loop(env, agent, 4)
    assert pol.fused_acting(ev.observation) and ev.observation.shape == (8, 15, 7)
    w = pol.value_net.packed_weights()
    assert torch.equal(w[:105 * 128].view(105, 128), pol.value_net.layers[0].weight.detach().t())  # follows Adam


def test_grid_mlp_in_the_loop(hip_device):
    from topotrafficrl_amd.envs import VecHighwayEnv
    obs = {"type": "OccupancyGrid", "features": KIN["features"], "features_range": KIN["features_range"],
           "grid_size": [[-27.5, 27.5], [-27.5, 27.5]], "grid_step": [5, 5], "absolute": False}
    env = VecHighwayEnv({"num_envs": 8, "vehicles_count": 20, "observation": obs, "device": hip_device})
    agent = BatchedDQNAgent.from_env(env, {"model": GRID, "batch_size": 16, "memory_capacity": 256}, seed=1)
    pol = agent.policy
    assert pol.obs_shape == (7, 11, 11) and pol.value_net.layers[0].in_features == 847 and pol.n_actions == 5
    ev = _loop(env, agent, 4)
    assert pol.fused_acting(ev.observation) and ev.observation.shape == (8, 7, 11, 11)
    assert float(ev.observation[:, 0].sum()) > 0  # the grid is drawn
