"""Policy in the loop (BASELINE config 5): the ttrl_agent DQN ego-attention network,
batched over every env of the simulator and fed the Kinematics observation in place.

Restates ttrl_agent/agents/common/models.py — MultiLayerPerceptron (:50-76),
EgoAttention (:157-194), EgoAttentionNetwork (:237-312), attention (:370-388) — and the
acting side of the DQN agent: AbstractDQNAgent.act (deep_q_network/abstract.py:65-83)
with EpsilonGreedy exploration (exploration/epsilon_greedy.py:7-57; schedule from
scripts/configs/IntersectionEnv/agents/DQNAgent/baseline.json:12-17).  The forward is a
dense contraction (7->64->64 embeddings, 2-head attention over 15 entities, 64->64->64->n
head): it runs as torch GEMMs on the same HIP stream as the simulator (hipBLASLt/MFMA),
no host round trip between env.step and the next action.

The other value nets of models.model_factory (:431-441) are restated too, with the reference's
state-dict names: MultiLayerPerceptron with its activation (baseline.json, grid.json),
DuelingNetwork (:79-104) and ConvolutionalNetwork (:107-154, grid_convnet.json); ``model_factory``
sizes them from the observation shape as size_model_config (:404-428) does and ``QNetworkPolicy``
acts with them, through the fused MLP forward (ttrl::mlp_act) where it covers the network.
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.nn import functional as F

EGO_ATTENTION_2H = {  # configs/IntersectionEnv/agents/DQNAgent/ego_attention.json + ego_attention_2h.json
    "type": "EgoAttentionNetwork",
    "presence_feature_idx": 0,
    "embedding_layer": {"type": "MultiLayerPerceptron", "layers": [64, 64], "reshape": False, "in": 7},
    "others_embedding_layer": {"type": "MultiLayerPerceptron", "layers": [64, 64], "reshape": False, "in": 7},
    "self_attention_layer": None,
    "attention_layer": {"type": "EgoAttention", "feature_size": 64, "heads": 2},
    "output_layer": {"type": "MultiLayerPerceptron", "layers": [64, 64], "reshape": False},
}


def activation_factory(activation_type: str):
    """models.py:391-397"""
    if activation_type == "RELU":
        return F.relu
    if activation_type == "TANH":
        return torch.tanh
    raise ValueError(f"Unknown activation_type: {activation_type}")


def xavier_reset(module: nn.Module, generator: torch.Generator | None = None) -> nn.Module:
    """BaseModule._init_weights (models.py:24-33) over every Linear / Conv2d: Xavier-uniform weights,
    zero biases, drawn from ``generator``."""
    for m in module.modules():
        if isinstance(m, (nn.Linear, nn.Conv2d)):
            fan_in, fan_out = nn.init._calculate_fan_in_and_fan_out(m.weight)
            bound = math.sqrt(6.0 / (fan_in + fan_out))
            with torch.no_grad():
                m.weight.uniform_(-bound, bound, generator=generator)
                if m.bias is not None:
                    m.bias.zero_()
    return module


def _mlp_in_kernel_domain(layers, n_out: int) -> bool:
    """The sizes ttrl_mlp_q covers (include/ttrl_qnet.h); ``n_out``: the head's columns."""
    return (1 <= len(layers) <= 3 and 1 <= layers[0].in_features <= 1024 and 1 <= n_out <= 16
            and all(lin.out_features % 16 == 0 and 16 <= lin.out_features <= 128 for lin in layers))


class _FusedMlp:
    """packed_weights / fused_q of the value nets the fused MLP forward covers (ttrl::mlp_q):
    subclasses give ``_fused_parts()`` = (hidden Linear layers, head Linear layers, dueling)."""

    def reset(self, generator: torch.Generator | None = None):
        return xavier_reset(self, generator)

    def fused_spec(self):
        """(widths, n_actions, dueling) as ttrl::mlp_q / ttrl::mlp_act take them."""
        layers, heads, dueling = self._fused_parts()
        return [lin.out_features for lin in layers], heads[0].out_features, dueling

    def packed_weights(self) -> torch.Tensor:
        """The weights in the ttrl_mlp_q packed layout (include/ttrl_qnet.h), cached until a
        parameter changes (optimizer steps bump the tensors' versions)."""
        layers, heads, _ = self._fused_parts()
        tensors = [t for lin in list(layers) + list(heads) for t in (lin.weight, lin.bias)]
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        if getattr(self, "_packed_key", None) != key:
            # matrices as [in][out]; a dueling head is one [last][A + 1] matrix, the value column last
            parts = [t.detach().t().reshape(-1) if t.dim() == 2 else t.detach() for lin in layers
                     for t in (lin.weight, lin.bias)]
            parts.append(torch.cat([h.weight.detach().t() for h in heads], dim=1).reshape(-1))
            parts.append(torch.cat([h.bias.detach() for h in heads]))
            self._packed = torch.cat([p.float() for p in parts]).contiguous()
            self._packed_key = key
        return self._packed

    @torch.no_grad()
    def fused_q(self, x: torch.Tensor) -> torch.Tensor:
        """Q-values through the fused HIP forward (torch.ops.ttrl.mlp_q): inference only."""
        from . import ops
        widths, n_actions, dueling = self.fused_spec()
        return ops.T.mlp_q(x.float(), self.packed_weights(), widths, n_actions, dueling)


class MultiLayerPerceptron(_FusedMlp, nn.Module):
    def __init__(self, inp: int, layers, out: int | None = None, reshape: bool = False, activation: str = "RELU"):
        super().__init__()
        sizes = [inp] + list(layers)
        self.layers = nn.ModuleList([nn.Linear(sizes[i], sizes[i + 1]) for i in range(len(sizes) - 1)])
        self.predict = nn.Linear(sizes[-1], out) if out else None
        self.reshape = reshape
        self.activation_type = activation
        self.activation = activation_factory(activation)

    def forward(self, x):
        if self.reshape:
            x = x.reshape(x.shape[0], -1)
        for layer in self.layers:
            x = self.activation(layer(x))
        return self.predict(x) if self.predict is not None else x

    def _fused_parts(self):
        return list(self.layers), [self.predict], False

    def fused_supported(self) -> bool:
        return (self.activation_type == "RELU" and self.predict is not None
                and _mlp_in_kernel_domain(self.layers, self.predict.out_features))


class DuelingNetwork(_FusedMlp, nn.Module):
    """models.py:79-104: q = value + advantage - mean(advantage) over a shared base module."""

    def __init__(self, inp: int, out: int, config: dict | None = None):
        super().__init__()
        c = config or {}
        base, value, adv = (dict(c.get(k) or {}) for k in ("base_module", "value", "advantage"))
        self.base_module = _mlp_from_config(base, inp, None)
        last = self.base_module.layers[-1].out_features if len(self.base_module.layers) else inp
        self.value = _mlp_from_config({"layers": [], **value}, last, 1)
        self.advantage = _mlp_from_config({"layers": [], **adv}, last, out)
        self.out = out

    def forward(self, x):
        x = self.base_module(x)
        value = self.value(x).expand(-1, self.out)
        advantage = self.advantage(x)
        return value + advantage - advantage.mean(1).unsqueeze(1).expand(-1, self.out)

    def _fused_parts(self):
        return list(self.base_module.layers), [self.advantage.predict, self.value.predict], True

    def fused_supported(self) -> bool:
        return (self.base_module.activation_type == "RELU" and len(self.value.layers) == 0
                and len(self.advantage.layers) == 0
                and _mlp_in_kernel_domain(self.base_module.layers, self.out + 1))


class ConvolutionalNetwork(nn.Module):
    """models.py:107-154: three 2x2 stride-2 convolutions over a CHW observation and an MLP head.
    It runs as torch kernels (12 k parameters, not on a measured hot path): never fused."""

    def __init__(self, obs_shape, out: int, config: dict | None = None):
        super().__init__()
        c = config or {}
        channels, height, width = (int(v) for v in obs_shape)
        self.activation = activation_factory(c.get("activation", "RELU"))
        self.conv1 = nn.Conv2d(channels, 16, kernel_size=2, stride=2)
        self.conv2 = nn.Conv2d(16, 32, kernel_size=2, stride=2)
        self.conv3 = nn.Conv2d(32, 64, kernel_size=2, stride=2)

        def size_out(size, kernel_size=2, stride=2):
            return (size - (kernel_size - 1) - 1) // stride + 1

        convw, convh = size_out(size_out(size_out(width))), size_out(size_out(size_out(height)))
        if convw <= 0 or convh <= 0:
            raise ValueError(f"a {height} x {width} observation is too small for three stride-2 convolutions")
        self.head = _mlp_from_config({"layers": [], **dict(c.get("head_mlp") or {})}, convw * convh * 64, out)

    def reset(self, generator: torch.Generator | None = None):
        return xavier_reset(self, generator)

    def fused_supported(self) -> bool:
        return False

    def forward(self, x):
        x = self.activation(self.conv1(x))
        x = self.activation(self.conv2(x))
        x = self.activation(self.conv3(x))
        return self.head(x)


def _mlp_from_config(c: dict, inp: int, out: int | None) -> MultiLayerPerceptron:
    """MultiLayerPerceptron.default_config (models.py:62-67): layers [64, 64], RELU, reshape."""
    return MultiLayerPerceptron(inp, c.get("layers", [64, 64]), out=out, reshape=bool(c.get("reshape", True)),
                                activation=c.get("activation", "RELU"))


def model_factory(config: dict, obs_shape, n_actions: int) -> nn.Module:
    """models.model_factory (models.py:431-441) on a config sized as size_model_config does
    (:404-428): ``in`` = prod(obs_shape), CHW for the convolutional net, ``out`` = n_actions."""
    kind = config.get("type")
    obs_shape = tuple(int(v) for v in obs_shape)
    if kind == "MultiLayerPerceptron":
        return _mlp_from_config(config, math.prod(obs_shape), n_actions)
    if kind == "DuelingNetwork":
        return DuelingNetwork(math.prod(obs_shape), n_actions, config)
    if kind == "ConvolutionalNetwork":
        return ConvolutionalNetwork(obs_shape, n_actions, config)
    if kind == "EgoAttentionNetwork":
        return EgoAttentionNetwork(n_actions, {**EGO_ATTENTION_2H, **config})
    raise ValueError("Unknown model type")


class EgoAttention(nn.Module):
    def __init__(self, feature_size: int = 64, heads: int = 2):
        super().__init__()
        self.f, self.h = feature_size, heads
        self.dph = feature_size // heads
        self.value_all = nn.Linear(feature_size, feature_size, bias=False)
        self.key_all = nn.Linear(feature_size, feature_size, bias=False)
        self.query_ego = nn.Linear(feature_size, feature_size, bias=False)
        self.attention_combine = nn.Linear(feature_size, feature_size, bias=False)

    def forward(self, ego, others, mask=None):
        b, n = others.shape[0], others.shape[1] + 1
        x = torch.cat((ego.view(b, 1, self.f), others), dim=1)
        k = self.key_all(x).view(b, n, self.h, self.dph).permute(0, 2, 1, 3)
        v = self.value_all(x).view(b, n, self.h, self.dph).permute(0, 2, 1, 3)
        q = self.query_ego(ego).view(b, 1, self.h, self.dph).permute(0, 2, 1, 3)
        # one query per env: the [1 x d] @ [d x n] products as broadcast multiply + reduce
        # (a batched GEMM of 16k 1x32x15 problems is ~20x slower on hipBLASLt)
        scores = (q * k).sum(-1, keepdim=True).transpose(-2, -1) / math.sqrt(self.dph)
        if mask is not None:
            scores = scores.masked_fill(mask.view(b, 1, 1, n).repeat(1, self.h, 1, 1), -1e9)
        p = F.softmax(scores, dim=-1)
        out = (p.transpose(-2, -1) * v).sum(-2, keepdim=True)
        return (self.attention_combine(out.reshape(b, self.f)) + ego.squeeze(1)) / 2, p


class EgoAttentionNetwork(nn.Module):
    def __init__(self, n_actions: int = 5, config: dict | None = None):
        super().__init__()
        c = config or EGO_ATTENTION_2H
        e, o, a, h = c["embedding_layer"], c["others_embedding_layer"], c["attention_layer"], c["output_layer"]
        self.presence_idx = c.get("presence_feature_idx", 0)
        self.ego_embedding = MultiLayerPerceptron(e["in"], e["layers"])
        self.others_embedding = MultiLayerPerceptron(o["in"], o["layers"])
        self.attention_layer = EgoAttention(a["feature_size"], a["heads"])
        self.output_layer = MultiLayerPerceptron(a["feature_size"], h["layers"], out=n_actions)

    def reset(self, generator: torch.Generator | None = None):
        """BaseModule._init_weights (models.py:24-33): Xavier-uniform weights, zero biases."""
        for m in self.modules():
            if isinstance(m, nn.Linear):
                bound = math.sqrt(6.0 / (m.in_features + m.out_features))
                with torch.no_grad():
                    m.weight.uniform_(-bound, bound, generator=generator)
                    if m.bias is not None:
                        m.bias.zero_()
        return self

    def packed_weights(self) -> torch.Tensor:
        """The weights in the ttrl_ego_attention_q packed layout (include/ttrl_mi355x.h), cached
        until a parameter changes (optimizer steps bump the tensors' versions)."""
        ps = [self.ego_embedding.layers[0], self.ego_embedding.layers[1], self.others_embedding.layers[0],
              self.others_embedding.layers[1]]
        a = self.attention_layer
        h = self.output_layer
        tensors = []
        for lin in ps[:2]:
            tensors += [lin.weight, lin.bias]
        for lin in ps[2:]:
            tensors += [lin.weight, lin.bias]
        tensors += [a.value_all.weight, a.key_all.weight, a.query_ego.weight, a.attention_combine.weight]
        tensors += [h.layers[0].weight, h.layers[0].bias, h.layers[1].weight, h.layers[1].bias,
                    h.predict.weight, h.predict.bias]
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        if getattr(self, "_packed_key", None) != key:
            # matrices as [in][out] (Linear.weight transposed): coalesced reads in the kernels
            self._packed = torch.cat([(t.detach().t() if t.dim() == 2 else t.detach()).reshape(-1).float()
                                      for t in tensors]).contiguous()
            self._packed_key = key
        return self._packed

    def fused_supported(self) -> bool:
        e = self.ego_embedding
        return (len(e.layers) == 2 and e.layers[0].out_features == 64 and e.layers[1].out_features == 64
                and len(self.others_embedding.layers) == 2 and self.attention_layer.f == 64
                and len(self.output_layer.layers) == 2 and self.output_layer.layers[0].out_features == 64
                and self.output_layer.layers[1].out_features == 64 and self.output_layer.predict is not None
                and self.presence_idx == 0 and e.layers[0].in_features in (5, 7, 8))

    @torch.no_grad()
    def fused_q(self, x: torch.Tensor) -> torch.Tensor:
        """Q-values through the fused HIP forward (torch.ops.ttrl.ego_attention_q): inference only."""
        from . import ops
        return ops.T.ego_attention_q(x.float(), self.packed_weights(), self.attention_layer.h,
                                     self.output_layer.predict.out_features)

    def forward(self, x):
        # contiguous copies: hipBLASLt takes a 6x slower path on the strided [:, 1:, :] view
        ego, others = x[:, 0:1, :].contiguous(), x[:, 1:, :].contiguous()
        mask = x[:, :, self.presence_idx:self.presence_idx + 1] < 0.5
        att, _ = self.attention_layer(self.ego_embedding(ego), self.others_embedding(others), mask)
        return self.output_layer(att)


class _EpsilonGreedyPolicy:
    """Batched DQN acting: Q = value_net(obs); epsilon-greedy on the device.  Subclasses build the
    value net and name their fused acting operator (``_fused_act``)."""

    def __init__(self, device, value_net: nn.Module, n_actions: int, seed: int, tau: float, temperature: float,
                 final_temperature: float, fused: bool, env_id_offset: int):
        self.device = torch.device(device)
        # the global env id of obs row 0 (a data-parallel rank's shard offset, sharding.shard): the
        # fused draws are keyed on the global env, so every shard of one seed explores independently
        # and any split of the global batch draws the same action for the same env
        self.env_id_offset = int(env_id_offset)
        self.fused = fused  # acting through the fused HIP forward on a GPU (training uses the torch graph)
        g = torch.Generator(device="cpu")
        g.manual_seed(seed)
        self.value_net = value_net.reset(g).to(self.device).eval()
        self.n_actions = n_actions
        self.tau, self.t0, self.t1 = tau, temperature, final_temperature
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed + 1)
        self.seed = int(seed) + 1  # the fused acting's Philox key
        self.time = 0  # EpsilonGreedy.time: the number of act() calls so far
        self.last_epsilon = None  # the epsilon of the latest act() (EpsilonGreedy.epsilon)

    def epsilon(self, t: int) -> float:
        """EpsilonGreedy.update (epsilon_greedy.py:37-48): epsilon at exploration time t."""
        return self.t1 + (self.t0 - self.t1) * math.exp(-t / self.tau)

    def fused_acting(self, obs: torch.Tensor) -> bool:
        return self.fused and obs.device.type == "cuda" and self.value_net.fused_supported()

    @torch.no_grad()
    def q_values(self, obs: torch.Tensor) -> torch.Tensor:
        if self.fused_acting(obs):
            return self.value_net.fused_q(obs)
        return self.value_net(obs)

    @torch.no_grad()
    def act(self, obs: torch.Tensor, t: int | None = None, epsilon: torch.Tensor | None = None,
            step: torch.Tensor | None = None, dtype: torch.dtype = torch.int64) -> torch.Tensor:
        """AbstractDQNAgent.act (dqn/abstract.py:65-83) for a batch: the exploration time is stepped
        first (step_time, :77-78), then EpsilonGreedy.update sets epsilon from it and the greedy
        action (np.argmax, first maximum), then the action is drawn from {a: epsilon / A +
        (1 - epsilon) [a == greedy]} (epsilon_greedy.py:32-48).  ``t``: the exploration time before
        this call (default: the policy's own counter).  ``epsilon`` / ``step`` (device scalars, float32 /
        int64) override the schedule and the draw counter: a captured graph refreshes them before
        every replay.  ``dtype``: the actions' index type (int64, or int32 -- the env's own, which
        env.step takes without a cast launch).

        On a GPU the forward, argmax and draw are ONE launch (ttrl::ego_attention_act or ttrl::mlp_act,
        Philox keyed on (seed, env_id_offset + row, step)); elsewhere, and for a network the fused
        forward does not cover, the torch forward with torch's generator."""
        t = self.time if t is None else int(t)
        self.time = t + 1
        self.last_epsilon = self.epsilon(self.time) if epsilon is None else epsilon
        if self.fused_acting(obs):
            act = self._fused_act(obs, self.last_epsilon if epsilon is None else 0.0, epsilon, step,
                                  dtype == torch.int32)
            return act if act.dtype == dtype else act.to(dtype)
        epsilon = self.last_epsilon
        q = self.value_net(obs)
        greedy = q.argmax(dim=1)
        e = obs.shape[0]
        u = torch.rand(e, device=self.device, generator=self.gen)
        rnd = torch.randint(0, self.n_actions, (e,), device=self.device, generator=self.gen)
        return torch.where(u < epsilon, rnd, greedy).to(dtype)


class EgoAttentionPolicy(_EpsilonGreedyPolicy):
    """Acting with the EgoAttention value net on obs[E, V, F]."""

    def __init__(self, device, n_actions: int = 5, seed: int = 0, tau: float = 15000.0, temperature: float = 1.0,
                 final_temperature: float = 0.05, fused: bool = True, env_id_offset: int = 0):
        super().__init__(device, EgoAttentionNetwork(n_actions), n_actions, seed, tau, temperature, final_temperature,
                         fused, env_id_offset)

    def _fused_act(self, obs, eps, epsilon_dev, step_dev, int32_actions):
        from . import ops
        net = self.value_net
        act, _ = ops.T.ego_attention_act(obs.float(), net.packed_weights(), net.attention_layer.h,
                                         net.output_layer.predict.out_features, eps, self.seed, self.time,
                                         epsilon_dev, step_dev, int32_actions=int32_actions,
                                         env_offset=self.env_id_offset)
        return act


class QNetworkPolicy(_EpsilonGreedyPolicy):
    """Acting with the value net ``model_factory`` builds from ``model`` (an agent config's "model"
    dict) on obs[E, *obs_shape].  A MultiLayerPerceptron or DuelingNetwork inside the fused
    forward's domain (``fused_supported``) acts through ttrl::mlp_act on a GPU, unless ``fused`` is
    False; every other network acts through the torch path."""

    def __init__(self, device, model: dict, obs_shape, n_actions: int = 5, seed: int = 0, tau: float = 15000.0,
                 temperature: float = 1.0, final_temperature: float = 0.05, fused: bool = True,
                 env_id_offset: int = 0):
        self.obs_shape = tuple(int(v) for v in obs_shape)
        super().__init__(device, model_factory(model, self.obs_shape, n_actions), n_actions, seed, tau, temperature,
                         final_temperature, fused, env_id_offset)

    def _fused_act(self, obs, eps, epsilon_dev, step_dev, int32_actions):
        from . import ops
        net = self.value_net
        widths, n_actions, dueling = net.fused_spec()
        act, _ = ops.T.mlp_act(obs.float(), net.packed_weights(), widths, n_actions, dueling, eps, self.seed,
                               self.time, epsilon_dev, step_dev, int32_actions=int32_actions,
                               env_offset=self.env_id_offset)
        return act
