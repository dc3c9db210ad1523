"""``GCN`` — the reference's Q-network class (src/training/train_gcn_dqn.py:50-70)
with an identical ``state_dict`` layout, so ``data/models/*.pth`` load unchanged:

    conv1.att_src [1,1,32]  conv1.att_dst [1,1,32]  conv1.bias [32]
    conv1.lin.weight [32,7] lin1.weight [32,32] lin1.bias [32] lin2.weight [9,32] lin2.bias [9]

``forward(data)`` runs GATConv(7->32, heads=1, add_self_loops=False) -> tanh ->
lin1 -> relu -> lin2 for every graph of the batch in one HIP launch
(``swarm_q_forward``).  By default it is an inference forward (no autograd graph): the
learner's backward is the fused hand-written one in ``swarm_td_grad``.
``GCN(..., autograd=True)`` makes ``forward`` differentiable in the parameters: the same launch
computes Q (bitwise the same values), and ``loss.backward()`` runs one ``swarm_q_backward`` call
for whatever dL/dQ the loss produced, so the reference's ``train_step_dqn`` text (and any other
loss) trains these kernels.  ``data.x`` gets no gradient: the reference never differentiates the
observations.
``conv="gcn"`` selects the GCNConv variant (parity unpinned), which
reuses conv1.lin.weight / conv1.bias and ignores the attention vectors.

``GCN(7, 8, 9, layers=3)`` is the same class with its commented conv2/conv3 layers
(train_gcn_dqn.py:54-55, 65-68): conv1 -> tanh -> conv2 -> relu -> conv3 -> relu ->
lin1 -> relu -> lin2, hidden 8 — the architecture of the reference's Flocking checkpoints
(``data/models/experiment_Flocking-seed_*.pth``, ``SWARM_NET_GAT3``).  ``GAT3`` is that network as
a class of its own, and the one that takes ``autograd=True``: ``loss.backward()`` then runs one
``swarm_gat3_q_backward`` call, with the semantics above (Q bitwise the inference forward's, no
gradient for ``data.x``).  On the device it is trained by ``SwarmGat3Engine`` (engine.py) and
``DQNTrainer(..., net="gat3")``, whose ``model`` / ``target_model`` are ``GAT3`` objects; the fused
tick and populations do not train it.
``GCN.from_state_dict(sd)`` picks the architecture from the checkpoint's keys (a ``GAT3`` for a
checkpoint that holds conv2).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from ._lib import call, ptr
from .engine import param_order
from .graph import Data, _round4, edges_to_mult, q_backward


class GATConvParams(nn.Module):
    """Parameter holder with PyG 2.5.3 GATConv's names and registration order."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.att_src = nn.Parameter(torch.empty(1, 1, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, 1, out_channels))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        for p in (self.att_src, self.att_dst):
            bound = (6.0 / (1 + out_channels)) ** 0.5
            nn.init.uniform_(p, -bound, bound)
        bound = (6.0 / (in_channels + out_channels)) ** 0.5
        nn.init.uniform_(self.lin.weight, -bound, bound)


class _QFunction(torch.autograd.Function):
    """Q = GCN.forward(x) as one ``swarm_q_forward`` launch; backward = one ``swarm_q_backward``
    (three-layer network: ``swarm_gat3_q_backward``) call, its flat gradient sliced in
    ``param_order(model.net)``.  No gradient for x."""

    @staticmethod
    def forward(ctx, model, x, cfg, mult, *params):
        ctx.flat = model.flat_params(x.device)   # the weights this Q was computed with
        ctx.x, ctx.cfg, ctx.mult, ctx.net = x, cfg, mult, model.net
        ctx.params = params
        return model._q_forward(ctx.flat, x, cfg, mult)

    @staticmethod
    def backward(ctx, dq):
        if ctx.cfg.n_envs == 0:   # an empty batch: zero gradients, nothing to launch
            flat = torch.zeros(sum(p.numel() for p in ctx.params), dtype=torch.float32, device=ctx.x.device)
        else:
            flat = q_backward(ctx.flat, ctx.x, ctx.cfg, ctx.mult, dq)
        grads, o = [], 0
        for i, ((_, shape), p) in enumerate(zip(param_order(ctx.net), ctx.params)):
            n = p.numel()
            grads.append(flat[o:o + n].reshape(shape).to(p.device, p.dtype) if ctx.needs_input_grad[4 + i] else None)
            o += n
        return (None, None, None, None, *grads)


class GCN(nn.Module):
    _trains_three_layers = False   # GAT3 does

    def __init__(self, input_dim: int = 7, hidden_dim: int = 32, output_dim: int = 9, conv: str = "gat",
                 layers: int = 1, autograd: bool = False):
        super().__init__()
        shapes = {1: (7, 32, 9), 3: (7, 8, 9)}
        if shapes.get(layers) != (input_dim, hidden_dim, output_dim):
            raise ValueError("the HIP kernels are specialised for GCN(7, 32, 9) (train_gcn_dqn.py:81) and the "
                             "Flocking checkpoints' GCN(7, 8, 9, layers=3)")
        if layers == 3 and conv != "gat":
            raise ValueError("the three-layer network is a GAT")
        if layers == 3 and autograd and not self._trains_three_layers:
            raise ValueError("GCN(7, 8, 9, layers=3) is forward only: the differentiable three-layer network is "
                             "GAT3(autograd=True); GCN(autograd=True) needs GCN(7, 32, 9)")
        self.conv1 = GATConvParams(input_dim, hidden_dim)
        if layers == 3:
            self.conv2 = GATConvParams(hidden_dim, hidden_dim)
            self.conv3 = GATConvParams(hidden_dim, hidden_dim)
        self.lin1 = nn.Linear(hidden_dim, hidden_dim)
        self.lin2 = nn.Linear(hidden_dim, output_dim)
        self.conv = conv
        self.layers = layers
        self.autograd = bool(autograd)
        self.net = "gat3" if layers == 3 else "gcn"
        self.net_id = _lib.NET_GAT3 if layers == 3 else _lib.NET_GCN
        self._flat = None
        self._flat_key = None

    @classmethod
    def from_state_dict(cls, sd, conv: str = "gat", autograd: bool = False) -> "GCN":
        """A model of the checkpoint's architecture, loaded: a ``GAT3`` (three GATConvs) if it holds
        conv2, else ``cls(7, 32, 9)``."""
        m = GAT3(conv, autograd=autograd) if "conv2.lin.weight" in sd else cls(7, 32, 9, conv, autograd=autograd)
        m.load_state_dict(sd)
        return m

    def flat_params(self, device="cuda") -> torch.Tensor:
        sd = dict(self.named_parameters())
        order = param_order(self.net)
        key = tuple((id(sd[k]), sd[k]._version) for k, _ in order) + (str(device),)
        if self._flat is None or self._flat_key != key:
            self._flat = torch.cat([sd[k].detach().reshape(-1) for k, _ in order]).to(device, torch.float32)
            self._flat_key = key
        return self._flat

    def _q_forward(self, params, x, cfg, mult) -> torch.Tensor:
        q = torch.empty(x.shape[0], 9, dtype=torch.float32, device=x.device)
        call(_lib.load(), "swarm_q_forward", cfg, ptr(params), ptr(x), ptr(mult), ptr(q))
        return q

    def forward(self, data: Data) -> torch.Tensor:
        _lib.load()
        x = data.x.to("cuda", torch.float32).contiguous()
        conv = _lib.CONV_GAT if self.conv == "gat" else _lib.CONV_GCN
        M = x.shape[0]
        if data.swarm is not None:
            m = data.swarm
            mult = None
            cfg = _lib.SwarmConfig(m["n_graphs"], m["n_nodes"], 0, m["graph"], m["k"], conv, 0, 0, 0,
                                   float(m.get("radius", 0.0)), self.net_id)
        else:
            G = data.num_graphs
            if M % G:
                raise ValueError("GCN.forward: graphs of unequal size are not supported")
            N = M // G
            mult = edges_to_mult(data.edge_index, G, N)
            cfg = _lib.SwarmConfig(G, N, 0, _lib.GRAPH_DENSE, 0, conv, 0, 0, 0, 0.0, self.net_id)
        if self.autograd and torch.is_grad_enabled():
            sd = dict(self.named_parameters())
            params = [sd[k] for k, _ in param_order(self.net)]
            if any(p.requires_grad for p in params):
                return _QFunction.apply(self, x.detach(), cfg, mult, *params)
        return self._q_forward(self.flat_params(x.device), x, cfg, mult)


class GAT3(GCN):
    """``GCN(7, 8, 9, layers=3)``, the Flocking checkpoints' network, with ``autograd`` allowed:
    ``GAT3(autograd=True)`` is differentiable in its parameters through ``swarm_gat3_q_backward``."""
    _trains_three_layers = True

    def __init__(self, conv: str = "gat", autograd: bool = False):
        super().__init__(7, 8, 9, conv, layers=3, autograd=autograd)


__all__ = ["GCN", "GAT3", "GATConvParams", "_round4"]
