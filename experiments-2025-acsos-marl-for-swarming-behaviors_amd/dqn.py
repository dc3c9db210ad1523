"""``DQNTrainer`` / ``GraphReplayBuffer`` with the reference's API
(src/training/train_gcn_dqn.py:25-231), driven by the fused device engine.

``train_model(config)`` runs the reference's episode loop (:139-204): per episode
reset, then ``max_steps`` fused training ticks (act -> env.step -> replay push ->
TD update -> target sync every ``update_target_every`` ticks), ε schedule
``max(min_epsilon, epsilon * exp(-epsilon_decay * episode))`` (:180), model saved
as ``experiment_{experiment}-seed_{seed}.pth`` (:201) and the stats CSV with the
reference's ``i // 10`` indexing (:225-231).  One episode is captured once into a
hipGraph and replayed.

``DQNTrainer(..., net="gat3")`` trains the Flocking checkpoints' three-layer GAT (``GAT3`` models, a
``SwarmGat3Engine``): the same loop, each tick four launches (act + push, TD gradient, optimizer step)
instead of the fused two, captured and replayed the same way; the saved ``.pth`` has that network's
keys.  Whether a tick ran an update is taken from ``ctrl.adam_step`` advancing (its optimizer step is
applied at once, so ``trained`` stays 0).  Such trainers form a ``Gat3PopulationTrainer`` (a
``SwarmGat3Population``: all of them in the four launches per tick of one), not a ``PopulationTrainer``.

Optional evaluation inside training (not in the reference, whose training loop never evaluates):
with ``config["eval_every"] = E`` every E-th episode ends with a greedy rollout of the current
weights on ``eval_envs`` evaluation environments (``eval_seed``; ``eval_graph`` / ``eval_knn_k``
default to the training graph), one row per evaluation in ``trainer.eval_rows`` and in
``experiment_{experiment}-seed_{seed}-eval.csv``.  A ``PopulationTrainer`` evaluates all its
members in one launch (``SwarmPopulation.evaluate``).  Training itself keeps every bit.

Optional population-based training (``PopulationTrainer`` only): with ``config["pbt_every"] = K`` (a
multiple of ``eval_every``) the evaluation of every K-th episode is followed by one
``SwarmPopulation.exploit`` round: the score is each member's evaluation reward summed over envs and
agents, formed on the device, ``round`` counts the rounds from 0 and ``config.get("pbt", {})`` holds
``exploit``'s other keywords.  Each trainer keeps ``pbt_rows`` (episode, parent, lr, gamma after the
round), written as ``experiment_{experiment}-seed_{seed}-pbt.csv``.  Without ``pbt_every`` nothing
changes: the same launches, files and bits.

Deliberate, documented differences (SURVEY §7 "RNG", "Vectorisation fixes"):
random draws come from Philox keyed by (seed, tick, env), not Python ``random``;
with ``num_envs`` > 1 each env draws its own exploration coin.
"""
from __future__ import annotations

import csv
import math
import os
import random
from typing import Optional

import numpy as np
import torch

from . import _lib
from .engine import SwarmEngine, SwarmGat3Engine, flatten_state_dict, glorot_init, unflatten_params
from .gcn import GAT3, GCN
from .graph import Batch, Data, create_graph_from_observations
from .population import SwarmGat3Population, SwarmPopulation, evaluation_engine


class SummaryWriter:
    """Minimal stand-in for torch.utils.tensorboard.SummaryWriter (not installed):
    keeps the scalars the reference logs ('Loss', 'Reward'; :136,174) in memory."""

    def __init__(self, *args, **kwargs):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars.setdefault(tag, []).append((int(step), float(value)))

    def close(self):
        pass


class GraphReplayBuffer:
    """Ring of (graph, actions, rewards, next_graph) with the reference's push/sample/len.

    Standalone buffer for API users; stores node features on the device.  The
    fused trainer uses the engine's SoA replay ring instead (same semantics,
    one slot per tick holding every env's transition)."""

    def __init__(self, capacity: int):
        self.capacity = capacity
        self.buffer = []
        self.position = 0

    def push(self, graph_observation, actions, rewards, next_graph_observation):
        if len(self.buffer) < self.capacity:
            self.buffer.append(None)
        self.buffer[self.position] = (graph_observation, actions, rewards, next_graph_observation)
        self.position = (self.position + 1) % self.capacity

    def sample(self, batch_size: int):
        sample = random.sample(self.buffer, batch_size)
        obs = [s[0] for s in sample]
        acts = [s[1] for s in sample]
        rews = [s[2] for s in sample]
        nxt = [s[3] for s in sample]
        return Batch.from_data_list(obs), torch.cat(acts), torch.cat(rews), Batch.from_data_list(nxt)

    def __len__(self):
        return len(self.buffer)


class _EngineReplayView:
    """len() view of the engine's replay ring, in graphs."""

    def __init__(self, engine: SwarmEngine):
        self.engine = engine

    def __len__(self):
        return self.engine.replay_len()


def set_seed(seed: int):
    """train_gcn_dqn.py:233-239."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


class DQNTrainer:
    def __init__(self, env, seed: int, models_path: str, stats_path: str, experiment: str, *,
                 batch_size: int = 32, update_target_every: int = 200, lr: float = 1e-3, gamma: float = 0.99,
                 replay_capacity: int = 1_000_000, use_graph: bool = True, net: str = "gcn"):
        if net not in ("gcn", "gat3"):
            raise ValueError(f"net must be 'gcn' or 'gat3', not {net!r}")
        self.net = net
        self.env = env
        self.seed = seed
        self.models_path = models_path
        self.stats_path = stats_path
        self.experiment = experiment
        self.n_input = env.observation_space["agent0"].shape[0] + 1
        self.n_output = env.action_space["agent0"].n
        if net == "gat3":   # the Flocking checkpoints' three-layer network, trained by SwarmGat3Engine
            self.model, self.target_model = GAT3(), GAT3()
            init = glorot_init(torch.Generator().manual_seed(seed), net)
        else:
            self.model = GCN(input_dim=self.n_input, hidden_dim=32, output_dim=self.n_output)
            self.target_model = GCN(input_dim=self.n_input, hidden_dim=32, output_dim=self.n_output)
            init = glorot_init(torch.Generator().manual_seed(seed))
        self.model.load_state_dict(unflatten_params(init, net))
        self.target_model.load_state_dict(self.model.state_dict())
        self.batch_size = batch_size
        self.update_target_every = update_target_every
        self.use_graph = use_graph
        scen = env.scenario
        engine_cls = SwarmGat3Engine if net == "gat3" else SwarmEngine
        self.engine = engine_cls(scenario=scen.SCENARIO_ID, n_agents=env.n_agents, n_envs=env.num_envs,
                                 seed=seed, params=init, batch=batch_size, gamma=gamma, lr=lr,
                                 update_target_every=update_target_every, replay_capacity=replay_capacity,
                                 shared_reset=True, random_oa=bool(getattr(scen, "random", False)))
        self.optimizer = SimpleAdamView(self.engine)
        self.replay_buffer = _EngineReplayView(self.engine)
        self.writer = SummaryWriter()
        self.episode_rewards = []
        self.episode_losses = []
        self.episode_obstacle_hits = []
        self.rewards_buffer = []
        self.obstacle_hits_buffer = []
        self.eval_rows = []     # (episode, mean reward per tick, hits, final distance) per evaluation
        self.pbt_rows = []      # (episode, parent member, lr, gamma after the round) per PBT round
        self._eval_engine = None

    def create_graph_from_observations(self, observations) -> Data:
        return create_graph_from_observations(observations)

    def _sync_models(self):
        self.engine.flush()
        self.model.load_state_dict(unflatten_params(self.engine.params.detach().cpu(), self.net))
        self.target_model.load_state_dict(unflatten_params(self.engine.target.detach().cpu(), self.net))

    def train_step_dqn(self, batch_size, model=None, target_model=None, ticks=None, gamma=0.99,
                       update_target_every=10) -> float:
        """One TD update on the engine's replay (train_gcn_dqn.py:112-137)."""
        if len(self.replay_buffer) < batch_size:
            print("Not enough samples in the replay buffer")
            return 0
        eng = self.engine
        eng.hp.batch = batch_size
        eng.hp.gamma = gamma
        eng.hp.update_target_every = update_target_every
        if ticks is not None:   # the kernels sync when (ctrl.tick + 1) % every == 0
            eng.ctrl[0] = int(ticks) - 1
        eng.td_update()
        c = eng.read_ctrl()
        self._sync_models()
        self.writer.add_scalar("Loss", c["loss"], c["tick"])
        return c["loss"]

    def _episode_fn(self, max_steps: int):
        """One training tick plus the bookkeeping the reference does on the host every tick
        (train_gcn_dqn.py:174-177), kept on the device: the episode's reward and loss sums, and
        per tick the summed agent reward ('Reward', :174), the TD loss and whether an update
        ran ('Loss' is logged only by updates, :113-115,136).  The tick's slot in the per-tick
        buffers is fixed when the call is made, so a captured episode replays into the same
        slots; train_model reads them once per episode."""
        eng = self.engine
        n = self.env.n_agents
        calls = [0]

        # the unfused optimizer step (net="gat3") leaves `trained` 0: an update ran iff adam_step advanced
        unfused = self.net == "gat3"
        step_before = torch.zeros((), dtype=torch.int32, device=eng.device)

        def tick():
            i = calls[0] % max_steps
            calls[0] += 1
            if unfused:
                step_before.copy_(eng.ctrl[_lib.CTRL["adam_step"]])
            eng.train_tick(full_out=False)
            self._acc_reward.add_(eng.reward[:, 0].mean() / n)
            self._acc_loss.add_(eng.ctrl.view(torch.float32)[5])
            self._tick_reward[i].copy_(eng.reward.sum(dim=1).mean())
            self._tick_loss[i].copy_(eng.ctrl.view(torch.float32)[5])
            self._tick_trained[i].copy_(eng.ctrl[_lib.CTRL["adam_step"]] - step_before if unfused else eng.ctrl[7])
        return tick

    def _check_episode(self):
        self.engine.check_handoffs()   # an overrun hand-off dropped TD graphs: fail loudly (one 4-byte read)
        if self.engine.peer is not None:
            self.engine.peer.check()   # an expired peer-exchange wait: the summed gradient is wrong

    def _evaluate(self, ev: dict, n_ticks: int):
        """The lone trainer's evaluation: swarm_env_reset + swarm_rollout on an evaluation engine of
        its own, with the training engine's weights as they stand (no flush)."""
        if self._eval_engine is None or self._eval_key != tuple(ev.values()):
            self._eval_engine = evaluation_engine(self.engine.cfg, ev["envs"], ev["seed"], ev["graph"], ev["knn_k"])
            self._eval_key = tuple(ev.values())
        e = self._eval_engine
        e.reset(0)
        res = e.rollout(n_ticks, tick0=0, eps=0.0, params=self.engine.params)
        return [{k: v.cpu() for k, v in res.items()}]

    def train_model(self, config):
        _train_loop(self, self.engine, [self], (), config, "", "Model saved successfully!")

    def save_eval_to_csv(self):
        os.makedirs(self.stats_path, exist_ok=True)
        with open(f"{self.stats_path}/experiment_{self.experiment}-seed_{self.seed}-eval.csv", mode="w",
                  newline="") as f:
            w = csv.writer(f)
            w.writerow(["Episode", "Reward", "Collisions", "Distance (end)"])
            w.writerows(self.eval_rows)

    def save_pbt_to_csv(self):
        os.makedirs(self.stats_path, exist_ok=True)
        with open(f"{self.stats_path}/experiment_{self.experiment}-seed_{self.seed}-pbt.csv", mode="w",
                  newline="") as f:
            w = csv.writer(f)
            w.writerow(["Episode", "Parent", "lr", "gamma"])
            w.writerows(self.pbt_rows)

    def save_metrics_to_csv(self):
        os.makedirs(self.stats_path, exist_ok=True)
        with open(f"{self.stats_path}/experiment_{self.experiment}-seed_{self.seed}.csv", mode="w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["Episode", "Reward", "Loss"])
            for i in range(len(self.episode_losses)):
                if (i + 1) % 10 == 0:   # reference quirk: losses indexed with i // 10 (:231)
                    w.writerow([i, float(self.episode_rewards[i // 10]), self.episode_losses[i // 10]])


class _PopulationDriver:
    """What ``PopulationTrainer`` and ``Gat3PopulationTrainer`` share: the trainers' engines re-homed
    into one population of ``population_class``, the per-tick bookkeeping on [P] device tensors, the
    evaluation of all members in one launch and the loop."""
    net = "gcn"
    population_class = SwarmPopulation
    refusal = ""

    def __init__(self, trainers):
        self.trainers = list(trainers)
        first = self.trainers[0]
        if any(t.net != self.net for t in self.trainers):
            raise ValueError(self.refusal)
        for t in self.trainers:
            if (t.env.max_steps, t.env.n_agents, t.use_graph) != (first.env.max_steps, first.env.n_agents,
                                                                   first.use_graph):
                raise ValueError("the trainers of a population share max_steps, n_agents and use_graph")
        self.population = self.population_class.from_engines([t.engine for t in self.trainers])

    def _episode_fn(self, max_steps: int):
        """DQNTrainer._episode_fn for every member at once: the same per-tick bookkeeping, on
        [P]-shaped device tensors (a fixed number of launches whatever P is)."""
        pop = self.population
        n = self.trainers[0].env.n_agents
        ctrl_f = pop.ctrl.view(torch.float32)
        calls = [0]
        # the unfused optimizer step (net="gat3") leaves `trained` 0: an update ran iff adam_step advanced
        unfused = self.net == "gat3"
        step = pop.ctrl[:, _lib.CTRL["adam_step"]]
        step_before = torch.zeros(pop.P, dtype=torch.int32, device=pop.device)

        def tick():
            i = calls[0] % max_steps
            calls[0] += 1
            if unfused:
                step_before.copy_(step)
            pop.train_tick(full_out=False)
            self._acc_reward.add_(pop.reward[:, :, 0].mean(dim=1) / n)
            self._acc_loss.add_(ctrl_f[:, 5])
            self._tick_reward[i].copy_(pop.reward.sum(dim=2).mean(dim=1))
            self._tick_loss[i].copy_(ctrl_f[:, 5])
            self._tick_trained[i].copy_(step - step_before if unfused else pop.ctrl[:, 7])
        return tick

    def _evaluate(self, ev: dict, n_ticks: int):
        """Every member's evaluation in one launch (DQNTrainer._evaluate's rows, member by member)"""
        res = self.population.evaluate(ev["envs"], n_ticks, seed=ev["seed"], episode=0, graph=ev["graph"],
                                       knn_k=ev["knn_k"])
        self._eval_reward = res["reward"]   # [P, envs, N] on the device: what a PBT round scores
        res = {k: v.cpu() for k, v in res.items()}
        return [{k: v[m] for k, v in res.items()} for m in range(self.population.P)]

    def train_model(self, config):
        _train_loop(self, self.population, self.trainers, (self.population.P,), config, "Seed {seed}, ",
                    "Models saved successfully!")


class PopulationTrainer(_PopulationDriver):
    """Several ``DQNTrainer`` objects over one scenario and agent count (the reference's seeds
    0-9 of one experiment, train_gcn_dqn.py:262-290) trained together: their engines become the
    members of one ``SwarmPopulation``, so a training tick of all of them is two launches.

    ``train_model(config)`` runs the loop of ``DQNTrainer.train_model`` for all trainers at once and
    leaves each trainer as its own ``train_model`` would: the same episode lists and writer scalars,
    the same ``.pth`` and ``.csv`` files (members compute a lone engine's bits).

    The trainers may differ in ``lr``, ``gamma`` and ``update_target_every`` (a sweep: the population
    then ticks with one optimizer row per member), and ``config``'s ``epsilon``, ``epsilon_decay`` and
    ``min_epsilon`` may each be a sequence of one value per trainer; they share ``batch_size``, the
    ring capacity and everything else of the configuration."""
    refusal = ("a PopulationTrainer trains the one-layer network: DQNTrainer(net='gat3') objects form a "
               "Gat3PopulationTrainer (SwarmGat3Engine has the unfused tick only)")

    def _check_episode(self):
        self.population.check_handoffs()

    def _pbt_round(self, episode: int, rnd: int, kw: dict):
        """One exploit round scored by the evaluation just run: each member's reward summed over
        envs and agents, on the device.  One row per trainer: who it now descends from and the lr
        and gamma it goes on with."""
        pop = self.population
        score = self._eval_reward.sum(dim=(1, 2))
        parent = pop.exploit(score, round=rnd, **kw).tolist()
        if pop._hp_stale:   # kw asked for sync=False: the rows below and the final flush need the host hp
            pop.sync_hp()
        for m, t in enumerate(self.trainers):
            t.pbt_rows.append((episode, parent[m], t.engine.hp.lr_d, t.engine.hp.gamma))


class Gat3PopulationTrainer(_PopulationDriver):
    """``PopulationTrainer`` for ``DQNTrainer(net="gat3")`` objects (the reference's Flocking
    experiment: ten seeds, one environment each): their ``SwarmGat3Engine``s become the members of one
    ``SwarmGat3Population``, so a training tick of all of them is the four launches one of them
    costs.  ``train_model(config)`` leaves each trainer as its own ``train_model`` would: the same
    lists, writer scalars, ``.pth`` and ``.csv`` / ``-eval.csv`` files; the second and later episodes
    are captured; ``eval_every`` evaluates all members in one launch.  An update ran when
    ``ctrl.adam_step`` advanced, as in the lone trainer.  The trainers may differ in ``lr``, ``gamma``
    and ``update_target_every`` and the epsilon schedule may be per member, as ``PopulationTrainer``
    documents.  There is no population-based training: ``pbt_every`` raises ValueError."""
    net = "gat3"
    population_class = SwarmGat3Population
    refusal = ("a Gat3PopulationTrainer trains the three-layer network: DQNTrainer(net='gcn') objects form a "
               "PopulationTrainer")

    def _check_episode(self):
        """the unfused tick has no hand-off to check"""


def _is_sequence(v) -> bool:
    return isinstance(v, (list, tuple)) or hasattr(v, "tolist") and getattr(v, "ndim", 0) > 0


def eval_row(episode: int, res: dict, n_ticks: int) -> tuple:
    """(episode, mean reward per tick, hits, final distance) of one policy's evaluation rollout
    (host tensors of ``SwarmEngine.rollout``): Simulator's result.csv columns (the agents' summed
    reward per tick, the hits summed over the ticks, the last tick's mean goal distance), each a
    mean over the evaluation environments."""
    return (episode, float(res["reward"].sum(dim=1).mean()) / max(n_ticks, 1), float(res["hits"].mean()),
            float(res["avg_dist"].mean()))


def pbt_schedule(config):
    """``config["pbt_every"]`` checked: None (no PBT) or an integer >= 1 that ``eval_every`` divides
    (a round is scored by the evaluation that precedes it)."""
    every = config.get("pbt_every")
    if every is None:
        return None
    if isinstance(every, bool) or int(every) != every or every < 1:
        raise ValueError(f"pbt_every must be an integer >= 1 or None, not {every!r}")
    eval_every = config.get("eval_every")
    if eval_every is None or isinstance(eval_every, bool) or eval_every < 1 or every % eval_every != 0:
        raise ValueError(f"pbt_every = {every!r} needs eval_every to divide it (eval_every = {eval_every!r}): a PBT "
                         "round is scored by the evaluation of its episode")
    return int(every)


def _train_loop(driver, group, trainers, shape, config, prefix: str, saved: str):
    """The reference's episode loop (train_gcn_dqn.py:139-204) for ``trainers`` ticked together by
    ``group`` (a SwarmEngine with its one trainer, or a SwarmPopulation): reset / set_eps / capture.
    ``driver`` owns what differs between the two: the tick with its device-side bookkeeping
    (``_episode_fn``, on per-episode buffers of ``shape``, per-tick ones of [max_steps, *shape]: () for
    a lone engine, (P,) for a population) and the end-of-episode checks (``_check_episode``)."""
    first, P = trainers[0], len(trainers)
    # with a population each of the three may be one value per member: the same schedule, evaluated
    # per member (a lone trainer's, with scalars, is unchanged)
    schedule = [config["epsilon"], config["epsilon_decay"], config["min_epsilon"]]
    per_member_eps = shape != () and any(_is_sequence(v) for v in schedule)
    if per_member_eps:
        schedule = [list(v) if _is_sequence(v) else [v] * P for v in schedule]
        if any(len(v) != P for v in schedule):
            raise ValueError(f"epsilon, epsilon_decay and min_epsilon: scalars or {P} values each")
    initial_epsilon, epsilon_decay, min_epsilon = schedule
    episodes = config["episodes"]
    max_steps = first.env.max_steps or 100
    eval_every = config.get("eval_every")   # absent or None: no evaluation
    if eval_every is not None and (isinstance(eval_every, bool) or int(eval_every) != eval_every or eval_every < 1):
        raise ValueError(f"eval_every must be an integer >= 1 or None, not {eval_every!r}")
    ev = dict(envs=config.get("eval_envs", 8), seed=config.get("eval_seed", 6967), graph=config.get("eval_graph"),
              knn_k=config.get("eval_knn_k"))
    pbt_every = pbt_schedule(config)
    if pbt_every is not None:
        if not hasattr(driver, "_pbt_round"):
            raise ValueError("pbt_every needs a PopulationTrainer: a lone trainer has nobody to exploit, and "
                             "population-based training works on the one-layer network's populations only (not on "
                             "a Gat3PopulationTrainer)")
        group.per_member_hp = True   # before the episode is captured: the rows will change
    epsilon = initial_epsilon
    driver._acc_reward = torch.zeros(shape, device=group.device)
    driver._acc_loss = torch.zeros(shape, device=group.device)
    driver._tick_reward = torch.zeros((max_steps, *shape), device=group.device)
    driver._tick_loss = torch.zeros((max_steps, *shape), device=group.device)
    driver._tick_trained = torch.zeros((max_steps, *shape), dtype=torch.int32, device=group.device)
    tick_fn = driver._episode_fn(max_steps)
    ticks = 0
    graph = None
    for episode in range(episodes):
        group.reset()
        group.set_eps(epsilon)
        driver._acc_reward.zero_()
        driver._acc_loss.zero_()
        if first.use_graph and episode > 0:
            if graph is None:   # episode 0 ran eagerly (warm-up); capture one whole episode once
                graph = group.capture(max_steps, tick_fn)
            graph.replay()
        else:
            for _ in range(max_steps):
                tick_fn()
        if per_member_eps:
            epsilon = [max(lo, e0 * np.exp(-d * episode)) for e0, d, lo in zip(*schedule)]
        else:
            epsilon = max(min_epsilon, initial_epsilon * np.exp(-epsilon_decay * episode))
        # the episode's scalars of every member, read once: the sums [P], the per-tick ones [max_steps][P]
        acc_loss, acc_reward = driver._acc_loss.reshape(P).tolist(), driver._acc_reward.reshape(P).tolist()
        rew_t, loss_t, tr_t = (x.reshape(max_steps, P).tolist()
                               for x in (driver._tick_reward, driver._tick_loss, driver._tick_trained))
        driver._check_episode()
        for m, t in enumerate(trainers):
            average_loss = acc_loss[m] / max_steps
            ep_reward = acc_reward[m]
            # the per-tick scalars of the episode (train_gcn_dqn.py:136,174)
            for i in range(max_steps):
                t.writer.add_scalar("Reward", rew_t[i][m], ticks + i + 1)
                if tr_t[i][m]:
                    t.writer.add_scalar("Loss", loss_t[i][m], ticks + i + 1)
            t.episode_losses.append(average_loss)
            t.rewards_buffer.append(torch.tensor(ep_reward))
            if (episode + 1) % 10 == 0:
                t.episode_rewards.append(sum(t.rewards_buffer) / 10)
                t.rewards_buffer = []
            print(f"{prefix.format(seed=t.seed)}Episode {episode}, Loss: {average_loss}, "
                  f"Reward: {ep_reward * t.env.n_agents}, Epsilon: {epsilon[m] if per_member_eps else epsilon}")
        ticks += max_steps
        if eval_every is not None and (episode + 1) % eval_every == 0:
            for t, res in zip(trainers, driver._evaluate(ev, max_steps)):
                t.eval_rows.append(eval_row(episode, res, max_steps))
        if pbt_every is not None and (episode + 1) % pbt_every == 0:
            driver._pbt_round(episode, (episode + 1) // pbt_every - 1, dict(config.get("pbt", {})))
    print("Training completed")
    for t in trainers:
        t._sync_models()
        os.makedirs(t.models_path, exist_ok=True)
        torch.save(t.model.state_dict(), f"{t.models_path}/experiment_{t.experiment}-seed_{t.seed}.pth")
        t.save_metrics_to_csv()
        if eval_every is not None:
            t.save_eval_to_csv()
        if pbt_every is not None:
            t.save_pbt_to_csv()
    print(saved)


class SimpleAdamView:
    """Exposes the device Adam state the way code inspecting ``trainer.optimizer`` expects."""

    def __init__(self, engine: SwarmEngine):
        self.engine = engine

    def state_dict(self):
        e = self.engine
        return {"step": e.read_ctrl()["adam_step"], "exp_avg": e.adam_m.cpu(), "exp_avg_sq": e.adam_v.cpu(),
                "lr": e.hp.lr, "betas": (e.hp.beta1, e.hp.beta2), "eps": e.hp.eps}
