"""``Simulator`` — the reference's scalability-evaluation loop (src/simulation/simulator.py:28-166)
on the device: per episode one ``swarm_rollout`` launch runs ``max_steps`` ticks of
kNN graph -> GAT -> argmax -> env.step with frozen weights and records per-tick
positions, average distance and hits; the CSV outputs keep the reference's
layout (``result.csv``, ``positions/positions_episode_{e}_{x,y}.csv``,
``data/distances_episode_{e}.csv``).  ``knn_k`` defaults to the code's 10; the
reference's committed outputs were produced with 5.  ``graph="radius"`` with
``radius=r`` evaluates on the north_star's radius-neighbour graph instead (not in the
reference).
With ``num_envs`` > 1, metrics are averaged over envs and trajectories of env 0
are written.

``PopulationSimulator`` runs the same loop for several models on one env (the evaluation grid's
model seeds on the same starts): per episode one reset and ONE ``swarm_pop_rollout`` launch for
all models; every model's files are what a lone ``Simulator`` writes.
"""
from __future__ import annotations

import csv
import ctypes
import os
import time

import torch

from . import _lib
from .population import _PopRollout


class Simulator:
    def __init__(self, env, model, episodes, env_name, seed, output_dir="test_stats/", render=False, knn_k: int = 10,
                 graph: str = "knn", radius: float = 0.3):
        self.env = env
        self.model = model
        self.episode_rewards = []
        self.distance_at_the_end = []
        self.distance_at_the_beginning = []
        self.total_collisions = []
        self.episodes = episodes
        self.env_name = env_name
        self.seed = seed
        self.output_dir = output_dir
        self.render = render
        self.knn_k = knn_k
        if graph not in ("knn", "radius"):
            raise ValueError("graph must be 'knn' (simulator.py:15-24) or 'radius'")
        self.graph = _lib.GRAPH_KNN if graph == "knn" else _lib.GRAPH_RADIUS
        self.radius = float(radius)
        self.all_positions_x = []
        self.all_positions_y = []
        self.all_distances = []
        self.all_hits = []

    def run_simulation(self):
        if self.graph == _lib.GRAPH_KNN and self.knn_k > self.env.n_agents:
            raise RuntimeError("selected index k out of range")
        eng = self.env.engine
        params = self.model.flat_params(eng.device)
        saved = (eng.cfg.graph, eng.cfg.knn_k, eng.cfg.conv, eng.cfg.radius, eng.cfg.net)
        eng.cfg.graph, eng.cfg.knn_k, eng.cfg.conv, eng.cfg.radius, eng.cfg.net = self._evaluation_cfg()
        T = self.env.max_steps
        try:
            for episode in range(self.episodes):
                self.env.reset()
                t0 = time.time()
                res = eng.rollout(T, tick0=episode * T, eps=0.0, traj=True, params=params)
                self._record_episode(res, episode, T, t0)
        finally:
            eng.cfg.graph, eng.cfg.knn_k, eng.cfg.conv, eng.cfg.radius, eng.cfg.net = saved
        self.save_metrics_to_csv()

    def _evaluation_cfg(self):
        """(graph, knn_k, conv, radius, net) of the engine's configuration while this model runs"""
        conv = _lib.CONV_GAT if getattr(self.model, "conv", "gat") == "gat" else _lib.CONV_GCN
        net = getattr(self.model, "net_id", _lib.NET_GCN)   # the Flocking checkpoints' GAT3
        return self.graph, self.knn_k, conv, self.radius, net

    def _record_episode(self, res, episode, T, t0):
        """one episode's rollout results (``SwarmEngine.rollout`` with traj=True) into the lists"""
        pos = res["traj_pos"][:, 0].cpu()            # [T, N, 2] env 0
        dist = res["traj_dist"].mean(dim=1).cpu()     # [T]
        hits = res["traj_hits"].mean(dim=1).cpu()
        total_reward = res["reward"].sum(dim=1).mean()
        self.all_positions_x.append(pos[:, :, 0].tolist())
        self.all_positions_y.append(pos[:, :, 1].tolist())
        self.all_distances.append(dist.tolist())
        self.all_hits.append(hits.tolist())
        print(f"It took: {time.time() - t0}s for {T} steps of episode {episode} with "
              f"{float(total_reward)} total reward, on device {self.env.engine.device} for test_gcn_vmas scenario.")
        self.total_collisions.append(hits.sum())
        self.distance_at_the_end.append(dist[-1])
        self.distance_at_the_beginning.append(dist[0])
        self.episode_rewards.append(float(total_reward) / T)

    def save_metrics_to_csv(self):
        where = self.output_dir
        os.makedirs(where, exist_ok=True)
        with open(where + "/result.csv", mode="w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["Episode", "Reward", "Collisions", "Distance (end)", "Distance (beginning)"])
            for i in range(self.episodes):
                w.writerow([i, self.episode_rewards[i], float(self.total_collisions[i]),
                            float(self.distance_at_the_end[i]), float(self.distance_at_the_beginning[i])])
        pdir = f"{where}/positions"
        os.makedirs(pdir, exist_ok=True)
        for axis, allp in (("x", self.all_positions_x), ("y", self.all_positions_y)):
            for i, ep in enumerate(allp):
                with open(f"{pdir}/positions_episode_{i}_{axis}.csv", mode="w", newline="") as f:
                    w = csv.writer(f)
                    w.writerow(["Tick"] + [f"{axis.upper()}{j}" for j in range(len(ep[0]))])
                    for j, row in enumerate(ep):
                        w.writerow([j] + row)
        ddir = f"{where}/data"
        os.makedirs(ddir, exist_ok=True)
        for i in range(len(self.all_distances)):
            with open(f"{ddir}/distances_episode_{i}.csv", mode="w", newline="") as f:
                w = csv.writer(f)
                w.writerow(["Tick", "Distance", "Hits"])
                for j in range(len(self.all_distances[i])):
                    w.writerow([j, self.all_distances[i][j], self.all_hits[i][j]])


class PopulationSimulator:
    """``Simulator.run_simulation`` for several models on one env: ``models[m]``'s outputs go to
    ``output_dirs[m]``.  Each episode is one ``env.reset()``; the start (Flocking's stored spread
    included) is copied into one state buffer per model, and one ``swarm_pop_rollout`` launch runs
    every model's ``max_steps`` ticks.  Every file is byte for byte what a lone ``Simulator`` with
    that model writes from a fresh env of the same seed (tests/test_gpu_pop_rollout.py).  The
    models must share the conv and the net (one configuration per launch).  The env's own state
    stays at the episode's start."""

    def __init__(self, env, models, episodes, env_name, seed, output_dirs, knn_k: int = 10, graph: str = "knn",
                 radius: float = 0.3):
        models, output_dirs = list(models), list(output_dirs)
        if not models or len(models) != len(output_dirs):
            raise ValueError("one output directory per model, and at least one model")
        self.env = env
        self.simulators = [Simulator(env, m, episodes, env_name, seed, output_dir=d, knn_k=knn_k, graph=graph,
                                     radius=radius) for m, d in zip(models, output_dirs)]
        if len({s._evaluation_cfg() for s in self.simulators}) != 1:
            raise ValueError("the models of a PopulationSimulator share one conv and one net")
        self.episodes = episodes

    def run_simulation(self):
        first = self.simulators[0]
        if first.graph == _lib.GRAPH_KNN and first.knn_k > self.env.n_agents:
            raise RuntimeError("selected index k out of range")
        eng = self.env.engine
        P, T = len(self.simulators), self.env.max_steps
        params = [s.model.flat_params(eng.device).contiguous() for s in self.simulators]
        roll = _PopRollout(eng.lib, eng.device, eng.cfg, P)
        c = roll.cfg
        c.graph, c.knn_k, c.conv, c.radius, c.net = first._evaluation_cfg()
        start = eng._state_buf
        states = torch.zeros(P, start.numel(), dtype=torch.float32, device=eng.device)
        for episode in range(self.episodes):
            self.env.reset()
            t0 = time.time()
            states.copy_(start.expand_as(states))
            res = roll.prepare(T, [eng.cfg.seed] * P, [p.data_ptr() for p in params],
                               [states[m].data_ptr() for m in range(P)], episode * T, 0.0, True)
            roll.launch(T)
            for m, sim in enumerate(self.simulators):
                sim._record_episode({k: v[m] for k, v in res.items()}, episode, T, t0)
        for sim in self.simulators:
            sim.save_metrics_to_csv()
