"""VDN acting at the config-4 size (512 agents x 8192 env rows, n_obs 4, 10 actions), one process, HIP events:

  1. BatchedQNet.sample_action(fused=True) (one flock::vdn_act launch) against fused=False (the torch chain), after a
     warm-up, the two paths alternated ROUNDS times; median and spread (max - min) of the rounds for each, and the
     kernel alone (act_into on pre-drawn coins / ids) against its two floors: moved bytes / HBM rate and
     FLOPs / the f32 MFMA peak.
  2. the actor-driven loop  act -> step (fused ring insert, auto_reset=True, reset=env.any_done) -> train_overlapped
     every 150 steps  beside the same loop on random action ids (bench.py's config-4 workload), ms per step.
  3. the kernel alone at forced row_split values (blocks per agent) and at half the agents.

Prints one JSON line (committed under profiles/vdn_act/).  ENVS / AGENTS / STEPS / ROUNDS override the sizes;
--launches: only three launches of the kernel at the full size (for a counter-collection run of their own)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from marl_range_flocking_amd import FlockConfig, VecFlockEnv
from marl_range_flocking_amd.learners.vdn import VDNLearner

HBM_BPS, MFMA_F32_PEAK = 8.0e12, 157.3e12  # bench.py's roofline constants
dev = torch.device("cuda", 0)
E, N = int(os.environ.get("ENVS", 8192)), int(os.environ.get("AGENTS", 512))
K, NA, EPS, EVERY = 4, 10, 0.1, 150
STEPS, ROUNDS, CALLS = int(os.environ.get("STEPS", 300)), int(os.environ.get("ROUNDS", 3)), 10


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / n


def stats(xs):
    return {"median_ms": float(np.median(xs)), "spread_ms": float(max(xs) - min(xs)),
            "rounds_ms": [float(x) for x in xs]}


def acting():
    L = VDNLearner(N, K, NA, device=dev, seed=0, buffer_limit=16)
    q = L.q
    g = torch.Generator(device=dev).manual_seed(1)
    obs = torch.rand(E, N, K, device=dev, generator=g) * 14
    hid = torch.rand(E, N, 32, device=dev, generator=g) * 2 - 1
    coin = torch.rand(E, device=dev, generator=g)
    rnd = torch.randint(0, NA, (E, N), device=dev, generator=g)
    h_out, ids = torch.empty_like(hid), torch.empty(E, N, dtype=torch.int64, device=dev)
    paths = {"fused": lambda: q.sample_action(obs, hid, EPS, generator=g, fused=True),
             "chain": lambda: q.sample_action(obs, hid, EPS, generator=g, fused=False),
             "kernel": lambda: q.act_into(obs, hid, h_out, ids, coin=coin, rnd=rnd, epsilon=EPS)}
    for fn in paths.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            ms[k].append(timed(fn, CALLS))
    out = {k: stats(v) for k, v in ms.items()}
    rows = E * N
    bytes_row = 4 * K + 128 + 128 + 8 + 8  # obs, h in, h out, int64 id, the random id read
    flop_row = 2 * (64 * K + 32 * 64 + 2 * 96 * 32 + NA * 32)
    km = out["kernel"]["median_ms"] * 1e-3
    out["kernel"].update(bytes_per_row=bytes_row, flop_per_row=flop_row,
                         hbm_floor_ms=rows * bytes_row / HBM_BPS * 1e3,
                         mfma_floor_ms=rows * flop_row / MFMA_F32_PEAK * 1e3,
                         hbm_frac=rows * bytes_row / km / HBM_BPS, mfma_frac=rows * flop_row / km / MFMA_F32_PEAK)
    f, c = out["fused"], out["chain"]
    out["speedup"] = c["median_ms"] / f["median_ms"]
    out["faster_beyond_spread"] = bool(c["median_ms"] - f["median_ms"] > max(c["spread_ms"], f["spread_ms"]))
    return out


SPLIT_CASES = ((N, 0), (N, 1), (N, 2), (N, 3), (N, 6), (N // 2, 1), (N // 2, 3), (N // 2, 6), (N, 0))


def splits(cases=SPLIT_CASES, calls=CALLS):
    """The kernel alone (greedy, int64 ids) at forced blocks-per-agent values: the automatic choice against its
    neighbours, and one block per CU against a full device (how much the co-resident blocks hide of each other)."""
    out = []
    for agents, split in cases:
        L = VDNLearner(agents, K, NA, device=dev, seed=0, buffer_limit=16)
        g = torch.Generator(device=dev).manual_seed(1)
        obs = torch.rand(E, agents, K, device=dev, generator=g) * 14
        hid = torch.rand(E, agents, 32, device=dev, generator=g) * 2 - 1
        h_out, ids = torch.empty_like(hid), torch.empty(E, agents, dtype=torch.int64, device=dev)
        fn = lambda: L.q.act_into(obs, hid, h_out, ids, row_split=split)  # noqa: E731
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        ms = timed(fn, calls)
        out.append({"agents": agents, "row_split": split, "ms": ms, "ns_per_row": ms * 1e6 / (agents * E)})
    return out


def loop(actor):
    box = float(round(np.sqrt(250.0 * N)))  # bench.py's density
    env = VecFlockEnv(FlockConfig(variant="uw_discrete", num_envs=E, num_agents=N, k=K, collision_distance=2.5,
                                  range_start=(0, box), sensor_range=14.0, seed=1234, track_indices=False), device=dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    env.positions.copy_(torch.rand(E, N, 2, device=dev, generator=g) * box)
    env.headings.copy_((1.0 - torch.rand(E, N, device=dev, generator=g)) * (np.pi / 1.2))
    pool = [torch.randint(0, NA, (E, N), device=dev, generator=g) for _ in range(8)]
    L = VDNLearner(N, K, NA, device=dev, seed=0)
    obs = env.observation()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for s in range(EVERY + STEPS):  # the first EVERY steps warm up (and capture the update's graph)
        if s == EVERY:
            L.sync()
            torch.cuda.synchronize(dev)
            e0.record()
        a = L.act(obs, EPS, reset=env.any_done) if actor else pool[s % len(pool)]
        obs = env.step(a, ring=L.replay_slots(E), auto_reset=True)[0]
        if (s + 1) % EVERY == 0 and L.size() > L.chunk:
            L.train_overlapped()
    L.sync()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / STEPS


if __name__ == "__main__":
    if "--launches" in sys.argv:  # a few launches of the kernel alone, for a counter-collection run
        print(json.dumps(splits(cases=((N, 0),), calls=3)))
        sys.exit(0)
    res = {"tool": "vdn_act_bench", "envs": E, "agents": N, "n_obs": K, "n_actions": NA, "epsilon": EPS,
           "device": torch.cuda.get_device_name(dev), "calls_per_round": CALLS, "sample_action": acting(),
           "row_split": splits()}
    torch.cuda.empty_cache()
    rand_ms = loop(False)
    torch.cuda.empty_cache()
    act_ms = loop(True)
    res["loop"] = {"steps": STEPS, "train_every": EVERY, "random_actions_ms_per_step": rand_ms,
                   "actor_driven_ms_per_step": act_ms}
    print(json.dumps(res))
