"""RNN-MADDPG acting (1024 agents, k 4, hidden 400/300), one process, HIP events:

  1. at 1024 agents x 2048 env rows (the torch chain's scratch fits there): MADDPGLearner.get_actions(fused=True) (one
     flock::maddpg_act launch on the chain's own OU draw) against fused=False (the torch chain, the code path of the
     commit before the kernel), after a warm-up, the two paths alternated ROUNDS times; median and spread (max - min)
     of the rounds for each, and the kernel alone (act_into on a pre-drawn noise tensor) against its two floors: moved
     bytes / HBM rate and FLOPs / the f32 MFMA peak.
  2. the kernel alone at forced row_split values (blocks per agent).
  3. the kernel alone at config 5's own shape, 1024 x 16384 (the chain is not run there).

Prints one JSON line (committed under profiles/maddpg_act/).  ENVS / BIG_ENVS / AGENTS / ROUNDS override the sizes;
--launches: only three launches of the kernel at 1024 x ENVS (for a counter-collection run of their own)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from marl_range_flocking_amd.learners.core import FlatParams, maddpg_act
from marl_range_flocking_amd.learners.maddpg import MADDPGLearner, _init, actor_shapes

HBM_BPS, MFMA_F32_PEAK = 8.0e12, 157.3e12  # bench.py's roofline constants
dev = torch.device("cuda", 0)
E, BIG_E, N = int(os.environ.get("ENVS", 2048)), int(os.environ.get("BIG_ENVS", 16384)), int(os.environ.get("AGENTS", 1024))
K, H1, H2 = 4, 400, 300
ROUNDS, CALLS = int(os.environ.get("ROUNDS", 5)), 5
BYTES_ROW = 4 * K + 128 + 128 + 8 + 8  # obs, h in, h out, the noise pair, the action pair
FLOP_ROW = 2 * (32 * K + 2 * 96 * 32 + H1 * 32 + H2 * H1 + 2 * H2)


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


def floors(ms, rows):
    s = ms * 1e-3
    return {"bytes_per_row": BYTES_ROW, "flop_per_row": FLOP_ROW, "hbm_floor_ms": rows * BYTES_ROW / HBM_BPS * 1e3,
            "mfma_floor_ms": rows * FLOP_ROW / MFMA_F32_PEAK * 1e3, "hbm_frac": rows * BYTES_ROW / s / HBM_BPS,
            "mfma_frac": rows * FLOP_ROW / s / MFMA_F32_PEAK, "ns_per_row": ms * 1e6 / rows}


def inputs(envs, g):
    obs = torch.rand(envs, N, K, device=dev, generator=g) * 14
    hid = torch.rand(envs, N, 32, device=dev, generator=g) * 2 - 1
    noise = torch.randn(envs, N, 2, device=dev, generator=g) * 0.02
    return obs, hid, noise


def acting(L):
    g = torch.Generator(device=dev).manual_seed(1)
    obs, hid, noise = inputs(E, g)
    hid_ne = hid.transpose(0, 1).contiguous()  # get_actions' [N, E, 32]
    h_out, act = torch.empty_like(hid), torch.empty(E, N, 2, device=dev)
    paths = {"fused": lambda: L.get_actions(obs, hid_ne, fused=True),
             "chain": lambda: L.get_actions(obs, hid_ne, fused=False),
             "kernel": lambda: L.act_into(obs, hid, h_out, act, noise=noise)}
    for fn in paths.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            ms[k].append(timed(fn, CALLS))
    out = {k: stats(v) for k, v in ms.items()}
    out["kernel"].update(floors(out["kernel"]["median_ms"], E * N))
    f, c = out["fused"], out["chain"]
    out["speedup"] = c["median_ms"] / f["median_ms"]
    out["faster_beyond_spread"] = bool(c["median_ms"] - f["median_ms"] > max(c["spread_ms"], f["spread_ms"]))
    split = []
    for s in (0, 1, 2, 4, 8):
        fn = lambda: L.act_into(obs, hid, h_out, act, noise=noise, row_split=s)  # noqa: E731
        fn()
        split.append({"row_split": s, "ms": timed(fn, CALLS)})
    return out, split


def config5(L):
    g = torch.Generator(device=dev).manual_seed(2)
    obs, hid, noise = inputs(BIG_E, g)
    h_out, act = torch.empty_like(hid), torch.empty(BIG_E, N, 2, device=dev)
    fn = lambda: L.act_into(obs, hid, h_out, act, noise=noise)  # noqa: E731
    fn()
    out = stats([timed(fn, 3) for _ in range(ROUNDS)])
    out.update(floors(out["median_ms"], BIG_E * N))
    return out


def launches():
    """Three launches of the kernel alone on stacked actor parameters (no learner, no chain)."""
    g = torch.Generator(device=dev).manual_seed(1)
    P = FlatParams(actor_shapes(K, H1, H2, True), dev, N, adam=False)
    _init(P, g)
    obs, hid, noise = inputs(E, g)
    h_out, act = torch.empty_like(hid), torch.empty(E, N, 2, device=dev)
    params = [P.view(P.data, n) for n in P.shapes]
    for _ in range(3):
        maddpg_act(obs, hid, params, h_out, act, noise=noise)
    torch.cuda.synchronize(dev)
    return {"agents": N, "envs": E, "launches": 3}


if __name__ == "__main__":
    if "--launches" in sys.argv:
        print(json.dumps(launches()))
        sys.exit(0)
    L = MADDPGLearner(N, K, recurrent=True, hidden1=H1, hidden2=H2, batch_size=8, chunk_size=2, buffer_capacity=16,
                      min_size_buffer=8, device=dev, seed=0, use_graph=False)
    res = {"tool": "maddpg_act_bench", "agents": N, "envs": E, "k": K, "hidden": [H1, H2],
           "device": torch.cuda.get_device_name(dev), "calls_per_round": CALLS}
    res["get_actions"], res["row_split"] = acting(L)
    torch.cuda.empty_cache()
    res["config5_kernel"] = dict(envs=BIG_E, **config5(L))
    print(json.dumps(res))
