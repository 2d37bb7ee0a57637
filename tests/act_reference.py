"""Inputs and references of the fused shared-critic acting tests (flock_sc_act, csrc/flock_act.hip): a float64 actor
written with elementary ops, actor parameters whose tanh outputs are not saturated, a Python mirror of the launcher's
dispatch, and the sweep table. No tests and no fixtures here: tests/test_act_inputs_cpu.py checks these inputs on the
CPU, tests/test_gpu_act.py uses them on the GPU.

Why the heads are scaled: with mu.weight / mu.bias at U(-0.5, 1) over a positive post-ReLU hidden layer the pre-tanh
sums are in the tens and every output is exactly +-1.0 in f32, whatever fc2 computed. With mu.weight at
U(+-1/sqrt(fc2)) and mu.bias at U(+-0.25) the pre-tanh values stay within +-1.5, where tanh has a slope of 0.18 or more
and an error in one fc2 k-step or column moves the output by hundreds of times the comparison's tolerance.
"""
import math
from collections import OrderedDict

import torch

RTOL, ATOL = 1e-5, 1e-6  # the project's acting tolerance against the f32 torch chain
OBS_SCALE = 14.0         # observations are neighbour distances within the sensor range


def _shapes(in_dim, fc1, fc2):
    from marl_range_flocking_amd.learners.shared_critic import actor_shapes

    return actor_shapes(in_dim, fc1, fc2, 2)


def actor_params(n_agents, in_dim, fc1, fc2, seed, b1_shift=0.0):
    """The ten actor tensors [n_agents, *shape] as f32 CPU tensors, drawn from a CPU generator (the same values on
    every machine): fc1 / fc2 at the reference init U(+-1/sqrt(out_features)), LayerNorm affines U(-0.5, 1)
    (trained-looking, not the init's (1, 0)), mu.weight U(+-1/sqrt(fc2)), mu.bias U(+-0.25); b1_shift is added to every
    fc1.bias."""
    g = torch.Generator().manual_seed(int(seed))
    P = OrderedDict()
    for name, shp in _shapes(in_dim, fc1, fc2).items():
        u = torch.rand((n_agents, *shp), generator=g)
        layer = name.split(".")[0]
        if layer in ("bn1", "bn2"):
            v = u * 1.5 - 0.5
        elif name == "mu.bias":
            v = (u * 2 - 1) * 0.25
        else:  # fc1, fc2 (bound by their out_features, as the reference) and mu.weight (by its in_features)
            bound = 1.0 / math.sqrt(fc2 if layer in ("fc2", "mu") else fc1)
            v = (u * 2 - 1) * bound
        P[name] = v
    if b1_shift:
        P["fc1.bias"] = P["fc1.bias"] + float(b1_shift)
    return P


def trained_actors_(L, seed, b1_shift=0.0):
    """Fill the actors of a SharedCriticLearner with actor_params(...) of its widths, in place. Returns the CPU
    tensors."""
    P = actor_params(L.n_agents, L.input_dim, L.fc1, L.fc2, seed, b1_shift)
    with torch.no_grad():
        for name, v in P.items():
            L.actors.view(L.actors.data, name).copy_(v)
    return P


def learner_params(L):
    """name -> [A, *shape] views of a learner's actor buffer."""
    return {n: L.actors.view(L.actors.data, n) for n in L.actors.shapes}


def case_obs(rows, n_agents, in_dim, seed):
    """Observations [rows, n_agents, in_dim] in [0, 14), f32 on the CPU."""
    g = torch.Generator().manual_seed(1000 + int(seed))
    return torch.rand((rows, n_agents, in_dim), generator=g) * OBS_SCALE


def _layer_norm64(z, w, b):
    mean = z.mean(-1, keepdim=True)
    var = z.var(-1, unbiased=False, keepdim=True)
    return (z - mean) * torch.rsqrt(var + 1e-5) * w.unsqueeze(1) + b.unsqueeze(1)


def actor_forward64(params, obs):
    """The actor of ddpg_network.py:132-141 (fc1 -> LayerNorm -> ReLU -> fc2 -> LayerNorm -> ReLU -> mu -> tanh;
    LayerNorm eps 1e-5, biased variance) in float64 on the CPU, from the f32 parameters [A, *shape] and f32
    observations [rows, A, in] cast up, so it differs from an f32 evaluation by arithmetic only. Written with
    elementary ops; shares nothing with learners.shared_critic.actor_forward. Returns (mu, pre_tanh), [rows, A, 2]."""
    P = {n: v.detach().to("cpu", torch.float64) for n, v in params.items()}
    x = obs.detach().to("cpu", torch.float64).transpose(0, 1)  # [A, rows, in]
    z = torch.matmul(x, P["fc1.weight"].transpose(1, 2)) + P["fc1.bias"].unsqueeze(1)
    h = torch.clamp(_layer_norm64(z, P["bn1.weight"], P["bn1.bias"]), min=0.0)
    z = torch.matmul(h, P["fc2.weight"].transpose(1, 2)) + P["fc2.bias"].unsqueeze(1)
    h = torch.clamp(_layer_norm64(z, P["bn2.weight"], P["bn2.bias"]), min=0.0)
    pre = torch.matmul(h, P["mu.weight"].transpose(1, 2)) + P["mu.bias"].unsqueeze(1)
    return torch.tanh(pre).transpose(0, 1).contiguous(), pre.transpose(0, 1).contiguous()


# ---------------------------------------------------------------------------------------------------- dispatch
LDS_FLOATS = 16384   # 64 KB
KC, KC16_PITCH = 16, 10  # kKC; kBP16 = FLOCK_ACT16_KC + 2


def sc_act_path(in_dim, fc1, fc2):
    """Which kernel flock_sc_act launches for these widths: ("act16", NT), ("act32", NT, INC, staged) or
    ("refused", reason). A MIRROR of csrc/flock_act.hip, to be kept in step with it by hand: the argument check and
    the dispatch at the end of flock_sc_act (the in_dim == 4 switch over (fc2 + 15) / 16 and the two switches over
    nt = (fc2 + 63) / 64), act16_lds / launch_act16 (the 16 x 16 block's LDS), launch_act_tm (the 32 x 32 block's LDS
    and its "too wide" refusal) and launch_act (staged when the kKC-deep chunk buffer still fits 64 KB)."""
    if not (1 <= in_dim <= 16 and fc1 >= 8 and fc1 % 8 == 0 and 1 <= fc2 <= 320):
        return ("refused", "needs 1 <= in_dim <= 16, fc1 a multiple of 8, 1 <= fc2 <= 320")
    inp = (in_dim + 3) & ~3
    nt16 = (fc2 + 15) // 16
    if in_dim == 4 and nt16 in (7, 19, 20):
        if 8 * fc1 + 64 * 4 + 2 * 64 + (5 + KC16_PITCH) * 16 * nt16 <= LDS_FLOATS:
            return ("act16", nt16)
    nt = min(max((fc2 + 63) // 64, 1), 5)
    base = fc1 * inp + 4 * fc1 + 64 * inp + 8 * 64
    if base > LDS_FLOATS:
        return ("refused", "fc1 too wide for the LDS staging")
    staged = base + 64 * nt * (KC + 4) <= LDS_FLOATS
    return ("act32", nt, 4 if in_dim == 4 else 0, staged)


ALL_PATHS = ({("act16", n) for n in (7, 19, 20)}
             | {("act32", nt, inc, stg) for nt in range(1, 6) for inc in (4, 0) for stg in (True, False)})

# The sweep: (n_agents, rows, in_dim, fc1, fc2). Together: every instantiation of ALL_PATHS; the fc2 tile edges of the
# 16 x 16 kernel (97, 112, 289, 304, 305, 320) and of the 32 x 32 kernel (32/33, 64/65, 128/129, 192/193, 256/257);
# fc1 8, 24, 40 (the staged 32 x 32 kernel's half-filled last chunk, fc1 % 16 == 8); in_dim 1, 3, 4, 7, 12, 16; rows 1,
# 63, 64, 65, 130; n_agents * ceil(rows / 64) a multiple of 8 (8, 16, 24: the XCD work map) and not.
CASES = [
    (4, 130, 4, 64, 97),      # act16<7>, 12 work items
    (8, 65, 4, 24, 112),      # act16<7>, 16 work items, half chunk
    (3, 64, 4, 40, 289),      # act16<19>
    (8, 130, 4, 400, 304),    # act16<19>, 24 work items, the reference fc1
    (5, 63, 4, 72, 305),      # act16<20>
    (2, 1, 4, 8, 320),        # act16<20>, fc1 8, one row
    (3, 65, 4, 8, 1),         # act32<1, 4, staged>, fc2 1: LayerNorm-2 erases fc2
    (8, 64, 4, 40, 32),       # act32<1, 4, staged>, 8 work items, the second column half empty
    (3, 63, 4, 24, 65),       # act32<2, 4, staged>
    (2, 130, 4, 48, 129),     # act32<3, 4, staged>
    (1, 65, 4, 56, 193),      # act32<4, 4, staged>
    (4, 1, 4, 16, 257),       # act32<5, 4, staged>
    (1, 65, 4, 1800, 33),     # act32<1, 4, global>
    (2, 63, 4, 1640, 128),    # act32<2, 4, global>
    (1, 130, 4, 1480, 192),   # act32<3, 4, global>
    (2, 64, 4, 1320, 256),    # act32<4, 4, global>
    (8, 1, 4, 1160, 288),     # act32<5, 4, global>, 8 work items
    (3, 65, 3, 8, 33),        # act32<1, 0, staged>, in_dim 3, fc1 8
    (6, 130, 1, 24, 64),      # act32<1, 0, staged>, in_dim 1
    (8, 130, 12, 40, 128),    # act32<2, 0, staged>, in_dim 12, 24 work items
    (5, 64, 16, 88, 192),     # act32<3, 0, staged>, in_dim 16
    (7, 63, 7, 104, 256),     # act32<4, 0, staged>, in_dim 7
    (2, 65, 3, 120, 320),     # act32<5, 0, staged>
    (8, 130, 16, 680, 64),    # act32<1, 0, global>, 24 work items
    (1, 63, 16, 616, 65),     # act32<2, 0, global>
    (4, 64, 16, 552, 129),    # act32<3, 0, global>
    (2, 130, 16, 488, 193),   # act32<4, 0, global>
    (3, 65, 16, 424, 320),    # act32<5, 0, global>
    (2, 65, 12, 552, 300),    # act32<5, 0, global>, in_dim 12
]


def case_id(c):
    return f"a{c[0]}_r{c[1]}_in{c[2]}_{c[3]}x{c[4]}"


def case_seed(c):
    """The seed of a sweep case's parameters and observations."""
    return 11 + CASES.index(tuple(c))
