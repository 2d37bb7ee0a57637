"""Fused shared-critic acting (flock_sc_act / torch.ops.flock.sc_act, csrc/flock_act.hip) against the batched torch
chain of the same actors (actor_forward: ddpg_network.py:132-141), a float64 evaluation of the same actor
(act_reference.actor_forward64) and the OU step of choose_action (agent_simple_shared_critic.py:92-107,
OUActionNoiseGPU utils.py:15-18).

Inputs (act_reference.trained_actors_): heads scaled so that every |pre-tanh| < 1.5, the outputs are not saturated and
a wrong fc2 sum shows (tests/test_act_inputs_cpu.py checks that on the CPU).

Tolerances: mu within rtol 1e-5 / atol 1e-6 of the f32 torch chain (both f32; the fc2 sums run in a different order);
against float64, max|kernel - f64| <= max(M_F64 max|chain - f64|, 1e-6) per case, M_F64 from the errors measured over the
sweep (profiles/act_sweep/); the OU state is bitwise the torch op sequence on the same N(0, 1) draws.
"""
import pytest
import torch

from act_reference import (ATOL, CASES, RTOL, actor_forward64, case_id, case_obs, case_seed, learner_params,
                           sc_act_path, trained_actors_)

pytestmark = pytest.mark.gpu

# e_kernel <= max(M_F64 e_chain, ATOL): the smallest power of two that is at least twice the largest e_kernel / e_chain
# measured over the sweep and the shifted cases (profiles/act_sweep/errors.json, tools/act_sweep_errors.py)
M_F64 = 8
SENTINEL = -777.0

WIDTHS = [  # (n_agents, rows, in_dim, fc1, fc2)
    (6, 200, 4, 400, 300),   # the reference widths, rows not a multiple of the 64-row tile
    (5, 7, 4, 16, 8),
    (3, 65, 3, 64, 100),     # runtime observation width, fc2 not a multiple of 32
    (9, 64, 6, 48, 257),
    (4, 130, 4, 64, 100),    # in_dim 4, fc2 100: the 16 x 16 kernel's seven-tile instantiation
]

# (in_dim, fc2) whose fc1 axis is walked to the LDS limits: every 32 x 32 tile count and every 16 x 16 instantiation
LIMIT_WIDTHS = [(4, 32), (4, 128), (4, 192), (4, 256), (4, 288), (4, 100), (4, 300), (4, 320),
                (16, 64), (16, 128), (16, 192), (16, 256), (16, 320)]


def _learner(A, n_in, fc1, fc2, dev, seed=0, fill=7, b1_shift=0.0, **kw):
    from marl_range_flocking_amd.learners.shared_critic import SharedCriticLearner

    L = SharedCriticLearner(A, n_in, fc1=fc1, fc2=fc2, device=dev, seed=seed, buffer_size=64, **kw)
    trained_actors_(L, fill, b1_shift)  # trained-looking LayerNorm affines and unsaturated heads
    return L


def _ou_args(L):
    import math

    o = L.ou
    return float(o["theta"]), float(o["dt"]), float(o["sigma"] * math.sqrt(o["dt"]))


def _launch(L, obs, ou0=None, z=None):
    """torch.ops.flock.sc_act into NaN-filled actions (and ou_state = ou0) that are the first rows of allocations with
    64 more sentinel rows. Returns (actions, ou_state): the tails are checked here."""
    from marl_range_flocking_amd.learners.core import _ops

    R, A = obs.shape[:2]
    big_a = torch.full((R + 64, A, 2), SENTINEL, device=obs.device)
    act = big_a[:R]
    act.fill_(float("nan"))
    big_o = ou = None
    if ou0 is not None:
        big_o = torch.full((R + 64, A, 2), SENTINEL, device=obs.device)
        ou = big_o[:R]
        ou.copy_(ou0)
    _ops().sc_act(obs, L.actors.data, act, ou, z, L.fc1, L.fc2, *_ou_args(L))
    assert not torch.isnan(act).any()
    assert (big_a[R:] == SENTINEL).all()
    if ou0 is not None:
        assert (big_o[R:] == SENTINEL).all()
    return act, ou


def _errors(L, obs, act, spread=True):
    """(e_kernel, e_chain, chain): max |. - f64| of the kernel's and of the f32 torch chain's mu."""
    chain = L.choose_action(obs, noise=False, fused=False)
    mu64, pre = actor_forward64(learner_params(L), obs)
    assert float(pre.abs().max()) < 1.5  # unsaturated: the comparison has content
    assert not spread or float(mu64.std()) > 0.05
    e_kernel = float((act.double().cpu() - mu64).abs().max())
    e_chain = float((chain.double().cpu() - mu64).abs().max())
    return e_kernel, e_chain, chain


@pytest.mark.parametrize("A,R,n_in,fc1,fc2", WIDTHS, ids=[f"{w[3]}x{w[4]}_in{w[2]}" for w in WIDTHS])
def test_sc_act_matches_torch_chain(A, R, n_in, fc1, fc2, cuda):
    L = _learner(A, n_in, fc1, fc2, cuda)
    assert L.fused_act_ok()
    obs = torch.rand(R, A, n_in, device=cuda) * 14
    mu = L.choose_action(obs, noise=False)
    ref = L.choose_action(obs, noise=False, fused=False)
    torch.testing.assert_close(mu, ref, rtol=1e-5, atol=1e-6)
    assert float(mu.abs().max()) < 0.95 and float(mu.std()) > 0.05  # not saturated: the comparison has content


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_sc_act_sweep(c, cuda):
    """Every instantiation flock_sc_act dispatches to, at the tile edges of both kernels (act_reference.CASES)."""
    A, R, n_in, fc1, fc2 = c
    L = _learner(A, n_in, fc1, fc2, cuda, fill=case_seed(c), fused=False)
    assert L.fused_act_ok() and sc_act_path(n_in, fc1, fc2)[0] != "refused"
    obs = case_obs(R, A, n_in, case_seed(c)).to(cuda)
    act, _ = _launch(L, obs)
    e_kernel, e_chain, chain = _errors(L, obs, act)
    print(f"{case_id(c)} {sc_act_path(n_in, fc1, fc2)} e_kernel {e_kernel:.3e} e_chain {e_chain:.3e}")
    torch.testing.assert_close(act, chain, rtol=RTOL, atol=ATOL)
    assert e_kernel <= max(M_F64 * e_chain, ATOL)


@pytest.mark.parametrize("A,R,n_in,fc1,fc2", [(4, 65, 4, 400, 300), (3, 65, 3, 40, 100)], ids=["400x300", "40x100_in3"])
def test_sc_act_shifted_fc1(A, R, n_in, fc1, fc2, cuda):
    """fc1.bias + 100: every fc1 output of a row sits near 100 with a spread of ~1. Guards the c = z(k = 0) shift of
    the kernels' one-pass LayerNorm-1 statistics (unshifted, S2 / n - mean^2 would cancel to nothing in f32). The f32
    chain itself is ~1e-5 off float64 here, so only the float64 bound applies."""
    L = _learner(A, n_in, fc1, fc2, cuda, fill=5, b1_shift=100.0)
    obs = case_obs(R, A, n_in, 5).to(cuda)
    act, _ = _launch(L, obs)
    e_kernel, e_chain, _ = _errors(L, obs, act)
    print(f"shifted {fc1}x{fc2} e_kernel {e_kernel:.3e} e_chain {e_chain:.3e}")
    assert e_kernel <= max(M_F64 * e_chain, ATOL)


@pytest.mark.parametrize("A,R,n_in,fc1,fc2", [(4, 5, 4, 400, 300), (3, 5, 3, 40, 100)], ids=["400x300", "40x100_in3"])
def test_sc_act_constant_row(A, R, n_in, fc1, fc2, cuda):
    """obs all zero and fc1.bias all equal: every fc1 output of a row is the same value, the LayerNorm-1 variance is
    exactly 0 and rstd = 1 / sqrt(1e-5)."""
    L = _learner(A, n_in, fc1, fc2, cuda, fill=5)
    L.actors.view(L.actors.data, "fc1.bias").fill_(0.37)
    obs = torch.zeros(R, A, n_in, device=cuda)
    act, _ = _launch(L, obs)
    chain = L.choose_action(obs, noise=False, fused=False)
    mu64, _ = actor_forward64(learner_params(L), obs)
    e_kernel, e_chain = (float((t.double().cpu() - mu64).abs().max()) for t in (act, chain))
    print(f"constant {fc1}x{fc2} e_kernel {e_kernel:.3e} e_chain {e_chain:.3e}")
    assert float(mu64.std()) > 0.05
    torch.testing.assert_close(act, chain, rtol=RTOL, atol=ATOL)
    assert e_kernel <= max(M_F64 * e_chain, ATOL)


def test_sc_act_ou_state_bitwise(cuda):
    La = _learner(4, 4, 400, 300, cuda, seed=3)
    Lb = _learner(4, 4, 400, 300, cuda, seed=3)
    obs = torch.rand(2, 50, 4, 4, device=cuda) * 14  # two leading dims (envs, sub-envs)
    for _ in range(3):
        a = La.choose_action(obs)
        b = Lb.choose_action(obs, fused=False)
        assert a.shape == b.shape == (2, 50, 4, 2)
        assert torch.equal(La.ou_state, Lb.ou_state)
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("A,R,n_in,fc1,fc2,path", [
    (3, 70, 3, 40, 100, ("act32", 2, 0, True)),
    (2, 70, 16, 424, 320, ("act32", 5, 0, False)),
    (3, 70, 4, 72, 310, ("act16", 20)),
    (2, 70, 4, 400, 300, ("act16", 19)),
], ids=["act32_staged_in3", "act32_global", "act16_20", "act16_19"])
def test_sc_act_ou_state_bitwise_paths(A, R, n_in, fc1, fc2, path, cuda):
    """The OU epilogue of both kernels from a NON-zero state, rows not a multiple of 64, ou_state with a sentinel tail:
    two steps, the state bitwise the torch op sequence of choose_action(fused=False) on the same draws."""
    assert sc_act_path(n_in, fc1, fc2) == path
    L = _learner(A, n_in, fc1, fc2, cuda, seed=3, fused=False)
    obs = case_obs(R, A, n_in, 9).to(cuda)
    ou = (torch.randn(R, A, 2, generator=torch.Generator().manual_seed(4)) * 0.3).to(cuda)
    for _ in range(2):
        gen_state = L.gen.get_state()
        z = torch.randn((R, A, 2), device=cuda, generator=L.gen)  # the draw choose_action makes
        act, ou_new = _launch(L, obs, ou0=ou, z=z)
        L.gen.set_state(gen_state)
        L.ou_state = ou.clone()
        ref = L.choose_action(obs, fused=False)
        assert torch.equal(ou_new, L.ou_state) and not torch.equal(ou_new, ou)
        torch.testing.assert_close(act, ref, rtol=RTOL, atol=ATOL)
        ou = ou_new.clone()


def test_sc_act_bench_size(cuda):
    """4096 env rows x 256 agents (config 3), sampled agents against the torch chain."""
    from marl_range_flocking_amd.learners.shared_critic import actor_forward

    L = _learner(256, 4, 400, 300, cuda)
    obs = torch.rand(4096, 256, 4, device=cuda) * 14
    mu = L.choose_action(obs, noise=False)
    assert float(mu.abs().max()) < 1.0 and float(mu.std()) > 0.05  # no output saturated to +-1
    for i in (0, 1, 77, 255):
        P = {n: L.actors.view(L.actors.data, n, i) for n in L.actors.shapes}
        ref = actor_forward(P, obs[:, i])[0]
        torch.testing.assert_close(mu[:, i], ref, rtol=1e-5, atol=1e-6)


def _fc1_limits(n_in, fc2):
    """Along fc1 (multiples of 8): the last fc1 of every path sc_act_path names, and the first refused one."""
    last = {}
    for fc1 in range(8, 4096, 8):
        p = sc_act_path(n_in, fc1, fc2)
        if p[0] == "refused":
            return last, fc1
        last[p] = fc1
    raise AssertionError("no refusal")


@pytest.mark.parametrize("n_in,fc2", LIMIT_WIDTHS, ids=[f"in{w[0]}_fc2_{w[1]}" for w in LIMIT_WIDTHS])
def test_sc_act_lds_limits(n_in, fc2, cuda):
    """The widest fc1 of every path launches and is right; the next multiple of 8 past the widest of all is refused
    by the launcher, fused_act_ok() says so, and the default choose_action takes the torch chain there."""
    from marl_range_flocking_amd.learners.core import _ops

    last, refused = _fc1_limits(n_in, fc2)
    obs = case_obs(7, 1, n_in, 3).to(cuda)
    for path, fc1 in last.items():
        L = _learner(1, n_in, fc1, fc2, cuda, fused=False)
        assert L.fused_act_ok(), (path, fc1)
        act, _ = _launch(L, obs)
        e_kernel, e_chain, chain = _errors(L, obs, act, spread=False)  # (one agent, 7 rows)
        print(f"in{n_in} {fc1}x{fc2} {path} e_kernel {e_kernel:.3e} e_chain {e_chain:.3e}")
        torch.testing.assert_close(act, chain, rtol=RTOL, atol=ATOL)
    assert refused == max(last.values()) + 8
    L = _learner(1, n_in, refused, fc2, cuda, fused=False)
    assert not L.fused_act_ok()
    act = torch.full((7, 1, 2), SENTINEL, device=cuda)
    with pytest.raises(RuntimeError, match="too wide"):
        _ops().sc_act(obs, L.actors.data, act, None, None, refused, fc2, *_ou_args(L))
    assert (act == SENTINEL).all()
    mu = L.choose_action(obs, noise=False)  # fused=None: the chain, not an error
    assert torch.equal(mu, L.choose_action(obs, noise=False, fused=False))
    mu64, _ = actor_forward64(learner_params(L), obs)
    torch.testing.assert_close(mu.double().cpu(), mu64, rtol=RTOL, atol=ATOL)


def test_sc_act_no_rows(cuda):
    """rows == 0: no launch, no error, nothing written."""
    from marl_range_flocking_amd.learners.core import _ops

    L = _learner(3, 4, 16, 8, cuda)
    big = torch.full((4, 3, 2), SENTINEL, device=cuda)
    big_o = torch.full((4, 3, 2), SENTINEL, device=cuda)
    obs = torch.zeros(0, 3, 4, device=cuda)
    _ops().sc_act(obs, L.actors.data, big[:0], None, None, 16, 8, *_ou_args(L))
    _ops().sc_act(obs, L.actors.data, big[:0], big_o[:0], torch.zeros(0, 3, 2, device=cuda), 16, 8, *_ou_args(L))
    assert (big == SENTINEL).all() and (big_o == SENTINEL).all()
    assert L.choose_action(obs, noise=False).shape == (0, 3, 2)


def test_sc_act_opcheck_and_errors(cuda):
    from marl_range_flocking_amd.learners.core import _ops

    flock = _ops()
    L = _learner(3, 4, 16, 8, cuda)
    obs = torch.rand(10, 3, 4, device=cuda)
    act = torch.empty(10, 3, 2, device=cuda)
    ou = torch.zeros(10, 3, 2, device=cuda)
    z = torch.randn(10, 3, 2, device=cuda)
    torch.library.opcheck(flock.sc_act.default, (obs, L.actors.data, act, ou, z, 16, 8, 0.2, 0.01, 0.015),
                          test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))
    with pytest.raises(RuntimeError, match="fc1 a multiple of 8"):
        flock.sc_act(obs, L.actors.data, act, None, None, 12, 8, 0.2, 0.01, 0.015)
    with pytest.raises(RuntimeError, match="ou_state and noise"):
        flock.sc_act(obs, L.actors.data, act, ou, None, 16, 8, 0.2, 0.01, 0.015)
