"""The inputs of the fused shared-critic acting tests (tests/act_reference.py), checked on the CPU: the sweep reaches
every kernel instantiation flock_sc_act can launch, its outputs are not saturated, and a missing fc2 k-step or column
would move them by far more than the tolerance the GPU tests compare with. These tests test the tests.
"""
import json
import os

import pytest
import torch

from act_reference import (ALL_PATHS, ATOL, CASES, RTOL, actor_forward64, actor_params, case_id, case_obs, case_seed,
                           sc_act_path)

ERRORS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "act_sweep",
                      "errors.json")


def _case(c):
    A, R, n_in, fc1, fc2 = c
    s = case_seed(c)
    return actor_params(A, n_in, fc1, fc2, s), case_obs(R, A, n_in, s)


def test_sweep_reaches_every_instantiation():
    paths = {sc_act_path(*c[2:]) for c in CASES}
    assert len(ALL_PATHS) == 23
    assert paths == ALL_PATHS, (sorted(ALL_PATHS - paths), sorted(paths - ALL_PATHS))


def test_sweep_covers_the_listed_edges():
    fc2s, fc1s = {c[4] for c in CASES}, {c[3] for c in CASES}
    assert {97, 112, 289, 304, 305, 320} <= {c[4] for c in CASES if c[2] == 4}  # the 16 x 16 kernel's tile edges
    assert {32, 33, 64, 65, 128, 129, 192, 193, 256, 257} <= fc2s and 2 not in fc2s
    assert {8, 24, 40} <= fc1s
    assert {c[2] for c in CASES} >= {1, 3, 4, 7, 12, 16}
    assert {c[1] for c in CASES} >= {1, 63, 64, 65, 130}
    work = {c[0] * ((c[1] + 63) // 64) for c in CASES}
    assert {8, 16, 24} <= work and any(w % 8 for w in work)
    assert all(c[0] <= 8 and c[1] <= 130 for c in CASES)
    # a staged 32 x 32 case whose last 16-deep chunk is half filled
    assert any(sc_act_path(*c[2:])[0] == "act32" and sc_act_path(*c[2:])[3] and c[3] % 16 == 8 for c in CASES)


def test_dispatch_mirror_boundaries():
    """The LDS arithmetic at the widths DESIGN.md states: in_dim 16 stops at fc1 736, in_dim 4 at 1952; the 16 x 16
    kernel hands over to the 32 x 32 kernel past fc1 1784 / 1424 / 1400 (7 / 19 / 20 tiles)."""
    assert sc_act_path(16, 736, 300)[0] == "act32" and sc_act_path(16, 744, 300)[0] == "refused"
    assert sc_act_path(4, 1952, 300) == ("act32", 5, 4, False) and sc_act_path(4, 1960, 300)[0] == "refused"
    for fc2, last in ((100, 1784), (300, 1424), (320, 1400)):
        assert sc_act_path(4, last, fc2)[0] == "act16" and sc_act_path(4, last + 8, fc2)[0] == "act32"
    assert sc_act_path(4, 400, 300) == ("act16", 19)
    assert sc_act_path(4, 1152, 288) == ("act32", 5, 4, True) and sc_act_path(4, 1160, 288) == ("act32", 5, 4, False)
    assert sc_act_path(4, 12, 8)[0] == sc_act_path(17, 16, 8)[0] == sc_act_path(4, 16, 321)[0] == "refused"


def test_fused_act_ok_agrees_with_the_dispatch():
    """SharedCriticLearner.fused_act_ok() (its own statement of the LDS bound) against the mirror, over every in_dim
    and fc1 up to past the widest limit (the launchers themselves: test_gpu_act.py::test_sc_act_lds_limits)."""
    from types import SimpleNamespace

    from marl_range_flocking_amd.learners.shared_critic import SharedCriticLearner

    for n_in in range(0, 18):
        for fc2 in (1, 64, 100, 300, 320, 321):
            for fc1 in range(4, 2000, 4):
                L = SimpleNamespace(n_actions=2, input_dim=n_in, fc1=fc1, fc2=fc2)
                assert SharedCriticLearner.fused_act_ok(L) == (sc_act_path(n_in, fc1, fc2)[0] != "refused"), (
                    n_in, fc1, fc2)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_outputs_have_content(c):
    P, obs = _case(c)
    mu, pre = actor_forward64(P, obs)
    assert float(pre.abs().max()) < 1.5
    assert float(mu.std()) > 0.05


@pytest.mark.parametrize("c", [c for c in CASES if c[4] >= 8], ids=case_id)
def test_outputs_feel_one_k_step_and_one_column(c):
    """Zeroing the last 8-deep k-step of one agent's fc2.weight, or its last valid column, moves that agent's f64
    output by more than 100 times the f32 comparison's tolerance somewhere."""
    P, obs = _case(c)
    agent = c[0] - 1
    mu, _ = actor_forward64(P, obs)
    for what in ("k-step", "column"):
        Q = {n: v.clone() for n, v in P.items()}
        if what == "k-step":
            Q["fc2.weight"][agent, :, -8:] = 0.0
        else:
            Q["fc2.weight"][agent, -1, :] = 0.0
        mu2, _ = actor_forward64(Q, obs)
        moved = (mu2 - mu)[:, agent].abs()
        tol = 100 * (ATOL + RTOL * mu[:, agent].abs())
        assert bool((moved > tol).any()), (what, float(moved.max()))
        others = [a for a in range(c[0]) if a != agent]
        assert torch.equal(mu2[:, others], mu[:, others])


def test_fc2_of_one_column_is_erased():
    """fc2 == 1: LayerNorm over one column is 0 whatever fc2 computed, so mu = tanh(relu(bn2.bias) mu.weight +
    mu.bias). The sweep's fc2 1 case checks the kernel's handling of the width, not its fc2 sum."""
    cases = [c for c in CASES if c[4] == 1]
    assert cases
    for c in cases:
        P, obs = _case(c)
        mu, _ = actor_forward64(P, obs)
        P64 = {n: v.double() for n, v in P.items()}
        h = torch.clamp(P64["bn2.bias"], min=0.0)  # [A, 1]
        want = torch.tanh(h * P64["mu.weight"][:, :, 0] + P64["mu.bias"])  # [A, 2]
        assert torch.equal(mu, want.unsqueeze(0).expand_as(mu))


@pytest.mark.parametrize("A,n_in,fc1,fc2", [(4, 4, 400, 300), (3, 3, 40, 100)])
def test_shifted_outputs_have_content(A, n_in, fc1, fc2):
    """The b1_shift = 100 inputs of the GPU tests: LayerNorm-1 removes the shift, the outputs stay unsaturated."""
    mu, pre = actor_forward64(actor_params(A, n_in, fc1, fc2, 5, b1_shift=100.0), case_obs(65, A, n_in, 5))
    assert float(pre.abs().max()) < 1.5 and float(mu.std()) > 0.05


def test_recorded_errors_give_the_bound():
    """profiles/act_sweep/errors.json: one record per sweep case and M the smallest power of two that is at least
    twice the largest measured e_kernel / e_chain; tests/test_gpu_act.py asserts with that M."""
    import test_gpu_act

    with open(ERRORS) as f:
        rec = json.load(f)
    by_id = {r["case"]: r for r in rec["sweep"]}
    assert set(by_id) == {case_id(c) for c in CASES}
    worst = max(r["e_kernel"] / r["e_chain"] for r in rec["sweep"] + rec["shifted"] if r["e_chain"] > 0)
    m = 1
    while m < 2 * worst:
        m *= 2
    assert rec["M"] == m == test_gpu_act.M_F64
