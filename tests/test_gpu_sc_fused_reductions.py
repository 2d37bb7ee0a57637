"""The shared-critic late launch's fused fc1 / LN1 reduction strips (obs dim 4) against the four separate reduction
families (flock_set_diag("sc_red_legacy", 1)): every learner tensor bitwise equal.

Shapes are the smallest at which the strips take another path: the reference widths (25 full strips, two full row
batches per row group), a partial last 16-column strip (fc1 40) and a full one (fc1 32) with a batch that is no
multiple of 16 and fills one ragged row batch (40), a batch above 256 (the row-statistics stride and a third row
batch), and obs dim 20, where both knob values must select the four families."""
import pytest
import torch

pytestmark = pytest.mark.gpu

AGENTS = (0, 3, 3, 1, 5, 2, 0)  # a repeated agent; update_rate 3: learns with and without the soft updates

# (obs dim, fc1, fc2, batch)
SHAPES = [(4, 400, 300, 256), (4, 40, 24, 40), (4, 32, 24, 40), (4, 72, 40, 300), (20, 400, 300, 256)]


def _rows(cuda, d, n=600):
    g = torch.Generator(device=cuda).manual_seed(9)
    return (torch.rand(n, d, device=cuda, generator=g), torch.rand(n, 2, device=cuda, generator=g) * 2 - 1,
            torch.rand(n, 1, device=cuda, generator=g), torch.rand(n, d, device=cuda, generator=g),
            torch.rand(n, device=cuda, generator=g) > 0.8)


def _state(L):
    C, A = L.critic, L.actors
    return {"critic": C.data, "critic exp_avg": C.exp_avg, "critic exp_avg_sq": C.exp_avg_sq, "critic grad": C.grad,
            "actors": A.data, "actors target": A.target, "actors exp_avg_sq": A.exp_avg_sq, "actors grad": A.grad,
            "actor_steps": L.actor_steps, "losses": L.losses}


def _learner(cuda, shape, path):
    from marl_range_flocking_amd.learners.shared_critic import SharedCriticLearner

    d, fc1, fc2, B = shape
    L = SharedCriticLearner(6, d, fc1=fc1, fc2=fc2, device=cuda, seed=3, batch_size=B, buffer_size=1000,
                            snapshot=path == "pipeline", n_slots=3, use_graph=False)
    L.store_transitions(*_rows(cuda, d))
    return L


def _learns(L, cuda, path):
    if path == "pipeline":  # merged rounds: a learn's critic phase beside the previous learn's actor phase
        ls = torch.cuda.Stream(device=cuda)
        main = torch.cuda.current_stream(cuda)
        for a in AGENTS:
            assert L.pipeline_learn(a, main.cuda_stream, ls.cuda_stream)
        L.pipeline_flush(ls.cuda_stream)
        main.wait_stream(ls)
    else:  # learn(): the critic phase, then the actor phase, each a launch set of its own
        for a in AGENTS:
            assert L.learn(a)[2]
    torch.cuda.synchronize()


def _grad_round(L):
    """One gradient-only learn (do_adam = 0, as the data-parallel rounds run it) of agent 4 on one rank: the critic
    phase into critic.grad, the actor phase into a caller's bucket (actor_grad_out), no critic view."""
    from marl_range_flocking_amd.learners import shared_critic as sc

    T = sc._ops()
    T.sc_prep(L.static_agent, L.static_idx, len(L.replay), L.seed, 99, 4)
    bucket = torch.zeros(L.actors.per_agent, device=L.device)
    T.sc_round(L._sc_learner, L._sc_job_grads, [], L._sc_dims_grads, L._sc_hyper)
    T.sc_round(L._sc_learner, [], L._sc_job_grads + [bucket], L._sc_dims_grads, L._sc_hyper)
    torch.cuda.synchronize()
    return bucket


@pytest.mark.parametrize("path", ["pipeline", "serial"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "in%d_fc%d_%d_B%d" % s)
def test_fused_strips_equal_four_families(shape, path, cuda):
    from marl_range_flocking_amd import _native

    lib = _native.lib()
    out = []
    try:
        for legacy in (0, 1):
            assert lib.flock_set_diag(b"sc_red_legacy", legacy) == 0  # read when the jobs / the pipeline are built
            L = _learner(cuda, shape, path)
            _learns(L, cuda, path)
            st = {k: v.clone() for k, v in _state(L).items()}
            if path == "serial":
                before = [L.critic.data.clone(), L.actors.data.clone(), L.actor_steps.clone()]
                st["grad-only actor bucket"] = _grad_round(L)
                st["grad-only critic grad"] = L.critic.grad.clone()
                for x, y in zip(before, (L.critic.data, L.actors.data, L.actor_steps)):
                    assert torch.equal(x, y)  # gradients only: no Adam, no step
                assert st["grad-only actor bucket"].abs().sum() > 0
            out.append(st)
    finally:
        lib.flock_set_diag(b"sc_red_legacy", 0)
    a, b = out
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.isfinite(a[k].float()).all(), k
    assert (a["losses"] != 0).all()
    assert a["critic grad"].abs().sum() > 0 and a["actors grad"].abs().sum() > 0
    assert a["actor_steps"].tolist() == [2, 1, 1, 2, 0, 1]
