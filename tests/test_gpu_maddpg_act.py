"""flock::maddpg_act on the GPU: the MADDPG actors' acting step of every (env row, agent) in one launch
(csrc/flock_maddpg_act.hip) against the torch chain it replaces (learners/maddpg.py actor_forward, what
MADDPGLearner.get_actions(fused=False) runs) and against the reference actors' recorded outputs (tests/golden/
learn_maddpg_*.npz).

Tolerances. Actions and h' against the chain: rtol 1e-5 / atol 1e-6, the project's acting tolerance
(tests/test_gpu_act.py, tests/test_gpu_vdn_act.py); inputs are obs in [0, 14) and h in [-1, 1], for which reordering
the 400-term fc2 sum moves the actions by about 6e-8. Against the fixtures: rtol 1e-4 / atol 1e-5
(tests/test_gpu_vdn_act.py). Row split, layouts, noise and reset are compared bitwise: a row's result depends on
nothing but that row and the weights."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
RTOL, ATOL = 1e-5, 1e-6


def _learner(A, k, h1, h2, cuda, recurrent=True, seed=3, **kw):
    from marl_range_flocking_amd.learners.maddpg import MADDPGLearner

    kw = {"batch_size": 8, "chunk_size": 4, "buffer_capacity": 64, "min_size_buffer": 8, **kw}
    return MADDPGLearner(A, k, recurrent=recurrent, hidden1=h1, hidden2=h2, device=cuda, seed=seed, use_graph=False,
                         **kw)


def _inputs(B, A, k, cuda, seed=11):
    g = torch.Generator(device=cuda).manual_seed(seed)
    obs = torch.rand(B, A, k, device=cuda, generator=g) * 14
    hid = torch.rand(B, A, 32, device=cuda, generator=g) * 2 - 1
    return obs, hid


def _fused(L, obs, hid, noise=None, reset=None, row_split=0):
    """One launch into NaN-filled outputs: (actions [B, A, 2], h' [B, A, 32] or None)."""
    B, A = obs.shape[:2]
    act = torch.full((B, A, 2), float("nan"), device=obs.device)
    h = torch.full((B, A, 32), float("nan"), device=obs.device) if L.recurrent else None
    L.act_into(obs, hid if L.recurrent else None, h, act, noise=noise, reset=reset, row_split=row_split)
    return act, h


def _chain(L, obs, hid):
    from marl_range_flocking_amd.learners.maddpg import actor_forward

    P = {n: L.actors.view(L.actors.data, n) for n in L.actors.shapes}
    with torch.no_grad():
        mu, h = actor_forward(P, obs.transpose(0, 1), hid.transpose(0, 1), L.recurrent)
    return mu.transpose(0, 1), h.transpose(0, 1)


SHAPES = [(3, 7, 4, 32, 24, True), (2, 65, 4, 400, 300, True), (5, 130, 16, 40, 20, True), (1, 64, 1, 8, 1, True),
          (4, 200, 7, 512, 320, True), (3, 70, 9, 32, 24, False), (2, 65, 9, 400, 300, False)]


@pytest.mark.parametrize("A,B,k,h1,h2,rec", SHAPES,
                         ids=[f"A{a}-B{b}-k{k}-{h1}x{h2}-{'rnn' if r else 'ff'}" for a, b, k, h1, h2, r in SHAPES])
def test_matches_the_chain(A, B, k, h1, h2, rec, cuda):
    L = _learner(A, k, h1, h2, cuda, recurrent=rec)
    assert L.fused_act_ok()
    obs, hid = _inputs(B, A, k, cuda)
    act, h = _fused(L, obs, hid)
    mu, hc = _chain(L, obs, hid)
    print("max |action - chain|", (act - mu).abs().max().item())
    torch.testing.assert_close(act, mu.contiguous(), rtol=RTOL, atol=ATOL)
    if rec:
        print("max |h' - chain|", (h - hc).abs().max().item())
        torch.testing.assert_close(h, hc.contiguous(), rtol=RTOL, atol=ATOL)
        assert not torch.equal(h, hid)
    if (h1, h2) == (400, 300):  # the row split itself: one, two and five blocks per agent give the same bits
        for s in (1, 2, 5):
            acts, hs = _fused(L, obs, hid, row_split=s)
            assert torch.equal(acts, act), s
            assert not rec or torch.equal(hs, h), s


def _sd(z, prefix):
    return {k[len(prefix) + 1:]: z[k] for k in z.files if k.startswith(prefix + "/")}


@pytest.mark.parametrize("name", ["rnn", "rnn_prod", "ff"])
def test_reference_fixture(name, cuda):
    """get_actions(obs0, None, test=True, fused=True) against the reference actors' recorded choose_action (the actors
    are frozen by the reference's detach, so the fixture's initial actors are the ones that acted)."""
    z = np.load(os.path.join(GOLD, f"learn_maddpg_{name}.npz"))
    m = json.loads(str(z["meta"]))
    N, rec = m["n_agents"], name != "ff"
    L = _learner(N, m["k"], m["hidden1"], m["hidden2"], cuda, recurrent=rec, batch_size=m["batch"],
                 chunk_size=m["chunk"], buffer_capacity=m["capacity"], min_size_buffer=m["batch"])
    if name == "rnn_prod":
        from golden import compact

        L.load_reference_state({tag: sd for tag, sd in compact.rebuild(m["specs"]).items()})
    else:
        nets = ("actor", "critic", "target_actor", "target_critic")
        L.load_reference_state({f"{nm}{i}": _sd(z, f"init/{nm}{i}") for i in range(N) for nm in nets})
    assert L.fused_act_ok()
    acts, hid = L.get_actions(torch.tensor(z["obs"][0], device=cuda), None, test=True, fused=True)
    print("max |action - fixture|", np.abs(acts.cpu().numpy() - z["act_out"]).max())
    np.testing.assert_allclose(acts.cpu().numpy(), z["act_out"], rtol=1e-4, atol=1e-5)
    if rec:
        assert hid.shape == (N, 1, 32)
        np.testing.assert_allclose(hid[:, 0].cpu().numpy(), z["act_hidden"], rtol=1e-4, atol=1e-5)


def test_noise_and_generator_state(cuda):
    A, E, k = 4, 70, 4
    La, Lb = (_learner(A, k, 32, 24, cuda, seed=21) for _ in range(2))
    obs, hid = _inputs(E, A, k, cuda)
    hid_ne = hid.transpose(0, 1).contiguous()  # get_actions' [N, E, 32] layout
    greedy, hg = La.get_actions(obs, hid_ne, test=True, fused=True)
    g2 = torch.Generator(device=cuda)
    g2.set_state(La.gen.get_state())
    noisy, hn = La.get_actions(obs, hid_ne, fused=True)
    # the same SharedOU sample, drawn by hand from a copy of the generator (the process starts at x = 0)
    from marl_range_flocking_amd.learners.maddpg import SharedOU

    rp = La.random_process
    ou = SharedOU(2, rp.theta, rp.mu, rp.sigma, rp.sigma_min, rp.dt, cuda, g2)
    assert torch.equal(noisy, greedy + ou.sample(A, E))
    assert torch.equal(hn, hg) and hn.shape == (A, E, 32)
    # test=True reads no noise: a NaN-filled noise tensor is never passed, and the launch itself adds none
    nan = torch.full((E, A, 2), float("nan"), device=cuda)
    plain, _ = _fused(La, obs, hid)
    assert torch.equal(plain, greedy) and not torch.isnan(greedy).any()
    withnan, _ = _fused(La, obs, hid, noise=nan)
    assert torch.isnan(withnan).all()  # (the tensor is read when it is given)
    # equal seeds, one fused and one chain: the generator and the OU state agree after two calls
    Lc, Ld = (_learner(A, k, 32, 24, cuda, seed=22) for _ in range(2))
    for _ in range(2):
        af, hf = Lc.get_actions(obs, hid_ne, fused=True)
        ac, hc = Ld.get_actions(obs, hid_ne, fused=False)
        torch.testing.assert_close(af, ac, rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(hf, hc, rtol=RTOL, atol=ATOL)
    assert torch.equal(Lc.gen.get_state(), Ld.gen.get_state())
    assert torch.equal(Lc.random_process.x, Ld.random_process.x)
    assert torch.equal(torch.rand(4, device=cuda, generator=Lc.gen), torch.rand(4, device=cuda, generator=Ld.gen))


def test_layouts_and_strided_observations(cuda):
    from marl_range_flocking_amd.learners.core import maddpg_act

    A, B, k = 3, 150, 4
    L = _learner(A, k, 40, 20, cuda)
    obs, hid = _inputs(B, A, k, cuda)
    noise = torch.rand(B, A, 2, device=cuda) - 0.5
    act, h = _fused(L, obs, hid, noise=noise)
    P = [L.actors.view(L.actors.data, n) for n in L.actors.shapes]
    # agent-major buffers [A, B, .], passed as their transposed views
    am = [t.transpose(0, 1).contiguous() for t in (obs, hid, noise)]
    h_am, act_am = torch.zeros(A, B, 32, device=cuda), torch.zeros(A, B, 2, device=cuda)
    L.act_into(am[0].transpose(0, 1), am[1].transpose(0, 1), h_am.transpose(0, 1), act_am.transpose(0, 1),
               noise=am[2].transpose(0, 1))
    assert torch.equal(h_am.transpose(0, 1), h) and torch.equal(act_am.transpose(0, 1), act)
    # a slice of a wider [B, A, k + 3] tensor is read in place (the op gets the strided view itself)
    wide = torch.rand(B, A, k + 3, device=cuda)
    wide[:, :, 2:2 + k] = obs
    view = wide[:, :, 2:2 + k]
    assert not view.is_contiguous()
    h2, a2 = torch.zeros_like(h), torch.zeros_like(act)
    maddpg_act(view, hid, P, h2, a2, noise=noise)
    assert torch.equal(h2, h) and torch.equal(a2, act)
    with pytest.raises(RuntimeError, match="unit stride"):  # a strided feature dimension cannot be read in place
        maddpg_act(wide[:, :, 0:2 * k:2], hid, P, h2, a2)
    with pytest.raises(RuntimeError, match="overlaps"):
        maddpg_act(obs, hid, P, hid, a2)
    both = torch.zeros(B + 1, A, 32, device=cuda)
    with pytest.raises(RuntimeError, match="overlaps"):
        maddpg_act(obs, both[:B], P, both[1:], a2)


@pytest.mark.parametrize("kw", [{"k": 17}, {"h1": 520}, {"h1": 36}, {"h2": 321}], ids=lambda kw: str(kw))
def test_sizes_beyond_the_limits_are_refused(kw, cuda):
    d = {"k": 4, "h1": 32, "h2": 24, **kw}
    L = _learner(2, d["k"], d["h1"], d["h2"], cuda)
    assert not L.fused_act_ok()
    obs, hid = _inputs(5, 2, d["k"], cuda)
    with pytest.raises(RuntimeError, match="fused acting kernel"):
        _fused(L, obs, hid)
    with pytest.raises(RuntimeError, match="fused acting kernel"):
        L.get_actions(obs, None, test=True, fused=True)  # never the torch chain instead
    L.act(obs, test=True)  # the loop's call takes the chain for such a network


def test_reset_rows(cuda):
    A, B, k = 3, 70, 4
    L = _learner(A, k, 32, 24, cuda)
    obs, hid = _inputs(B, A, k, cuda)
    keep = hid.clone()
    reset = torch.zeros(B, dtype=torch.bool, device=cuda)
    reset[[0, 3, 69]] = True
    act, h = _fused(L, obs, hid, reset=reset)
    assert torch.equal(hid, keep)  # h_in is read only
    zeroed = hid.clone()
    zeroed[[0, 3, 69]] = 0.0
    act2, h2 = _fused(L, obs, zeroed)
    assert torch.equal(h, h2) and torch.equal(act, act2)
    actu, hu = _fused(L, obs, hid, reset=reset.to(torch.uint8))
    assert torch.equal(hu, h) and torch.equal(actu, act)
    act0, h0 = _fused(L, obs, hid)  # the other rows are unchanged, the reset ones are not
    assert torch.equal(h0[~reset], h[~reset]) and torch.equal(act0[~reset], act[~reset])
    assert not torch.equal(h0[reset], h[reset])
    # chain path: reset zeroes the same rows first
    ac, hc = L.get_actions(obs, hid.transpose(0, 1).contiguous(), test=True, reset=reset)
    torch.testing.assert_close(act, ac, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(h, hc.transpose(0, 1).contiguous(), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("B", [7, 65])
@pytest.mark.parametrize("rec", [True, False], ids=["rnn", "ff"])
def test_guarded_outputs(B, rec, cuda):
    """h_out and action are views into larger sentinel-filled allocations: the sentinels on both sides stay, every
    element in range is overwritten (the outputs start from NaN)."""
    A, k, pad, S = 3, 4, 2, -777.0
    L = _learner(A, k, 40, 20, cuda, recurrent=rec)
    obs, hid = _inputs(B, A, k, cuda)
    big_h = torch.full((B + 2 * pad, A, 32), S, device=cuda)
    big_a = torch.full((B + 2 * pad, A, 2), S, device=cuda)
    h, act = big_h[pad:pad + B], big_a[pad:pad + B]
    h.fill_(float("nan"))
    act.fill_(float("nan"))
    L.act_into(obs, hid if rec else None, h if rec else None, act)
    assert not torch.isnan(act).any()
    assert (big_a[:pad] == S).all() and (big_a[pad + B:] == S).all()
    assert (big_h[:pad] == S).all() and (big_h[pad + B:] == S).all()
    assert torch.isnan(h).all() if not rec else not torch.isnan(h).any()
    ref, href = _fused(L, obs, hid)
    assert torch.equal(act, ref) and (not rec or torch.equal(h, href))
    # guards inside a row as well: the agents of a wider [B, A + 2, .] allocation
    wide_a = torch.full((B, A + 2, 2), S, device=cuda)
    wide_h = torch.full((B, A + 2, 32), S, device=cuda)
    L.act_into(obs, hid if rec else None, wide_h[:, 1:1 + A] if rec else None, wide_a[:, 1:1 + A])
    assert (wide_a[:, 0] == S).all() and (wide_a[:, -1] == S).all() and torch.equal(wide_a[:, 1:1 + A], ref)
    assert (wide_h[:, 0] == S).all() and (wide_h[:, -1] == S).all()


def test_act_in_the_vectorized_loop(cuda):
    """act(obs, reset=env.any_done) -> step(ring=replay_slots(E), auto_reset=True) for 6 steps on a v2 env. Each step
    is compared with the chain driven the same way: get_actions(fused=False) of an equally seeded learner (the same OU
    draws) on the same observation, reset mask and incoming hidden state."""
    from marl_range_flocking_amd import FlockConfig, VecFlockEnv

    E, N, k = 8, 16, 4
    env = VecFlockEnv(FlockConfig(variant="v2", num_envs=E, num_agents=N, k=k), device=cuda)
    L, Lc = (_learner(N, k, 40, 20, cuda, seed=31, buffer_capacity=40) for _ in range(2))
    assert L.fused_act_ok() and L.act_hidden() is None
    obs = env.reset()["actors"].reshape(E, N, k)
    h_prev = torch.zeros(E, N, 32, device=cuda)
    ptrs = []
    for t in range(6):
        reset = env.any_done.clone()
        o = obs.clone()
        a = L.act(obs, reset=reset)
        ptrs.append(L.act_hidden().data_ptr())
        ac, hc = Lc.get_actions(o, h_prev.transpose(0, 1).contiguous(), fused=False, reset=reset)
        assert a.shape == (E, N, 2) and a.dtype == torch.float32
        torch.testing.assert_close(a, ac, rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(L.act_hidden(), hc.transpose(0, 1).contiguous(), rtol=RTOL, atol=ATOL)
        h_prev = L.act_hidden().clone()
        ring = L.replay_slots(E)
        start = ring.start
        obs = env.step(a, ring=ring, auto_reset=True)[0]["actors"].reshape(E, N, k)
        rows = (start + torch.arange(E, device=cuda)) % L.replay.capacity
        assert torch.equal(L.replay.bufs["action"][rows], a)  # the stored ring actions are the actions returned
        assert torch.equal(L.replay.bufs["state"][rows], o)
    assert ptrs[0] != ptrs[1] and ptrs[::2] == [ptrs[0]] * 3 and ptrs[1::2] == [ptrs[1]] * 3  # two buffers, swapped
    assert torch.equal(L.gen.get_state(), Lc.gen.get_state())
    L.reset_hidden()
    assert torch.count_nonzero(L.act_hidden()).item() == 0
    L.act(torch.rand(3, N, k, device=cuda), test=True)  # another E: new buffers
    assert L.act_hidden().shape == (3, N, 32)


def test_overlap_and_misaligned_hidden_refusal(cuda):
    """Refused by the C entry before any launch: an h_out that overlaps h_in, and hidden rows that are not 16-byte
    aligned (a base pointer off by one float; a row pitch of 33 floats)."""
    from marl_range_flocking_amd.learners.core import _ops

    flock = _ops()
    A, B, k = 2, 3, 4
    L = _learner(A, k, 8, 1, cuda)
    obs, hid = _inputs(B, A, k, cuda)
    P = [L.actors.view(L.actors.data, n).detach() for n in L.actors.shapes]
    h, act = torch.zeros(B, A, 32, device=cuda), torch.zeros(B, A, 2, device=cuda)
    with pytest.raises(RuntimeError, match="overlaps"):
        flock.maddpg_act(obs, hid, P, hid, act, None, None, 0)
    both = torch.zeros(B + 1, A, 32, device=cuda)
    with pytest.raises(RuntimeError, match="overlaps"):
        flock.maddpg_act(obs, both[:B], P, both[1:], act, None, None, 0)
    off = torch.zeros(B * A * 32 + 4, device=cuda)[1:1 + B * A * 32].view(B, A, 32)
    pitch = torch.zeros(B, A, 33, device=cuda)[:, :, :32]
    for bad in (off, pitch):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            flock.maddpg_act(obs, bad, P, h, act, None, None, 0)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            flock.maddpg_act(obs, hid, P, bad, act, None, None, 0)
    assert torch.count_nonzero(h).item() == 0 and torch.count_nonzero(act).item() == 0  # nothing was launched
    flock.maddpg_act(obs, hid, P, h, act, None, None, 0)  # the aligned, disjoint pair is served
    assert torch.isfinite(h).all() and torch.count_nonzero(h).item() > 0


def test_opcheck(cuda):
    from marl_range_flocking_amd.learners.core import _ops

    flock = _ops()
    A, B, k = 3, 10, 4
    obs, hid = _inputs(B, A, k, cuda)
    noise = torch.rand(B, A, 2, device=cuda)
    reset = torch.zeros(B, dtype=torch.bool, device=cuda)
    for rec in (True, False):
        L = _learner(A, k, 32, 24, cuda, recurrent=rec)
        P = [L.actors.view(L.actors.data, n).detach() for n in L.actors.shapes]
        h = torch.zeros(B, A, 32, device=cuda) if rec else None
        act = torch.zeros(B, A, 2, device=cuda)
        torch.library.opcheck(flock.maddpg_act.default, (obs, hid if rec else None, P, h, act, noise, reset, 0),
                              test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))
        torch.library.opcheck(flock.maddpg_act.default, (obs, hid if rec else None, P, h, act, None, None, 2),
                              test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))
