"""flock::vdn_act on the GPU: the VDN QNet's acting step of every (env row, agent) in one launch
(csrc/flock_vdn_act.hip) against the torch chain it replaces (BatchedQNet.sample_action(fused=False) / BatchedQNet
forward: learners/vdn/net.py:27-37, :52-58) and against the reference QNet's recorded forward (tests/golden/
learn_vdn*.npz).

Tolerances. q and h' against the chain: rtol 1e-5 / atol 1e-6, the project's acting tolerance (tests/test_gpu_act.py).
Greedy actions must be equal on every (row, agent) whose chain top-2 Q margin exceeds 1e-4 (more than twice the q
tolerance at |q| of 1-2), and at most 1 % of them may fall under that margin. Against the fixtures: rtol 1e-4 / atol
1e-5 (tests/test_gpu_learners.py), actions on rows whose fixture margin exceeds 1e-3. Row split, layouts, exploration,
reset and the action dtype are compared bitwise: a row's result depends on nothing but that row."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
RTOL, ATOL, MARGIN = 1e-5, 1e-6, 1e-4


def _net(A, n, na, cuda, seed=11):
    from marl_range_flocking_amd.learners.vdn import BatchedQNet

    g = torch.Generator(device=cuda).manual_seed(seed)
    return BatchedQNet(A, n, na, device=cuda, generator=g), g


def _inputs(B, A, n, cuda, g):
    obs = torch.rand(B, A, n, device=cuda, generator=g) * 14
    hid = torch.rand(B, A, 32, device=cuda, generator=g) * 2 - 1
    return obs, hid


def _fused(q, obs, hid, coin=None, rnd=None, eps=0.0, reset=None, row_split=0, dtype=torch.float32, want_q=True):
    B, A = obs.shape[:2]
    h = torch.full((B, A, 32), float("nan"), device=obs.device)
    act = torch.full((B, A), -7, dtype=dtype, device=obs.device)
    qo = torch.full((B, A, q.n_actions), float("nan"), device=obs.device) if want_q else None
    q.act_into(obs, hid, h, act, q_out=qo, coin=coin, rnd=rnd, epsilon=eps, reset=reset, row_split=row_split)
    return h, qo, act


def _check_greedy(act, q_ref, margin=MARGIN, max_left_out=0.01):
    """act equals argmax q_ref wherever q_ref's top-2 margin exceeds `margin`; the share left out is bounded."""
    top = q_ref.topk(2, dim=-1).values
    sure = (top[..., 0] - top[..., 1]) > margin
    left_out = (~sure).sum().item()
    print(f"rows under the margin: {left_out} of {sure.numel()}")
    assert left_out <= max_left_out * sure.numel(), (left_out, sure.numel())
    assert torch.equal(act.long()[sure], q_ref.argmax(-1)[sure])
    assert ((act >= 0) & (act < q_ref.shape[-1])).all()
    return left_out


def _against_chain(q, obs, hid, h, qo, act):
    qc, hc = q(obs, hid)
    print("max |q - chain|", (qo - qc).abs().max().item(), "max |h' - chain|", (h - hc).abs().max().item())
    torch.testing.assert_close(qo, qc.contiguous(), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(h, hc.contiguous(), rtol=RTOL, atol=ATOL)
    _check_greedy(act, qc)


SHAPES = [(5, 200, 4, 10, 0), (3, 7, 4, 4, 0), (3, 65, 7, 4, 0), (4, 130, 16, 16, 0), (6, 64, 1, 2, 0),
          (2, 300, 4, 10, 2)]


@pytest.mark.parametrize("A,B,n,na,split", SHAPES, ids=[f"A{a}-B{b}-n{n}-na{na}-s{s}" for a, b, n, na, s in SHAPES])
def test_matches_the_chain(A, B, n, na, split, cuda):
    q, g = _net(A, n, na, cuda)
    assert q.fused_act_ok()
    obs, hid = _inputs(B, A, n, cuda, g)
    h, qo, act = _fused(q, obs, hid, row_split=split)
    _against_chain(q, obs, hid, h, qo, act)
    a2, h2 = q.sample_action(obs, hid, 0.0, generator=g, fused=True)  # the public call, automatic split
    assert a2.dtype == torch.float32 and a2.shape == (B, A) and h2.shape == (B, A, 32)
    if split:  # the row split itself: one, two and five blocks per agent give the same bits
        for s in (1, 5):
            hs, qs, acts = _fused(q, obs, hid, row_split=s)
            assert torch.equal(hs, h) and torch.equal(qs, qo) and torch.equal(acts, act), s
    else:
        assert torch.equal(a2, act) and torch.equal(h2, h)


def test_layouts_and_strided_observations(cuda):
    from marl_range_flocking_amd.learners.core import vdn_act

    A, B, n, na = 3, 150, 4, 10
    q, g = _net(A, n, na, cuda)
    obs, hid = _inputs(B, A, n, cuda, g)
    h, qo, act = _fused(q, obs, hid)
    # agent-major buffers [A, B, .], passed as their transposed views
    obs_am, hid_am = obs.transpose(0, 1).contiguous(), hid.transpose(0, 1).contiguous()
    h_am = torch.zeros(A, B, 32, device=cuda)
    q_am = torch.zeros(A, B, na, device=cuda)
    act_am = torch.zeros(A, B, device=cuda)
    q.act_into(obs_am.transpose(0, 1), hid_am.transpose(0, 1), h_am.transpose(0, 1), act_am.transpose(0, 1),
               q_out=q_am.transpose(0, 1))
    assert torch.equal(h_am.transpose(0, 1), h) and torch.equal(q_am.transpose(0, 1), qo)
    assert torch.equal(act_am.transpose(0, 1), act)
    # a slice of a wider [B, A, k + 3] tensor is read in place (the op gets the strided view itself)
    wide = torch.rand(B, A, n + 3, device=cuda, generator=g)
    wide[:, :, 2:2 + n] = obs
    view = wide[:, :, 2:2 + n]
    assert not view.is_contiguous()
    h2, a2 = torch.zeros_like(h), torch.zeros_like(act)
    vdn_act(view, hid, [q.P.params[k] for k in q.P.shapes], h2, a2)
    assert torch.equal(h2, h) and torch.equal(a2, act)
    with pytest.raises(RuntimeError, match="unit stride"):  # a strided feature dimension cannot be read in place
        vdn_act(wide[:, :, 0:2 * n:2], hid, [q.P.params[k] for k in q.P.shapes], h2, a2)


def test_exploration_and_generator_state(cuda):
    A, B, n, na = 4, 100, 4, 10
    q, g = _net(A, n, na, cuda)
    obs, hid = _inputs(B, A, n, cuda, g)
    coin = torch.rand((B,), device=cuda, generator=g)
    rnd = torch.randint(0, na, (B, A), device=cuda, generator=g)
    h0, _, greedy = _fused(q, obs, hid, coin=coin, rnd=rnd, eps=0.0)
    hg, _, greedy2 = _fused(q, obs, hid)
    assert torch.equal(greedy, greedy2) and torch.equal(h0, hg)
    h3, _, a3 = _fused(q, obs, hid, coin=coin, rnd=rnd, eps=0.3)
    explore = coin <= 0.3
    assert 0 < explore.sum().item() < B
    assert torch.equal(a3[explore], rnd[explore].float()) and torch.equal(a3[~explore], greedy[~explore])
    h1, _, a1 = _fused(q, obs, hid, coin=coin, rnd=rnd, eps=1.0)
    assert torch.equal(a1, rnd.float())
    assert torch.equal(h3, h0) and torch.equal(h1, h0)
    # the fused call consumes the generator exactly as the chain does
    g1, g2 = (torch.Generator(device=cuda).manual_seed(99) for _ in range(2))
    for _ in range(2):
        af, _ = q.sample_action(obs, hid, 0.3, generator=g1, fused=True)
        ac, _ = q.sample_action(obs, hid, 0.3, generator=g2, fused=False)
        top = q(obs, hid)[0].topk(2, dim=-1).values
        diff = af != ac  # exploring rows return the same draws; greedy ones may differ only under the margin
        assert ((top[..., 0] - top[..., 1])[diff] <= MARGIN).all() and diff.sum().item() <= 0.01 * diff.numel()
    assert torch.equal(torch.rand(4, device=cuda, generator=g1), torch.rand(4, device=cuda, generator=g2))


def test_reset_rows_and_action_dtype(cuda):
    A, B, n, na = 3, 70, 4, 10
    q, g = _net(A, n, na, cuda)
    obs, hid = _inputs(B, A, n, cuda, g)
    keep = hid.clone()
    reset = torch.zeros(B, dtype=torch.bool, device=cuda)
    reset[[0, 3]] = True
    h, qo, act = _fused(q, obs, hid, reset=reset)
    assert torch.equal(hid, keep)  # h_in is read only
    zeroed = hid.clone()
    zeroed[[0, 3]] = 0.0
    h2, q2, act2 = _fused(q, obs, zeroed)
    assert torch.equal(h, h2) and torch.equal(qo, q2) and torch.equal(act, act2)
    hu, _, actu = _fused(q, obs, hid, reset=reset.to(torch.uint8))
    assert torch.equal(hu, h) and torch.equal(actu, act)
    assert not torch.equal(h, _fused(q, obs, hid)[0])
    # chain path: reset zeroes the same rows first
    ac, hc = q.sample_action(obs, hid, -1.0, reset=reset)
    torch.testing.assert_close(h, hc.contiguous(), rtol=RTOL, atol=ATOL)
    # int64 ids (what VecFlockEnv.step takes) equal the f32 ids
    _, _, act64 = _fused(q, obs, hid, reset=reset, dtype=torch.int64)
    assert act64.dtype == torch.int64 and torch.equal(act64.float(), act)


def _sd(z, prefix):
    return {k[len(prefix) + 1:]: z[k] for k in z.files if k.startswith(prefix + "/")}


def _check_fixture(q, z, max_left_out, cuda):
    obs, hid = torch.tensor(z["fwd_obs"], device=cuda), torch.tensor(z["fwd_hidden"], device=cuda)
    h, qo, act = _fused(q, obs, hid)
    np.testing.assert_allclose(qo.cpu().numpy(), z["fwd_q"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(h.cpu().numpy(), z["fwd_h"], rtol=1e-4, atol=1e-5)
    fq = torch.tensor(z["fwd_q"], device=cuda)
    n = fq.shape[0] * fq.shape[1]
    left = _check_greedy(act, fq, margin=1e-3, max_left_out=(max_left_out + 0.5) / n)
    assert left <= max_left_out


def test_reference_fixture(cuda):
    from marl_range_flocking_amd.learners.vdn import BatchedQNet

    z = np.load(os.path.join(GOLD, "learn_vdn.npz"))
    m = json.loads(str(z["meta"]))
    q = BatchedQNet(m["n_agents"], m["k"], m["n_actions"], device=cuda)
    q.load_reference_state_dict(_sd(z, "final_q"))
    _check_fixture(q, z, 0, cuda)


def test_reference_fixture_prod(cuda):
    """64 agents: the fixture's forward was recorded after the reference train() (tests/test_gpu_learners.py)."""
    from golden import compact
    from marl_range_flocking_amd.learners.vdn import VDNLearner

    z = np.load(os.path.join(GOLD, "learn_vdn_prod.npz"))
    m = json.loads(str(z["meta"]))
    init = compact.rebuild(m["specs"])
    L = VDNLearner(m["n_agents"], m["k"], m["n_actions"], lr=m["lr"], gamma=m["gamma"], batch_size=m["batch"],
                   chunk_size=m["chunk"], update_iter=m["update_iter"], grad_clip_norm=m["grad_clip_norm"],
                   device=cuda, use_graph=False)
    L.q.load_reference_state_dict(init["q"])
    L.q.load_reference_state_dict(init["target_q"], target=True)
    for t in range(m["T"]):
        L.put(z["s"][t], z["a"][t], z["r"][t], z["s_prime"][t], [int(z["done"][t])])
    L.train(starts=z["starts"])
    _check_fixture(L.q, z, 1, cuda)


def _learner(cuda, seed=5, **kw):
    from marl_range_flocking_amd.learners.vdn import VDNLearner

    return VDNLearner(8, 4, 10, batch_size=8, chunk_size=4, update_iter=3, buffer_limit=300, device=cuda, seed=seed,
                      **kw)


def test_learner_act_carries_and_resets_hidden(cuda):
    E, A, eps = 6, 8, 0.3
    L = _learner(cuda)
    g = torch.Generator(device=cuda).manual_seed(3)
    obs = [torch.rand(E, A, 4, device=cuda, generator=g) * 14 for _ in range(3)]
    reset = torch.tensor([False, True, False, False, True, False], device=cuda)
    masks = [None, reset, None]
    g2 = torch.Generator(device=cuda)
    g2.set_state(L.gen.get_state())
    assert L.act_hidden() is None
    ids, hids = [], []
    for o, m in zip(obs, masks):
        ids.append(L.act(o, eps, reset=m))
        hids.append(L.act_hidden().clone())
    hid = L.q.init_hidden(E)
    for t, (o, m) in enumerate(zip(obs, masks)):  # the chain on the same draws, hidden state chained by hand
        h_in = hid if m is None else hid.masked_fill(m[:, None, None], 0.0)
        qc, _ = L.q(o, h_in)
        st = g2.get_state()
        coin = torch.rand((E,), device=cuda, generator=g2)
        g2.set_state(st)
        ac, hid = L.q.sample_action(o, hid, eps, generator=g2, reset=m)
        assert ids[t].dtype == torch.int64 and ids[t].shape == (E, A)
        torch.testing.assert_close(hids[t], hid.contiguous(), rtol=RTOL, atol=ATOL)
        ex = coin <= eps
        assert torch.equal(ids[t][ex], ac[ex].long())
        if (~ex).any():
            _check_greedy(ids[t][~ex], qc[~ex])
    assert not torch.equal(hids[0], hids[1])
    L.reset_hidden()
    assert torch.count_nonzero(L.act_hidden()).item() == 0
    L.act(torch.rand(3, A, 4, device=cuda), 0.0, greedy=True)  # another E: new buffers
    assert L.act_hidden().shape == (3, A, 32)


def test_learner_act_after_overlapped_train_and_env_ring(cuda):
    from marl_range_flocking_amd import FlockConfig, VecFlockEnv

    E = 6
    out = []
    for overlapped in (True, False):
        L = _learner(cuda)
        g = torch.Generator(device=cuda).manual_seed(17)
        for _ in range(3):
            s, s2 = (torch.rand(60, L.A, 4, device=cuda, generator=g) * 14 for _ in range(2))
            a = torch.randint(0, 10, (60, L.A), device=cuda, generator=g)
            L.put(s, a, torch.rand(60, L.A, device=cuda, generator=g), s2,
                  (torch.rand(60, device=cuda, generator=g) < 0.1).float())
        obs = torch.rand(E, L.A, 4, device=cuda, generator=g) * 14
        before = L.q.P.data.clone()
        L.train_overlapped() if overlapped else L.train()
        ids = L.act(obs, 0.0, greedy=True)  # waits for the overlapped update: reads the new parameters
        out.append((L, ids, L.act_hidden().clone(), obs))
        torch.cuda.synchronize()
        assert not torch.equal(before, L.q.P.data)
    (La, ia, ha, obs), (Lb, ib, hb, _) = out
    torch.testing.assert_close(ha, hb, rtol=RTOL, atol=ATOL)
    qb, _ = Lb.q(obs, Lb.q.init_hidden(E))
    _check_greedy(ia, qb)
    _check_greedy(ib, qb)
    # the ids feed the env step with the fused replay insert as they are
    env = VecFlockEnv(FlockConfig(variant="uw_discrete", num_envs=E, num_agents=La.A, k=4), device=cuda)
    o = env.reset()
    ids = La.act(o, 0.5)
    ring = La.replay_slots(E)
    start = ring.start
    env.step(ids, ring=ring)
    rows = (start + torch.arange(E, device=cuda)) % La.replay.capacity
    assert torch.equal(La.replay.bufs["a"][rows], ids.float())
    assert torch.equal(La.replay.bufs["s"][rows], o if o.dim() == 3 else o.reshape(E, La.A, -1))


def test_config4_size(cuda):
    """512 agents x 8192 rows once (about 1.1 GB): agents 0, 1, 255, 511 against the per-agent chain."""
    A, B, n, na = 512, 8192, 4, 10
    q, g = _net(A, n, na, cuda)
    obs, hid = _inputs(B, A, n, cuda, g)
    h, qo, act = _fused(q, obs, hid, dtype=torch.int64)
    idx = torch.tensor([0, 1, 255, 511], device=cuda)
    P = {k: v[idx] for k, v in q.P.params.items()}
    with torch.no_grad():
        qc, hc = q.forward_am(obs[:, idx].transpose(0, 1).contiguous(), hid[:, idx].transpose(0, 1).contiguous(), P)
    qc, hc = qc.transpose(0, 1), hc.transpose(0, 1)
    torch.testing.assert_close(qo[:, idx], qc, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(h[:, idx], hc, rtol=RTOL, atol=ATOL)
    _check_greedy(act[:, idx], qc)
    assert ((act >= 0) & (act < na)).all() and not torch.isnan(h).any()


def test_opcheck_and_overlap_refusal(cuda):
    from marl_range_flocking_amd.learners.core import _ops

    flock = _ops()
    A, B, n, na = 3, 10, 4, 5
    q, g = _net(A, n, na, cuda)
    obs, hid = _inputs(B, A, n, cuda, g)
    P = [q.P.params[k].detach() for k in q.P.shapes]
    h, act, qo = torch.zeros(B, A, 32, device=cuda), torch.zeros(B, A, device=cuda), torch.zeros(B, A, na, device=cuda)
    coin = torch.rand(B, device=cuda)
    rnd = torch.randint(0, na, (B, A), device=cuda)
    reset = torch.zeros(B, dtype=torch.bool, device=cuda)
    torch.library.opcheck(flock.vdn_act.default, (obs, hid, *P, h, act, qo, coin, rnd, reset, 0.3, 0),
                          test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))
    torch.library.opcheck(flock.vdn_act.default, (obs, hid, *P, h, act.long(), None, None, None, None, 0.0, 2),
                          test_utils=("test_schema", "test_faketensor", "test_aot_dispatch_dynamic"))
    with pytest.raises(RuntimeError, match="overlaps"):
        flock.vdn_act(obs, hid, *P, hid, act, None, None, None, None, 0.0, 0)
    both = torch.zeros(B + 1, A, 32, device=cuda)
    with pytest.raises(RuntimeError, match="overlaps"):
        flock.vdn_act(obs, both[:B], *P, both[1:], act, None, None, None, None, 0.0, 0)
    with pytest.raises(RuntimeError, match="coin and rnd"):
        flock.vdn_act(obs, hid, *P, h, act, None, coin, None, None, 0.3, 0)
    # hidden rows that are not 16-byte aligned: a base pointer off by one float, a row pitch of 33 floats
    off = torch.zeros(B * A * 32 + 4, device=cuda)[1:1 + B * A * 32].view(B, A, 32)
    pitch = torch.zeros(B, A, 33, device=cuda)[:, :, :32]
    for bad in (off, pitch):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            flock.vdn_act(obs, bad, *P, h, act, None, None, None, None, 0.0, 0)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            flock.vdn_act(obs, hid, *P, bad, act, None, None, None, None, 0.0, 0)
