"""flock::maddpg_act (the MADDPG actors' fused acting step, csrc/flock_maddpg_act.hip) without a GPU: the schema
carries the mutation annotations, the Meta kernel runs the op's own checks, CPU tensors are refused (no CPU kernel),
the C entry rejects bad arguments with its return codes before any launch, the ctypes signature has the header's
argument count, and the chain path's reset mask equals zeroing those rows' hidden state by hand."""
import ctypes
import os
import re

import pytest
import torch

from marl_range_flocking_amd import _native, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def flock():
    build.build()
    from marl_range_flocking_amd import torch_ops

    return torch_ops.load()


def _params(A, k, h1, h2, rec, e, d):
    from marl_range_flocking_amd.learners.maddpg import actor_shapes

    return [e(A, *shp, **d) for shp in actor_shapes(k, h1, h2, rec).values()]


def _args(B=10, A=3, k=4, h1=40, h2=20, H=32, rec=True, device="meta", noise=True, reset=True):
    d = dict(device=device)
    e = torch.empty if device == "meta" else torch.zeros
    return [e(B, A, k, **d), e(B, A, H, **d) if rec else None, _params(A, k, h1, h2, rec, e, d),
            e(B, A, H, **d) if rec else None, e(B, A, 2, **d), e(B, A, 2, **d) if noise else None,
            e(B, dtype=torch.bool, **d) if reset else None, 0]


def test_schema_annotations(flock):
    s = str(flock.maddpg_act.default._schema)
    for arg in ("Tensor obs", "Tensor? h_in", "Tensor[] params", "Tensor(a!)? h_out", "Tensor(b!) action",
                "Tensor? noise", "Tensor? reset", "int row_split"):
        assert arg in s, arg
    assert s.endswith("-> ()")


def test_meta_kernel_accepts_good_shapes(flock):
    flock.maddpg_act(*_args())
    flock.maddpg_act(*_args(rec=False, k=9))
    flock.maddpg_act(*_args(noise=False, reset=False))
    flock.maddpg_act(*_args(k=16, h1=512, h2=320))
    flock.maddpg_act(*_args(k=1, h1=8, h2=1))
    a = _args(k=16)
    a[0] = torch.empty(10, 3, 19, device="meta")[:, :, :16]  # a slice of a wider observation tensor
    flock.maddpg_act(*a)
    a = _args()
    for i in (0, 1, 3, 4, 5):  # agent-major buffers as transposed views
        a[i] = torch.empty(3, 10, a[i].shape[2], device="meta").transpose(0, 1)
    flock.maddpg_act(*a)


def test_meta_kernel_raises_the_ops_errors(flock):
    with pytest.raises(RuntimeError, match=r"k must be in \[1, 16\]"):
        flock.maddpg_act(*_args(k=17))
    with pytest.raises(RuntimeError, match=r"h1 must be a multiple of 8 in \[8, 512\]"):
        flock.maddpg_act(*_args(h1=36))
    with pytest.raises(RuntimeError, match=r"h1 must be a multiple of 8 in \[8, 512\]"):
        flock.maddpg_act(*_args(h1=520))
    with pytest.raises(RuntimeError, match=r"h2 must be in \[1, 320\]"):
        flock.maddpg_act(*_args(h2=321))
    with pytest.raises(RuntimeError, match=r"hidden state must be \[B, A, 32\]"):
        flock.maddpg_act(*_args(H=16))
    a = _args()
    a[2] = a[2][:13]  # a wrong parameter count
    with pytest.raises(RuntimeError, match="14 .recurrent. or 6 .feed-forward."):
        flock.maddpg_act(*a)
    a = _args(rec=False)
    a[1] = torch.empty(10, 3, 32, device="meta")  # a hidden state with the feed-forward actor
    with pytest.raises(RuntimeError, match="h_in and h_out go with the recurrent"):
        flock.maddpg_act(*a)
    a = _args()
    a[2][8] = torch.empty(3, 20, 48, device="meta")  # fc2.weight against fc1's width
    with pytest.raises(RuntimeError, match="fc2.weight must have shape"):
        flock.maddpg_act(*a)
    a = _args()
    a[3] = torch.empty(10, 3, 33, device="meta")
    with pytest.raises(RuntimeError, match="h_out must have shape"):
        flock.maddpg_act(*a)
    a = _args()
    a[4] = torch.empty(10, 3, 2, dtype=torch.float64, device="meta")
    with pytest.raises(RuntimeError, match="action must be Float"):
        flock.maddpg_act(*a)
    a = _args()
    a[0] = a[0].to(torch.float16)
    with pytest.raises(RuntimeError, match="obs must be Float"):
        flock.maddpg_act(*a)
    a = _args()
    a[6] = torch.empty(10, dtype=torch.int32, device="meta")
    with pytest.raises(RuntimeError, match="reset must be bool or uint8"):
        flock.maddpg_act(*a)
    a = _args()
    a[0] = torch.empty(10, 3, 8, device="meta")[:, :, ::2]
    with pytest.raises(RuntimeError, match="obs must have a unit stride"):
        flock.maddpg_act(*a)
    a = _args()
    a[7] = -1
    with pytest.raises(RuntimeError, match="row_split must be >= 0"):
        flock.maddpg_act(*a)


def test_cpu_tensors_are_refused(flock):
    with pytest.raises(NotImplementedError):
        flock.maddpg_act(*_args(device="cpu"))


def test_ctypes_signature_has_the_headers_argument_count():
    text = open(os.path.join(ROOT, "include", "flock_learn.h")).read()
    m = re.search(r"int flock_maddpg_act\((.*?)\);", text, re.S)
    assert m, "flock_maddpg_act is not declared in include/flock_learn.h"
    n_header = len([a for a in m.group(1).split(",") if a.strip()])
    assert len(_native.SIGNATURES["flock_maddpg_act"]) == n_header == 38


def test_c_entry_return_codes_without_a_launch():
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_float * 64)()  # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = ctypes.c_void_p(p.value + 4)

    def call(A=2, B=8, k=4, h1=40, h2=20, rec=1, gru=p, fc=p, obs=p, h_in=p, h_out=p, action=p, fc2=None, split=0,
             hs=(64, 32)):
        return lib.flock_maddpg_act(None, A, B, k, h1, h2, rec, *([gru] * 6), fc, fc, fc2 or fc, fc, fc, fc, gru, gru,
                                    obs, 8, 4, h_in, *hs, h_out, *hs, action, 4, 2, None, 0, 0, None, split)

    assert call(fc=None) == -3
    assert b"NULL" in lib.flock_learn_last_error()
    assert call(obs=None) == -3 and call(action=None) == -3
    assert call(gru=None) == -3 and call(h_in=None) == -3 and call(h_out=None) == -3
    assert call(k=0) == -2 and call(k=17) == -2
    assert b"k must" in lib.flock_learn_last_error()
    assert call(h1=0) == -2 and call(h1=36) == -2 and call(h1=520) == -2
    assert call(h2=0) == -2 and call(h2=321) == -2
    assert call(split=-1) == -5
    assert call(fc2=off) == -5
    assert call(hs=(66, 33)) == -5  # hidden rows off the 16-byte grid
    assert call() == -5  # h_out is h_in
    assert b"overlaps" in lib.flock_learn_last_error()
    assert call(B=0, fc=None, obs=None) == 0 and call(A=0) == 0


def test_fused_act_ok_needs_a_hip_device():
    from marl_range_flocking_amd.learners.maddpg import MADDPGLearner

    L = MADDPGLearner(2, 4, hidden1=16, hidden2=8, batch_size=4, chunk_size=2, buffer_capacity=16, min_size_buffer=4,
                      device="cpu", use_graph=False)
    assert not L.fused_act_ok()
    with pytest.raises(RuntimeError, match="fused acting kernel"):
        L.get_actions(torch.zeros(3, 2, 4), None, test=True, fused=True)  # never the torch chain instead


def _torch_gru_cell(x, h, W_ih, W_hh, b_ih, b_hh):
    """nn.GRUCell in plain torch, batched over agents (the package's gru_cell launches a HIP kernel)."""
    gi = torch.baddbmm(b_ih.unsqueeze(1), x, W_ih.transpose(1, 2))
    gh = torch.baddbmm(b_hh.unsqueeze(1), h, W_hh.transpose(1, 2))
    ir, iz, inn = gi.chunk(3, -1)
    hr, hz, hn = gh.chunk(3, -1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(inn + r * hn)
    return (h - n) * z + n


@pytest.mark.parametrize("rec", [True, False], ids=["rnn", "ff"])
def test_chain_reset_mask_equals_zeroed_rows(rec, monkeypatch):
    from marl_range_flocking_amd.learners import maddpg
    from marl_range_flocking_amd.learners.maddpg import MADDPGLearner

    monkeypatch.setattr(maddpg, "gru_cell", _torch_gru_cell)  # the GRU gate kernel has no CPU build
    N, E, k = 3, 6, 4
    L = MADDPGLearner(N, k, recurrent=rec, hidden1=16, hidden2=8, batch_size=4, chunk_size=2, buffer_capacity=16,
                      min_size_buffer=4, device="cpu", use_graph=False)
    g = torch.Generator().manual_seed(2)
    obs = torch.rand(E, N, k, generator=g) * 14
    hid = torch.rand(N, E, 32, generator=g) * 2 - 1
    mask = torch.tensor([False, True, False, False, True, False])
    keep = hid.clone()
    a1, h1 = L.get_actions(obs, hid, test=True, fused=False, reset=mask)
    assert torch.equal(hid, keep)  # the caller's hidden state is not written
    zeroed = hid.clone()
    zeroed[:, mask] = 0.0
    a2, h2 = L.get_actions(obs, zeroed, test=True)
    assert torch.equal(a1, a2) and torch.equal(h1, h2)
    a3, h3 = L.get_actions(obs, hid, test=True)  # and without the mask: exactly today's call
    assert torch.equal(a3[~mask], a1[~mask])
    if rec:
        assert not torch.equal(h3, h1)
        a4, _ = L.act(obs, test=True), None  # the loop's call on the chain (no HIP device): zero hidden state
        a5, _ = L.get_actions(obs, None, test=True)
        assert torch.equal(a4, a5) and L.act_hidden().shape == (E, N, 32)
