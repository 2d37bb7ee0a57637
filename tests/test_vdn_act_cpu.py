"""flock::vdn_act (the VDN QNet's fused acting step, csrc/flock_vdn_act.hip) without a GPU: the schema carries the
mutation annotations, the Meta kernel runs the op's own checks, CPU tensors are refused (no CPU kernel), and the C
entry rejects bad arguments with its return codes before any launch."""
import ctypes

import pytest
import torch

from marl_range_flocking_amd import _native, build


@pytest.fixture(scope="module")
def flock():
    build.build()
    from marl_range_flocking_amd import torch_ops

    return torch_ops.load()


def _args(B=10, A=3, n=4, na=5, H=32, device="meta", coin=True, rnd=True, act_dtype=torch.float32):
    d = dict(device=device)
    e = torch.empty if device == "meta" else torch.zeros
    return [e(B, A, n, **d), e(B, A, H, **d), e(A, 64, n, **d), e(A, 64, **d), e(A, 32, 64, **d), e(A, 32, **d),
            e(A, 96, 32, **d), e(A, 96, 32, **d), e(A, 96, **d), e(A, 96, **d), e(A, na, 32, **d), e(A, na, **d),
            e(B, A, H, **d), e(B, A, dtype=act_dtype, **d), e(B, A, na, **d),
            e(B, **d) if coin else None, e(B, A, dtype=torch.int64, **d) if rnd else None,
            e(B, dtype=torch.bool, **d), 0.1, 0]


def test_schema_annotations(flock):
    s = str(flock.vdn_act.default._schema)
    for arg in ("Tensor obs", "Tensor h_in", "Tensor(a!) h_out", "Tensor(b!) action", "Tensor(c!)? q_out",
                "Tensor? coin", "Tensor? rnd", "Tensor? reset", "float epsilon", "int row_split"):
        assert arg in s, arg
    assert s.endswith("-> ()")


def test_meta_kernel_accepts_good_shapes(flock):
    flock.vdn_act(*_args())
    flock.vdn_act(*_args(act_dtype=torch.int64))
    a = _args(coin=False, rnd=False)
    a[14] = None  # no q_out
    a[17] = None  # no reset
    flock.vdn_act(*a)
    a = _args(n=16, na=16)
    a[0] = torch.empty(10, 3, 19, device="meta")[:, :, :16]  # a slice of a wider observation tensor
    flock.vdn_act(*a)
    a = _args()
    for i in (0, 1, 12):  # agent-major buffers as transposed views
        a[i] = torch.empty(3, 10, a[i].shape[2], device="meta").transpose(0, 1)
    flock.vdn_act(*a)


def test_meta_kernel_raises_the_ops_errors(flock):
    with pytest.raises(RuntimeError, match=r"n_obs must be in \[1, 16\]"):
        flock.vdn_act(*_args(n=17))
    with pytest.raises(RuntimeError, match=r"n_actions must be in \[1, 16\]"):
        flock.vdn_act(*_args(na=17))
    with pytest.raises(RuntimeError, match="hidden width must be 32"):
        flock.vdn_act(*_args(H=16))
    with pytest.raises(RuntimeError, match="coin and rnd go together"):
        flock.vdn_act(*_args(rnd=False))
    a = _args()
    a[12] = torch.empty(10, 3, 33, device="meta")
    with pytest.raises(RuntimeError, match="h_out must have shape"):
        flock.vdn_act(*a)
    a = _args()
    a[13] = torch.empty(10, 3, dtype=torch.int32, device="meta")
    with pytest.raises(RuntimeError, match="action must be float32 or int64"):
        flock.vdn_act(*a)
    a = _args()
    a[0] = torch.empty(10, 3, 8, device="meta")[:, :, ::2]
    with pytest.raises(RuntimeError, match="obs must have a unit stride"):
        flock.vdn_act(*a)


def test_cpu_tensors_are_refused(flock):
    with pytest.raises(NotImplementedError):
        flock.vdn_act(*_args(device="cpu"))


def test_c_entry_return_codes_without_a_launch():
    build.build()
    lib = _native.lib()
    buf = (ctypes.c_float * 64)()  # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(A=2, B=8, n=4, na=5, params=p, obs=p, h_in=p, h_out=p, action=p, coin=None, rnd=None, split=0):
        return lib.flock_vdn_act(None, A, B, n, na, *([params] * 10), obs, 8, 4, h_in, 64, 32, h_out, 64, 32, action,
                                 2, 1, None, 0, 0, coin, rnd, None, 0.0, 0, split)

    assert call(params=None) == -3
    assert b"NULL" in lib.flock_learn_last_error()
    assert call(obs=None) == -3 and call(h_in=None) == -3 and call(h_out=None) == -3 and call(action=None) == -3
    assert call(coin=p) == -3  # coin without rnd
    assert call(n=0) == -2 and call(n=17) == -2
    assert b"n_obs" in lib.flock_learn_last_error()
    assert call(na=0) == -2 and call(na=17) == -2
    assert call(split=-1) == -5
    assert call() == -5  # h_out is h_in
    assert b"overlaps" in lib.flock_learn_last_error()
    assert call(B=0, params=None, obs=None) == 0


def test_fused_act_ok_needs_a_hip_device():
    from marl_range_flocking_amd.learners.vdn import BatchedQNet

    q = BatchedQNet(2, 4, 5, device="cpu")
    assert not q.fused_act_ok()
    with pytest.raises(RuntimeError, match="fused acting kernel"):
        q.sample_action(torch.zeros(3, 2, 4), q.init_hidden(3), 0.0, fused=True)  # never the torch chain instead
