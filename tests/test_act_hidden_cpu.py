"""learners.core.ActHidden (the swapped hidden-state pair behind VDNLearner.act / MADDPGLearner.act) and act_obs (the
observation normalisation of both act_into methods), on CPU tensors: no kernel runs."""
import torch

from marl_range_flocking_amd.learners.core import ActHidden, act_obs


def test_first_use_allocates_zeros():
    st = ActHidden(3, 32, "cpu")
    assert st.current() is None
    st.zero()  # nothing to clear yet: no error, still nothing allocated
    assert st.current() is None
    h_in, h_out = st.pair(5)
    for h in (h_in, h_out):
        assert h.shape == (5, 3, 32) and h.dtype == torch.float32 and torch.count_nonzero(h) == 0
    assert h_in.data_ptr() != h_out.data_ptr()
    assert st.current() is h_in


def test_same_E_keeps_the_buffers_and_a_new_E_reallocates_zeros():
    st = ActHidden(2, 32, "cpu")
    h_in, h_out = st.pair(4)
    h_in.fill_(1.0)
    h_out.fill_(2.0)
    again = st.pair(4)
    assert again[0] is h_in and again[1] is h_out and torch.all(h_in == 1.0) and torch.all(h_out == 2.0)
    n_in, n_out = st.pair(6)
    for h in (n_in, n_out):
        assert h.shape == (6, 2, 32) and torch.count_nonzero(h) == 0
    assert torch.all(h_in == 1.0) and torch.all(h_out == 2.0)  # the old pair is left alone


def test_swap_exchanges_the_roles():
    st = ActHidden(2, 32, "cpu")
    h_in, h_out = st.pair(4)
    st.swap()
    assert st.current() is h_out
    s_in, s_out = st.pair(4)
    assert s_in is h_out and s_out is h_in
    st.swap()
    assert st.pair(4)[0] is h_in


def test_zero_clears_only_the_current_input_buffer():
    st = ActHidden(2, 32, "cpu")
    h_in, h_out = st.pair(4)
    h_in.fill_(1.0)
    h_out.fill_(2.0)
    st.zero()
    assert torch.count_nonzero(h_in) == 0 and torch.all(h_out == 2.0)
    st.swap()
    st.zero()
    assert torch.count_nonzero(h_out) == 0


def test_act_obs_copies_only_what_the_kernels_cannot_read():
    x = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    assert act_obs(x) is x
    wide = torch.zeros(2, 3, 7)[:, :, :4]  # a slice of a wider tensor: unit last stride, read in place
    assert act_obs(wide) is wide
    am = torch.zeros(3, 2, 4).transpose(0, 1)  # agent-major storage: still a unit last stride
    assert act_obs(am) is am
    t = x.transpose(1, 2)  # last stride 4
    y = act_obs(t)
    assert y.stride(-1) == 1 and torch.equal(y, t)
    d = act_obs(x.double())
    assert d.dtype == torch.float32 and torch.equal(d, x)
    one = torch.zeros(2, 3, 5)[:, :, 2:3]  # a single column: its stride does not matter
    assert act_obs(one) is one
