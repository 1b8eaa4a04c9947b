"""CPU tests of the MLP policy's host side: how policies.pack_mlp / MLPPolicy lay a network out for clothhip_set_policy_mlp, every
shape it refuses, the float64 reference evaluation on a hand-computed example, and the library's new symbols. No GPU."""
import numpy as np
import pytest

from gym_cloth_amd import _lib
from gym_cloth_amd.policies import MLPPolicy, pack_mlp


class FakeEnv(object):
    """What MLPPolicy reads of an env: the grid size, the batch size, and where it uploads itself."""

    def __init__(self, P=4, E=2):
        self.P, self.E, self.uploaded = P, E, None

    def set_policy(self, mlp):
        self.uploaded = mlp


def _layers(widths, seed=0):
    r = np.random.RandomState(seed)
    return [(r.normal(size=(widths[l + 1], widths[l])), r.normal(size=widths[l + 1])) for l in range(len(widths) - 1)]


def test_pack_layout_dtype_and_widths():
    layers = _layers([12, 5, 7, 4], seed=3)
    env = FakeEnv(P=4)
    pol = MLPPolicy(env, layers)
    assert env.uploaded is pol
    widths, blob = pol.pack()
    assert widths.dtype == np.int32 and widths.tolist() == [12, 5, 7, 4]
    assert blob.dtype == np.float32 and blob.flags["C_CONTIGUOUS"]
    assert blob.size == 12 * 5 + 5 + 5 * 7 + 7 + 7 * 4 + 4
    o = 0
    for W, b in layers:                                  # W[out][in] row-major, then b[out], layer after layer
        n_out, n_in = W.shape
        assert np.array_equal(blob[o:o + n_out * n_in].reshape(n_out, n_in), W.astype(np.float32)); o += n_out * n_in
        assert np.array_equal(blob[o:o + n_out], b.astype(np.float32)); o += n_out
    assert o == blob.size
    w1, b1 = pack_mlp(layers[:1] + [(np.zeros((4, 5)), np.zeros(4))])
    assert w1.tolist() == [12, 5, 4] and b1.size == 12 * 5 + 5 + 5 * 4 + 4
    w0, b0 = pack_mlp([(np.ones((4, 12)), np.arange(4.0))])                  # L = 1: a linear policy
    assert w0.tolist() == [12, 4] and np.array_equal(b0[-4:], [0, 1, 2, 3])


@pytest.mark.parametrize("name,layers", [
    ("no layers", []),
    ("five layers", _layers([12, 3, 3, 3, 3, 4])),
    ("not a pair", [(np.zeros((4, 12)),)]),
    ("W not 2-d", [(np.zeros(12), np.zeros(4))]),
    ("b of the wrong shape", [(np.zeros((4, 12)), np.zeros(5))]),
    ("b 2-d", [(np.zeros((4, 12)), np.zeros((4, 1)))]),
    ("widths do not chain", [(np.zeros((5, 12)), np.zeros(5)), (np.zeros((4, 6)), np.zeros(4))]),
    ("wrong input width", _layers([11, 5, 4])),
    ("last width not 4", _layers([12, 5, 3])),
    ("hidden width 257", _layers([12, 257, 4])),
    ("empty hidden layer", [(np.zeros((0, 12)), np.zeros(0)), (np.zeros((4, 0)), np.zeros(4))]),
    ("non-finite weight", [(np.full((4, 12), np.nan), np.zeros(4))]),
    ("non-finite bias", [(np.zeros((4, 12)), np.array([0, np.inf, 0, 0]))]),
])
def test_every_refused_shape_is_a_value_error(name, layers):
    with pytest.raises(ValueError):
        MLPPolicy(FakeEnv(P=4), layers)
    with pytest.raises(ValueError):
        pack_mlp(layers, n_in=12)


def test_hidden_width_256_is_accepted():
    widths, _ = pack_mlp(_layers([12, 256, 1, 4]), n_in=12)
    assert widths.tolist() == [12, 256, 1, 4]


def test_reference_on_a_hand_computed_two_layer_network():
    # P = 1: x = (1, -2, 3). Layer 0: h = relu(W0 x + b0), W0 = [[1, 1, 1], [1, 0, -1]], b0 = (0.5, 1)  ->  relu(2.5, -1) = (2.5, 0)
    # layer 1 (linear): y = W1 h + b1, W1 = [[2, 5], [-1, 5], [0, 5], [0.5, 5]], b1 = (0, 1, -7, 0.25)  ->  (5, -1.5, -7, 1.5)
    layers = [(np.array([[1., 1., 1.], [1., 0., -1.]]), np.array([0.5, 1.0])),
              (np.array([[2., 5.], [-1., 5.], [0., 5.], [0.5, 5.]]), np.array([0., 1., -7., 0.25]))]
    pol = MLPPolicy(FakeEnv(P=1, E=1), layers)
    y = pol.reference(np.array([[1.0, -2.0, 3.0]]))
    assert y.dtype == np.float64 and y.shape == (1, 4)
    assert np.array_equal(y[0], [5.0, -1.5, -7.0, 1.5])
    # the hidden unit the ReLU cut does reach the output once it is positive: x = (1, 2, -3) -> h = (0.5, 5) -> (26, 25.5, 18, 25.5)
    assert np.array_equal(pol.reference(np.array([[1.0, 2.0, -3.0]]))[0], [26.0, 25.5, 18.0, 25.5])
    # the weights are float32, the input is rounded to float32, the arithmetic is float64
    w = np.float32(0.1)
    lin = MLPPolicy(FakeEnv(P=1, E=1), [(np.full((4, 3), 0.1), np.zeros(4))])
    x = np.array([[1.0 / 3.0, 0.0, 0.0]])
    assert lin.reference(x)[0, 0] == float(w) * float(np.float32(1.0 / 3.0))


def test_noise_streams_are_per_env_and_seeded():
    layers = _layers([12, 4])
    a, b = MLPPolicy(FakeEnv(), layers, noise_std=0.5, seed=7), MLPPolicy(FakeEnv(), layers, noise_std=0.5, seed=7)
    d0, d1 = a.draw(0), a.draw(1)
    assert d0.shape == (4,) and not np.array_equal(d0, d1)
    assert np.array_equal(b.draw(1), d1) and np.array_equal(b.draw(0), d0)          # env streams do not depend on the order of use
    assert np.array_equal(d0, np.random.RandomState(7).normal(size=4) * 0.5)
    quiet = MLPPolicy(FakeEnv(), layers)
    assert np.array_equal(quiet.draw(0), np.zeros(4))


def test_library_constants_and_symbols():
    assert _lib.POLICY_MLP == 3
    assert (_lib.POLICY_TABLE, _lib.POLICY_ORACLE_CORNER, _lib.POLICY_HIGHEST_POINT) == (0, 1, 2)
    names = [s[0] for s in _lib.SYMBOLS]
    assert "clothhip_set_policy_mlp" in names and "clothhip_policy_eval" in names
    L = _lib.load()
    assert L.clothhip_abi_version() == _lib.ABI_VERSION == 7
    assert L.clothhip_set_policy_mlp is not None and L.clothhip_policy_eval is not None
    # NULL handle: the calls answer with a status instead of touching a device
    assert L.clothhip_set_policy_mlp(None, 0, None, None, 0) == _lib.EINVAL
    assert L.clothhip_policy_eval(None, None, 0, None) == _lib.EINVAL
