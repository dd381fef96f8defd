"""ctr_actor_load on the host (no GPU): it refuses bad arguments with CTR_EINVAL (-1) and a telling
ctr_last_error before any HIP call (the device pointers are fake and never dereferenced), with the
shape checks of the other actor entry points; the addition is a symbol within ABI 17; an actor
on the host has no blob to load into."""
import ctypes

import numpy as np
import pytest


def _actor(hidden=(64, 64), in_dim=19):
    from ctr_reach_amd import _abi
    a = _abi.CtrActor()
    a.in_dim, a.n_hidden = in_dim, len(hidden)
    for l, w in enumerate(hidden):
        a.width[l] = w
    for i in range(6):
        a.scale[i] = 0.5
    a.blob = 1 << 20
    return a


def _ptrs(*values):
    return (ctypes.c_void_p * 4)(*values)


FAKE = (16, 16, 16, 16)


def _refused(lib, actor, W, b, word):
    assert lib.ctr_actor_load(actor, W, b, None) == -1, word
    assert word in lib.ctr_last_error(), (word, lib.ctr_last_error())


def test_symbol_within_abi_17():
    from ctr_reach_amd import _abi
    lib = _abi.load()
    assert _abi.CTR_ABI_VERSION == 17 and lib.ctr_abi_version() == 17
    assert "ctr_actor_load" in _abi.EXPORTED and hasattr(lib, "ctr_actor_load")
    assert lib.ctr_actor_load.restype is ctypes.c_int and len(lib.ctr_actor_load.argtypes) == 4


def test_shapes_are_validated():
    """The bad shapes of test_host_actor.test_actor_shapes_are_validated, and a NULL actor."""
    from ctr_reach_amd import _abi
    lib = _abi.load()
    W = _ptrs(*FAKE)
    _refused(lib, None, W, W, b"actor is NULL")
    for nh in (0, 4):
        a = _actor()
        a.n_hidden = nh
        _refused(lib, a, W, W, b"n_hidden")
    for w in (0, 48, 288):
        _refused(lib, _actor((64, w)), W, W, b"width")
    for d in (18, 21):
        _refused(lib, _actor(in_dim=d), W, W, b"in_dim")
    _refused(lib, _actor((256, 256)), W, W, b"CTR_ACTOR_MAX_BYTES")
    msg = lib.ctr_last_error()
    assert b"163840 B of weights" in msg and b"2176 B of biases" in msg, msg


def test_null_pointers_and_the_blob_are_validated():
    from ctr_reach_amd import _abi
    lib = _abi.load()
    a = _actor()                                     # two hidden layers: W[0..2], b[0..2] are read
    W = _ptrs(*FAKE)
    _refused(lib, a, None, W, b"W or b is NULL")
    _refused(lib, a, W, None, b"W or b is NULL")
    for l in range(3):
        hole = _ptrs(*[None if i == l else 16 for i in range(4)])
        _refused(lib, a, hole, W, b"NULL layer")
        _refused(lib, a, W, hole, b"NULL layer")
    # (a pointer past the output layer is not read)
    a.blob = None
    _refused(lib, a, W, W, b"blob is NULL")
    a.blob = (1 << 20) + 8
    _refused(lib, a, W, W, b"16-B aligned")


def test_a_host_actor_has_nothing_to_load_into():
    from ctr_reach_amd.policy import MlpActor
    rng = np.random.default_rng(0)
    layers = [(rng.standard_normal((32, 19)).astype(np.float32), np.zeros(32, dtype=np.float32)),
              (rng.standard_normal((6, 32)).astype(np.float32), np.zeros(6, dtype=np.float32))]
    act = MlpActor(layers, np.ones(6), device=None)
    with pytest.raises(RuntimeError, match="on the host"):
        act.load_(layers)
    assert act.weights is not None                   # the host copies stay
    act.emulate(np.zeros((1, 19), dtype=np.float32))
