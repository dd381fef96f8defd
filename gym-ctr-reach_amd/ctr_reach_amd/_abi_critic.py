"""ctypes mirrors of ctr_critic_t and ctr_her_td_t and the prototypes of the critic's entry points
(include/ctr_reach_amd.h, "MLP critic and the TD target": added within ABI 17).  ``_abi.load`` binds
them; tests/test_host_critic.py checks the mirrors against the header."""
import ctypes

from ._abi import CTR_ACTOR_MAX_HIDDEN, CtrActor, CtrHer, CtrHerBatch, _P


class CtrCritic(ctypes.Structure):
    """ctr_critic_t: an MLP critic and its packed device blob."""
    _fields_ = [("in_dim", ctypes.c_int32), ("n_hidden", ctypes.c_int32),
                ("width", ctypes.c_int32 * CTR_ACTOR_MAX_HIDDEN), ("pad", ctypes.c_int32), ("blob", _P)]


class CtrHerTd(ctypes.Structure):
    """ctr_her_td_t: the target networks and the outputs of ctr_her_sample_td."""
    _fields_ = [("actor", ctypes.POINTER(CtrActor)), ("critic", ctypes.POINTER(CtrCritic)),
                ("gamma", ctypes.c_float), ("pad", ctypes.c_int32), ("target", _P), ("q_next", _P),
                ("next_action", _P)]


def bind(L):
    i64 = ctypes.c_int64
    L.ctr_critic_blob_bytes.argtypes = [ctypes.POINTER(CtrCritic)]
    L.ctr_critic_blob_bytes.restype = i64
    L.ctr_critic_pack.argtypes = [ctypes.POINTER(CtrCritic), ctypes.POINTER(_P), ctypes.POINTER(_P), _P]
    L.ctr_critic_load.argtypes = [ctypes.POINTER(CtrCritic), ctypes.POINTER(_P), ctypes.POINTER(_P), _P]
    L.ctr_critic.argtypes = [ctypes.POINTER(CtrCritic), _P, _P, i64, _P, _P]
    L.ctr_her_sample_td.argtypes = [ctypes.POINTER(CtrHer), i64, ctypes.c_uint64, ctypes.c_uint64,
                                    ctypes.POINTER(CtrHerBatch), ctypes.POINTER(CtrHerTd), _P]
