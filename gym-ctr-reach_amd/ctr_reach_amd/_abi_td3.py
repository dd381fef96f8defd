"""ctypes mirror of ctr_her_td3_t and the prototypes of ctr_her_sample_td3, ctr_td3_workspace_bytes and
ctr_td3_critic_step (include/ctr_reach_amd.h, "TD3": added within ABI 17).  ``_abi.load`` binds them;
tests/test_host_td3.py checks the mirror against the header."""
import ctypes

from ._abi import CtrActor, CtrHer, CtrHerBatch, _P
from ._abi_critic import CtrCritic
from ._abi_ddpg import CtrDdpgAdam, CtrDdpgNet


class CtrHerTd3(ctypes.Structure):
    """ctr_her_td3_t: the target networks, the smoothing noise and the outputs of ctr_her_sample_td3."""
    _fields_ = [("actor", ctypes.POINTER(CtrActor)), ("critic1", ctypes.POINTER(CtrCritic)),
                ("critic2", ctypes.POINTER(CtrCritic)), ("gamma", ctypes.c_float), ("sigma", ctypes.c_float),
                ("clip", ctypes.c_float), ("pad", ctypes.c_int32), ("target", _P), ("q1_next", _P), ("q2_next", _P),
                ("next_action", _P)]


CriticPair = ctypes.POINTER(CtrCritic) * 2         # const ctr_critic_t *const critic[2]
NetPair = ctypes.POINTER(CtrDdpgNet) * 2           # const ctr_ddpg_net_t *const net[2]


def bind(L):
    i64 = ctypes.c_int64
    L.ctr_her_sample_td3.argtypes = [ctypes.POINTER(CtrHer), i64, ctypes.c_uint64, ctypes.c_uint64,
                                     ctypes.POINTER(CtrHerBatch), ctypes.POINTER(CtrHerTd3), _P]
    L.ctr_td3_workspace_bytes.argtypes = [ctypes.POINTER(CtrActor), ctypes.POINTER(CtrCritic), ctypes.POINTER(CtrCritic),
                                          i64]
    L.ctr_td3_workspace_bytes.restype = i64
    L.ctr_td3_critic_step.argtypes = [ctypes.POINTER(CriticPair), ctypes.POINTER(NetPair), ctypes.POINTER(CtrDdpgAdam),
                                      _P, _P, _P, _P, i64, _P, _P, i64, _P]
