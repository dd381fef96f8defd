"""ctypes mirrors of ctr_ddpg_net_t and ctr_ddpg_adam_t and the prototypes of ctr_ddpg_workspace_bytes,
ctr_ddpg_critic_step and ctr_ddpg_actor_step (include/ctr_reach_amd.h, "DDPG's two updates": added
within ABI 17).  ``_abi.load`` binds them; tests/test_host_ddpg.py checks the mirrors against the
header."""
import ctypes

from ._abi import CtrActor, _P
from ._abi_critic import CtrCritic

CTR_DDPG_MAX_B = 65536


class CtrDdpgNet(ctypes.Structure):
    """ctr_ddpg_net_t: one learning network's parameters, gradients and Adam state (device)."""
    _fields_ = [("W", ctypes.POINTER(_P)), ("b", ctypes.POINTER(_P)),
                ("gW", ctypes.POINTER(_P)), ("gb", ctypes.POINTER(_P)),
                ("mW", ctypes.POINTER(_P)), ("mb", ctypes.POINTER(_P)),
                ("vW", ctypes.POINTER(_P)), ("vb", ctypes.POINTER(_P)),
                ("pow", _P)]


class CtrDdpgAdam(ctypes.Structure):
    """ctr_ddpg_adam_t: Adam's constants."""
    _fields_ = [("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("eps", ctypes.c_float)]


def bind(L):
    i64 = ctypes.c_int64
    L.ctr_ddpg_workspace_bytes.argtypes = [ctypes.POINTER(CtrActor), ctypes.POINTER(CtrCritic), i64]
    L.ctr_ddpg_workspace_bytes.restype = i64
    L.ctr_ddpg_critic_step.argtypes = [ctypes.POINTER(CtrCritic), ctypes.POINTER(CtrDdpgNet), ctypes.POINTER(CtrDdpgAdam),
                                       _P, _P, _P, _P, i64, _P, _P, i64, _P]
    L.ctr_ddpg_actor_step.argtypes = [ctypes.POINTER(CtrActor), ctypes.POINTER(CtrDdpgNet), ctypes.POINTER(CtrDdpgAdam),
                                      ctypes.POINTER(CtrCritic), ctypes.POINTER(_P), ctypes.POINTER(_P),
                                      _P, i64, _P, _P, i64, _P]
