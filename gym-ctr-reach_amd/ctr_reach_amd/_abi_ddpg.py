"""ctypes mirrors of ctr_ddpg_net_t, ctr_ddpg_adam_t and ctr_ddpg_update_t and the prototypes of
ctr_ddpg_workspace_bytes, ctr_ddpg_critic_step, ctr_ddpg_actor_step and ctr_ddpg_update
(include/ctr_reach_amd.h, "DDPG's two updates" and "A run of DDPG / TD3 updates": added within ABI 17).
``_abi.load`` binds them; tests/test_host_ddpg.py and tests/test_host_ddpg_update.py check the mirrors
against the header."""
import ctypes

from ._abi import CtrActor, CtrHer, CtrHerBatch, _P
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


class CtrDdpgUpdate(ctypes.Structure):
    """ctr_ddpg_update_t: everything a run of DDPG or TD3 updates takes (ctr_ddpg_update), once."""
    _fields_ = [("her", ctypes.POINTER(CtrHer)), ("batch_size", ctypes.c_int64), ("draw_seed", ctypes.c_uint64),
                ("draw_counter", ctypes.c_uint64), ("batch", ctypes.POINTER(CtrHerBatch)), ("target", _P), ("q1_next", _P),
                ("q2_next", _P), ("next_action", _P), ("gamma", ctypes.c_float), ("tau", ctypes.c_float),
                ("n_critics", ctypes.c_int32), ("sigma", ctypes.c_float), ("clip", ctypes.c_float),
                ("policy_delay", ctypes.c_int32), ("update_index", ctypes.c_uint64),
                ("policy", ctypes.POINTER(CtrActor)), ("policy_net", ctypes.POINTER(CtrDdpgNet)),
                ("policy_adam", ctypes.POINTER(CtrDdpgAdam)), ("critic", ctypes.POINTER(CtrCritic) * 2),
                ("critic_net", ctypes.POINTER(CtrDdpgNet) * 2), ("critic_adam", ctypes.POINTER(CtrDdpgAdam)), ("scale", _P),
                ("actor_targ", ctypes.POINTER(CtrActor)), ("W_targ_actor", ctypes.POINTER(_P)),
                ("b_targ_actor", ctypes.POINTER(_P)), ("critic_targ", ctypes.POINTER(CtrCritic) * 2),
                ("W_targ", ctypes.POINTER(_P) * 2), ("b_targ", ctypes.POINTER(_P) * 2), ("actor", ctypes.POINTER(CtrActor)),
                ("critic_loss", _P), ("actor_loss", _P), ("workspace", _P), ("workspace_bytes", ctypes.c_int64),
                ("history", _P)]


def bind(L):
    i64 = ctypes.c_int64
    L.ctr_ddpg_workspace_bytes.argtypes = [ctypes.POINTER(CtrActor), ctypes.POINTER(CtrCritic), i64]
    L.ctr_ddpg_workspace_bytes.restype = i64
    L.ctr_ddpg_critic_step.argtypes = [ctypes.POINTER(CtrCritic), ctypes.POINTER(CtrDdpgNet), ctypes.POINTER(CtrDdpgAdam),
                                       _P, _P, _P, _P, i64, _P, _P, i64, _P]
    L.ctr_ddpg_actor_step.argtypes = [ctypes.POINTER(CtrActor), ctypes.POINTER(CtrDdpgNet), ctypes.POINTER(CtrDdpgAdam),
                                      ctypes.POINTER(CtrCritic), ctypes.POINTER(_P), ctypes.POINTER(_P),
                                      _P, i64, _P, _P, i64, _P]
    if hasattr(L, "ctr_ddpg_update"):              # (a build from before the symbol lacks it)
        L.ctr_ddpg_update.argtypes = [ctypes.POINTER(CtrDdpgUpdate), ctypes.c_int32, _P]
