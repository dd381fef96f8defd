"""ctypes mirrors of ctr_sac_alpha_t, ctr_her_sac_t and ctr_sac_update_t and the prototypes of
ctr_gauss_blob_bytes, ctr_gauss_pack, ctr_gauss_load, ctr_gauss_act, ctr_sac_workspace_bytes,
ctr_sac_actor_step, ctr_her_sample_sac, ctr_collect_gauss and ctr_sac_update (include/ctr_reach_amd.h,
"SAC" and next to ctr_collect: added within ABI 17).  ``_abi.load`` binds them; tests/test_host_sac.py,
tests/test_host_sac_target.py, tests/test_host_collect_gauss.py and tests/test_host_sac_update.py check
the mirrors against the header."""
import ctypes

from ._abi import CtrActor, CtrBatch, CtrEnvConfig, CtrHer, CtrHerBatch, CtrRolloutAux, CtrStepOut, _P
from ._abi_critic import CtrCritic
from ._abi_ddpg import CtrDdpgAdam, CtrDdpgNet
from ._abi_td3 import CriticPair


class CtrSacAlpha(ctypes.Structure):
    """ctr_sac_alpha_t: the temperature's Adam state, gradient, learning rate and switch."""
    _fields_ = [("state", _P), ("grad", _P), ("lr", ctypes.c_float), ("learn", ctypes.c_int32)]


class CtrHerSac(ctypes.Structure):
    """ctr_her_sac_t: the current policy, the target critics, the temperature and the outputs of
    ctr_her_sample_sac."""
    _fields_ = [("actor", ctypes.POINTER(CtrActor)), ("critic1", ctypes.POINTER(CtrCritic)),
                ("critic2", ctypes.POINTER(CtrCritic)), ("log_alpha", _P), ("gamma", ctypes.c_float),
                ("pad", ctypes.c_int32), ("target", _P), ("q1_next", _P), ("q2_next", _P), ("next_action", _P),
                ("next_logp", _P)]


LayersPair = ctypes.POINTER(_P) * 2                # const float *const *const critic_W[2]


class CtrSacUpdate(ctypes.Structure):
    """ctr_sac_update_t: everything a run of SAC updates takes (ctr_sac_update), once."""
    _fields_ = [("her", ctypes.POINTER(CtrHer)), ("batch_size", ctypes.c_int64), ("draw_seed", ctypes.c_uint64),
                ("draw_counter", ctypes.c_uint64), ("batch", ctypes.POINTER(CtrHerBatch)), ("target", _P), ("q1_next", _P),
                ("q2_next", _P), ("next_action", _P), ("next_logp", _P), ("gamma", ctypes.c_float), ("tau", ctypes.c_float),
                ("policy", ctypes.POINTER(CtrActor)), ("policy_net", ctypes.POINTER(CtrDdpgNet)),
                ("policy_adam", ctypes.POINTER(CtrDdpgAdam)), ("critic", ctypes.POINTER(CtrCritic) * 2),
                ("critic_net", ctypes.POINTER(CtrDdpgNet) * 2), ("critic_adam", ctypes.POINTER(CtrDdpgAdam)), ("scale", _P),
                ("critic_targ", ctypes.POINTER(CtrCritic) * 2), ("W_targ", ctypes.POINTER(_P) * 2),
                ("b_targ", ctypes.POINTER(_P) * 2), ("seed", ctypes.c_uint64), ("step_counter", ctypes.c_uint64),
                ("log_alpha", _P), ("alpha", ctypes.POINTER(CtrSacAlpha)), ("target_entropy", ctypes.c_float),
                ("pad", ctypes.c_int32), ("critic_loss", _P), ("actor_loss", _P), ("logp_mean", _P), ("workspace", _P),
                ("workspace_bytes", ctypes.c_int64), ("history", _P)]


def bind(L):
    i64, u64, i32 = ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32
    A = ctypes.POINTER(CtrActor)
    L.ctr_gauss_blob_bytes.argtypes = [A]
    L.ctr_gauss_blob_bytes.restype = i64
    L.ctr_gauss_pack.argtypes = [A, ctypes.POINTER(_P), ctypes.POINTER(_P), _P]
    L.ctr_gauss_load.argtypes = [A, ctypes.POINTER(_P), ctypes.POINTER(_P), _P]
    L.ctr_gauss_act.argtypes = [A, _P, i64, u64, u64, i64, i32, _P, _P, _P, _P, _P]
    L.ctr_sac_workspace_bytes.argtypes = [A, ctypes.POINTER(CtrCritic), ctypes.POINTER(CtrCritic), i64]
    L.ctr_sac_workspace_bytes.restype = i64
    L.ctr_sac_actor_step.argtypes = [A, ctypes.POINTER(CtrDdpgNet), ctypes.POINTER(CtrDdpgAdam), ctypes.POINTER(CriticPair),
                                     ctypes.POINTER(LayersPair), ctypes.POINTER(LayersPair), _P, i64, u64, u64, _P,
                                     ctypes.POINTER(CtrSacAlpha), ctypes.c_float, _P, _P, _P, i64, _P]
    if hasattr(L, "ctr_her_sample_sac"):           # (a build from before the symbol lacks it)
        L.ctr_her_sample_sac.argtypes = [ctypes.POINTER(CtrHer), i64, u64, u64, ctypes.POINTER(CtrHerBatch),
                                         ctypes.POINTER(CtrHerSac), _P]
    if hasattr(L, "ctr_collect_gauss"):            # (a build from before the symbol lacks it)
        L.ctr_collect_gauss.argtypes = [ctypes.POINTER(CtrEnvConfig), ctypes.POINTER(CtrBatch), A, u64, u64,
                                        ctypes.POINTER(CtrHer), i32, ctypes.POINTER(CtrStepOut), i32,
                                        ctypes.POINTER(CtrRolloutAux), _P]
    if hasattr(L, "ctr_sac_update"):               # (a build from before the symbol lacks it)
        L.ctr_sac_update.argtypes = [ctypes.POINTER(CtrSacUpdate), i32, _P]
