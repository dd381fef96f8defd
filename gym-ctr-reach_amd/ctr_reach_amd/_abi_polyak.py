"""ctypes mirror of ctr_polyak_net_t and the prototype of ctr_polyak (include/ctr_reach_amd.h, "The
soft (Polyak) update of target networks": added within ABI 17).  ``_abi.load`` binds it;
tests/test_host_polyak.py checks the mirror against the header."""
import ctypes

from ._abi import CtrActor, _P
from ._abi_critic import CtrCritic

CTR_POLYAK_MAX_NETS = 4


class CtrPolyakNet(ctypes.Structure):
    """ctr_polyak_net_t: one target network (its shape and blob), its online and its target tensors."""
    _fields_ = [("actor", ctypes.POINTER(CtrActor)), ("critic", ctypes.POINTER(CtrCritic)),
                ("W", ctypes.POINTER(_P)), ("b", ctypes.POINTER(_P)),
                ("W_targ", ctypes.POINTER(_P)), ("b_targ", ctypes.POINTER(_P))]


def bind(L):
    L.ctr_polyak.argtypes = [ctypes.POINTER(CtrPolyakNet), ctypes.c_int32, ctypes.c_float, _P]
