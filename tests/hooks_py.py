"""Loader for the TEST build of the HIP library (tests/gpu_helpers/libgie_hip_test.so = the product's sources compiled with
-DGIE_TEST_HOOKS): the only build whose behaviour can be steered through GIE_* environment switches (forced tile lists, pool
base, staging chunk size, un-completed batch-EDT export ...) and that exports the gie_debug_* hooks.  The product library
(gie.Mapper, libgie_hip.so) has neither (tests/test_capi_symbols.py).  Switches are read once per process and switch: set them
(monkeypatch.setenv) BEFORE the first mapper that needs them is created."""
import ctypes as C
import os

import numpy as np

from gie import _capi
from gie.mapper import Mapper, load_library

HERE = os.path.dirname(os.path.abspath(__file__))
TEST_SO = os.path.join(HERE, "gpu_helpers", "libgie_hip_test.so")
_fns = None
_lib = None


def load():
    global _fns, _lib
    if _fns is None:
        if not os.path.exists(TEST_SO):
            import sys
            sys.path.insert(0, os.path.dirname(HERE))
            import __graft_entry__
            __graft_entry__.build_hip_test_hooks()
        load_library()                                  # (torch's HIP runtime first, as the package does it)
        _lib = C.CDLL(TEST_SO)
        _fns = _capi.bind(_lib, "gie_", _capi.DEVICE_ONLY)
        _lib.gie_debug_fault_barrier.argtypes = [C.c_void_p, C.c_int]
        _lib.gie_debug_place_probe.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
        _lib.gie_debug_nbr_check.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        _lib.gie_debug_set_frame.argtypes = [C.c_void_p, C.c_int]
    return _fns


class HooksMapper(Mapper):
    """gie.Mapper on the test build of the library."""

    def __init__(self, cfg):
        super(Mapper, self).__init__(load(), cfg)

    def debug_fault_barrier(self, updates):
        return _lib.gie_debug_fault_barrier(self._h, int(updates))

    def debug_place_probe(self, reps):
        ms = C.c_float(0)
        rc = _lib.gie_debug_place_probe(self._h, int(reps), C.byref(ms))
        if rc:
            raise RuntimeError(self._err())
        return ms.value

    def debug_nbr_check(self):
        """rows of the neighbour table of waves A / B that disagree with the hash, over every live block"""
        bad = C.c_int32(-1)
        if _lib.gie_debug_nbr_check(self._h, C.byref(bad)):
            raise RuntimeError(self._err())
        return bad.value

    def debug_tile_state(self):
        """the per-tile state the last map update leaves to the next one (gie_debug_tile_state); call it before read_batch_edt"""
        return read_tile_state(_lib, self)

    def debug_set_frame(self, ct):
        """the frame counter as if `ct` map updates had run (gie_debug_set_frame): the next set_pose counts ct + 1"""
        if _lib.gie_debug_set_frame(self._h, int(ct)):
            raise RuntimeError(self._err())


# gie_debug_tile_state's scalars, in order (gie_api.inc.h GIE_DBG_TS_*)
TILE_STATE_SCALARS = ("prev_valid", "coc_defer", "lazy_ok", "zstream", "zwide", "zfail", "lazy_exact", "tskip_count", "caught_up",
                      "lazy_written_out")


def read_tile_state(lib, m):
    """gie_debug_tile_state of a mapper on `lib` (the test build or the emulation): per-tile arrays shaped [tz][ty][tx] (zredo: [y][x // 16])
    and the scalars by name"""
    X, Y, Z = m.size
    tshape = ((Z + 7) // 8, (Y + 7) // 8, (X + 7) // 8)
    out = {k: np.zeros(tshape, np.uint8) for k in ("tknown", "tskip", "tlazy")}
    out.update({k: np.zeros(tshape, np.int32) for k in ("tmax", "tbmax")})
    out["zredo"] = np.zeros((Y, (X + 15) // 16), np.uint32)
    sc = np.zeros(len(TILE_STATE_SCALARS), np.int32)
    f = lib.gie_debug_tile_state
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] + [C.c_void_p] * 7
    p = lambda a: a.ctypes.data_as(C.c_void_p)        # noqa: E731
    if f(m._h, p(out["tknown"]), p(out["tskip"]), p(out["tlazy"]), p(out["tmax"]), p(out["tbmax"]), p(out["zredo"]), p(sc)):
        raise RuntimeError(m._err())
    out.update({k: int(v) for k, v in zip(TILE_STATE_SCALARS, sc)})
    return out
