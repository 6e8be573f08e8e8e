"""The shape of the C ABI: one batched-warp entry point, the retired forwarders gone from header and library, and every export of
stitching_amd._lib declared exactly once (no compute calls here)."""
import ctypes
import os
import re

from stitching_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the six variants stx_warp_batch absorbed, and the seven forwarders nobody called
RETIRED = ["stx_warp_batch_rects", "stx_warp_batch_gain", "stx_warp_batch_rects_kept", "stx_warp_batch_gain_kept", "stx_warp_batch_with_rois",
           "stx_warp_batch_with_rois_kept",
           "stx_block_gain_apply", "stx_blend_feed_contrib", "stx_strip_pack_batch", "stx_comm_exchange", "stx_comm_exchange_begin",
           "stx_comm_exchange_end", "stx_exposure_feed"]


def declared_functions():
    names = []
    for fn in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if fn.endswith(".h"):
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", fn)).read(), flags=re.S)
            names += re.findall(r"\b(stx_[a-z0-9_]+)\s*\(", text)
    return names


def test_retired_names_are_neither_declared_nor_exported():
    assert len(RETIRED) == 13
    declared = declared_functions()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in RETIRED:
        assert name not in declared, name
        assert not hasattr(L, name), name
        assert name not in _lib.EXPORTS, name


def test_one_batched_warp_entry_point():
    assert [n for n in declared_functions() if n.startswith("stx_warp_batch")] == ["stx_warp_batch"]


def test_every_export_has_one_prototype():
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    assert set(_lib.EXPORTS) == set(_lib.PROTOTYPES)
    for name, argtypes in _lib.PROTOTYPES.items():
        assert argtypes is None or isinstance(argtypes, (list, tuple)), name
    declared = declared_functions()
    assert len(declared) == len(set(declared))  # the header declares each function once, too


def test_prototypes_are_applied_to_the_library():
    L = _lib.lib()
    for name, argtypes in _lib.PROTOTYPES.items():
        fn = getattr(L, name)
        assert list(fn.argtypes or []) == list(argtypes or []), name
        assert fn.restype is (ctypes.c_char_p if name == "stx_last_error" else ctypes.c_int), name


def test_warp_batch_without_a_context_fails_without_a_device():
    L = _lib.lib()
    assert len(_lib.PROTOTYPES["stx_warp_batch"]) == 15
    rc = L.stx_warp_batch(None, _lib.WARP_SPHERICAL, 100.0, 0, None, None, None, None, None, None, 0, None, None, None, None)
    assert rc != 0
    assert L.stx_last_error()
