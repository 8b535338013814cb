"""The dropout / training-state entry points of the C ABI (include/mpn.h), the part that needs no GPU: both library flavours export
them, and a NULL handle is refused before anything touches the device."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mpn_frcnn_train_set_dropout", "mpn_frcnn_train_get_state", "mpn_frcnn_train_set_state", "mpn_frcnn_train_get_trunk_state",
           "mpn_frcnn_train_set_trunk_state")


def test_both_flavours_export_the_five_symbols():
    for name in ("libmpn_hip.so", "libmpn_hip_dbg.so"):
        out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "multipathnet_amd", name)]).decode()
        syms = set(ln.split()[-1] for ln in out.splitlines() if ln.strip())
        assert not [s for s in SYMBOLS if s not in syms], (name, [s for s in SYMBOLS if s not in syms])
    header = open(os.path.join(ROOT, "include", "mpn.h")).read()
    cdef = open(os.path.join(ROOT, "multipathnet_amd", "lua", "mpn_cdef.lua")).read()
    for s in SYMBOLS:
        assert "int %s(mpn_frcnn *p" % s in header and "int %s(mpn_frcnn *p" % s in cdef, s


def test_null_handle_is_an_invalid_argument():
    import multipathnet_amd
    for flavour in ("product", "debug"):
        lib = multipathnet_amd._lib.load(flavour)
        lib.mpn_last_error.restype = ctypes.c_char_p
        assert lib.mpn_frcnn_train_set_dropout(None, ctypes.c_float(0.5), ctypes.c_long(1)) == -1
        assert b"invalid argument" in lib.mpn_last_error()
        step = ctypes.c_long(-7)
        assert lib.mpn_frcnn_train_get_state(None, *([None] * 8), ctypes.byref(step), None) == -1 and step.value == -7
        assert lib.mpn_frcnn_train_set_state(None, *([None] * 8), ctypes.c_long(0), None) == -1
        assert lib.mpn_frcnn_train_get_trunk_state(None, 0, None, None, None) == -1
        assert lib.mpn_frcnn_train_set_trunk_state(None, 0, None, None, None) == -1
    assert multipathnet_amd.load().mpn_version() == 600
