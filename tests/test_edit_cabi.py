"""The speech-editing entry points of the C ABI: declared in include/zipvoice_hip.h with the
documented signatures, bound in engine.SIGNATURES with matching argument lists, and exported by
both operand builds of the library.  No GPU: nothing is called that touches a device."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "zipvoice_hip.h")

DECLS = {
    "zv_edit_create": "zv_edit_handle zv_edit_create(void);",
    "zv_edit_destroy": "void zv_edit_destroy(zv_edit_handle h);",
    "zv_edit_device_bytes": "int64_t zv_edit_device_bytes(zv_edit_handle h);",
    "zv_edit_gather": "int zv_edit_gather(zv_edit_handle h, const float* feat, int B, int Lmax, int F, "
                      "const int32_t* host_lens, const float* fill, const int32_t* host_table, "
                      "const int32_t* host_row_ptr, int T, float* out, uint8_t* mask, void* stream);",
    "zv_edit_splice": "int zv_edit_splice(zv_edit_handle h, const float* orig, int64_t ld, "
                      "const int32_t* host_lens, const float* gen, int64_t ldg, const int32_t* host_gen_lens, "
                      "int B, int C, const int32_t* host_table, const int32_t* host_row_ptr, "
                      "const float* host_gains, int fade, float* out, int64_t out_ld, int64_t out_cols, "
                      "void* stream);",
}
CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}


def header():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.sub(r"\s+", " ", src)


def test_header_declares_the_documented_signatures():
    h = header()
    assert "typedef struct zv_edit* zv_edit_handle;" in h
    for name, decl in DECLS.items():
        assert decl in h, name


def test_ctypes_table_matches_the_header():
    from zipvoice_amd.engine import SIGNATURES
    for name, decl in DECLS.items():
        res, args = SIGNATURES[name]
        params = decl[decl.index("(") + 1:decl.rindex(")")]
        want = []
        for p in ([] if params == "void" else params.split(", ")):
            ty = p.rsplit(" ", 1)[0]
            want.append(ctypes.c_void_p if "*" in ty or ty.endswith("_handle") else CTYPE[ty])
        assert args == want, name
        ret = decl.split(" zv_")[0]
        assert res == {"void": None, "int": ctypes.c_int, "int64_t": ctypes.c_int64,
                       "zv_edit_handle": ctypes.c_void_p}[ret], name


def test_both_libraries_export_the_symbols():
    from zipvoice_amd.csrc.build import build
    build(verbose=False)
    from zipvoice_amd import engine
    for lib in (engine.load_library(), engine.load_library(operand="f16")):
        for name in DECLS:
            assert hasattr(lib, name), name
        # a null handle is refused with a message, before anything touches a device
        assert lib.zv_edit_device_bytes(None) == 0
        assert lib.zv_edit_gather(None, None, 1, 1, 1, None, None, None, None, 1, None, None, None) != 0
        assert b"null edit handle" in lib.zv_last_error()
