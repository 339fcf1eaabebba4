"""CPU: morig_amd/abi.py, the reader that turns include/morig_hip.h into the ctypes binding -- its grammar on small header strings, the
real header consumed whole, and the library's refusal of a wrong struct_size at every entry point that takes an argument struct."""
import ctypes as C
import re

import pytest

from morig_amd import abi, native

SMALL = """
/* a header in the small */
#ifndef H
#define H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define MORIG_FLAG_A 2   /* a comment that starts behind the value
                            and ends two lines further down: int morig_hidden(void);
                          */
#define MORIG_NEG -3
#define MORIG_SIZE 24u
#define MORIG_MACRO(x) ((x) + 1)
typedef struct morig_t_args {
    uint32_t struct_size;     /* first */
    int32_t M, N, K;
    const float* X; int32_t ldx;
    const struct morig_t_args* next;
    uint64_t* keys; double scale;
} morig_t_args;
int         morig_version(void);
const char* morig_name(int kind);
int morig_run(const morig_t_args* a, void** out, uint64_t* keys, const uint8_t* mask /* host */,
              char* buf, float tau, int64_t n, void* stream);
int64_t morig_bytes(int32_t n);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_grammar_on_a_small_header():
    structs, sigs, consts = abi.parse(SMALL)
    assert consts == dict(MORIG_FLAG_A=2, MORIG_NEG=-3, MORIG_SIZE=24)          # no function-like macro, no include guard
    T = structs["morig_t_args"]
    assert list(structs) == ["morig_t_args"] and issubclass(T, C.Structure)
    assert T._fields_ == [("struct_size", C.c_uint32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),       # one declaration, three members
                          ("X", C.c_void_p), ("ldx", C.c_int32),                                                  # two members on a line
                          ("next", C.c_void_p),                                                                   # const struct X* member: opaque
                          ("keys", C.c_void_p), ("scale", C.c_double)]
    assert C.sizeof(T) == 56
    assert list(sigs) == ["morig_version", "morig_name", "morig_run", "morig_bytes"]       # the prototype inside the comment is not one
    assert sigs["morig_version"] == (C.c_int, [])                                           # (void)
    assert sigs["morig_name"] == (C.c_char_p, [C.c_int])                                    # const char* return
    res, args = sigs["morig_run"]
    assert res is C.c_int and args[0]._type_ is T and args[1]._type_ is C.c_void_p          # typed struct pointer; void**
    assert args[2:] == [C.c_void_p, C.c_void_p, C.c_char_p, C.c_float, C.c_int64, C.c_void_p]      # uint64_t*, const uint8_t*, char*
    assert sigs["morig_bytes"] == (C.c_int64, [C.c_int32])


@pytest.mark.parametrize("text, quoted", [
    ("int morig_f(short n);", "short"),                                                               # a scalar outside the list
    ("int morig_f(int32_t n);\nstatic const int morig_limit = 4;\nint morig_g(void);", "static const int morig_limit = 4;"),    # a stray statement
    ("typedef struct morig_a_args { uint32_t struct_size; } morig_b_args;", "morig_b_args"),         # tag and typedef name differ
    ("int morig_f(const float* x[4]);", "x[4]"),
    ("int morig_f(int32_t);", "int32_t"),                                                             # a parameter without a name
    ("typedef struct morig_a_args { uint32_t struct_size; int32_t a, *b; } morig_a_args;", "*b"),
    ("int morig_f(morig_later_args* a);", "morig_later_args"),
    ("int morig_f(int32_t n);\nint morig_f(int64_t n);", "int morig_f(int64_t n);"),                 # one name, two declarations                                        # a struct that is not declared (yet)
])
def test_reader_refuses_what_it_cannot_read(text, quoted):
    with pytest.raises(native.MorigNativeError) as e:
        abi.parse(text)
    assert quoted in str(e.value)


_SIZE_DEFINE = dict(morig_ik_args="MORIG_IK_SOLVE_STRUCT_BYTES", morig_nce_args="MORIG_NCE_STRUCT_BYTES",
                    morig_logratio_args="MORIG_LOGRATIO_STRUCT_BYTES")


def _size_define(struct_name):
    stem = struct_name.upper()                                       # morig_gemm_args -> MORIG_GEMM_ARGS
    for name in (stem + "_SIZE", stem + "_V3_SIZE", _SIZE_DEFINE.get(struct_name)):
        if name in abi.CONSTANTS:
            return abi.CONSTANTS[name]
    raise AssertionError(f"include/morig_hip.h states no size for {struct_name}")


def test_real_header_is_consumed_whole():
    text = re.sub(r"/\*.*?\*/", " ", open(abi.HEADER).read(), flags=re.S)
    assert set(abi.SIGNATURES) == set(re.findall(r"\b(morig_[a-z0-9_]+)\s*\(", text)) == set(native.EXPORTS)
    assert set(abi.STRUCTS) == set(re.findall(r"typedef\s+struct\s+(\w+)", text)) and len(abi.STRUCTS) == 8
    assert set(re.findall(r"#define\s+(MORIG_\w+)[ \t]+-?\d", text)) == set(abi.CONSTANTS)
    for name, cls in abi.STRUCTS.items():
        assert cls._fields_[0] == ("struct_size", C.c_uint32), name
        assert C.sizeof(cls) == _size_define(name), (name, C.sizeof(cls))
    aliases = [native.GemmArgs, native.EdgeConvArgs, native.EdgeConvX3Args, native.PointConvArgs, native.SegmaxArgs, native.IkArgs,
               native.NceArgs, native.LogRatioArgs]
    assert set(aliases) == set(abi.STRUCTS.values())
    assert native.ABI_VERSION == abi.CONSTANTS["MORIG_ABI_VERSION"]


def test_every_struct_entry_point_refuses_a_wrong_struct_size():
    """Every export whose first parameter is an argument struct copies it through take_args (csrc/common.h) before anything else: a
    struct_size of 0, below the version-3 size or above 1024 is MORIG_E_INVALID with nothing read or launched, so this runs without a GPU.
    morig_edgeconv_can_split_out answers a question instead of returning a status: its refusal is 0."""
    lib = native.load_library()
    assert abi.CONSTANTS["MORIG_ABI_VERSION"] == lib.morig_abi_version()
    takers = {name: args for name, (_, args) in abi.SIGNATURES.items() if args and getattr(args[0], "_type_", None) in abi.STRUCTS.values()}
    assert len(takers) == 12 and {a[0]._type_ for a in takers.values()} == set(abi.STRUCTS.values())
    for name, args in takers.items():
        refusal = 0 if name == "morig_edgeconv_can_split_out" else abi.CONSTANTS["MORIG_E_INVALID"]
        for bad in (0, 8, 4096):
            a = args[0]._type_()
            a.struct_size = bad
            assert getattr(lib, name)(C.byref(a), *[None] * (len(args) - 1)) == refusal, (name, bad)
