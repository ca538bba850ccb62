"""The header parser of the binding (_native.parse_header) on literal strings, and the two
hand-written ctypes structs against the header's own struct blocks. CPU only."""
import ctypes

import pytest

from multimodal_sequencing_amd import _native as N

PRE = """
typedef int mmseq_status;
typedef enum { MMSEQ_F32 = 0, MMSEQ_BF16 = 1 } mmseq_dtype;
"""


def sig(decl, name="mmseq_f"):
    return N.parse_header(PRE + decl)[0][name]


def test_struct_by_value():
    assert sig("mmseq_status mmseq_f(int rows, const void* x, mmseq_rows xl, mmseq_stream stream);") == \
        (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, N.Rows, ctypes.c_void_p])


def test_dropout_pointer_against_another_pointer():
    assert sig("mmseq_status mmseq_f(const mmseq_dropout* drop, const mmseq_rows* r, float* y);")[1] \
        == [N._dp, ctypes.c_void_p, ctypes.c_void_p]


def test_pointer_to_and_value_of_one_type():
    assert sig("mmseq_status mmseq_f(uint64_t* bits, const uint64_t *more, uint64_t seed, "
               "uint32_t stream_id);")[1] == \
        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32]


def test_double_float_and_int64():
    assert sig("int64_t mmseq_f(double n_ref, float eps, int64_t n);") == \
        (ctypes.c_int64, [ctypes.c_double, ctypes.c_float, ctypes.c_int64])


def test_enum_typed_argument_and_int_typedef():
    assert sig("mmseq_status mmseq_f(mmseq_dtype in_dtype, mmseq_status last);")[1] == \
        [ctypes.c_int, ctypes.c_int]
    with pytest.raises(N.NativeError, match="mmseq_dtype"):  # collected from the header, no list
        N.parse_header("typedef int mmseq_status;\nmmseq_status mmseq_f(mmseq_dtype d);")


def test_multi_line_prototype_with_comments():
    got = sig("""
/* block comment with a prototype inside: mmseq_status mmseq_not(int x); */
mmseq_status mmseq_f(int rows,   /* the rows */
                     const float* x,  // the input; with, commas
                     int64_t ldx /* stride */,
                     mmseq_stream stream);
""")
    assert got == (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p])
    assert "mmseq_not" not in N.parse_header(PRE + "/* mmseq_status mmseq_not(int x); */")[0]


def test_void_and_char_return():
    assert sig("const char* mmseq_f(void);") == (ctypes.c_char_p, [])
    assert sig("const char *mmseq_f();") == (ctypes.c_char_p, [])


@pytest.mark.parametrize("decl,word", [
    ("mmseq_status mmseq_f(size_t n);", "size_t"),
    ("mmseq_status mmseq_f(unsigned int n);", "unsigned"),
    ("mmseq_status mmseq_f(mmseq_dropout drop);", "mmseq_dropout"),
    ("void mmseq_f(int n);", "mmseq_f"),
    ("mmseq_status mmseq_f(int n)", "mmseq_f"),
    ("mmseq_status mmseq_f(int n;", "mmseq_f"),
])
def test_what_does_not_parse_raises(decl, word):
    with pytest.raises(N.NativeError, match=word):
        N.parse_header(PRE + decl + "\nmmseq_status mmseq_g(int n);")


def test_constants():
    _, c, _ = N.parse_header("""
#ifndef MMSEQ_H
#define MMSEQ_H
#define MMSEQ_MAX_K 8   /* a limit */
#define MMSEQ_MASK 0x10
#define MMSEQ_NAME "text"
enum { MMSEQ_OK = 0, MMSEQ_EINVAL = -1 };
typedef enum {
  MMSEQ_A = 0, MMSEQ_B = 5
} mmseq_kind;
#endif
""")
    assert c == {"MMSEQ_MAX_K": 8, "MMSEQ_MASK": 16, "MMSEQ_OK": 0, "MMSEQ_EINVAL": -1,
                 "MMSEQ_A": 0, "MMSEQ_B": 5}
    with pytest.raises(N.NativeError, match="MMSEQ_C"):
        N.parse_header("enum { MMSEQ_A = 0, MMSEQ_C };")


def test_python_constants_are_the_headers():
    c = N.CONSTANTS
    assert (N.F32, N.BF16, N.GEMM_AUTO, N.EUNSUPPORTED, N.XENT_EVAL_MAX_K) == (0, 1, 1, -2, 8)
    assert N.ACT == {"none": 0, "gelu": 1, "quickgelu": 2, "tanh": 3, "gelu_tanh": 4}
    assert c["MMSEQ_GEMM_PINGPONG"] == 6 and "6 =" in N.gemm_set_fast.__doc__
    from multimodal_sequencing_amd import kernels
    assert (kernels.GELU, kernels.QGELU, kernels.TANH, kernels.GELU_TANH) == (1, 2, 3, 4)


def test_structs_match_the_header():
    """Rows and Dropout keep hand-written _fields_: names and types, in order, are the header's."""
    assert set(N.STRUCTS) == {"mmseq_rows", "mmseq_dropout"}
    assert N.Rows._fields_ == N.STRUCTS["mmseq_rows"]
    assert N.Dropout._fields_ == N.STRUCTS["mmseq_dropout"]


def test_missing_header_names_the_path(monkeypatch):
    monkeypatch.setattr(N, "HEADER_PATH", "/nonexistent/mmseq.h")
    with pytest.raises(N.NativeError, match="/nonexistent/mmseq.h"):
        N._read_header()
