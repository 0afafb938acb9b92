"""The ctypes signatures come from the C headers (clean_pvnet_amd._native.declarations): every library exports exactly what its
header declares, the reader maps each type of its rules and refuses what they do not cover, and a symbol no header declares is
still an AttributeError.  No GPU, no compute call."""
import ctypes

import pytest

import lib
from tests import capi

native = capi.native
PTR = ctypes.c_void_p


@pytest.mark.parametrize("name", list(lib.load_build().HIP_LIBS))
def test_every_library_exports_exactly_what_its_header_declares(name):
    declared, exported = capi.declared(name), capi.exported(name)
    assert declared and declared == exported, (sorted(declared - exported), sorted(exported - declared))
    L = capi.load(name)
    for symbol, (restype, argtypes) in native.declarations("pvnet_%s.h" % name).items():
        fn = getattr(L, symbol)
        assert fn.restype is restype and fn.argtypes == argtypes, symbol


def test_the_seven_headers_are_read_once_and_hold_the_known_signatures():
    total = sum(len(native.declarations("pvnet_%s.h" % name)) for name in lib.load_build().HIP_LIBS)
    assert total == 82
    assert native.declarations("pvnet_vote.h") is native.declarations("pvnet_vote.h")            # parsed once per process
    vote = native.declarations("pvnet_vote.h")
    assert vote["pvv_last_error"] == (ctypes.c_char_p, []) and vote["pvv_abi_version"] == (ctypes.c_int, [])
    assert vote["pvv_workspace_bytes"] == (ctypes.c_size_t, [PTR])                                # const pvv_problem *
    assert vote["pvv_default_cap"] == (ctypes.c_int, [ctypes.c_int] * 3)                          # int32_t
    assert vote["pvv_dcn_backward_workspace_bytes"] == (ctypes.c_longlong, [ctypes.c_int] * 15)
    assert vote["pvv_optim_step"][1] == [ctypes.c_int, PTR, PTR, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_int, PTR]
    assert vote["pvv_stage_hint_query"] == (ctypes.c_int, [PTR] * 4)
    assert native.declarations("pvnet_nn.h")["findNearestPointIdxLauncher"] == (None, [PTR] * 3 + [ctypes.c_int] * 5)
    assert native.declarations("pvnet_pnp.h")["uncertainty_pnp"] == (None, [PTR] * 6 + [ctypes.c_int])


RULES = [("int", ctypes.c_int), ("int32_t", ctypes.c_int), ("long long", ctypes.c_longlong), ("int64_t", ctypes.c_longlong),
         ("size_t", ctypes.c_size_t), ("double", ctypes.c_double), ("float", ctypes.c_float), ("uint64_t", ctypes.c_uint64),
         ("unsigned", ctypes.c_uint), ("uint32_t", ctypes.c_uint)]


@pytest.mark.parametrize("ctype,want", RULES, ids=[r[0].replace(" ", "_") for r in RULES])
def test_reader_maps_each_scalar_type_as_parameter_and_as_return(ctype, want):
    got = native.parse("%s f(%s a, const %s b, %s);" % (ctype, ctype, ctype, ctype))
    assert got == {"f": (want, [want] * 3)}


def test_reader_pointers_void_and_empty_parameter_lists():
    got = native.parse("""
        const char *name(void);
        const char * spaced ( void ) ;
        void nothing();
        int takes(const float *d_a, void **marks, const pvv_problem *p, uint8_t *d_out, const void *, void *stream);
    """)
    assert got == {"name": (ctypes.c_char_p, []), "spaced": (ctypes.c_char_p, []), "nothing": (None, []),
                   "takes": (ctypes.c_int, [PTR] * 6)}


def test_reader_skips_comments_preprocessor_lines_structs_and_the_extern_braces():
    got = native.parse("""
        /* int in_a_block_comment(int a);
           int over_two_lines(void); */
        // int in_a_line_comment(void);
        #ifndef GUARD_H_
        #define GUARD_H_
        #include <stddef.h>
        #define MACRO(x) \\
            int continued(int x);
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef struct row {
            void *p, *g;          /* int inside_a_struct(void); */
            long long numel;
            float s[8];
        } row;
        int over_several_lines(const row *d_rows,
                               long long n,   /* a comment between parameters */
                               float clip,
                               void *stream);
        size_t query(int B, int H);  int same_line(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    assert got == {"over_several_lines": (ctypes.c_int, [PTR, ctypes.c_longlong, ctypes.c_float, PTR]),
                   "query": (ctypes.c_size_t, [ctypes.c_int] * 2), "same_line": (ctypes.c_int, [])}
    assert list(got) == ["over_several_lines", "query", "same_line"]                                # the header's order


REFUSED = {
    "unknown_parameter_type": "int f(short a);",
    "unknown_typedef": "int f(hipStream_t stream);",
    "struct_by_value": "int f(pvv_problem p);",
    "unsigned_int": "int f(unsigned int a);",
    "long_alone": "int f(long a);",
    "unknown_return_type": "bool f(int a);",
    "pointer_return_other_than_const_char": "float *f(int a);",
    "char_pointer_return_without_const": "char *f(void);",
    "function_pointer_parameter": "int f(int (*callback)(int), void *stream);",
    "array_parameter": "int f(float s[8]);",
    "variadic": "int f(int a, ...);",
    "storage_class": "static int f(int a);",
    "a_variable": "int counter;",
    "enum": "enum kind { A, B };",
    "declared_twice": "int f(int a); int f(int a);",
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_reader_refuses_what_its_rules_do_not_cover(case):
    text = "int before(void);\n%s\nint after(void);" % REFUSED[case]
    with pytest.raises(ImportError) as ei:
        native.parse(text, "include/pvnet_case.h")
    msg = str(ei.value)
    assert "include/pvnet_case.h" in msg and "`%s`" % REFUSED[case].split(";")[0] in msg, msg       # the header and the declaration


def test_a_missing_header_is_an_import_error_that_names_it():
    with pytest.raises(ImportError) as ei:
        native.declarations("pvnet_nowhere.h")
    assert "include/pvnet_nowhere.h" in str(ei.value) and "no CPU fallback" in str(ei.value)


def test_a_symbol_no_header_declares_is_still_an_attribute_error():
    bound = native.bind("probe", "libpvnet_vote.so", last_error="pvv_last_error")
    for L in (capi.load(), bound):
        with pytest.raises(AttributeError):
            L.pvv_no_such_symbol
    assert bound.pvv_last_error.restype is ctypes.c_char_p and bound.pvv_abi_version() == 8
