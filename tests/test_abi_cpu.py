"""The Python binding is read from the C headers (apertis_llm_amd/_lib.py: parse_header): the reader on synthetic header text, and
the chain header -> compiler -> library -> callers on the real tree.  No GPU and no built library."""
import ctypes
import glob
import os
import re

import pytest

from conftest import ROOT

from apertis_llm_amd import _lib
from apertis_llm_amd._lib import ApertisHipError, parse_header

VP = ctypes.c_void_p
CSRC = os.path.join(ROOT, "apertis_llm_amd", "csrc")


def _sigs(text):
    return parse_header(text, "synthetic.h")[0]


# ------------------------------------------------------------------------------------------------ the reader, synthetic text
VALUE_TYPES = [("int", ctypes.c_int), ("int64_t", ctypes.c_int64), ("uint32_t", ctypes.c_uint32), ("uint64_t", ctypes.c_uint64),
               ("float", ctypes.c_float), ("double", ctypes.c_double)]


@pytest.mark.parametrize("spelling,ctype", VALUE_TYPES)
def test_each_value_type_as_parameter_and_as_return(spelling, ctype):
    sigs = _sigs(f"{spelling} apertis_f({spelling} a, const {spelling} b);\nint apertis_g({spelling} only);\n")
    assert sigs == {"apertis_f": (ctype, [ctype, ctype]), "apertis_g": (ctypes.c_int, [ctype])}
    assert all(isinstance(args, list) for _, args in sigs.values())


def test_pointer_spacings_struct_pointers_and_char_return():
    sigs = _sigs("int apertis_p(const float *a, float* b, void*c, const int32_t * d, int64_t n);\n"
                 "int apertis_s(const apertis_opt_tensor *tensors, uint8_t *mask, int64_t n);\n"
                 "const char *apertis_name(int code);\nconst char* apertis_name2(void);\n")
    assert sigs["apertis_p"] == (ctypes.c_int, [VP, VP, VP, VP, ctypes.c_int64])
    assert sigs["apertis_s"] == (ctypes.c_int, [VP, VP, ctypes.c_int64])            # a struct pointer is a pointer
    assert sigs["apertis_name"] == (ctypes.c_char_p, [ctypes.c_int]) and sigs["apertis_name2"] == (ctypes.c_char_p, [])


def test_declaration_over_three_lines_void_and_empty_lists_and_order():
    sigs = _sigs("int apertis_b(const void *x, int64_t x_rs,\n"
                 "              float eps /* inline */, uint64_t seed,\n"
                 "              void *stream);   /* trailing */\n"
                 "int64_t apertis_a(void);\nint apertis_c();\n")
    assert list(sigs) == ["apertis_b", "apertis_a", "apertis_c"]                    # declaration order, not sorted
    assert sigs["apertis_b"] == (ctypes.c_int, [VP, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64, VP])
    assert sigs["apertis_a"] == (ctypes.c_int64, []) and sigs["apertis_c"] == (ctypes.c_int, [])


def test_comments_preprocessor_lines_and_other_statements_are_not_declarations():
    sigs, consts = parse_header("/* int apertis_in_block(int a);\n * call apertis_foo(x, y) first */\n"
                                "// int apertis_in_line(int a);\n"
                                "#include \"apertis_other.h\"\n#ifdef __cplusplus\nextern \"C\" {\n#endif\n"
                                "typedef struct apertis_rec {\n  float *p, *g;\n  int64_t numel;\n} apertis_rec;\n"
                                "int apertis_real(int a); // int apertis_after(int b);\n"
                                "#ifdef __cplusplus\n}\n#endif\n", "synthetic.h")
    assert list(sigs) == ["apertis_real"] and consts == {}


def test_integer_defines_of_every_form_and_what_is_skipped():
    _, consts = parse_header("#ifndef APERTIS_X_H\n#define APERTIS_X_H\n"
                             "#define APERTIS_OK 0\n#define APERTIS_ERR_ARG (-1)   /* bad argument */\n"
                             "#define APERTIS_FLAG 0x100\n#define APERTIS_INTS 512 // one per XCD\n"
                             "#define APERTIS_VERSION ((4 << 16) | 12)\n"
                             "#define APERTIS_MAX(a, b) ((a) > (b) ? (a) : (b))\n#define APERTIS_SQ(x) 4\n"
                             "#define APERTIS_SCALE 1.5f\n#define APERTIS_NAME \"gfx950\"\n#define APERTIS_ALIAS APERTIS_OK\n"
                             "#define OTHER_THING 7\n#endif\n", "synthetic.h")
    assert consts == {"APERTIS_OK": 0, "APERTIS_ERR_ARG": -1, "APERTIS_FLAG": 256, "APERTIS_INTS": 512,
                      "APERTIS_VERSION": (4 << 16) | 12}
    assert all(type(v) is int for v in consts.values())


@pytest.mark.parametrize("text,names", [
    ("int apertis_f(const void *x, size_t n);", ("apertis_f", "size_t")),                  # a type outside the table
    ("int apertis_f(unsigned int n);", ("apertis_f", "unsigned int n")),
    ("int apertis_f(const void *x, int64_t);", ("apertis_f", "int64_t")),                  # nameless parameters
    ("int apertis_f(const float *, int64_t n);", ("apertis_f", "const float *")),
    ("size_t apertis_f(int64_t n);", ("apertis_f", "size_t")),                             # return types outside the table
    ("float *apertis_f(int64_t n);", ("apertis_f", "float *")),
    ("int apertis_ok(int a);\nint apertis_f(const void *x, int64_t n\n", ("apertis_f",)),  # unterminated
    ("int apertis_f(const void *x, int64_t n)\nint apertis_g(int a);", ("apertis_f",)),    # no semicolon
    ("int\napertis_f(int a);", ("apertis_f",)),                                            # starts, but not `RET name(ARGS);`
    ("int apertis_f(int (*cb)(int), int n);", ("apertis_f",)),
    ("int apertis_f(int a);\nint apertis_f(int a);", ("apertis_f", "twice")),
    ("#define APERTIS_BAD (1 <<)\n", ("APERTIS_BAD",)),
])
def test_what_the_reader_cannot_type_is_an_error_not_a_skip(text, names):
    with pytest.raises(ApertisHipError) as e:
        parse_header(text, "synthetic.h")
    assert "synthetic.h" in str(e.value) and all(n in str(e.value) for n in names), str(e.value)


def test_a_missing_header_is_an_error_with_its_path(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "INCLUDE_DIR", str(tmp_path))
    with pytest.raises(ApertisHipError, match=re.escape(os.path.join(str(tmp_path), "apertis_hip.h"))):
        _lib._read_header("apertis_hip.h")


# ------------------------------------------------------------------------------------------------ the real headers
def _header(name):
    with open(os.path.join(ROOT, "include", name), encoding="utf-8") as f:
        return f.read()


def test_the_tables_are_the_two_headers():
    main, ext = parse_header(_header("apertis_hip.h"), "apertis_hip.h"), parse_header(_header("apertis_hip_ext.h"), "apertis_hip_ext.h")
    assert len(main[0]) == 123 and len(ext[0]) == 2 and not set(main[0]) & set(ext[0])
    assert list(_lib.SIGNATURES.items()) == list(main[0].items()) and list(_lib.EXT_SIGNATURES.items()) == list(ext[0].items())
    assert type(_lib.SIGNATURES) is dict and type(_lib.EXT_SIGNATURES) is dict
    assert ext[1] == {}                                               # #include is not followed: no constant of the first header
    assert os.path.samefile(_lib.INCLUDE_DIR, os.path.join(ROOT, "include")) and _lib.HEADERS == ("apertis_hip.h", "apertis_hip_ext.h")
    for name, n in (("apertis_moe_enter_small", 33), ("apertis_sample_next", 28), ("apertis_boundary_router_bwd", 29)):
        assert len(_lib.SIGNATURES[name][1]) == n and _lib.SIGNATURES[name][0] is ctypes.c_int
    assert _lib.SIGNATURES["apertis_arch"] == (ctypes.c_char_p, []) and _lib.SIGNATURES["apertis_strerror"] == (ctypes.c_char_p, [ctypes.c_int])
    assert _lib.SIGNATURES["apertis_adamw_step"][1][4:9] == [ctypes.c_double] * 5
    assert ctypes.c_uint32 in _lib.SIGNATURES["apertis_scan_gate_fwd"][1]


def test_the_constants_are_the_headers_defines():
    c = _lib.CONSTANTS
    assert (_lib.OK, _lib.ERR_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_LAUNCH) == (0, -1, -2, -3)
    assert (_lib.F32, _lib.BF16) == (0, 1) and (_lib.ACT_NONE, _lib.ACT_GELU, _lib.ACT_RELU, _lib.ACT_SILU) == (0, 1, 2, 3)
    assert (_lib.ACT_SAVE_GRAD, _lib.ACT_MUL_SAVED) == (0x100, 0x200) and _lib.ABI_VERSION == (4 << 16) | 12
    assert c["APERTIS_NT_QUEUE_INTS"] == 512 and c["APERTIS_ATTN_DECODE_MAX_SPLITS"] == 64
    assert c["APERTIS_SAMPLE_MAX_VOCAB"] == 262144 and c["APERTIS_SAMPLE_MAX_ROWS"] == 65535
    hdr = re.sub(r"/\*.*?\*/", "", _header("apertis_hip.h"), flags=re.S)
    valued = set(re.findall(r"^#define (APERTIS_\w+)[ \t]+\S", hdr, flags=re.M))
    assert valued == set(c), valued ^ set(c)                          # every valued #define of the header is an integer it read


def _definitions():
    """{file: [names]} of the `extern "C" ... apertis_name(` definitions in csrc/*.hip."""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path, encoding="utf-8") as f:
            names = re.findall(r'extern\s+"C"\s+[\w \t*]+?\b(apertis_\w+)\s*\(', f.read())
        if names:
            out[path] = names
    return out


def test_defined_and_declared_entry_points_are_the_same_set():
    defined = [n for names in _definitions().values() for n in names]
    declared = [*_lib.SIGNATURES, *_lib.EXT_SIGNATURES]
    assert len(defined) == len(set(defined)) == len(declared) >= 125
    assert set(defined) == set(declared), set(defined) ^ set(declared)


def _reached(path, seen):
    """Every file `path` reaches through quoted #includes (relative to the including file), itself included."""
    path = os.path.realpath(path)
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    with open(path, encoding="utf-8") as f:
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', f.read(), flags=re.M):
            _reached(os.path.join(os.path.dirname(path), inc), seen)
    return seen


def test_every_definition_is_compiled_against_its_declaration():
    """clang rejects a C-linkage definition that differs from a visible declaration, so the definition's file must see it."""
    home = {n: os.path.realpath(os.path.join(ROOT, "include", h))
            for h, table in zip(_lib.HEADERS, (_lib.SIGNATURES, _lib.EXT_SIGNATURES)) for n in table}
    defs = _definitions()
    assert sum(len(names) for names in defs.values()) == len(home)
    for path, names in defs.items():
        seen = _reached(path, set())
        assert all(p.startswith(os.path.realpath(ROOT) + os.sep) for p in seen), (path, seen)
        missing = [n for n in names if home[n] not in seen]
        assert not missing, (os.path.basename(path), missing)


def test_every_entry_point_the_python_code_names_is_declared():
    files = glob.glob(os.path.join(ROOT, "apertis_llm_amd", "**", "*.py"), recursive=True)
    files += glob.glob(os.path.join(ROOT, "tools", "*.py")) + [os.path.join(ROOT, "__graft_entry__.py")]
    assert len(files) > 20
    declared = set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES)
    unknown, seen = {}, set()
    for path in files:
        with open(path, encoding="utf-8") as f:
            for name in re.findall(r"\.(apertis_\w+)\b", f.read()):
                seen.add(name)
                if name not in declared:
                    unknown.setdefault(os.path.relpath(path, ROOT), set()).add(name)
    assert not unknown, unknown
    assert len(seen) > 100                                            # (the pattern does find the call sites)
