"""ctypes binding of libapertis_hip.so (the C ABI declared in include/apertis_hip.h).  The argument lists and constants are
not repeated here: they are read from the headers at import (parse_header), so declaring an entry point there binds it.

The library is loaded lazily (safe after fork(); DataLoader workers never touch HIP) and there
is NO fallback: if the .so is missing or a call returns an error code, ApertisHipError is
raised.  Nothing in this package routes compute through PyTorch eager ops or the CPU oracle.
"""
import ctypes
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# APERTIS_HIP_LIB: developer switch - another build of the same library (tools/ A/B runs); never a fallback
LIB_PATH = os.environ.get("APERTIS_HIP_LIB") or os.path.join(_HERE, "libapertis_hip.so")
# the C headers: what the library is compiled against (build.py watches these two files) and what this binding is read from
INCLUDE_DIR = os.path.join(_HERE, "..", "include")
HEADERS = ("apertis_hip.h", "apertis_hip_ext.h")


class ApertisHipError(RuntimeError):
    pass


_lock = threading.Lock()
_lib = None

# The closed table of value types the headers use; every pointer parameter is a c_void_p and `const char *` is returned as c_char_p.
_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double}
_DECL = re.compile(r"^[ \t]*([\w \t*]+?)[ \t]*\b(apertis_\w+)[ \t]*\(([^()]*)\)\s*;", re.M)
_PARAM = re.compile(r"\s*(?:const\s+)?(\w+)(\s*\*\s*|\s+)(\w+)\s*")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(APERTIS_\w+)[ \t]+(\S.*?)[ \t]*$", re.M)
_INT_EXPR = re.compile(r"(?:0[xX][0-9a-fA-F]+|\d+|<<|[()|\- ])+")


def parse_header(text, where):
    """(signatures, constants) of one C header's text: `RET apertis_name(ARGS);` -> name: (restype, [argtypes]) in declaration
    order, and `#define APERTIS_NAME <integer expression>` -> APERTIS_NAME: int.  #include is not followed.  Function-like macros
    and non-integer values are skipped; a declaration this reader cannot type raises ApertisHipError (`where` names the header)
    - a row skipped or guessed here would be a call with the wrong argument list."""
    def fail(what, why):
        raise ApertisHipError(f"{where}: {what}: {why}")

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {}
    for name, value in _DEFINE.findall(text):
        if _INT_EXPR.fullmatch(value):
            try:
                consts[name] = int(eval(value, {"__builtins__": {}}))       # digits, hex, ( ) << | - only: see _INT_EXPR
            except (SyntaxError, TypeError):
                fail(f"#define {name} {value}", "not an integer expression")
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    sigs = {}
    for ret, name, params in _DECL.findall(text):
        ret = " ".join(ret.replace("*", " * ").split())
        restype = ctypes.c_char_p if ret == "const char *" else _CTYPES.get(ret)
        if restype is None or name in sigs:
            fail(f"declaration of {name}", "declared twice" if name in sigs else f"return type `{ret}` is not in the binding's type table")
        argtypes = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            m = _PARAM.fullmatch(p)
            if m is None:
                fail(f"declaration of {name}", f"parameter `{p.strip()}` is not `type name`")
            ctype = ctypes.c_void_p if "*" in m.group(2) else _CTYPES.get(m.group(1))
            if ctype is None:
                fail(f"declaration of {name}", f"parameter type `{m.group(1)}` is not in the binding's type table")
            argtypes.append(ctype)
        sigs[name] = (restype, argtypes)
    stray = re.search(r"\bapertis_\w+\s*\(", _DECL.sub("", text))
    if stray:
        fail(f"declaration of {stray.group()[:-1].strip()}", "starts here but does not parse as `RET apertis_name(ARGS);`")
    return sigs, consts


def _read_header(name):
    path = os.path.join(INCLUDE_DIR, name)
    try:
        with open(path, encoding="utf-8") as f:
            return parse_header(f.read(), name)
    except OSError as e:
        raise ApertisHipError(f"{path}: the C header this binding is read from cannot be opened ({e.strerror}); "
                              "there is no built-in table") from None


# name -> (restype, argtypes), in declaration order: the headers ARE the tables (read once, here, at import).  EXT_SIGNATURES holds
# the entry points added after the 4.12 table (apertis_hip_ext.h): exported by the same library under the same ABI version.
(SIGNATURES, CONSTANTS), (EXT_SIGNATURES, _ext_consts) = (_read_header(h) for h in HEADERS)
CONSTANTS.update(_ext_consts)
ABI_VERSION, F32, BF16 = (CONSTANTS["APERTIS_" + n] for n in ("ABI_VERSION", "F32", "BF16"))
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU = (CONSTANTS["APERTIS_ACT_" + n] for n in ("NONE", "GELU", "RELU", "SILU"))
ACT_SAVE_GRAD, ACT_MUL_SAVED = CONSTANTS["APERTIS_ACT_SAVE_GRAD"], CONSTANTS["APERTIS_ACT_MUL_SAVED"]   # flags of grouped_gemm_nt's `act`
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_LAUNCH = (CONSTANTS["APERTIS_" + n] for n in ("OK", "ERR_ARG", "ERR_UNSUPPORTED", "ERR_LAUNCH"))


class _Lib:
    """CDLL wrapper that binds each entry point on first use with its declared signature (either table)."""

    def __init__(self, cdll):
        self._cdll = cdll

    def __getattr__(self, name):
        table = SIGNATURES if name in SIGNATURES else EXT_SIGNATURES
        if name not in table:
            raise AttributeError(name)
        try:
            fn = getattr(self._cdll, name)
        except AttributeError:
            raise ApertisHipError(f"{LIB_PATH} does not export {name}: rebuild with "
                                  "`python -m apertis_llm_amd.build --force`") from None
        fn.restype, fn.argtypes = table[name]
        setattr(self, name, fn)
        return fn


def load():
    """Return the loaded library. Raises ApertisHipError if the .so is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ApertisHipError(
                f"{LIB_PATH} not found: build it with `python -m apertis_llm_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU or eager fallback.")
        cdll = ctypes.CDLL(LIB_PATH)
        # the binding below is written against ONE version of include/apertis_hip.h: another build of the library (a stale
        # in-tree .so, or APERTIS_HIP_LIB pointing at an older one) would be called with the wrong argument lists
        try:
            got = int(cdll.apertis_abi_version())
        except AttributeError:
            got = -1
        if got != ABI_VERSION:
            raise ApertisHipError(f"{LIB_PATH} has ABI version {got >> 16}.{got & 0xffff} but this binding needs "
                                  f"{ABI_VERSION >> 16}.{ABI_VERSION & 0xffff}: rebuild with `python -m apertis_llm_amd.build --force`")
        _lib = _Lib(cdll)
    return _lib


def check(rc, what):
    if rc != 0:
        msg = load().apertis_strerror(int(rc)).decode()
        raise ApertisHipError(f"{what} failed: {msg} (code {rc})")


def ptr(t):
    """Device pointer of a tensor (or None) as a plain integer: every entry point has its argtypes declared, so ctypes
    converts it itself (a c_void_p object per argument was a third of the Python time of a launch)."""
    return None if t is None else t.data_ptr()


_raw_stream = None


def stream_ptr():
    """torch's current stream of the current device, as the integer the C ABI takes.  torch.cuda.current_stream() builds a
    Stream object through three Python layers (5 us; a step makes thousands of launches): ask the binding directly."""
    global _raw_stream
    if _raw_stream is None:
        import torch
        get_dev, get_raw = getattr(torch._C, "_cuda_getDevice", None), getattr(torch._C, "_cuda_getCurrentRawStream", None)
        if get_dev is not None and get_raw is not None:
            _raw_stream = lambda: get_raw(get_dev())                            # noqa: E731
        else:
            _raw_stream = lambda: torch.cuda.current_stream().cuda_stream       # noqa: E731
    return _raw_stream()


def dtype_code(t):
    import torch
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise ApertisHipError(f"unsupported dtype {t.dtype}: kernels take float32 or bfloat16")
