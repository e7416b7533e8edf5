"""ctypes binding of the C-ABI in include/tsmarl.h (lib/libtsmarl_hip.so).

This is the only place the package touches native code.  There is NO fallback: if the HIP
library is missing or a call fails, the op raises (ImportError / RuntimeError / ValueError /
MalformedBufferError) -- nothing here ever routes through oracle/ or a CPU path.
PyTorch is used by callers only to own device memory and streams; this module sees raw pointers.

The header is the only statement of the ABI: at import `read_header` derives every struct, signature and constant from it,
so an entry point is added by declaring it in tsmarl.h and nowhere else.  It reads the C the header is written in --
`/* */` comments, `#define NAME INT`, `enum { NAME = INT, .. };`, `typedef struct [tag] { .. } name;`, one prototype per `;`,
several declarators per member line, array lengths INT | NAME | NAME + INT -- and raises ValueError on anything else.
The mapping rules:
  - scalars map directly: int, int32_t, uint32_t, int64_t, uint64_t, float, double, uint8_t;
  - [const] char * is c_char_p, as argument and as return;
  - a pointer to a struct declared in the header is POINTER(that struct);
  - every other pointer is c_void_p (device pointers, void **, int *, const float *const *);
  - struct members follow the same rules, except that ANY pointer member is c_void_p; an array is type * n, a nested
    struct is stored by value; names and order are the header's, _pad fields included;
  - a function returns a status (`call` raises on non-zero) unless its return type is not int or TSM_VALUE marks it.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from types import SimpleNamespace

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtsmarl_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tsmarl.h")


class MalformedBufferError(RuntimeError):
    """Mirror of tianshou.data.buffer.buffer_base.MalformedBufferError (buffer_base.py:17-18)."""


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double, "uint8_t": C.c_uint8}
_PTRS = r"((?:\*\s*)*)"  # the stars of a declarator


def _ctype(base: str, n_ptr: int, structs: dict, member: bool = False):
    """ctypes type of `base` behind n_ptr stars: the mapping rules of the module docstring."""
    if n_ptr == 0 and base in _SCALARS:
        return _SCALARS[base]
    if n_ptr == 0 and base in structs:
        return structs[base]
    if n_ptr == 1 and not member and base == "char":
        return C.c_char_p
    if n_ptr == 1 and not member and base in structs:
        return C.POINTER(structs[base])
    if n_ptr >= 1:
        return C.c_void_p
    raise ValueError(f"tsmarl.h reader: unknown type {base!r}")


def _length(expr: str, consts: dict) -> int:
    """An array length: INT, NAME or NAME + INT."""
    m = re.fullmatch(r"\s*(?:(\d+)|(\w+)(?:\s*\+\s*(\d+))?)\s*", expr)
    if not m or (m.group(2) and m.group(2) not in consts):
        raise ValueError(f"tsmarl.h reader: cannot resolve the array length [{expr}]")
    return int(m.group(1)) if m.group(1) else consts[m.group(2)] + int(m.group(3) or 0)


def read_header(txt: str) -> SimpleNamespace:
    """What a header text declares: defines / enums {name: int}, structs {name: ctypes.Structure class},
    signatures {name: (restype, argtypes)} and no_status, the functions whose return is a value.  ValueError on anything
    outside the subset of C the module docstring lists."""
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    defines, enums, structs, signatures, no_status = {}, {}, {}, {}, set()
    for name, value in re.findall(r"(?m)^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]*(.*?)[ \t]*$", txt):
        if value and not re.fullmatch(r"-?\d+", value):
            raise ValueError(f"tsmarl.h reader: #define {name} {value} is not an integer")
        if value:
            defines[name] = int(value)
    txt = re.sub(r"(?m)^[ \t]*#.*$", "", txt)
    txt = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", txt, flags=re.S)

    def enum(m):
        for entry in filter(None, (e.strip() for e in m.group(1).split(","))):
            em = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", entry)
            if not em:
                raise ValueError(f"tsmarl.h reader: enum entry `{entry}` needs an explicit integer value")
            enums[em.group(1)] = int(em.group(2))
        return ""

    def struct(m):
        fields = []
        for stmt in filter(None, (s.strip() for s in re.sub(r"\bconst\b", " ", m.group(1)).split(";"))):
            base, declarators = re.fullmatch(r"(\w*)(.*)", stmt, flags=re.S).groups()
            for d in declarators.split(","):
                dm = re.fullmatch(r"\s*" + _PTRS + r"(\w+)\s*(?:\[([^\]]*)\])?\s*", d)
                if not dm:
                    raise ValueError(f"tsmarl.h reader: unsupported member `{stmt}` of {m.group(2)}")
                t = _ctype(base, dm.group(1).count("*"), structs, member=True)
                fields.append((dm.group(2), t if dm.group(3) is None else t * _length(dm.group(3), {**defines, **enums})))
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        return ""

    txt = re.sub(r"\benum\s*\{(.*?)\}\s*;", enum, txt, flags=re.S)
    txt = re.sub(r"\btypedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", struct, txt, flags=re.S)
    for stmt in filter(None, (s.strip() for s in re.sub(r"\bconst\b", " ", txt).split(";"))):
        m = re.fullmatch(r"(TSM_VALUE\s+)?(\w+)\s*" + _PTRS + r"(\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m:
            raise ValueError(f"tsmarl.h reader: unsupported declaration `{stmt}`")
        value, base, stars, name, params = m.groups()
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            pm = re.fullmatch(r"\s*(\w+)\s*" + _PTRS + r"\w*\s*", p)
            if not pm:
                raise ValueError(f"tsmarl.h reader: unsupported parameter `{p.strip()}` of {name}")
            argtypes.append(_ctype(pm.group(1), pm.group(2).count("*"), structs))
        signatures[name] = (_ctype(base, stars.count("*"), structs), argtypes)
        if value or signatures[name][0] is not C.c_int:
            no_status.add(name)
    return SimpleNamespace(defines=defines, enums=enums, structs=structs, signatures=signatures, no_status=no_status)


try:
    with open(HEADER_PATH) as _f:
        _header = read_header(_f.read())
except OSError as _e:
    raise ImportError(f"{HEADER_PATH} is missing: the binding is derived from it, there is no second copy") from _e

# name -> (restype, argtypes) of every function the header declares; the names whose return is a value, not a status
SIGNATURES, _NO_STATUS = _header.signatures, _header.no_status
# every tsm_* struct under its name; TSM_OK and the other enum constants under theirs; every `#define TSM_X n` as X
# (ABI_VERSION, MAX_GATHER_FIELDS, the *_ROWS_PER_BLOCK and *_MAX_* limits)
globals().update(_header.structs)
globals().update(_header.enums)
globals().update({name[4:]: value for name, value in _header.defines.items() if name.startswith("TSM_")})

_lib = None


def header_symbols() -> list[str]:
    """Every function name declared in include/tsmarl.h."""
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tsm_[a-z0-9_]+)\s*\(", txt)))


def load() -> C.CDLL:
    """Load the HIP library (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m tianshou_marl_amd._build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.tsm_abi_version() != ABI_VERSION:
        raise ImportError(f"ABI version mismatch: library reports {lib.tsm_abi_version()}")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc == TSM_OK:
        return
    msg = load().tsm_last_error().decode("utf-8", "replace")
    if rc == TSM_ERR_INVALID:
        raise ValueError(msg)
    if rc == TSM_ERR_MALFORMED_BUFFER:
        raise MalformedBufferError(msg)
    raise RuntimeError(f"tsmarl error {rc}: {msg}")


def call(name: str, *args):
    """Call an ABI function; status-returning functions raise on failure."""
    fn = getattr(load(), name)
    out = fn(*args)
    if name in _NO_STATUS:
        return out
    check(out)
    return None


def ptr(t) -> int | None:
    """Device pointer of a torch tensor (None -> NULL).  Requires a contiguous CUDA/HIP tensor."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("tianshou_marl_amd ops need device (HIP) tensors; there is no CPU path")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()


_raw_stream = None


def stream_ptr() -> int:
    """hipStream_t of torch's current stream on the current device (the stream every op launches on; inside a capture, the
    capturing stream).  Asked of torch's C layer directly: `torch.cuda.current_stream().cuda_stream` builds a Stream object and
    resolves the device through four Python layers -- 4 us a call, six calls per step of the tag job (profiles/r05_host_tag.txt)."""
    global _raw_stream
    import torch

    if _raw_stream is None:
        get, dev = getattr(torch._C, "_cuda_getCurrentRawStream", None), getattr(torch._C, "_cuda_getDevice", None)
        if get is None or dev is None:
            _raw_stream = False
        else:
            torch.cuda.init()
            _raw_stream = (get, dev)
    if _raw_stream is False:
        return torch.cuda.current_stream().cuda_stream
    get, dev = _raw_stream
    return get(dev())
