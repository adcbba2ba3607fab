"""ctypes binding of the C ABI declared in include/morpheus_hip.h.

The header is the only description of an entry point: its declarations are parsed when this module is imported and give every
exported function its ctypes signature (parse_header, bind).  A new entry point is declared there and defined in a .hip file;
nothing is registered here.  Stream-taking entry points are called through launch(), host-only ones (size queries, mh_graph_*)
directly on load().
The product path has no CPU fallback: if the library is missing or a call fails this raises.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Optional

import torch

from .build import HEADER, SO as _BUILT_SO

# MORPHEUS_HIP_LIB: load another build of the SAME library (`python -m morpheus_amd.build --name NAME [--rev REV] [-- FLAG ...]`:
# the product's recipe and per-file flags on another revision or with extra flags, compared on one box by tools/gpu/lib_ab.sh);
# the default is the in-tree build, and there is still no fallback to anything that is not this library
SO = os.environ.get("MORPHEUS_HIP_LIB") or _BUILT_SO


class MorpheusHipError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double}
_DECL = re.compile(r"(?P<res>[\w\s*]+?)\s*\b(?P<name>mh_\w+)\s*\((?P<params>[^()]*)\)")


def _ctype(decl: str, what: str, result: bool = False):
    """ctypes type of one parameter (`const float *x`, `int64_t M`) or of the result type (`int`, `const char *`) of `decl`.
    Every pointer parameter is a c_void_p: callers pass raw addresses, None, ctypes.byref(...) and numpy's data_as(c_void_p)."""
    words = what.replace("*", " * ").split()
    if "*" in words:
        if not result:
            return ctypes.c_void_p
        if words == ["const", "char", "*"]:
            return ctypes.c_char_p
    else:
        words = [w for w in words if w != "const"]
        if len(words) == (1 if result else 2) and words[0] in _SCALARS:      # a parameter is `type name`
            return _SCALARS[words[0]]
    raise MorpheusHipError(f"include/morpheus_hip.h: no ctypes type for `{what.strip()}` in `{decl}` (pointers, "
                           f"{', '.join(_SCALARS)}; `const char *` as a result)")


def parse_header(text: str):
    """The header's text -> (MH_ABI_VERSION, {name: (restype, argtypes)} in header order).  Behind the comments and the
    preprocessor lines every statement must be a declaration `<result> mh_<name>(<parameters>)` of types _ctype knows: anything
    else raises, so that no exported function is left to ctypes' default signature (int arguments, int result)."""
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    abi = re.search(r"^[ \t]*#[ \t]*define[ \t]+MH_ABI_VERSION[ \t]+(\d+)[ \t]*$", text, flags=re.M)
    if abi is None:
        raise MorpheusHipError("include/morpheus_hip.h: no `#define MH_ABI_VERSION <number>`")
    text = re.sub(r'extern\s+"C"\s*\{|\}', " ", re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M))
    sigs = {}
    for decl in text.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = _DECL.fullmatch(decl)
        if m is None:
            raise MorpheusHipError(f"include/morpheus_hip.h: not a declaration of an mh_ entry point: `{decl}`")
        params = [] if m["params"].strip() == "void" else m["params"].split(",")
        sigs[m["name"]] = (_ctype(decl, m["res"], result=True), [_ctype(decl, p) for p in params])
    return int(abi[1]), sigs


with open(HEADER) as _f:
    _ABI, _DECLARED = parse_header(_f.read())
EXPORTS = tuple(_DECLARED)
_lib = None
_fns = {}           # name -> bound function of the loaded library (launch() looks entry points up here, not by getattr)


def bind(cdll, header_text: Optional[str] = None) -> dict:
    """Give every entry point the header declares its signature on `cdll` -- the product library or a side build of it -- and
    check that the library was built against this header's ABI version.  -> {name: bound function}"""
    abi, declared = (_ABI, _DECLARED) if header_text is None else parse_header(header_text)
    fns = {}
    for name, (res, args) in declared.items():
        fn = fns[name] = getattr(cdll, name)
        fn.restype, fn.argtypes = res, args
    if fns["mh_abi_version"]() != abi:
        raise MorpheusHipError(f"{cdll._name}: ABI version {fns['mh_abi_version']()}, include/morpheus_hip.h declares {abi} "
                               "(rebuild: `python -m morpheus_amd.build`)")
    return fns


def load():
    """Load libmorpheus_hip.so; never falls back to anything else."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise MorpheusHipError(
                f"{SO} not found: build it with `python -m morpheus_amd.build` (hipcc, gfx950). "
                "The hot path has no CPU/PyTorch fallback by design.")
        lib = ctypes.CDLL(SO)
        fns = bind(lib)
        if os.environ.get("MORPHEUS_GRID_STAGE_MIN_POINTS"):       # tuning knob, see include/morpheus_hip.h
            lib.mh_grid_stage_min_points(int(os.environ["MORPHEUS_GRID_STAGE_MIN_POINTS"]))
        if os.environ.get("MORPHEUS_WARP_SKIP_ZERO_LINES"):        # A/B switch, see include/morpheus_hip.h (0: fetch every parked row)
            lib.mh_warp_skip_zero_lines(int(os.environ["MORPHEUS_WARP_SKIP_ZERO_LINES"]))
        if os.environ.get("MORPHEUS_WARP_ELIDE_ZERO_LINES"):       # A/B switch, see include/morpheus_hip.h (0: every parked line is written)
            lib.mh_warp_elide_zero_lines(int(os.environ["MORPHEUS_WARP_ELIDE_ZERO_LINES"]))
        _fns.update(fns)
        _lib = lib
    return _lib


def ptr(t):
    """Device pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "C ABI takes contiguous buffers"
    return t.data_ptr()


# torch.cuda.current_stream() builds a Stream object through three Python layers (device-index resolution, an availability check
# that reads os.environ, Stream.__new__): ~7 us, once per C-ABI call, ~100 calls per eager real-view step whose host time IS the
# step time (tools/gpu/host_profile.py).  The raw handle of the same stream, through torch's accessors when it has them:
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda device: torch.cuda.current_stream(device).cuda_stream)
_CUR_DEVICE = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def stream():
    return _RAW_STREAM(_CUR_DEVICE())


def check(status: int, what: str):
    if status != 0:
        raise MorpheusHipError(f"{what}: {load().mh_status_string(status).decode()} (status {status})")


def launch(name: str, *args):
    """Call the stream-taking entry point `name` with torch's CURRENT stream behind `args`; a failing status raises, naming it.
    (~100 calls per eager training step: the function is looked up in the dict bind() made, stream() is written out.)"""
    if not _fns:
        load()
    status = _fns[name](*args, _RAW_STREAM(_CUR_DEVICE()))
    if status != 0:
        check(status, name)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise MorpheusHipError("morpheus_amd ops run on an MI355X only (tensor is on %s); there is no CPU path"
                                   % t.device)
