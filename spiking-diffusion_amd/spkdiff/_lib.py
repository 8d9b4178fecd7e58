"""ctypes binding of ``libspkdiff.so`` (the C-ABI declared in ``include/spkdiff.h``).

The library is the ONLY engine of this package: if it is missing (not built) the import fails loudly --
there is no PyTorch/CPU fallback anywhere in the product path.  ``torch`` is imported first so that the
HIP runtime the library binds to is the one PyTorch-ROCm already loaded (same ``libamdhip64.so`` soname),
which is what makes torch's device pointers and streams valid arguments.

The header is the single definition of the ABI.  This module reads it at import: every ``ret spk_name(args);``
declaration becomes the ``restype`` / ``argtypes`` of that symbol, ``SPK_VERSION`` becomes ``EXPECTED_VERSION`` and every
integer ``#define SPK_*`` an entry of ``CONSTANTS`` (the enumerations and limits ``ops.py`` names).  Adding an entry point
means the header plus the ``.hip`` file and nothing else.  The header is plain C with a tiny vocabulary, so the reader is a
few regular expressions; a declaration outside that vocabulary is an error at import, never a guess.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int, c_longlong, c_ulonglong, c_void_p
from types import MappingProxyType

import torch  # noqa: F401  (must precede the dlopen below: shares torch's HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPKDIFF_LIB") or os.path.join(_HERE, "libspkdiff.so")   # SPKDIFF_LIB: A/B builds
# the tree is used in place: the header lies where csrc/Makefile finds it
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "spkdiff.h"))


class SpkdiffError(RuntimeError):
    pass


# ---- the header reader -------------------------------------------------------------------------------------------
_BY_VALUE = {"int": c_int, "long long": c_longlong, "unsigned long long": c_ulonglong, "float": c_float,
             "spk_stream_t": c_void_p}
_TYPE = "|".join(sorted(_BY_VALUE, key=len, reverse=True))
_NAME = r"(?!(?:int|long|short|char|unsigned|signed|float|double|void|const|struct)\b)[A-Za-z_]\w*"
_PARAM = re.compile(rf"(?:const )?({_TYPE})(?: const)?(?: {_NAME})?")
_DECL = re.compile(rf"(.+?)\b(spk_\w+) ?\(([^()]*)\)")
_MACRO = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(SPK_\w+)[ \t]+(\(?)(-?(?:0[xX][0-9a-fA-F]+|0|[1-9]\d*))(\)?)[ \t]*$", re.M)


def _without_comments(text: str) -> str:
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def read_constants(text: str) -> dict:
    """``{name: value}`` of every ``#define SPK_NAME <integer literal>`` (also ``(-64)``).  Anything else a macro may
    expand to is skipped, not guessed."""
    return {name: int(digits, 0) for name, lp, digits, rp in _MACRO.findall(_without_comments(text))
            if bool(lp) == bool(rp)}


def read_signatures(text: str) -> dict:
    """``{name: (restype, [argtypes])}`` of every function the header text declares, in declaration order.  A pointer
    (anything with a ``*``) and ``spk_stream_t`` are ``c_void_p``; ``int``, ``long long``, ``unsigned long long`` and
    ``float`` go by value; a ``const char*`` return is ``c_char_p``.  Every other statement raises ``ValueError``."""
    text = re.sub(r"^[ \t]*#.*$", " ", _without_comments(text), flags=re.M)        # preprocessor lines
    text = re.sub(r'extern\s*"C"\s*\{|\}', " ", text)
    sigs = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        if not decl or decl.startswith("typedef "):
            continue
        m = _DECL.fullmatch(decl)
        if not m:
            raise ValueError(f"spkdiff.h: not a function declaration this binding can read: `{decl};`")
        ret, name, params = " ".join(m[1].replace("*", " * ").split()), m[2], m[3].strip()
        if name in sigs:
            raise ValueError(f"spkdiff.h: {name} is declared twice: `{decl};`")
        if ret != "const char *" and ret not in ("int", "long long", "unsigned long long", "float"):
            raise ValueError(f"spkdiff.h: return type `{ret}` of `{decl};` is outside the binding's vocabulary")
        args = []
        for p in ([] if params == "void" else params.split(",")):
            by_value = None if "*" in p else _PARAM.fullmatch(p.strip())
            if "*" not in p and not by_value:
                raise ValueError(f"spkdiff.h: parameter `{p.strip()}` of `{decl};` is outside the binding's vocabulary")
            args.append(_BY_VALUE[by_value[1]] if by_value else c_void_p)
        sigs[name] = (c_char_p if "*" in ret else _BY_VALUE[ret], args)
    return sigs


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"spkdiff: native library not found at {LIB_PATH}. Build it with "
            f"`make -C {os.path.join(os.path.dirname(_HERE), 'csrc')}` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no fallback path: the HIP kernels are the implementation.")
    if not os.path.exists(HEADER_PATH):
        raise ImportError(
            f"spkdiff: C-ABI header not found at {HEADER_PATH}. The binding reads its signatures and constants from it: "
            "use the package from its source tree, next to include/.")
    with open(HEADER_PATH) as f:
        return ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL), f.read()


lib, _header = _load()
CONSTANTS = MappingProxyType(read_constants(_header))      # the header's integer macros: SPK_MODE_LIF, SPK_ERR_ARG, ...
_sigs = read_signatures(_header)
EXPORTS = tuple(_sigs)
# The library has no settable launch options (every launch shape is fixed in the sources); code written against earlier
# revisions branches on this flag.
HAS_OPTIONS = False

for _name, (_res, _args) in _sigs.items():
    _fn = getattr(lib, _name)      # AttributeError here = header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


def check(rc: int, what: str = ""):
    """Translate a C-ABI return code into the exception the reference surface would raise."""
    if rc == 0:
        return
    msg = lib.spk_error_string(rc).decode()
    if rc == CONSTANTS["SPK_ERR_ARG"]:
        raise ValueError(f"{what}: {msg}")
    if rc == CONSTANTS["SPK_ERR_UNSUPPORTED"]:
        raise NotImplementedError(f"{what}: {msg}")
    raise SpkdiffError(f"{what}: HIP error {rc}: {msg}")


def version() -> int:
    return lib.spk_version()


# The signatures set above are those of include/spkdiff.h at its SPK_VERSION.  A stale libspkdiff.so or an SPKDIFF_LIB A/B
# variant built from another header would take arguments at the wrong positions (silently wrong results): refuse it here.
EXPECTED_VERSION = CONSTANTS["SPK_VERSION"]
if version() != EXPECTED_VERSION:
    raise ImportError(f"spkdiff: {LIB_PATH} reports C-ABI version {version()}, this binding declares version "
                      f"{EXPECTED_VERSION} (include/spkdiff.h SPK_VERSION). Rebuild the library: make -C "
                      f"{os.path.join(os.path.dirname(_HERE), 'csrc')}")
