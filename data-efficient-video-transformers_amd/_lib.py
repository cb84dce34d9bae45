"""ctypes binding of libdvt_hip.so, derived at import from include/dvt_hip.h.

The header is the one declaration of the C ABI.  It is written in a narrow subset of C -- ``typedef struct NAME { ... }
NAME;``, ``enum NAME { A = n, ... };``, prototypes ``RET dvt_xxx(args);``, two ``typedef void*`` handles and integer
``#define``s -- which ``_parse_header`` reads with three regular expressions into one ``ctypes.Structure`` per
descriptor (``STRUCTS``), ``SIGNATURES`` and the enum / macro values (``ENUMS``, ``MACROS``).  One type rule serves
fields, arguments and return types (``_ctype``); a declaration it does not cover raises at import, it never guesses.

The product path has no fallback: if the header or the shared library is missing or a call fails, a RuntimeError
(carrying ``dvt_last_error()`` for a failed call) is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# (DVT_LIB_PATH: development A/B of another build of the same ABI -- tools/dev/ab_libs.sh; the product loads the in-tree library)
LIB_PATH = os.environ.get("DVT_LIB_PATH") or os.path.join(_HERE, "libdvt_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dvt_hip.h")

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8,
            "unsigned char": C.c_ubyte, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
# the three forms of declaration besides prototypes
_STRUCT = r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;"
_ENUM = r"\benum\s+(\w+)\s*\{(.*?)\}\s*;"
_HANDLE = r"typedef\s+void\s*\*\s*(\w+)\s*;"


def _parse_header(path: str):
    """-> (structs, signatures, enums, macros) of the header, each keyed by its C name, in header order."""
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise RuntimeError(f"{path} is missing: the ctypes binding is derived from it at import; there is no "
                           "fallback table.") from e
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    macros = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"#ifdef __cplusplus.*?#endif", "", text, flags=re.S)        # the extern "C" braces
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    handles = set(re.findall(_HANDLE, text))
    structs, signatures, enums = {}, {}, {}

    def _ctype(ctype: str, where: str, ret: bool = False):
        """The type rule.  scalar -> the matching ctypes scalar; handle, void*, char* and pointer to a scalar -> c_void_p
        (callers pass data_ptr() integers, byref() and cast() results); pointer to a descriptor -> POINTER(its
        Structure); pointer to a handle -> POINTER(c_void_p); a returned const char* -> c_char_p."""
        words = [w for w in ctype.replace("*", " * ").split() if w != "const"]
        stars, base = words.count("*"), " ".join(w for w in words if w != "*")
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base]
        if stars == 0 and base in handles:
            return C.c_void_p
        if stars == 1 and base in structs:
            return C.POINTER(structs[base])
        if stars == 1 and base in handles:
            return C.POINTER(C.c_void_p)
        if stars == 1 and base == "char" and ret:
            return C.c_char_p
        if stars == 1 and (base in _SCALARS or base in ("void", "char")) and not ret:
            return C.c_void_p
        raise RuntimeError(f"{path}: no ctypes rule for the type `{ctype.strip()}` in `{' '.join(where.split())}`")

    for enum, body in re.findall(_ENUM, text, flags=re.S):
        items = [re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", item) for item in body.split(",")]
        if not all(items):
            raise RuntimeError(f"{path}: enum {enum} has an enumerator that is not `NAME = integer`")
        enums[enum] = {m.group(1): int(m.group(2)) for m in items}
    for name, body in re.findall(_STRUCT, text, flags=re.S):
        fields = []
        for decl in filter(None, (s.strip() for s in body.split(";"))):
            m = re.fullmatch(r"(.+?)\s*\b(\w+(?:\s*,\s*\w+)*)", decl, flags=re.S)     # `int32_t a, b` or `const float* p`
            if not m or ("*" in m.group(1) and "," in m.group(2)):
                raise RuntimeError(f"{path}: unparsed field `{decl}` of struct {name}")
            fields += [(f.strip(), _ctype(m.group(1), decl)) for f in m.group(2).split(",")]
        structs[name] = type(name, (C.Structure,), {"_fields_": fields})
    rest = text
    for form in (_STRUCT, _ENUM, _HANDLE):
        rest = re.sub(form, "", rest, flags=re.S)
    for decl in filter(None, (s.strip() for s in rest.split(";"))):
        m = re.fullmatch(r"(.+?)\b(dvt_\w+)\s*\((.*)\)", decl, flags=re.S)
        if not m:
            raise RuntimeError(f"{path}: unparsed declaration `{' '.join(decl.split())}`")
        args = [] if m.group(3).strip() == "void" else [re.fullmatch(r"\s*(.+[\s*])\w+\s*", a, flags=re.S)
                                                        for a in m.group(3).split(",")]
        if not all(args):
            raise RuntimeError(f"{path}: unparsed parameter in `{' '.join(decl.split())}`")
        signatures[m.group(2)] = (_ctype(m.group(1), decl, ret=True), [_ctype(a.group(1), decl) for a in args])
    if not (structs and signatures and enums and "DVT_ABI_VERSION" in macros):
        raise RuntimeError(f"{path}: no descriptors, entry points, enums or DVT_ABI_VERSION found; there is no fallback table.")
    return structs, signatures, enums, macros


# STRUCTS: C struct name -> ctypes.Structure; SIGNATURES: entry point -> (restype, argtypes); ENUMS: enum -> {enumerator: value}
STRUCTS, SIGNATURES, ENUMS, MACROS = _parse_header(HEADER_PATH)

GemmDesc = STRUCTS["dvt_gemm_desc"]
GemmPlanInfo = STRUCTS["dvt_gemm_plan_info"]
SplitKPending = STRUCTS["dvt_splitk_pending"]
AttnDesc = STRUCTS["dvt_attn_desc"]
AttnPlanInfo = STRUCTS["dvt_attn_plan_info"]
AttnLongPlanInfo = STRUCTS["dvt_attn_long_plan_info"]
AttnClsDesc = STRUCTS["dvt_attn_cls_desc"]
LnBwdDesc = STRUCTS["dvt_ln_bwd_desc"]
LnPending = STRUCTS["dvt_ln_pending"]
ConvDesc = STRUCTS["dvt_conv_desc"]
ConvPlanInfo = STRUCTS["dvt_conv_plan_info"]
Conv3dDesc = STRUCTS["dvt_conv3d_desc"]
BnAffine = STRUCTS["dvt_bn_affine"]
PackEntry = STRUCTS["dvt_pack_entry"]
HeadBceDesc = STRUCTS["dvt_head_bce_desc"]
EmitEntry = STRUCTS["dvt_emit_entry"]
RolloutDesc = STRUCTS["dvt_rollout_desc"]
RolloutPlanInfo = STRUCTS["dvt_rollout_plan_info"]

ABI_VERSION = MACROS["DVT_ABI_VERSION"]            # bumped with every descriptor layout change; load() refuses another
F32, BF16, F16 = (ENUMS["dvt_dtype"][n] for n in ("DVT_F32", "DVT_BF16", "DVT_F16"))
EPI_NONE, EPI_GELU, EPI_RELU, EPI_RESIDUAL, EPI_DGELU, EPI_DRELU = (
    ENUMS["dvt_epilogue"]["DVT_EPI_" + n] for n in ("NONE", "GELU", "RELU", "RESIDUAL", "DGELU", "DRELU"))

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared library (once).  Raises RuntimeError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
            "`python data-efficient-video-transformers_amd/build.py` (needs hipcc); there is no "
            "fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    if lib.dvt_version() != ABI_VERSION:
        raise RuntimeError(f"libdvt_hip.so ABI version {lib.dvt_version()} != {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().dvt_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libdvt_hip {what} failed (status {rc}): {msg}")
