"""ctypes binding of libgdlhip.so, read from the C-ABI's own declaration (include/gdlhip.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  There is NO
fallback: if the shared object is missing, every op raises -- the product path never routes
through PyTorch math or the CPU oracle.

Nothing of the ABI is restated here: ``SIGNATURES``, the four argument structs and the integer constants come out of the header
at import, by a parser that knows exactly the narrow C dialect the header is written in and raises on anything else.  Two views
of the library: ``load()`` returns every status to the caller, ``checked()`` raises on a non-zero one (what gdlhip.ops launches
through).
"""

from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

# GDL_LIB_PATH: an A/B build of the same sources (csrc/Makefile: BUILD= OUT= EXTRA=), for same-box comparisons only
LIB_PATH = Path(os.environ.get("GDL_LIB_PATH") or Path(__file__).resolve().parent / "libgdlhip.so")
INCLUDE = Path(__file__).resolve().parents[2] / "include"

c_i, c_l, c_f, c_p = C.c_int, C.c_int64, C.c_float, C.c_void_p

# ------------------------------------------------------------------ the header's dialect
_SCALARS = {"int": c_i, "int64_t": c_l, "float": c_f, "double": C.c_double}
_POINTEES = {"void", "char", "uint8_t", "int32_t", *_SCALARS}      # T* of these (and of the structs) is an address: c_void_p
# C struct -> (Python class, whether a `const S*` argument is POINTER(S): callers pass byref(S()); the others go through c_void_p)
_STRUCTS = {"gdl_conv_args": ("ConvArgs", True), "gdl_wgrad_args": ("WgradArgs", True),
            "gdl_dice_options": ("DiceOptions", False), "gdl_overlap_options": ("OverlapOptions", False)}
# host pointers the callers fill with typed ctypes objects (a c_int array, byref(c_int64())) rather than with an address
_TYPED = {("gdl_dice_options", "classes"): C.POINTER(c_i), ("gdl_overlap_options", "classes"): C.POINTER(c_i),
          ("gdl_conv_gemm_plan", "flops"): C.POINTER(c_l)}
_RENAMED = {"in": "inp"}                                 # C field names that are Python keywords
_PREPROCESSOR = re.compile(r'#\s*(ifndef \w+|define \w+|include <stdint\.h>|include "gdlhip\.h"|ifdef __cplusplus|endif)$|extern "C" \{$|\}$')
_DECLARATOR = re.compile(r"(?:const\s+)?(\w+)(\s*(?:\*\s*(?:const\s*)?)+|\s+)(\w+)\s*(\[\])?$")
_NEXT = re.compile(r"\S")
_STATEMENTS = [(kind, re.compile(rx)) for kind, rx in (
    ("define", r"#\s*define\s+(\w+)\s+(-?\d+(?:\.\d+)?)[ \t]*\n"),
    ("enum", r"enum\s*\{([^{}]*)\}\s*;"),
    ("stream", r"typedef\s+void\s*\*\s*gdl_stream_t\s*;"),
    ("struct", r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;"),
    ("function", r"((?:const\s+)?\w+\s*\*?)\s*\b(gdl_\w+)\s*\(([^(){};]*)\)\s*;"))]


class HeaderError(ValueError):
    """The header holds something the parser does not know; the message names the line."""


class Header:
    """What one header declares: ``functions`` {name: (restype, [argtypes])}, ``structs`` {C name: ctypes.Structure},
    ``constants`` {name: int or float} (enumerators and the #defines of one integer or decimal literal) and ``status`` (the functions whose int result is a
    gdl_status: exactly the int-returning ones that take a gdl_stream_t)."""

    def __init__(self, text: str) -> None:
        self.functions, self.structs, self.constants, self.status = {}, {}, {}, set()
        # comments go (their newlines stay: errors name the right line), then the guard / extern "C" lines
        text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)
        text = "\n".join("" if _PREPROCESSOR.match(line.strip()) else line for line in text.split("\n")) + "\n"
        pos = 0
        while (m := _NEXT.search(text, pos)):
            pos = m.start()
            line = text.count("\n", 0, pos) + 1
            for kind, rx in _STATEMENTS:
                if (m := rx.match(text, pos)):
                    break
            else:
                raise HeaderError(f"line {line}: not a declaration this parser reads: {text[pos:].splitlines()[0]!r}")
            getattr(self, "_" + kind)(line, *m.groups())
            pos = m.end()

    def _define(self, line: int, name: str, value: str) -> None:
        self.constants[name] = float(value) if "." in value else int(value)      # 0.25: a decimal literal is a float

    def _enum(self, line: int, body: str) -> None:
        for item in filter(None, (s.strip() for s in body.split(","))):
            m = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item)
            if not m:
                raise HeaderError(f"line {line}: enumerator without a literal value: {item!r}")
            self.constants[m.group(1)] = int(m.group(2))

    def _stream(self, line: int) -> None:
        pass      # gdl_stream_t is known to _ctype

    def _ctype(self, line: int, owner: str, decl: str):
        """'const float* mean' -> ('mean', c_void_p)."""
        m = _DECLARATOR.fullmatch(decl.strip())
        if not m:
            raise HeaderError(f"line {line}: {owner}: declarator not understood: {decl.strip()!r}")
        base, stars, name, array = m.groups()
        depth = stars.count("*") + bool(array)
        if (owner, name) in _TYPED:
            return name, _TYPED[owner, name]
        if depth == 0 and base in _SCALARS:
            return name, _SCALARS[base]
        if depth == 0 and base == "gdl_stream_t":
            return name, c_p
        if depth == 1 and base in self.structs and _STRUCTS[base][1]:
            return name, C.POINTER(self.structs[base])
        if depth >= 1 and (base in _POINTEES or base in self.structs):
            return name, c_p
        raise HeaderError(f"line {line}: {owner}: unknown type in {decl.strip()!r}")

    def _struct(self, line: int, body: str, cname: str) -> None:
        if cname not in _STRUCTS:
            raise HeaderError(f"line {line}: struct {cname} has no Python name in gdlhip._lib._STRUCTS")
        fields = []
        for decl in filter(None, (s.strip() for s in body.split(";"))):
            first, *more = decl.split(",")       # `int B, H, W, C`: the type stands with the first name
            name, ctype = self._ctype(line, cname, first)
            for n in (name, *(s.strip() for s in more)):
                if not re.fullmatch(r"[A-Za-z_]\w*", n):
                    raise HeaderError(f"line {line}: {cname}: declarator not understood: {decl!r}")
                fields.append((_RENAMED.get(n, n), ctype))
        self.structs[cname] = type(_STRUCTS[cname][0], (C.Structure,),
                                   {"_fields_": fields, "__doc__": f"{cname} of include/gdlhip.h, field for field."})

    def _function(self, line: int, res: str, name: str, params: str) -> None:
        res = " ".join(res.split())
        if res in ("const char*", "const char *"):
            restype = C.c_char_p
        elif res == "void":
            restype = None
        elif res in _SCALARS:
            restype = _SCALARS[res]
        else:
            raise HeaderError(f"line {line}: {name}: unknown return type {res!r}")
        args = [] if params.strip() == "void" else [self._ctype(line, name, p) for p in params.split(",")]
        if name in self.functions:
            raise HeaderError(f"line {line}: {name} is declared twice")
        self.functions[name] = (restype, [t for _, t in args])
        if restype is c_i and any(p.split()[0] == "gdl_stream_t" for p in params.split(",")):
            self.status.add(name)


# prefix of the module-level names -> the header of include/ that declares them: the C-ABI and its gdl_debug_* hooks first, then
# the whole-scene inference calls, stage by stage.  A new header is one line here.
HEADERS = {"": "gdlhip.h", "DEBUG": "gdlhip_debug.h", "SCENE": "gdlhip_scene.h", "SCENE_TTA": "gdlhip_scene_tta.h",
           "SCENE_NODATA": "gdlhip_scene_nodata.h", "SCENE_SIEVE": "gdlhip_scene_sieve.h", "SCENE_RINGS": "gdlhip_scene_rings.h",
           "SCENE_SIMPLIFY": "gdlhip_scene_simplify.h", "SCENE_REGIONS": "gdlhip_scene_regions.h",
           "SCENE_BURN": "gdlhip_scene_burn.h", "RASTER": "gdlhip_raster.h",
           "RASTER_TONE": "gdlhip_raster_tone.h"}
_PARSED = {prefix: Header((INCLUDE / name).read_text()) for prefix, name in HEADERS.items()}
_ABI = _PARSED[""]
for _prefix, _header in _PARSED.items():
    # SIGNATURES, DEBUG_SIGNATURES, SCENE_SIGNATURES, ...: name -> (restype, argtypes) of every symbol the header declares
    globals()[f"{_prefix}_SIGNATURES".lstrip("_")] = _header.functions
    # the header's enumerators and integer #defines without their GDL_ prefix: F32, BF16, ACT_*, FOCAL_* (the `form` argument of
    # the *_lowres_bwd calls), BCE_TARGET_* (the `target_type` of gdl_soft_bce_*), OVERLAP_* (gdl_overlap_options.kind),
    # SCENE_RINGS_SCAN_TILE, SCENE_BURN_BITS_MAX, RASTER_CUBIC, RASTER_MIN_VALID_WEIGHT (the one float), ...
    globals().update({k.removeprefix("GDL_"): v for k, v in _header.constants.items()})
STATUS_FUNCTIONS = frozenset(_ABI.status)      # they return a gdl_status; every other function returns a value
# what checked() gives the errcheck: the scene calls return a gdl_status too (the debug hooks are left to their callers)
_CHECKED = STATUS_FUNCTIONS.union(*(h.status for prefix, h in _PARSED.items() if prefix != "DEBUG"))
ConvArgs, WgradArgs, DiceOptions, OverlapOptions = (_ABI.structs[c] for c in _STRUCTS)

# environment variable -> the hook load() calls with its integer value (meanings: include/gdlhip_debug.h)
ENV_HOOKS = {
    "GDL_CONV_SF": "gdl_debug_set_conv_sf",
    "GDL_CONV_EPILOGUE": "gdl_debug_set_conv_epilogue",
    "GDL_CONV_NGROUP_KB": "gdl_debug_set_conv_ngroup_kb",
    "GDL_CONV_DUAL": "gdl_debug_set_conv_dual",
    "GDL_CONV_STAGE4": "gdl_debug_set_conv_stage4",
    "GDL_CONV_W4": "gdl_debug_set_conv_w4",
    "GDL_CONV_PERSIST": "gdl_debug_set_conv_persist",
    "GDL_CONV_W4P": "gdl_debug_set_conv_w4p",
    "GDL_FLASH_FWD": "gdl_debug_set_flash_fwd",      # second argument: GDL_FLASH_DEFER, default 6
    "GDL_TAPSUM_PERSIST": "gdl_debug_set_tapsum_persist",
    "GDL_TAPSUM_ROLL": "gdl_debug_set_tapsum_roll",
    "GDL_GATHER_MFMA": "gdl_debug_set_gather_mfma",
    "GDL_WGRAD_XCD_GROUP": "gdl_debug_set_wgrad_xcd_group",
    "GDL_WGRAD_OLD_SPLITS": "gdl_debug_set_wgrad_old_splits",
    "GDL_WGRAD_ROWS_XCD": "gdl_debug_set_wgrad_rows_xcd",
    "GDL_HEAD_MFMA": "gdl_debug_set_head_mfma",
    "GDL_WGRAD_MODE": "gdl_debug_force_wgrad_small",
}

_lib = None      # (raw view, checked view) once the library is loaded


class GdlHipError(RuntimeError):
    pass


def _open(errcheck=None) -> C.CDLL:
    """A CDLL object of its own over the (once-loaded) library, every declared symbol typed; `errcheck` on the status functions."""
    if not LIB_PATH.exists():
        msg = (f"{LIB_PATH} not found: the HIP extension is not built. Run "
               "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
               "There is no PyTorch/CPU fallback for the gdlhip ops.")
        raise GdlHipError(msg)
    lib = C.CDLL(str(LIB_PATH))
    for header in _PARSED.values():
        for name, (res, args) in header.functions.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
            if errcheck is not None and name in _CHECKED:
                fn.errcheck = errcheck
    return lib


def _views() -> tuple:
    global _lib
    if _lib is None:
        raw = _open()
        for var, hook in ENV_HOOKS.items():
            if os.environ.get(var) is not None:
                extra = [float(os.environ.get("GDL_FLASH_DEFER", "6"))] if var == "GDL_FLASH_FWD" else []
                getattr(raw, hook)(int(os.environ[var]), *extra)
        _lib = (raw, _open(status_errcheck))
    return _lib


def load() -> C.CDLL:
    """The raw view: libgdlhip.so with every declared symbol bound, statuses returned to the caller; raises if the build is
    missing.  The first call applies the tuning hooks the environment asks for (ENV_HOOKS)."""
    return (_lib or _views())[0]


def checked() -> C.CDLL:
    """The checked view: the same library, but a status function raises what check() raises instead of returning a non-zero
    status (ValueError for GDL_ERR_INVALID, GdlHipError otherwise; the message starts with the symbol).  Queries (`*_workspace`,
    `*_ok`, gdl_conv_gemm_plan, ...) return their value as in load()."""
    return (_lib or _views())[1]


def check(status: int, what: str) -> None:
    if status != 0:
        err = load().gdl_last_error().decode(errors="replace")
        if status == -1:
            raise ValueError(f"{what}: {err}")
        raise GdlHipError(f"{what}: status {status}: {err}")


def status_errcheck(status: int, fn, args) -> int:
    """ctypes errcheck of the status functions in checked()."""
    if status != 0:
        check(status, fn.__name__)
    return status
