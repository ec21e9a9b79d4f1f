"""ctypes binding of libitcv_hip.so (the C ABI declared in include/itcv_hip.h).

This is the only place the Python host touches native code.  There is NO fallback: if the
shared library is missing or a symbol does not resolve, importing this module raises, and
every op in the package raises with it -- a CPU/eager substitute would silently void the
parity and performance claims.

The ctypes prototypes and the integer constants are not written here: both are parsed out of the header at import
(``parse_header``), the file every .hip translation unit is compiled against.  A type outside the small closed map
raises; nothing is guessed.

PyTorch is used only as plumbing here: device memory (``tensor.data_ptr()``) and the current
HIP stream (``torch.cuda.current_stream().cuda_stream``).
"""
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
# ITCV_LIB: load another build of the same library (the -DITCV_DIAG diagnostic build of `make diag`, tools/abl.sh)
LIB_PATH = os.environ.get("ITCV_LIB") or os.path.join(PKG_ROOT, "lib", "libitcv_hip.so")
CSRC = os.path.join(PKG_ROOT, "csrc")
HEADER = os.path.join(os.path.dirname(PKG_ROOT), "include", "itcv_hip.h")

p, i32, i64, sz, f32, f64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t,
                             ctypes.c_float, ctypes.c_double)
_BY_VALUE = {"int": i32, "int64_t": i64, "long long": i64, "size_t": sz, "float": f32, "double": f64}


class HipExtensionError(RuntimeError):
    pass


def _ctype(decl, fn, named):
    """ctypes type of one return type or (``named``: the name may follow) parameter of ``fn``.  The map is closed: any
    pointer, ``const char*`` and the six by-value types of _BY_VALUE; anything else raises."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return ctypes.c_char_p if words[:2] == ["char", "*"] and words.count("*") == 1 else p
    for n in (len(words), len(words) - 1) if named else (len(words),):
        if " ".join(words[:n]) in _BY_VALUE:
            return _BY_VALUE[" ".join(words[:n])]
    raise HipExtensionError(f"{fn}: no ctypes mapping for '{' '.join(decl.split())}' (add the type to hipvae/abi.py)")


def parse_header(text):
    """(SIGNATURES, DEFINES) of the text of a C header: name -> (restype, [argtypes]) of every ``itcv_*`` prototype, and
    name -> value of every ``#define ITCV_*`` whose body is an integer literal or a parenthesised ``|`` of earlier such
    names (any other body, a cast or a shift, is skipped)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {}
    for name, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ITCV_\w+)[ \t]+(.+?)[ \t]*$", text, flags=re.M):
        if re.fullmatch(r"0[xX][0-9a-fA-F]+|\d+", body):
            defines[name] = int(body, 16 if body[:2] in ("0x", "0X") else 10)
        elif re.fullmatch(r"\(\s*ITCV_\w+(\s*\|\s*ITCV_\w+)*\s*\)", body):
            terms = re.findall(r"ITCV_\w+", body)
            if all(t in defines for t in terms):
                defines[name] = 0
                for t in terms:
                    defines[name] |= defines[t]
    signatures = {}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    for res, fn, params in re.findall(r"([A-Za-z_][\w\s*]*?)\b(itcv_\w+)\s*\(([^;{}]*)\)\s*;", text):
        if "(" in params:
            raise HipExtensionError(f"{fn}: no ctypes mapping for a function-pointer parameter '{' '.join(params.split())}'")
        params = [] if params.strip() in ("", "void") else params.split(",")
        signatures[fn] = (_ctype(res, fn, False), [_ctype(prm, fn, True) for prm in params])
    return signatures, defines


def _read_header():
    try:
        with open(HEADER) as f:
            return parse_header(f.read())
    except OSError as e:
        raise HipExtensionError(f"{HEADER} is missing or unreadable: the ctypes table is derived from it") from e


def _defs(prefix):
    """{NAME: value} of the header's ``#define <prefix>NAME`` integers, in header order."""
    return {k[len(prefix):]: v for k, v in DEFINES.items() if k.startswith(prefix)}


# name -> (restype, [argtypes]) of every prototype of include/itcv_hip.h, which every .hip file is compiled against
SIGNATURES, DEFINES = _read_header()

ABI_VERSION = DEFINES["ITCV_ABI_VERSION"]
TC_VAR_FROM_ROW, TC_EPS_DENSITY, TC_WEIGHTED, TC_LIVE = (_defs("ITCV_TC_")[n] for n in (
    "VAR_FROM_ROW", "EPS_DENSITY", "WEIGHTED", "LIVE"))
_bn = _defs("ITCV_BN_PATH_")
BN_PATHS = tuple(n.title().replace("_", "") for n in sorted(_bn, key=_bn.get))      # ONE_BLOCK -> "OneBlock", by value
LOSS_TYPES = {n.lower(): v for n, v in _defs("ITCV_LOSS_").items()}
OPT_MAXIMIZE, OPT_NESTEROV, OPT_AMSGRAD, OPT_DECOUPLED_WD, OPT_CENTERED = (_defs("ITCV_OPT_")[n] for n in (
    "MAXIMIZE", "NESTEROV", "AMSGRAD", "DECOUPLED_WD", "CENTERED"))
# option 'stream_nt': family name -> bit ("BN_APPLY", "WGRAD_SLABS", "FOLD", "WGRAD_OPS", "OPTIM", "BN_FWD"), plus the two
# masks "ALL" and "DEFAULT" (the value the library starts with)
STREAM_NT = _defs("ITCV_STREAM_NT_")


def build(verbose=False):
    """Compile libitcv_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", CSRC, "-j4"], capture_output=True, text=True)
    if verbose or out.returncode:
        print(out.stdout[-4000:], out.stderr[-4000:])
    if out.returncode:
        raise HipExtensionError("building libitcv_hip.so failed (see output above)")
    return LIB_PATH


def _load():
    if not os.path.exists(LIB_PATH):
        raise HipExtensionError(
            f"{LIB_PATH} is missing: build it with `make -C {CSRC}` (or __graft_entry__.build()). "
            "There is no CPU fallback for the HIP hot path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipExtensionError(f"{LIB_PATH} does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    if lib.itcv_abi_version() != ABI_VERSION:
        raise HipExtensionError(f"ABI version mismatch: library {lib.itcv_abi_version()} != header {ABI_VERSION}")
    return lib


class _Lib:
    """The loaded library with its pure query entry points (``*_supported``, ``*_workspace``, ``*_bytes``, ``*_elems``,
    ``*_variant``: integers in, integer out, no device work) memoised: an eager step asks several thousand such
    questions, and a dict hit is ~10x cheaper than a ctypes call."""

    _PURE = ("_supported", "_workspace", "_bytes", "_elems", "_variant", "_stat_tiles", "_slabs", "_max_descs")

    def __init__(self, cdll):
        object.__setattr__(self, "_cdll", cdll)

    def __getattr__(self, name):
        fn = getattr(self._cdll, name)
        if name.endswith(self._PURE):
            memo = {}

            def cached(*args, _fn=fn, _memo=memo):
                r = _memo.get(args)
                if r is None:
                    r = _memo[args] = _fn(*args)
                return r

            fn = cached
        object.__setattr__(self, name, fn)
        return fn

    def forget(self, name):
        """Drops the memo of one query (the few whose answer depends on a library option, after itcv_set_option)."""
        self.__dict__.pop(name, None)


lib = _Lib(_load())


def last_error():
    return lib.itcv_last_error().decode()


def check(rc, exc=RuntimeError):
    if rc:
        raise exc(last_error())


def stream():
    """Raw handle of torch's current HIP stream (torch.cuda.current_stream() builds a Stream object: ~9 us a call)."""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def need_device(*tensors):
    """Every tensor given (None entries are skipped) lives on the device, or HipExtensionError."""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipExtensionError("HIP kernels need device tensors (got a CPU tensor); there is no CPU path")


def ptr(t):
    """Device pointer of a dense fp32/fp64/int64 CUDA(HIP) tensor, or NULL for None."""
    if t is None:
        return None
    if not t.is_cuda:                    # tested here, not in a call: an eager step takes several thousand pointers
        need_device(t)
    if not t.is_contiguous():
        raise HipExtensionError("HIP kernels need contiguous tensors")
    return t.data_ptr()


def call(name, *args):
    check(getattr(lib, name)(*args), HipExtensionError)


def bn_plan_query(bwd, B, C, H, W, pool=0, up2=0, groups=1, planes=True, ns=2, ws_bytes=None, tile_stats=False):
    """(path name, slices per channel) of the launch plan itcv_bn_train_fwd (``bwd`` false) / itcv_bn_train_bwd would
    build for one BatchNorm group of (B, C, H, W).  Host arithmetic only; ``ws_bytes`` None: the workspace BnActFn
    hands in (itcv_bn_workspace * groups)."""
    if ws_bytes is None:
        ws_bytes = lib.itcv_bn_workspace(B, C, H * W) * max(int(groups), 1)
    path, splits = ctypes.c_int(-1), ctypes.c_int(-1)
    call("itcv_bn_plan_query", int(bool(bwd)), B, C, H, W, int(pool), int(up2), int(groups), int(bool(planes)), int(ns),
         ws_bytes, int(bool(tile_stats)), ctypes.byref(path), ctypes.byref(splits))
    return BN_PATHS[path.value], splits.value
