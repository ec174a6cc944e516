"""ctypes binding of libgradslam_hip.so (the C ABI declared in include/gradslam_hip.h).

PyTorch is used only as plumbing: it owns the HBM allocations (`tensor.data_ptr()`) and the HIP
stream (`torch.cuda.current_stream().cuda_stream`); every kernel on the hot path lives in the
shared library.  There is NO CPU fallback: if the library is missing, or a tensor is not on a HIP
device, the call raises.

SIGNATURES, the (restype, argtypes) every symbol is given when the library loads, is read from include/gradslam_hip.h at
import -- the header of this tree, the one the in-tree build compiles from -- so the two cannot disagree: see read_signatures.
"""
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgradslam_hip.so")
CSRC = os.path.join(_HERE, "csrc")

c_i, c_i64, c_f, c_p, c_sz = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t

_SCALARS = {"int": c_i, "int64_t": c_i64, "float": c_f, "size_t": c_sz, "gs_stream_t": c_p, "void": None}


def _ctype(words, decl):
    """ctypes type of one type spelling (a list of words, `*` its own word): any pointer is c_void_p, a scalar is one of the
    six spellings the header uses; anything else is an error that names the declaration -- never a guess."""
    words = [w for w in words if w != "const"]
    if "*" in words:
        return c_p
    if len(words) != 1 or words[0] not in _SCALARS:
        raise ValueError("gradslam_hip.h: unknown type '{}' in: {}".format(" ".join(words), decl))
    return _SCALARS[words[0]]


def read_signatures(header_text: str) -> dict:
    """name -> (restype, [argtypes]) of every `ret gs_name(args);` of the header, in header order.  A reader for this header
    (plain C by contract, one form of declaration), not a C parser."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", "", header_text, flags=re.S | re.M)
    split = lambda spelling: spelling.replace("*", " * ").split()
    sigs = {}
    for ret, name, params in re.findall(r"([\w \t*]+?)\s*\b(gs_\w+)\s*\(([^()]*)\)\s*;", text):
        decl = "{} {}({})".format(ret.strip(), name, " ".join(params.split()))
        res = ctypes.c_char_p if split(ret) == ["const", "char", "*"] else _ctype(split(ret), decl)
        args = [split(p) for p in params.split(",") if split(p) not in ([], ["void"])]
        sigs[name] = (res, [_ctype(a if "*" in a else a[:-1], decl) for a in args])  # (a scalar's last word is its name)
    return sigs


with open(os.path.join(os.path.dirname(_HERE), "include", "gradslam_hip.h")) as _f:
    SIGNATURES = read_signatures(_f.read())

_lib = None


def build(verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-s", "-C", CSRC, "-j4"]
    if verbose:
        cmd.remove("-s")
    subprocess.check_call(cmd)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """The loaded library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "gradslam_amd: native library {} is missing -- build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                "There is no CPU / PyTorch fallback for the hot path.".format(LIB_PATH)
            )
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the ABI lost a symbol
            fn.restype, fn.argtypes = res, args
        if handle.gs_abi_version() != 3:
            raise RuntimeError("gradslam_amd: ABI version mismatch")
        _lib = handle
    return _lib


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """Raw handle of torch's current HIP stream on the current device.  The raw accessors cost well under a
    microsecond; torch.cuda.current_stream() builds a Stream object (~10 us), which matters at ~80 us of host
    time per localisation step."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def current_device_index() -> int:
    """Index of the HIP device whose current stream `stream()` hands to the kernels."""
    return _raw_device() if _raw_device is not None else torch.cuda.current_device()


def require_hip(*tensors, op: str = "op"):
    """No CPU fallback: the hot path only runs on HIP tensors -- and only on the CURRENT device.  The C side
    takes raw pointers and a stream and never calls hipSetDevice: launching on the current device's stream with
    another device's pointers would fault, so a tensor elsewhere is an error here (one process per GPU, device
    selected with torch.cuda.set_device, is the deployment model; parallel.init_from_env does that)."""
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "gradslam_amd.{}: tensor is on {}; the ICP / PointFusion hot path only runs on a HIP "
                "device (no CPU fallback is provided).".format(op, t.device)
            )
        if cur is None:
            cur = current_device_index()
        if t.device.index != cur:
            raise RuntimeError(
                "gradslam_amd.{}: tensor is on {} but the current HIP device is cuda:{}; kernels are launched on "
                "the current device's stream -- call torch.cuda.set_device({}) (or wrap the call in "
                "`with torch.cuda.device(...)`) first.".format(op, t.device, cur, t.device.index)
            )


def call(name: str, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        msg = lib().gs_last_error().decode("utf-8", "replace")
        raise RuntimeError("{} failed (code {}): {}".format(name, rc, msg))


def ws_bytes(name: str, *args) -> int:
    return int(getattr(lib(), name)(*args))


_ws_cache = {}


def workspace(nbytes: int, device, tag: str = "default") -> torch.Tensor:
    """Grow-only scratch buffer per (device, stream, tag).  Kernels of one call finish with it before
    the next call on the same stream can start, so reuse is safe.  Sizes are rounded up to a power of two:
    a map that grows frame by frame then keeps its workspace ADDRESS for many frames, which is what lets
    gs_slam_localize replay its captured graph (the address is part of the graph's key)."""
    key = (str(device), stream(), tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(1 << max(int(nbytes) - 1, 255).bit_length(), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf
