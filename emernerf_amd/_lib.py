"""ctypes binding of libemernerf_hip.so -- the C-ABI boundary declared in include/emernerf_hip.h.

There is NO fallback: if the shared library is missing or a symbol does not resolve, importing the
product path raises.  A CPU/PyTorch fallback would void every parity claim.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_int, c_int64, c_void_p
from typing import Optional

# torch before the library: it ships its own HIP runtime (libamdhip64) and the process must end up with exactly one -- if this
# library were loaded before torch, it would bind the system copy and see no device once torch initialises its own
import torch
from torch import Tensor

from ._abi import CONST, FUNC, STRUCT, EmerError  # noqa: F401

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libemernerf_hip.so")
EMER_MAX_LEVELS = CONST["EMER_MAX_LEVELS"]

F32, F16 = CONST["EMER_F32"], CONST["EMER_F16"]
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TRUNC_EXP = (CONST["EMER_ACT_" + a] for a in ("NONE", "RELU", "SIGMOID", "TRUNC_EXP"))
STOT_TYPES = {k[len("EMER_STOT_"):].lower(): v for k, v in CONST.items() if k.startswith("EMER_STOT_")}  # TRANSFROM_DICT, nerfacc_prop_net.py:298-314

GridDesc = STRUCT["emer_grid_desc"]
_P = c_void_p

# name -> argtypes of the entry points that return an error code / of the workspace-size queries (int64), as include/emernerf_hip.h
# declares them
SIGNATURES = {name: args for name, (res, args) in FUNC.items() if res is c_int}
INT64_FUNCTIONS = {name: args for name, (res, args) in FUNC.items() if res is c_int64}

ALLOW_MISSING_SYMBOLS = False  # never set by the product path

_lib = None


def load() -> ctypes.CDLL:
    """Load the HIP library; raise (never fall back) when it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EmerError(
            f"{LIB_PATH} not found. Build it with `python -m emernerf_amd._build` (hipcc, gfx950). "
            "emernerf_amd has no CPU/PyTorch fallback by design.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in FUNC.items():
        try:
            fn = getattr(lib, name)  # AttributeError if the symbol is missing
        except AttributeError:
            if ALLOW_MISSING_SYMBOLS:  # tools/_libsel.py only: an older build of the library in a same-session A/B
                continue
            raise
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


class KernelTimer:
    """Opt-in per-entry-point timing with HIP events recorded on the stream the kernels are launched on
    (torch's current stream).  Used by bench.py to measure kernel durations live inside the timed region."""

    def __init__(self, names):
        self.names = set(names)
        self.events = {n: [] for n in self.names}
        self.tags = {n: [] for n in self.names}
        self.ns = {n: [] for n in self.names}   # grid entry points: samples of the launch (the roofline's algorithmic bytes are per sample)
        self.tag = None

    def elapsed_us(self):
        torch.cuda.synchronize()
        return {n: [a.elapsed_time(b) * 1e3 for a, b in ev] for n, ev in self.events.items()}


TIMER = None  # set to a KernelTimer to enable


# position of the sample count among the arguments of the grid entry points (include/emernerf_hip.h)
_N_ARG = {"emer_hashgrid_fwd": 8, "emer_hashgrid_fwd_jac": 9, "emer_hashgrid_bwd_params_sliced": 7, "emer_hashgrid_bwd_params_sliced_add": 7,
          "emer_hashgrid_bwd_params_sliced_levels": 7, "emer_hashgrid_bwd_params": 7, "emer_hashgrid_bwd_input": 8, "emer_hashgrid_bwd_input_jac": 6}
_TIGHT = ("emer_hashgrid_fwd", "emer_hashgrid_fwd_jac", "emer_hashgrid_bwd_params_sliced", "emer_hashgrid_bwd_params_sliced_add", "emer_hashgrid_bwd_params_sliced_levels")  # entries that record events around their kernel themselves


def call(name: str, *args) -> None:
    lib = load()
    t = TIMER
    if t is not None and name in t.names:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if name in _TIGHT:
            # the library re-records both events immediately around the kernel (hipExtLaunchKernelGGL): the measured
            # interval excludes the host's enqueue latency between two launches
            b.record()
            lib.emer_profile_next(c_void_p(a.cuda_event), c_void_p(b.cuda_event))
            rc = getattr(lib, name)(*args)
        else:
            rc = getattr(lib, name)(*args)
            b.record()
        t.events[name].append((a, b))
        tag = None
        if name.startswith("emer_hashgrid"):  # distinguish the main grid from the proposal grids
            d = args[0]._obj
            tag = (d.n_dims, d.n_levels, d.n_features)
        t.tags[name].append(tag)
        t.ns[name].append(int(args[_N_ARG[name]]) if name in _N_ARG else None)
    else:
        rc = getattr(lib, name)(*args)
    if rc != 0:
        raise EmerError(f"{name} failed (rc={rc}): {lib.emer_last_error().decode()}")


def make_grid_desc(n_dims, n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale) -> GridDesc:
    d = GridDesc()
    call("emer_grid_desc_init", ctypes.byref(d), n_dims, n_levels, n_features, log2_hashmap_size,
         base_resolution, per_level_scale)
    return d


# ------------------------------------------------------------------------------------------------ argument helpers of the op modules
def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _stream(t: Tensor):
    return c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ng(*args):
    """Arguments for a Function.apply call outside autograd recording (torch.no_grad, set_grad_enabled(False): evaluation,
    the proposal sampling of the steps that do not train the proposal nets).  A Function's forward still sees
    needs_input_grad == requires_grad of its inputs there (and torch.is_grad_enabled() is False inside EVERY forward), so
    the inputs are detached here: the forwards then skip what only a backward needs -- hidden activations (256 B per sample),
    the grid backward's bitmaps -- instead of writing it for nobody."""
    if torch.is_grad_enabled():
        return args
    return tuple(a.detach() if isinstance(a, Tensor) else a for a in args)


def _f32c(t: Tensor) -> Tensor:
    return t.detach().to(torch.float32).contiguous()
