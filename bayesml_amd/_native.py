"""What the ctypes bindings of the four small C ABIs of ``libgmmvb.so`` share (``_regression``, ``_expfam``, ``_ctree``,
``_mtree``): declaring a family's prototypes on the library, turning a status code into an ``EngineError`` with the
family's own last message, resolving the device, and the current stream as a C argument.

The ``gmmvb_*`` core keeps its own ``load_library`` / ``_check`` in ``_engine``.
"""
from __future__ import annotations

import ctypes

import torch

from ._engine import EngineError, EngineUnavailableError, _STATUS, load_library as _load_gmmvb

PLOT_MSG = "plotting is out of scope for bayesml_amd (SURVEY.md section 2)"


def bind(prefix: str, symbols: dict):
    """``(load_library, check)`` of the family whose entry points start with ``prefix``; ``symbols`` is its table
    name -> (restype, argtypes), every symbol its header declares."""
    declared = False

    def load_library() -> ctypes.CDLL:
        """The in-tree library with the family's prototypes declared, once (works without a GPU)."""
        nonlocal declared
        lib = _load_gmmvb()
        if not declared:
            for name, (res, args) in symbols.items():
                fn = getattr(lib, name)          # AttributeError here = header/library mismatch
                fn.restype = res
                fn.argtypes = args
            declared = True
        return lib

    def check(rc, what):
        if rc != 0:
            msg = getattr(load_library(), prefix + "_last_error")()
            raise EngineError(f"{what}: {_STATUS.get(rc, rc)}: {msg.decode() if msg else ''}")

    return load_library, check


def gpu_device(device, what: str) -> torch.device:
    """``device`` (None = the current GPU) as a ``torch.device``; there is no CPU fallback behind any of the engines."""
    if not torch.cuda.is_available():
        verb = "need" if what.endswith("s") else "needs"          # "... data passes need", "... engine needs"
        raise EngineUnavailableError(f"bayesml_amd's {what} {verb} an MI355X: there is no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise EngineUnavailableError(f"device {device} is not a GPU: there is no CPU fallback")
    return device


def stream_ptr(device) -> ctypes.c_void_p:
    """The current stream of ``device`` as the ``void* stream`` of an entry point."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
