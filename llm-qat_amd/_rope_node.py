"""Loader of the C++ autograd node of rope.rotary (csrc/fq_rope_node.cpp -> _fq_rope_node.so, built by build.py::build_node).

Host code only, as _act_node.py's: it replaces the Python `_Rotary` Function of rope.py so that neither the forward nor the backward runs
Python in front of its launch.  The kernels are the same C-ABI entry points of libllmqat_fakequant.so, handed over as function pointers;
results are the same bits either way.  Without the file -- or with LLMQAT_AMD_CPP_NODE=0 -- rope.py uses its Python node (`status()`).
"""
import ctypes
import importlib.util
import os

from . import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
NODE_PATH = os.path.join(HERE, "_fq_rope_node.so")

_mod = None
_why = None


def load():
    """-> the extension module, bound to the kernel library, or None (status() says why)"""
    global _mod, _why
    if _mod is not None or _why is not None:
        return _mod
    if os.environ.get("LLMQAT_AMD_CPP_NODE", "1") == "0":
        _why = "switched off (LLMQAT_AMD_CPP_NODE=0)"
        return None
    if not os.path.exists(NODE_PATH):
        _why = "not built (python llm-qat_amd/build.py)"
        return None
    try:
        import torch
        built_for = open(NODE_PATH + ".built_for").read().strip() if os.path.exists(NODE_PATH + ".built_for") else "?"
        if built_for != torch.__version__:      # a C++ extension is tied to the PyTorch it was compiled against: never load it under another one
            raise RuntimeError(f"built for PyTorch {built_for}, this is {torch.__version__}: run python llm-qat_amd/build.py")
        spec = importlib.util.spec_from_file_location("_fq_rope_node", NODE_PATH)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if mod.abi_version != _lib.ABI_VERSION:
            raise RuntimeError(f"built for C ABI {mod.abi_version}, the package speaks {_lib.ABI_VERSION}")
        lib = _lib.lib()
        addr = lambda name: ctypes.cast(lib[name], ctypes.c_void_p).value  # noqa: E731
        mod.bind(addr("fqr_rope_fwd"), addr("fqr_rope_bwd"), addr("fqr_rope_dense_strides"), addr("fq_last_error"))
    except Exception as e:  # noqa: BLE001 -- another torch build than the one it was compiled against, a stale file: the Python node serves
        _why = f"failed to load: {e!r}"
        return None
    _mod = mod
    return mod


def counters():
    """-> (fwd_launch, bwd_launch, copy_route) of the launches the node has made"""
    return _mod.counters() if _mod is not None else (0, 0, 0)


def status():
    return "loaded" if _mod is not None else (_why or "not loaded yet")
