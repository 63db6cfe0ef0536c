"""Handle lifecycle shared by the host mirrors of the native models (``Unet``, ``SD_VAE_Wrapper``, ``VQVAE``, ``MaskEncoder``).

Each model owns its parameters as torch tensors under the reference's names; the library keeps a packed copy inside a handle per device.
This base class reads the parameter table from a description-only handle (``device = -1``), registers the table as a module tree,
creates the handle on first use, and re-uploads the weights whenever the ``(data_ptr, _version)`` key of the table's parameters changes.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Tuple

import torch
from torch import nn

from . import _binding as B


def read_param_table(fc: str, create: str, *args) -> Tuple[List[Tuple[str, Tuple[int, ...], int]], int]:
    """``(table, flat_numel)`` of ``<fc>_<create>(*args, -1, &h)``: table rows are (name, shape, offset into the flat padded vector),
    ``flat_numel`` is ``<fc>_param_numel``.  Needs no GPU."""
    lib = B.lib()
    fn = lambda op: getattr(lib, f"{fc}_{op}")          # noqa: E731
    h = C.c_void_p()
    B.check(fn(create)(*args, -1, C.byref(h)))
    try:
        table = []
        for i in range(fn("param_count")(h)):
            name, shape, off = C.c_char_p(), (C.c_int64 * 4)(), C.c_int64()
            B.check(fn("param_info")(h, i, C.byref(name), C.byref(shape), C.byref(off)))
            table.append((name.value.decode(), tuple(int(s) for s in shape if s), int(off.value)))
        return table, int(fn("param_numel")(h))
    finally:
        fn("destroy")(h)


class _Node(nn.Module):
    """Parameter container; attribute names reproduce the reference's module tree."""


class NativeModule(nn.Module):
    """A model whose arithmetic runs in a library handle (``<_fc>_create`` ... ``<_fc>_destroy``).  Subclasses set ``_fc``, call
    ``_read_table`` and ``_register_table`` in their constructor, and may override ``_create_args``, ``_on_create`` and ``_on_use``."""

    _fc = ""                 # C prefix of the model's entry points, e.g. "fc_unet"
    _create = "create"       # the constructor's name after the prefix

    def __init__(self):
        super().__init__()
        self._handle, self._handle_device, self._synced = None, None, None

    def _fn(self, op: str):
        return getattr(B.lib(), f"{self._fc}_{op}")

    def _create_args(self) -> tuple:
        """Arguments of the constructor in front of the device."""
        return ()

    def _on_create(self, handle) -> None:
        """Runs once after a handle was created."""

    def _on_use(self, handle, device) -> None:
        """Runs on every ``_native`` call, before the weights are checked."""

    @property
    def _root(self) -> nn.Module:
        """The module the table's names are relative to."""
        return self

    # ---- parameters
    def _read_table(self) -> None:
        self._table, self._flat_numel = read_param_table(self._fc, self._create, *self._create_args())

    def _register_table(self, entries=None, requires_grad: bool = True) -> None:
        """Register ``entries`` ((name, shape) pairs, default: the table in its order) as uninitialised fp32 parameters under ``_root``."""
        for name, shape in entries if entries is not None else ((n, s) for n, s, _ in self._table):
            node = self._root
            *path, leaf = name.split(".")
            for part in path:
                if not hasattr(node, part):
                    node.add_module(part, _Node())
                node = getattr(node, part)
            node.register_parameter(leaf, nn.Parameter(torch.empty(shape, dtype=torch.float32), requires_grad=requires_grad))

    def _table_params(self) -> List[nn.Parameter]:
        sd = dict(self._root.named_parameters())
        return [sd[name] for name, _, _ in self._table]

    def _weights_version(self) -> tuple:
        return tuple((p.data_ptr(), p._version) for p in self._table_params())

    def mark_dirty(self) -> None:
        """Force a re-upload of the parameters on the next use.  Needed after writes the (data_ptr, _version) key cannot see:
        ``param.data.copy_(...)`` changes neither (the reference's EMA swaps weights that way, train_flow.py:56-71)."""
        self._synced = None

    # ---- native object
    def _native(self, device: torch.device):
        if self._handle is None or self._handle_device != device:
            self._release()
            h = C.c_void_p()
            B.check(self._fn(self._create)(*self._create_args(), device.index or 0, C.byref(h)))
            self._handle, self._handle_device, self._synced = h, device, None
            self._on_create(h)
        self._on_use(self._handle, device)
        params = self._table_params()
        ver = tuple((p.data_ptr(), p._version) for p in params)
        if ver != self._synced:
            flat = torch.zeros(self._flat_numel, dtype=torch.float32, device=device)
            for (_, shape, off), p in zip(self._table, params):
                flat[off:off + math.prod(shape)] = p.detach().reshape(-1).to(device)
            B.check(self._fn("load_params")(self._handle, flat.data_ptr(), flat.numel(), 1, B.current_stream(device)))
            torch.cuda.current_stream(device).synchronize()      # `flat` dies when this frame returns
            self._synced = ver
        return self._handle

    def _release(self):
        if getattr(self, "_handle", None) is not None:
            self._fn("destroy")(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass
