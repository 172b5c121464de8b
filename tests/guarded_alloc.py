"""Guard bands around the buffers a call is given (test helper, not a test).

A guarded buffer is ONE allocation of ``front guard | nbytes | rear guard``: the guards are at least ``GUARD_BYTES`` (256 KiB) each, the
handed-out view starts at a multiple of 256 B and the rear guard starts at the exact byte after it, with no rounding.  The guards (and
the interior of buffers asked for with ``empty`` / ``empty_like``) hold one byte value per ``Guards`` object, 0xFF (NaN / -1) or 0x00.
``check()`` synchronises the device and compares every guard with that byte, bit for bit: a kernel that writes a row past ``M`` or a
size function that is a few ints short leaves a dirty guard, whatever the caching allocator would have put there.

Two ways in:

* ``g.guarded(shape, dtype, device, name)`` / ``g.guarded_copy(tensor, name)`` for buffers the test passes itself (ctypes calls,
  device-resident inputs of a wrapper);
* ``with g.patched():`` puts a thin proxy in place of the module-level name ``torch`` in the ``sylber_amd`` modules (``MODULES``):
  ``torch.empty / zeros / ones / full`` and their ``_like`` forms go through ``guarded`` when the target is a GPU (or, with
  ``guard_cpu=True``, the host: the CPU tier's way to prove that the check would fire), everything else -- host and pinned
  allocations included -- is torch's own.  Every buffer is recorded with its call site (``file:line function``).

``covers(tensor)`` and ``handed_out(nbytes)`` answer from the ledger of everything handed out since the object was made (``check()``
releases the buffers and keeps the ledger), so a test can show it was not vacuous: what a wrapper returned lies in a guarded buffer,
and a buffer of exactly the bytes a size function returns was handed out."""
from __future__ import annotations

import contextlib
import importlib
import numbers
import os
import sys
from typing import List, Optional

import torch as _torch

GUARD_BYTES = 256 * 1024
ALIGN = 256
FILLS = (0xFF, 0x00)
MODULES = ("_index", "search", "pq", "units", "kmeans", "downstream", "quantizer", "segmenter", "synthesis", "ingest")
_HERE = os.path.abspath(__file__)


def _call_site() -> str:
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?"
    return "%s:%d %s" % (os.path.basename(f.f_code.co_filename), f.f_lineno, f.f_code.co_name)


class _Buffer:
    __slots__ = ("name", "nbytes", "raw", "off", "ptr")

    def __init__(self, name, nbytes, raw, off):
        self.name, self.nbytes, self.raw, self.off = name, nbytes, raw, off
        self.ptr = raw.data_ptr() + off


class Guards:
    """the guarded buffers of one run, all with the fill byte ``fill``"""

    def __init__(self, fill: int, guard_bytes: int = GUARD_BYTES, guard_cpu: bool = False):
        assert 0 <= int(fill) <= 255 and guard_bytes >= GUARD_BYTES
        self.fill = int(fill)
        self.guard_bytes = int(guard_bytes)
        self.guard_cpu = bool(guard_cpu)
        self.live: List[_Buffer] = []
        self.ledger: List[tuple] = []          # (name, ptr, nbytes) of everything handed out
        self.checked = 0                       # buffers compared so far

    # ---- allocation ----------------------------------------------------------------------------------------------------------------
    def wants(self, device, pin_memory: bool = False) -> bool:
        """does an allocation on ``device`` (``None``: torch's default, the host) go through the guards"""
        if pin_memory:
            return False
        dev = _torch.device(device) if device is not None else _torch.device("cpu")
        return dev.type != "cpu" or self.guard_cpu

    def guarded(self, shape, dtype=_torch.float32, device="cuda", name: Optional[str] = None, init=None) -> _torch.Tensor:
        """a contiguous tensor of this shape and dtype between two guards; ``init`` None: the interior holds the fill byte, a number:
        that value"""
        if isinstance(shape, int):
            shape = (shape,)
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        item = _torch.empty(0, dtype=dtype).element_size()
        nbytes = numel * item
        G = self.guard_bytes
        raw = _torch.empty(G + ALIGN + nbytes + G, dtype=_torch.uint8, device=device)
        raw.fill_(self.fill)
        off = G + (-(raw.data_ptr() + G)) % ALIGN
        b = _Buffer(name or _call_site(), nbytes, raw, off)
        view = raw[off:off + nbytes].view(dtype).view(shape)
        if init is not None:
            view.fill_(init)
        self.live.append(b)
        self.ledger.append((b.name, b.ptr, nbytes))
        return view

    def guarded_copy(self, tensor: _torch.Tensor, name: Optional[str] = None) -> _torch.Tensor:
        """``tensor``'s values (made contiguous) in a guarded buffer on its device"""
        out = self.guarded(tuple(tensor.shape), tensor.dtype, tensor.device, name or _call_site())
        out.copy_(tensor)
        return out

    # ---- the check -----------------------------------------------------------------------------------------------------------------
    def dirty(self) -> List[str]:
        """one line per dirty guard of the live buffers (after a device synchronise)"""
        if any(b.raw.is_cuda for b in self.live):
            _torch.cuda.synchronize()
        out = []
        for b in self.live:
            end = b.off + b.nbytes
            for side, lo, hi in (("front", 0, b.off), ("rear", end, end + self.guard_bytes)):
                bad = (b.raw[lo:hi] != self.fill).nonzero()
                if bad.numel():
                    first, last = int(bad[0]), int(bad[-1])
                    # offsets relative to the buffer: front bytes are negative (-1 = the byte just before it), rear bytes count from
                    # 0 = the byte just after it
                    rel = (first - b.off, last - b.off) if side == "front" else (first, last)
                    out.append("%s guard of %r (%d bytes) dirty: %d byte(s), first at %+d, last at %+d (fill 0x%02X)"
                               % (side, b.name, b.nbytes, bad.numel(), rel[0], rel[1], self.fill))
            self.checked += 1
        return out

    def check(self) -> None:
        """AssertionError naming every buffer with a dirty guard; releases the buffers either way (the ledger stays)"""
        try:
            lines = self.dirty()
        finally:
            self.live = []
        assert not lines, "write outside a buffer:\n  " + "\n  ".join(lines)

    # ---- non-vacuity ---------------------------------------------------------------------------------------------------------------
    def covers(self, tensor: _torch.Tensor) -> bool:
        """does every byte of ``tensor`` (a contiguous tensor or a view of one) lie inside one guarded buffer handed out so far"""
        if tensor is None:
            return False
        lo = tensor.data_ptr()
        if tensor.numel() == 0:
            return any(p <= lo <= p + n for _, p, n in self.ledger)
        span = 1 + sum((s - 1) * st for s, st in zip(tensor.shape, tensor.stride()))
        hi = lo + span * tensor.element_size()
        return any(p <= lo and hi <= p + n for _, p, n in self.ledger)

    def handed_out(self, nbytes: int) -> bool:
        """was a guarded buffer of exactly ``nbytes`` bytes handed out"""
        return any(n == int(nbytes) for _, _, n in self.ledger)

    def names(self) -> List[str]:
        return [n for n, _, _ in self.ledger]

    # ---- the wrappers' allocations -------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def patched(self, modules=MODULES, package: str = "sylber_amd"):
        """inside, the listed modules' ``torch`` is a proxy whose constructors allocate through these guards"""
        proxy = TorchProxy(self)
        mods = [m if not isinstance(m, str) else importlib.import_module(package + "." + m if package else m) for m in modules]
        saved = [(m, m.torch) for m in mods]
        try:
            for m in mods:
                m.torch = proxy
            yield self
        finally:
            for m, t in saved:
                m.torch = t


class TorchProxy:
    """``torch`` with ``empty / zeros / ones / full`` and their ``_like`` forms routed to ``Guards.guarded``; every other attribute is
    torch's own"""

    def __init__(self, guards: Guards):
        object.__setattr__(self, "_g", guards)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch proxy is read-only")

    def _new(self, init, size, kw):
        g = self._g
        if len(size) == 1 and not isinstance(size[0], numbers.Integral):
            size = tuple(size[0])
        dtype = kw.get("dtype") or _torch.get_default_dtype()
        extra = set(kw) - {"dtype", "device", "pin_memory"}
        if extra or not g.wants(kw.get("device"), bool(kw.get("pin_memory", False))):
            return None
        return g.guarded(size, dtype, kw.get("device") if kw.get("device") is not None else "cpu", _call_site(), init)

    def _like(self, init, t, kw):
        g = self._g
        device = kw.get("device") if kw.get("device") is not None else t.device
        extra = set(kw) - {"dtype", "device"}
        if extra or not g.wants(device):
            return None
        return g.guarded(tuple(t.shape), kw.get("dtype") or t.dtype, device, _call_site(), init)

    def empty(self, *size, **kw):
        r = self._new(None, size, kw)
        return _torch.empty(*size, **kw) if r is None else r

    def zeros(self, *size, **kw):
        r = self._new(0, size, kw)
        return _torch.zeros(*size, **kw) if r is None else r

    def ones(self, *size, **kw):
        r = self._new(1, size, kw)
        return _torch.ones(*size, **kw) if r is None else r

    def full(self, size, fill_value, **kw):
        if "dtype" not in kw:                      # torch infers the dtype from the value: leave that to torch, then guard a copy
            t = _torch.full(size, fill_value, **kw)
            return self._g.guarded_copy(t, _call_site()) if self._g.wants(t.device, bool(kw.get("pin_memory", False))) else t
        r = self._new(fill_value, (size,), kw)
        return _torch.full(size, fill_value, **kw) if r is None else r

    def empty_like(self, t, **kw):
        r = self._like(None, t, kw)
        return _torch.empty_like(t, **kw) if r is None else r

    def zeros_like(self, t, **kw):
        r = self._like(0, t, kw)
        return _torch.zeros_like(t, **kw) if r is None else r

    def ones_like(self, t, **kw):
        r = self._like(1, t, kw)
        return _torch.ones_like(t, **kw) if r is None else r

    def full_like(self, t, fill_value, **kw):
        r = self._like(fill_value, t, kw)
        return _torch.full_like(t, fill_value, **kw) if r is None else r


def three_runs(run, patched: bool = True):
    """``run(g)`` once plainly (``g = None``) and once per fill under guards (inside ``patched()`` unless told otherwise), ``check()``
    after each guarded run -> ``(plain, [(guards, result), (guards, result)])``"""
    plain = run(None)
    out = []
    for fill in FILLS:
        g = Guards(fill)
        with (g.patched() if patched else contextlib.nullcontext()):
            r = run(g)
        g.check()
        out.append((g, r))
    return plain, out


@contextlib.contextmanager
def recorded_sizes(lib, suffixes=("_workspace_bytes", "_workspace_floats"), names=None):
    """inside, every ``lib.sylber_*_workspace_bytes / _floats`` call is recorded: yields ``{function name: [bytes, ...]}`` (floats
    counted as 4 bytes each), so a test can ask ``handed_out`` for exactly what a wrapper was told.  ``lib``: any object whose
    size functions are plain attributes (the ctypes library of ``sylber_amd._lib.load()``); ``names``: the functions to wrap
    (default: every export of ``sylber_amd._lib.EXPORTS`` with one of the suffixes)."""
    if names is None:
        from sylber_amd import _lib
        names = [n for n in _lib.EXPORTS if n.endswith(tuple(suffixes))]
    seen = {}
    saved = {}

    def wrap(name, fn):
        scale = 4 if name.endswith("_floats") else 1

        def call(*args):
            r = fn(*args)
            if int(r) > 0:
                seen.setdefault(name, []).append(int(r) * scale)
            return r
        return call
    try:
        for n in names:
            saved[n] = getattr(lib, n)
            setattr(lib, n, wrap(n, saved[n]))
        yield seen
    finally:
        for n, fn in saved.items():
            setattr(lib, n, fn)
