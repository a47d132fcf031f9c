"""Guard bands: do kernels stay inside their tensors and workspaces?

A value test cannot see a kernel that writes past the end of its output, or a workspace query that returns too little: the caching
allocator rounds every block up and packs small ones into shared segments, so the stray bytes land in slack or in another live
tensor.  ``guarded(device)`` makes them visible.  Inside the block

  * ``ops.release_workspaces()`` has been called, so cached scratch is asked for again at its exact size, and the other device buffers
    ``snvc_amd.ops`` keeps across calls (scale scratch, maximum words, per-width constants) are made anew inside the arena, the
    maximum words one set per allocation (``_fresh_caches``);
  * device-side ``torch.empty / zeros / ones / full / empty_like / zeros_like / new_empty / new_zeros / new_full`` are served from
    ONE fresh ``uint8`` arena (a bump pointer; never reset, never reused: a view keeps its arena alive, so a cache that retains such
    a tensor stays valid and never aliases a later block's tensors);
  * every allocation starts 256-byte aligned, has 64 KiB of guard before it and 64 KiB after it, the latter starting at the exact
    last byte of the tensor (no rounding of the size); the arena has a lead-in and a tail of 1 MiB.  64 KiB is more than the largest
    staged tile image of any kernel here (a 6 x 6 x 34-piece plane is about 20 KB): an over-reach stays inside the arena -- one live
    allocation, nothing faults -- and stays visible;
  * guard zones hold byte 0xA5; the interior of an ``empty`` holds byte 0xFF, a NaN in every float width, so an element that a kernel
    fails to write shows up; ``zeros`` / ``ones`` / ``full`` fill the interior only;
  * ``place(t, misalign=.., index_fill=..)`` copies an operand of the test into the arena at ``256-aligned + misalign`` bytes.  A
    floating operand gets 0xFF guards: a read outside it that reaches the result makes the result NaN.  An integer operand (an index,
    a label) gets guards filled with ``index_fill`` -- a value INSIDE the valid range -- so that a stray read changes the result but
    never forms an address outside the arena (default 0).  No test may poison an index operand out of range;
  * with ``place_results=True`` every fresh tensor that any torch call inside the block returns on the device (``randn``, ``.to(dev)``,
    arithmetic, ``clone``, ...) is placed likewise, at ``misalign``: an existing test's builder, run unchanged inside the block, then has
    every one of its operands in the arena.  (Integer results get the tensor's own minimum as ``index_fill``.)  The floating buffers
    the factories hand out get NaN guards as well then, since one kernel's output is the next one's operand; a write into such a
    guard is seen all the same.

On exit, or on ``check()``, every byte of the arena outside the interiors must be what it was; a failure names the allocation (shape,
dtype, call site of the factory call), the side, the first changed byte's offset and how many bytes changed.

Falls through to torch, counted in ``unguarded``: an allocation for another device (a kernel cannot write it), one with a
``memory_format``, a ``*_like`` of a non-contiguous tensor (it would copy the layout), pinned / non-strided / ``out=`` requests.
Autograd runs single-threaded inside the block, so that a backward's allocations are seen too.  Not seen at all: allocations by
torch's own C++ (``clone``, ``contiguous``, ``randn`` -- unless ``place_results``).  A read outside a tensor whose value is discarded
cannot be seen this way either.
"""
import linecache
import os
import sys
from dataclasses import dataclass
from typing import List, Optional

import torch
from torch.overrides import TorchFunctionMode

GUARD = 64 * 1024
LEAD = 1 << 20
ALIGN = 256
GUARD_BYTE = 0xA5
POISON_BYTE = 0xFF

_HERE = os.path.abspath(__file__)
_TORCH_DIR = os.path.dirname(os.path.abspath(torch.__file__))


class GuardViolation(AssertionError):
    pass


class ArenaExhausted(RuntimeError):
    pass


@dataclass
class Allocation:
    kind: str                 # "empty", "zeros", ..., "place"
    shape: tuple
    dtype: torch.dtype
    offset: int               # first byte of the tensor in the arena
    nbytes: int
    site: str

    def __str__(self):
        return f"{self.kind} {tuple(self.shape)} {self.dtype} ({self.nbytes} bytes at arena+{self.offset}) from {self.site}"


@dataclass
class Unguarded:
    kind: str
    reason: str
    site: str

    def __str__(self):
        return f"{self.kind}: {self.reason}, from {self.site}"


def _site(frames: int = 1, source: bool = False) -> str:
    """The call site of a factory call: the innermost ``frames`` frames outside torch and this module, joined by " < "; with ``source``
    each frame is followed by its line of code (how ``run_case``'s ``loose`` tells one call of an op from another)."""
    f = sys._getframe(1)
    found = []
    while f is not None and len(found) < frames:
        name = os.path.abspath(f.f_code.co_filename)
        if name != _HERE and not name.startswith(_TORCH_DIR):
            text = f" [{linecache.getline(name, f.f_lineno).strip()}]" if source else ""
            found.append(f"{os.path.relpath(name) if name.startswith(os.getcwd()) else name}:{f.f_lineno} in {f.f_code.co_name}{text}")
        f = f.f_back
    return " < ".join(found) or "?"


def _norm_device(d) -> torch.device:
    d = torch.device(d)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def _shape_of(args, kwargs):
    if "size" in kwargs:
        s = kwargs["size"]
    elif len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        s = args[0]
    else:
        s = args
    return tuple(int(v) for v in s)


_FACTORIES = {}          # func -> (kind, takes a tensor first, fill: None / number / "arg")
for _f, _k, _t, _fill in ((torch.empty, "empty", False, None), (torch.zeros, "zeros", False, 0), (torch.ones, "ones", False, 1),
                          (torch.full, "full", False, "arg"), (torch.empty_like, "empty_like", True, None),
                          (torch.zeros_like, "zeros_like", True, 0), (torch.Tensor.new_empty, "new_empty", True, None),
                          (torch.Tensor.new_zeros, "new_zeros", True, 0), (torch.Tensor.new_full, "new_full", True, "arg")):
    _FACTORIES[_f] = (_k, _t, _fill)
_LIKE = ("empty_like", "zeros_like")


def _place_fresh(mode, out, args, kwargs):
    """Every tensor of ``out`` that is new memory on the mode's device -- not a view of an argument, not placed already -- moved by
    ``mode._put``."""
    def tensors(v, acc):
        if isinstance(v, torch.Tensor):
            acc.append(v)
        elif isinstance(v, (tuple, list)):
            for e in v:
                tensors(e, acc)
        elif isinstance(v, dict):
            for e in v.values():
                tensors(e, acc)
        return acc

    given = {t.untyped_storage().data_ptr() for t in tensors([args, kwargs], []) if t.layout is torch.strided and t.device == mode.device}

    def move(t):
        if not isinstance(t, torch.Tensor) or type(t) not in (torch.Tensor, torch.nn.Parameter) or t.device != mode.device:
            return t
        if t.layout is not torch.strided or t.numel() == 0 or mode._is_placed(t) or t.untyped_storage().data_ptr() in given:
            return t
        return mode._put(t)

    if isinstance(out, torch.Tensor):
        return move(out)
    if type(out) in (tuple, list):
        return type(out)(move(v) for v in out)
    return out


class _fresh_caches:
    """On entry: the process-wide device buffers that ``snvc_amd.ops`` keeps across calls are dropped -- the per-stream workspaces, the
    scale scratch (running maximum and arrival counter of ``snvc_f16x3_split_scale``), the per-width ones / zeros, the losses' flag
    word, the sheared layer's tap counts and the pool of maximum words -- so that the block creates them anew (inside the arena, when
    it is a ``guarded`` block); and the pool hands out ONE set of words per allocation instead of 64, so that every set a kernel's
    atomic maxima land in has guard zones for neighbours.
    On exit the pool size is restored and the buffers made inside the block are dropped again, so that nothing later writes into a
    finished block's arena.  A tag that still refers to an old word keeps it alive; dropping a pool is what ``ops.amax_word`` itself
    does with a full one."""

    @staticmethod
    def _drop():
        from snvc_amd import _loss, ops
        from snvc_amd.models import submodule
        ops.release_workspaces()
        ops._SCALE_SCRATCH.clear()
        ops._ONES_ZEROS.clear()
        ops._AMAX_POOL.__dict__.pop("pools", None)
        _loss._flags.clear()                  # the word the loss kernels OR their input-check bits into
        submodule._SHEAR_COUNTS.clear()       # read-only tap counts of the sheared first layer's backward

    def __enter__(self):
        from snvc_amd import ops
        self._drop()
        self._words, ops._AMAX_POOL_WORDS = ops._AMAX_POOL_WORDS, 1
        return self

    def __exit__(self, *exc):
        from snvc_amd import ops
        ops._AMAX_POOL_WORDS = self._words
        self._drop()
        return False


class guarded(TorchFunctionMode):
    """See the module's docstring.  ``with guarded(dev) as g: ...``; ``g.allocations``, ``g.unguarded``, ``g.counts``."""

    def __init__(self, device, arena_bytes: int = 64 << 20, align: int = ALIGN, place_results: bool = False, misalign: int = 0,
                 check_on_exit: bool = True):
        super().__init__()
        self.device = _norm_device(device)
        self.arena_bytes = int(arena_bytes)
        if self.arena_bytes < 2 * LEAD + 2 * GUARD + align:
            raise ValueError("arena_bytes leaves no room beside the lead-in and the tail")
        self.align, self.place_results, self.misalign, self.check_on_exit = int(align), bool(place_results), int(misalign), check_on_exit
        self.allocations: List[Allocation] = []
        self.unguarded: List[Unguarded] = []
        self.results = []                         # (kind, tensor) of every factory call for this device, in order
        self.arena = self.shadow = None
        self._cur = LEAD
        self._busy = False

    # ------------------------------------------------------------------------------------------------------------------ the block
    def __enter__(self):
        self._caches = _fresh_caches().__enter__()
        self.arena = torch.full((self.arena_bytes,), GUARD_BYTE, dtype=torch.uint8, device=self.device)
        self.shadow = self.arena.clone()          # what every byte outside the interiors must still be
        self._base = self.arena.untyped_storage().data_ptr()
        # autograd's worker threads have mode stacks of their own: a backward's allocations are seen only on this thread
        self._threads = torch.autograd.set_multithreading_enabled(False)
        self._threads.__enter__()
        return super().__enter__()

    def __exit__(self, et, ev, tb):
        super().__exit__(et, ev, tb)
        self._threads.__exit__(et, ev, tb)
        self._caches.__exit__(et, ev, tb)
        try:
            if et is None and self.check_on_exit:
                self.check()
        finally:
            self.arena = self.shadow = None       # views keep the arena alive; the block itself does not
        return False

    @property
    def counts(self):
        return {"guarded": len(self.allocations), "unguarded": len(self.unguarded)}

    def unguarded_on_device(self) -> List[Unguarded]:
        """The fall-throughs a kernel could have written: everything but allocations for another device."""
        return [u for u in self.unguarded if u.reason != "another device"]

    # ---------------------------------------------------------------------------------------------------------------- allocation
    def _reserve(self, nbytes: int, itemsize: int, misalign: int) -> int:
        if misalign % itemsize:
            misalign += itemsize - misalign % itemsize        # a float64 operand cannot sit at +4
        start = self._cur + GUARD
        start += (-(self._base + start)) % self.align
        start += misalign
        end = start + nbytes + GUARD
        if end + LEAD > self.arena_bytes:
            raise ArenaExhausted(f"guarded arena of {self.arena_bytes} bytes is exhausted: {len(self.allocations)} allocations hold "
                                 f"{self._cur} bytes and the next wants {nbytes} more (plus guards); pass a larger arena_bytes")
        self._cur = end
        return start

    def _carve(self, kind: str, shape, dtype: torch.dtype, misalign: int = 0) -> torch.Tensor:
        itemsize = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * itemsize
        off = self._reserve(nbytes, itemsize, misalign)
        self.allocations.append(Allocation(kind, tuple(shape), dtype, off, nbytes, _site()))
        # .data: a version counter of its own -- views of one arena would otherwise share the arena's, and every write anywhere in it
        # would look like an in-place update of every tensor (autograd's saved tensors, the tags of snvc_amd._derived)
        return self.arena[off:off + nbytes].view(dtype).view(shape).data

    def _set_guards(self, a: Allocation, byte: Optional[int] = None, value=None):
        for z0 in (a.offset - GUARD, a.offset + a.nbytes):
            for buf in (self.arena, self.shadow):
                if value is None:
                    buf[z0:z0 + GUARD].fill_(byte)
                else:
                    buf[z0:z0 + GUARD].view(a.dtype).fill_(value)

    def place(self, t: torch.Tensor, *, misalign: int = 0, index_fill=None) -> torch.Tensor:
        """A contiguous copy of ``t`` (host or device) in the arena at 256-aligned + ``misalign`` bytes; see the module's docstring."""
        busy, self._busy = self._busy, True
        try:
            src = t.detach()
            dst = self._carve("place", tuple(src.shape), src.dtype, misalign)
            dst.copy_(src)
            a = self.allocations[-1]
            if src.dtype.is_floating_point or src.dtype.is_complex:
                self._set_guards(a, byte=POISON_BYTE)
            else:
                self._set_guards(a, value=(0 if index_fill is None else index_fill))
            if t.requires_grad:
                dst.requires_grad_()
            return dst
        finally:
            self._busy = busy

    # -------------------------------------------------------------------------------------------------------------- interception
    def _fall(self, kind, reason, func, args, kwargs):
        self.unguarded.append(Unguarded(kind, reason, _site()))
        out = func(*args, **kwargs)
        if out.device == self.device:
            self.results.append((kind, out, _site(3, True)))
        return out

    def _factory(self, func, args, kwargs):
        kind, like, fill = _FACTORIES[func]
        given_args = args
        args = list(args)
        kw = dict(kwargs)
        proto = args.pop(0) if like else None
        if fill == "arg":
            if "fill_value" in kw:
                fill = kw.pop("fill_value")
            else:
                fill = args.pop(-1)
        device = kw.pop("device", None)
        device = _norm_device(device) if device is not None else (proto.device if like else _norm_device(torch.get_default_device()))
        if device != self.device:
            return self._fall(kind, "another device", func, given_args, kwargs)
        dtype = kw.pop("dtype", None)
        if dtype is None:
            if like:
                dtype = proto.dtype
            elif kind == "full":
                dtype = (torch.bool if isinstance(fill, bool) else torch.int64 if isinstance(fill, int)
                         else torch.get_default_dtype() if isinstance(fill, float) else None)
            else:
                dtype = torch.get_default_dtype()
        requires_grad = bool(kw.pop("requires_grad", False))
        mf = kw.pop("memory_format", None)
        why = None
        if mf not in (None, torch.contiguous_format, torch.preserve_format):
            why = "a memory_format"
        elif kind in _LIKE and not proto.is_contiguous() and mf is not torch.contiguous_format:
            why = "copies a non-contiguous layout"
        elif kw.pop("pin_memory", False):
            why = "pinned"
        elif kw.pop("layout", torch.strided) is not torch.strided:
            why = "not strided"
        elif kw.pop("out", None) is not None:
            why = "out="
        elif dtype is None:
            why = "fill value of no plain type"
        if why is None:
            try:
                shape = tuple(proto.shape) if kind in _LIKE else _shape_of(args, kw)
                kw.pop("size", None)
            except Exception:
                why = "size not understood"
        if why is None and kw:
            why = "keywords " + ", ".join(sorted(kw))
        if why is not None:
            return self._fall(kind, why, func, given_args, kwargs)
        out = self._carve(kind, shape, dtype)
        if self.place_results and dtype.is_floating_point:
            # an output here is the next kernel's operand (a split pair, a raw convolution result): NaN around it, like a placed one
            self._set_guards(self.allocations[-1], byte=POISON_BYTE)
        if fill is None:
            a = self.allocations[-1]
            self.arena[a.offset:a.offset + a.nbytes].fill_(POISON_BYTE)
        else:
            out.fill_(fill)
        self.results.append((kind, out, _site(3, True)))
        return out.requires_grad_() if requires_grad else out

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if self._busy or self.arena is None:
            return func(*args, **kwargs)
        self._busy = True
        try:
            if func in _FACTORIES:
                return self._factory(func, args, kwargs)
            out = func(*args, **kwargs)
            if self.place_results and getattr(func, "__name__", "") != "__get__":      # not what an attribute holds (``t.grad``)
                out = _place_fresh(self, out, args, kwargs)
            return out
        finally:
            self._busy = False

    def _in_arena(self, t: torch.Tensor) -> bool:
        p = t.untyped_storage().data_ptr()
        return self._base <= p < self._base + self.arena_bytes

    _is_placed = _in_arena          # what _place_fresh asks of either mode

    def _put(self, t: torch.Tensor) -> torch.Tensor:
        if t.requires_grad and not t.is_leaf:
            dst = self._carve("place", tuple(t.shape), t.dtype, self.misalign)
            self._set_guards(self.allocations[-1], byte=POISON_BYTE)
            return dst.copy_(t)                           # stays in the graph
        fill = None
        if not (t.dtype.is_floating_point or t.dtype.is_complex) and t.dtype is not torch.bool:
            fill = int(t.min())
        return self.place(t, misalign=self.misalign, index_fill=fill)

    # ------------------------------------------------------------------------------------------------------------------ checking
    def violations(self) -> List[str]:
        busy, self._busy = self._busy, True
        try:
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            for a in self.allocations:                    # interiors may hold anything
                if a.nbytes:
                    self.shadow[a.offset:a.offset + a.nbytes].copy_(self.arena[a.offset:a.offset + a.nbytes])
            if torch.equal(self.arena, self.shadow):
                return []
            found = []
            ne = self.arena != self.shadow
            for a in self.allocations:
                for side, z0 in (("before", a.offset - GUARD), ("after", a.offset + a.nbytes)):
                    z = ne[z0:z0 + GUARD]
                    count = int(z.sum())
                    if count:
                        first = int(z.nonzero()[0])
                        rel = z0 + first - a.offset if side == "before" else first
                        where = f"byte {rel} relative to its first byte" if side == "before" else f"byte {rel} past its end"
                        found.append(f"{side} {a}: {count} guard bytes changed, the first at {where}")
                    z.zero_()
            rest = int(ne.sum())
            if rest:
                found.append(f"{rest} arena bytes changed outside every guard zone, the first at arena+{int(ne.nonzero()[0])}")
            return found
        finally:
            self._busy = busy

    def check(self):
        found = self.violations()
        if found:
            raise GuardViolation("guard zones were written:\n  " + "\n  ".join(found))


# ================================================================================================ running an existing test guarded
class recording(TorchFunctionMode):
    """The unguarded run of a case: torch's own memory, the same list of factory results as ``guarded.results``, and -- so that the
    wrappers and launchers choose the same kernel forms -- every fresh device tensor moved to 256-aligned + ``misalign`` bytes too."""

    def __init__(self, device, misalign: int = 0):
        super().__init__()
        self.device = _norm_device(device)
        self.misalign = int(misalign)
        self.results = []
        self._buffers, self._mine, self._busy = [], set(), False

    def __enter__(self):
        self._caches = _fresh_caches().__enter__()
        self._threads = torch.autograd.set_multithreading_enabled(False)
        self._threads.__enter__()
        return super().__enter__()

    def __exit__(self, et, ev, tb):
        super().__exit__(et, ev, tb)
        self._threads.__exit__(et, ev, tb)
        self._caches.__exit__(et, ev, tb)
        return False

    def _is_placed(self, t):
        return t.untyped_storage().data_ptr() in self._mine

    def _put(self, t):
        itemsize = t.element_size()
        mis = self.misalign + (-self.misalign) % itemsize
        nbytes = t.numel() * itemsize
        buf = torch.empty(nbytes + 2 * ALIGN + mis, dtype=torch.uint8, device=self.device)
        self._buffers.append(buf)
        self._mine.add(buf.untyped_storage().data_ptr())
        off = (-buf.data_ptr()) % ALIGN + mis
        dst = buf[off:off + nbytes].view(t.dtype).view(t.shape).data
        if t.requires_grad and not t.is_leaf:
            return dst.copy_(t)
        dst.copy_(t.detach())
        return dst.requires_grad_() if t.requires_grad else dst

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if self._busy:
            return func(*args, **kwargs)
        self._busy = True
        try:
            out = func(*args, **kwargs)
            if func in _FACTORIES:
                if isinstance(out, torch.Tensor) and out.device == self.device:
                    kind, _, fill = _FACTORIES[func]
                    if fill is None and out.is_contiguous() and out.numel():
                        out.view(-1).view(torch.uint8).fill_(POISON_BYTE)       # as in the arena: what no kernel writes is equal in both runs
                    self.results.append((kind, out, _site(3, True)))
                return out
            return _place_fresh(self, out, args, kwargs) if getattr(func, "__name__", "") != "__get__" else out
        finally:
            self._busy = False


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def compare_runs(base, got, loose=()):
    """(b) and (c) for every tensor the case allocated through a factory; returns (what differs, how many tensors were compared).

    The guarded run's bytes must equal the unguarded run's -- all of them: an ``empty`` is born with 0xFF in every byte in both runs,
    so what no kernel writes is equal too, and an element that only one run wrote differs.  The k-th result of a call site (three
    frames, with their lines of code) with a kind, shape and dtype is paired with the k-th of the same in the other run; both runs
    start from dropped caches (``_fresh_caches``), so a site with different counts in the two runs is itself reported.
    One-dimensional ``uint8`` ``empty`` tensors are workspaces: their contents are not results.  ``loose``: (text, rtol, atol) triples
    for the forms with float atomics -- a result whose site holds ``text`` is held to |a - b| <= rtol * max(max|b|, 1) + atol, the form
    of the bound the op's existing test uses, instead of bit-equality."""
    def by_key(results):
        d = {}
        for i, (kind, t, site) in enumerate(results):
            d.setdefault((site, kind, tuple(t.shape), t.dtype), []).append((i, t))
        return d

    a, b = by_key(base), by_key(got)
    bad, compared = [], 0
    for key in a.keys() - b.keys():
        bad.append(f"{key[1]} {key[2]} {key[3]} from {key[0].split(' < ')[0]}: 0 in the guarded run, {len(a[key])} in the unguarded run")
    for key, theirs in b.items():
        ours = a.get(key, [])
        site, kind = key[0], key[1]
        where = site.split(" < ")[0]
        if len(ours) != len(theirs):
            bad.append(f"{kind} {key[2]} {key[3]} from {where}: {len(theirs)} in the guarded run, {len(ours)} in the unguarded run")
            continue
        tol = next(((r, t) for text, r, t in loose if text in site), None)
        for (_, x), (i, y) in zip(ours, theirs):
            if x.numel() == 0 or (x.dtype == torch.uint8 and x.dim() == 1 and kind == "empty"):
                continue
            compared += 1
            if tol is not None and y.dtype.is_floating_point:
                xd, yd = x.detach().double(), y.detach().double()
                bound = tol[0] * max(float(xd.abs().max()), 1.0) + tol[1]
                err = float((xd - yd).abs().max())
                if not err <= bound:
                    bad.append(f"factory result {i} ({kind} {tuple(y.shape)} {y.dtype} from {where}): differs from the unguarded run by "
                               f"{err:.3e}, above {bound:.3e}")
                continue
            xb, yb = _bytes(x), _bytes(y)
            differ = xb != yb
            n = int(differ.sum())
            if n:
                bad.append(f"factory result {i} ({kind} {tuple(y.shape)} {y.dtype} from {where}): {n} bytes differ from the "
                           f"unguarded run, the first at byte {int(differ.nonzero()[0])}")
    return bad, compared


def run_case(fn, device, misalign: int = 0, arena_bytes: int = 128 << 20, loose=(), allow_unguarded=(), what: str = ""):
    """Run ``fn()`` -- an existing test or its builder, unchanged -- once in torch's own memory and once inside
    ``guarded(place_results=True)``, in both runs with every device tensor it makes moved to 256-aligned + ``misalign`` bytes (the same kernel
    forms are chosen), in the second with those operands between poisoned guards and every buffer the ops allocate guarded.  Asserts
    (a) all guards intact, (b) + (c) the factory-allocated tensors bit-equal to the unguarded run's and at least one of them compared
    (``loose``: the results of calls with float atomics, at the tolerance of the op's existing test -- see ``compare_runs``),
    (d) no allocation on the device fell through (but those whose ``reason`` is in ``allow_unguarded``).  Returns the guarded block."""
    torch.manual_seed(20261)                  # a case that draws from torch's generator draws the same in both runs
    with recording(device, misalign) as rec:
        fn()
    base = rec.results
    torch.manual_seed(20261)
    g = guarded(device, arena_bytes, place_results=True, misalign=misalign, check_on_exit=False)
    failed = None
    with g:
        try:
            fn()
        except Exception as e:            # the guards are looked at first: a trampled neighbour is the likelier cause than the value
            failed = e
        found = g.violations()
    compared = 0
    if not found and failed is None:
        found, compared = compare_runs(base, g.results, loose)
    loose = [str(u) for u in g.unguarded_on_device() if u.reason not in allow_unguarded]
    ws = sum(1 for k, t, _ in g.results if k == "empty" and t.dtype == torch.uint8 and t.dim() == 1)
    ws_from = sorted({"/".join(f.split(" in ")[1] for f in site.split(" < ")[:2]) for k, t, site in g.results
                      if k == "empty" and t.dim() == 1 and t.dtype == torch.uint8})
    print(f"guarded {what} +{misalign}: {len(g.allocations)} guarded ({len(g.results)} by factories, {ws} byte workspaces), "
          f"{len(g.unguarded_on_device())} unguarded on the device, {len(g.unguarded) - len(g.unguarded_on_device())} for other devices, "
          f"{compared} compared with the unguarded run"
          + (f"; byte buffers of {', '.join(ws_from)}" if ws_from else ""))
    assert not found, "\n  ".join([f"{what} at +{misalign}:"] + found + ([f"and the case itself failed: {failed!r}"] if failed else []))
    if failed is not None:
        raise failed
    assert g.allocations, f"{what}: the guarded run allocated nothing on the device -- a cached result?"
    results = sum(1 for k, t, _ in g.results if t.numel() and not (k == "empty" and t.dtype == torch.uint8 and t.dim() == 1))
    assert compared == results, f"{what}: {compared} of the guarded run's {results} factory results were compared with the unguarded run's"
    assert not loose, f"{what}: allocations on the device that were not guarded:\n  " + "\n  ".join(loose)
    return g


def run_existing(module: str, name: str, kwargs: dict, device, misalign: int, **options):
    """``run_case`` on a test (or builder) of another test module, called with ``kwargs`` as pytest would call it."""
    import importlib
    fn = getattr(importlib.import_module(module), name)
    return run_case(lambda: fn(**kwargs), device, misalign, what=f"{module}.{name}({', '.join(f'{k}={v!r}' for k, v in kwargs.items())})",
                    **options)
