"""Fenced arena and launch recorder behind tests/test_gpu_fenced.py (importing this file needs no GPU).

The float64 gates pin what a kernel writes INSIDE its outputs.  This helper watches the rest: every buffer of a call is carved out
of one arena with `fence_bytes` of a known byte on both sides (a store past the end lands in the fence and is reported, it does not
fault), workspaces are exactly as long as their size function says, and everything a kernel does not own or must initialise itself
is filled with a poison byte first, so that a result which depends on such bytes differs between two poisons.

    Arena      one uint8 tensor; take() / take_bytes() carve regions, poison() refills, check() reports fence damage.
    record()   runs an `ops.*` call pattern once on ordinary buffers and notes every C-ABI launch it makes: launcher, arguments,
               which arguments are device tensors (and how long), which workspace sizes were asked for and from which size function.
    Replay     the same launches through `_native.call` with every device pointer moved into an Arena; parameter roles (input /
               output / workspace) come from the `const` qualifiers and names in include/awseg.h, not from the test.
"""
from __future__ import annotations

import contextlib
import ctypes
import re
from dataclasses import dataclass, field
from pathlib import Path

import torch

HEADER = Path(__file__).resolve().parents[1] / "include" / "awseg.h"
ALIGN = 256                                        # every region starts at `offset_bytes` past a multiple of this
SIZE_SUFFIXES = ("_workspace", "_partials", "_halfs", "_floats")
SCRATCH_PARAMS = ("workspace", "partials")         # parameter names whose buffers are scratch: contents undefined on entry and exit


# ----------------------------------------------------------------------------------------------------------------- the header
@dataclass(frozen=True)
class Param:
    name: str
    pointer: bool
    const: bool


def parse_header(path: Path = HEADER) -> dict:
    """name -> [Param] for every function include/awseg.h declares."""
    text = re.sub(r"/\*.*?\*/", " ", path.read_text(), flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    protos = {}
    for m in re.finditer(r"\b(awseg_\w+)\s*\(([^()]*)\)\s*;", text):
        params = []
        for raw in m.group(2).split(","):
            raw = " ".join(raw.split())
            if raw in ("void", ""):
                continue
            ident = re.findall(r"[A-Za-z_]\w*", raw)[-1]
            is_ptr = "*" in raw or raw.startswith("awseg_stream_t")
            params.append(Param(ident, is_ptr, raw.startswith("const ")))
        protos[m.group(1)] = params
    return protos


def is_size_function(name: str) -> bool:
    return name.endswith(SIZE_SUFFIXES)


# ------------------------------------------------------------------------------------------------------------------ the arena
@dataclass
class Region:
    name: str
    start: int            # byte offset of the first element inside the arena tensor
    nbytes: int
    kind: str             # "in" | "inout" | "out" | "scratch"
    before: int           # first byte of the fence in front (the fence is [before, start))
    after_end: int        # one past the last byte of the fence behind (the fence is [start + nbytes, after_end))
    view: torch.Tensor = field(repr=False, default=None)


class Arena:
    """One uint8 tensor; every region taken from it has `fence_bytes` of `fill` in front of it and behind it, the fence behind
    beginning at the byte after the region's last element."""

    def __init__(self, device, fence_bytes: int = 65536, fill: int = 0xA5, capacity: int = 8 << 20):
        self.fence_bytes, self.fill = int(fence_bytes), int(fill)
        self.buf = torch.full((int(capacity),), self.fill, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        self.regions: list[Region] = []
        self._cursor = 0

    @staticmethod
    def bytes_needed(sizes, fence_bytes: int = 65536) -> int:
        """An upper bound of the capacity a list of region lengths needs."""
        return sum(int(n) + 2 * fence_bytes + 2 * ALIGN for n in sizes) + ALIGN

    def take_bytes(self, n: int, offset_bytes: int = 0, kind: str = "scratch", name: str | None = None) -> torch.Tensor:
        """Exactly n bytes whose address is offset_bytes past a multiple of 256, fenced on both sides."""
        n = int(n)
        if n < 0 or not 0 <= offset_bytes < ALIGN:
            raise ValueError("take_bytes: n >= 0 and 0 <= offset_bytes < 256")
        start = self._cursor + self.fence_bytes
        start += (offset_bytes - (self.base + start)) % ALIGN
        end = start + n + self.fence_bytes
        if end > self.buf.numel():
            raise MemoryError(f"arena of {self.buf.numel()} bytes is too small for region {name!r} ({n} bytes)")
        region = Region(name or f"r{len(self.regions)}", start, n, kind, self._cursor, end, self.buf[start:start + n])
        self.regions.append(region)
        self._cursor = end
        return region.view

    def take(self, shape, dtype, offset_bytes: int = 0, kind: str = "out", name: str | None = None) -> torch.Tensor:
        """A contiguous tensor of `shape` / `dtype`; its length is rounded up to nothing."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        numel = 1
        for s in shape:
            numel *= int(s)
        esize = torch.empty((), dtype=dtype).element_size()
        if offset_bytes % esize:
            raise ValueError("offset_bytes must be a multiple of the element size")
        return self.take_bytes(numel * esize, offset_bytes, kind, name).view(dtype).view(shape)

    def region_of(self, view: torch.Tensor) -> Region:
        off = view.data_ptr() - self.base
        for r in self.regions:
            if r.start <= off < r.start + max(r.nbytes, 1):
                return r
        raise KeyError("tensor is not a region of this arena")

    def poison(self, byte: int, kinds=("scratch", "out")) -> None:
        """Refill every fence, and every region of the given kinds, with `byte` (which check() expects from then on)."""
        self.fill = int(byte)
        for r in self.regions:
            self.buf[r.before:r.start].fill_(self.fill)
            self.buf[r.start + r.nbytes:r.after_end].fill_(self.fill)
            if r.kind in kinds:
                r.view.fill_(self.fill)
        self.buf[self._cursor:].fill_(self.fill)

    def check(self) -> list:
        """[(region name, "before" | "after", offset of the first damaged byte relative to the region's first byte, damaged bytes)]"""
        damage = []
        spans = [(r.name, "before", r.before, r.start, r.start) for r in self.regions]
        spans += [(r.name, "after", r.start + r.nbytes, r.after_end, r.start) for r in self.regions]
        if self.regions:
            spans.append((self.regions[-1].name, "after", self._cursor, self.buf.numel(), self.regions[-1].start))
        for name, side, lo, hi, origin in spans:
            bad = (self.buf[lo:hi] != self.fill).nonzero()
            if bad.numel():
                damage.append((name, side, lo + int(bad[0]) - origin, int(bad.numel())))
        return damage


# --------------------------------------------------------------------------------------------------------------- the recorder
@dataclass
class Buffer:
    addr: int
    nbytes: int
    tensor: torch.Tensor = field(repr=False)
    scratch: bool = False
    requested: int | None = None        # workspace: the byte count the call pattern asked Workspace.get for


@dataclass
class Launch:
    name: str
    args: tuple
    allow: tuple | None                 # try_call's `allow`, None for call
    rc: int = 0


@dataclass
class Trace:
    launches: list = field(default_factory=list)
    buffers: dict = field(default_factory=dict)         # addr -> Buffer (the longest seen at that address)
    snapshots: dict = field(default_factory=dict)       # addr -> bytes of the buffer just before the first launch that takes it
    sizes: list = field(default_factory=list)           # (size function, args, result) in call order


def _bytes_of(t: torch.Tensor, nbytes: int) -> torch.Tensor:
    """The `nbytes` bytes of memory that start at t's first element, as a uint8 view (whatever t's strides)."""
    out = torch.empty(0, dtype=torch.uint8, device=t.device)
    return out.set_(t.untyped_storage(), t.storage_offset() * t.element_size(), (int(nbytes),), (1,))


def _span_bytes(t: torch.Tensor) -> int:
    if t.numel() == 0:
        return 0
    return (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size()


def _addr(a):
    return a.value if isinstance(a, ctypes.c_void_p) else None


@contextlib.contextmanager
def record(trace: Trace):
    """Note every launch the package's ops make inside the block.  Workspaces come as fresh buffers of exactly the size asked for."""
    from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N
    handle = N.lib()
    saved = (N.ptr, N.ptr_strided, N.call, N.try_call, N.check, N.workspace)

    def note(t, nbytes, scratch=False, requested=None):
        if t is None or nbytes == 0:
            return
        old = trace.buffers.get(t.data_ptr())
        if old is None or old.nbytes < nbytes:
            trace.buffers[t.data_ptr()] = Buffer(t.data_ptr(), int(nbytes), t, scratch or bool(old and old.scratch),
                                                 requested if requested is not None else (old.requested if old else None))

    def ptr(t):
        p = saved[0](t)
        if t is not None:
            note(t, t.numel() * t.element_size())
        return p

    def ptr_strided(t):
        p = saved[1](t)
        note(t, _span_bytes(t))
        return p

    class ExactWorkspace:
        def get(self, device, nbytes, tag="ws"):
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            note(buf, int(nbytes), scratch=True, requested=int(nbytes))
            return buf

    protos = parse_header()

    def launch(name, args, allow):
        entry = Launch(name, tuple(args), allow)
        for v in [_addr(a) for a in args] + _table_entries(entry, protos[name]):
            buf = trace.buffers.get(v)
            if buf is not None and (buf.addr not in trace.snapshots or trace.snapshots[buf.addr].numel() < buf.nbytes):
                trace.snapshots[buf.addr] = _bytes_of(buf.tensor, buf.nbytes).clone()
        trace.launches.append(entry)
        if allow is not None:
            entry.rc = saved[3](name, *args, allow=allow)
        else:                                                   # call(): note the code of an argument check, then raise as call() does
            entry.rc = saved[3](name, *args, allow=(-1, -2, -3))
            saved[4](entry.rc, name)
        return entry.rc

    def call(name, *args):
        launch(name, args, None)

    def try_call(name, *args, allow=(-2,)):
        return launch(name, args, tuple(allow))

    size_names = [n for n in N.SIGNATURES if is_size_function(n)]
    originals = {n: getattr(handle, n) for n in size_names}

    def sized(n):
        def f(*args):
            res = originals[n](*args)
            trace.sizes.append((n, tuple(args), int(res)))
            return res
        return f

    N.ptr, N.ptr_strided, N.call, N.try_call, N.workspace = ptr, ptr_strided, call, try_call, ExactWorkspace()
    for n in size_names:
        setattr(handle, n, sized(n))
    try:
        yield trace
    finally:
        N.ptr, N.ptr_strided, N.call, N.try_call, _, N.workspace = saved
        for n in size_names:
            setattr(handle, n, originals[n])


# ----------------------------------------------------------------------------------------------------------------- the replay
@dataclass
class Slot:
    """Maximal run of overlapping recorded buffers: one arena region."""
    addr: int
    nbytes: int
    kind: str = "in"
    params: set = field(default_factory=set)
    elem: int = 1                                    # element size of the buffers written here
    initial: torch.Tensor = field(repr=False, default=None)
    final: torch.Tensor = field(repr=False, default=None)
    region: Region = field(repr=False, default=None)


HOST_POINTER_TABLES = {"pieces": "n_pieces"}        # host arrays of device pointers: parameter -> the parameter that counts them


def _table_entries(launch: Launch, params: list) -> list:
    """The device addresses in a launch's host pointer table (awseg_gemm_split_pieces_bias_act's `pieces`)."""
    names = [p.name for p in params]
    out = []
    for table, count in HOST_POINTER_TABLES.items():
        if table in names:
            arr = ctypes.cast(launch.args[names.index(table)], ctypes.POINTER(ctypes.c_void_p))
            out += [arr[i] for i in range(int(launch.args[names.index(count)]))]
    return out


def plan(trace: Trace, protos: dict, inout=(), scratch=()) -> list:
    """Group the recorded buffers into slots and give each its role: `scratch` (a workspace), `out` (only ever written),
    `inout` (written, and named in `inout` or read by the launch that first writes it: residual == out, in-place) or `in`."""
    used = {}
    order = []
    for li, launch in enumerate(trace.launches):
        params = protos[launch.name]
        if len(params) != len(launch.args):
            raise AssertionError(f"{launch.name}: {len(launch.args)} arguments for {len(params)} parameters in the header")
        seen = [(p, _addr(a)) for p, a in zip(params, launch.args)]
        seen += [(Param("pieces", True, True), v) for v in _table_entries(launch, params)]
        for p, v in seen:
            buf = trace.buffers.get(v)
            if buf is None:
                continue
            if buf.addr not in used:
                used[buf.addr] = []
                order.append(buf.addr)
            used[buf.addr].append((li, p))
    slots: list[Slot] = []
    for addr in sorted(order):
        buf = trace.buffers[addr]
        if slots and addr < slots[-1].addr + slots[-1].nbytes:
            slots[-1].nbytes = max(slots[-1].nbytes, addr + buf.nbytes - slots[-1].addr)
        else:
            slots.append(Slot(addr, buf.nbytes))
    for s in slots:
        members = [a for a in order if s.addr <= a < s.addr + s.nbytes]
        uses = sorted(((li, p, a) for a in members for li, p in used[a]), key=lambda u: u[0])
        s.params = {p.name for _, p, _ in uses}
        written = [u for u in uses if not u[1].const]
        is_scratch = any(trace.buffers[a].scratch for a in members) or bool(s.params & (set(SCRATCH_PARAMS) | set(scratch)))
        if is_scratch:
            s.kind = "scratch"
        elif written:
            first = written[0][0]
            read_before = any(u[1].const and u[0] <= first for u in uses)
            s.kind = "inout" if (read_before or s.params & set(inout)) else "out"
            s.elem = max(trace.buffers[a].tensor.element_size() for _, p, a in written)
        s.initial = torch.empty(s.nbytes, dtype=torch.uint8, device=trace.buffers[members[0]].tensor.device)
        s.final = torch.empty_like(s.initial)
        for a in members:                              # the union of the members is the whole slot
            lo = a - s.addr
            s.initial[lo:lo + trace.buffers[a].nbytes] = trace.snapshots[a]
            s.final[lo:lo + trace.buffers[a].nbytes] = _bytes_of(trace.buffers[a].tensor, trace.buffers[a].nbytes)
    return slots


class Replay:
    """The recorded launches on one Arena.  run(byte): poison, load inputs and accumulators, launch, synchronise."""

    def __init__(self, trace: Trace, slots: list, device, fence_bytes: int = 65536, offsets: dict | None = None, protos: dict | None = None):
        self.trace, self.slots, self.protos = trace, slots, protos or parse_header()
        offsets = offsets or {}
        self.arena = Arena(device, fence_bytes, capacity=Arena.bytes_needed([s.nbytes for s in slots], fence_bytes))
        for s in slots:
            # by default a buffer sits where it sat in the plain run relative to a 256-byte boundary (ordinary allocations: 0), so
            # inputs a case passed off alignment stay off alignment and every kernel takes the path it took there
            off = next((o for name, o in offsets.items() if name in s.params), s.addr % ALIGN)
            name = "/".join(sorted(s.params))
            self.arena.take_bytes(s.nbytes, off, s.kind, name)
            s.region = self.arena.regions[-1]

    def _moved(self, a):
        v = _addr(a)
        if v is None:
            return a
        for s in self.slots:
            if s.addr <= v < s.addr + s.nbytes:
                return ctypes.c_void_p(s.region.view.data_ptr() + (v - s.addr))
        return a

    def _arguments(self, l: Launch) -> list:
        args = [self._moved(a) for a in l.args]
        names = [p.name for p in self.protos[l.name]]
        for table in HOST_POINTER_TABLES:
            if table in names:                           # a fresh host table with the moved device pointers
                moved = [self._moved(ctypes.c_void_p(v)) for v in _table_entries(l, self.protos[l.name])]
                arr = (ctypes.c_void_p * len(moved))(*[m.value for m in moved])
                args[names.index(table)] = ctypes.cast(arr, ctypes.c_void_p)
                self._keep = arr
        return args

    def load(self) -> None:
        for s in self.slots:
            if s.kind in ("in", "inout"):
                s.region.view.copy_(s.initial)

    def launch(self) -> None:
        from adverse_weather_semantic_segmentation_robustness_benchmark_amd import _native as N
        for l in self.trace.launches:
            args = self._arguments(l)
            allow = l.allow if l.allow is not None else ((l.rc,) if l.rc else None)      # a call() that raised in the plain run
            rc = N.try_call(l.name, *args, allow=allow) if allow is not None else (N.call(l.name, *args) or 0)
            if rc != l.rc:
                raise AssertionError(f"{l.name} returned {rc} on arena pointers and {l.rc} on ordinary buffers")
        torch.cuda.synchronize()

    def run(self, byte: int) -> None:
        self.arena.poison(byte)
        self.load()
        torch.cuda.synchronize()
        self.launch()

    def view_like(self, t: torch.Tensor) -> torch.Tensor:
        """The arena's copy of a contiguous tensor of the recorded call."""
        for s in self.slots:
            if s.addr <= t.data_ptr() < s.addr + s.nbytes:
                lo = t.data_ptr() - s.addr
                return s.region.view[lo:lo + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
        raise KeyError("tensor was not an argument of the recorded launches")


def unwritten(zero_run: torch.Tensor, ones_run: torch.Tensor, elem: int) -> torch.Tensor:
    """Indices of the elements (of `elem` bytes) that still hold the poison in BOTH runs: all 0x00 after the 0x00 run and all 0xFF
    after the 0xFF run.  An element the kernel wrote holds the same bytes in both."""
    n = zero_run.numel() // elem * elem
    z = (zero_run[:n].view(-1, elem) == 0).all(dim=1)
    o = (ones_run[:n].view(-1, elem) == 0xFF).all(dim=1)
    return (z & o).nonzero().flatten()
