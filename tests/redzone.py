"""Guard bands and poison around every tensor the product (and the case modules) allocate.

The op-level checks compare what a kernel was asked to write with a reference.  They do not see what ELSE it wrote, that it skipped a part of
an output which the caching allocator happened to hand back still holding the previous (correct) result, or that it read memory beside an
operand whose stale contents happened to be finite.  ``guarded(*modules)`` replaces the module-level name ``torch`` in the given modules by a
proxy whose ``empty / zeros / ones / full / *_like`` carve each tensor out of the middle of a larger flat buffer:

    [ band before | interior (numel elements) | band after ]       (+ up to 512 bytes in front where the allocator aligns to less)

* shape and strides come from the same call on ``device="meta"``: channels_last and ``*_like`` strides are exactly real torch's;
* a band is ``max(4096 bytes, 2 * stride(-2) * itemsize)`` rounded up to a multiple of 512 bytes, at most 1 MiB (two rows: a row written past M
  lands one leading dimension after the end); the interior starts on a 512-byte boundary, so every 16-byte eligibility rule of ops.py picks
  the kernel it picks without the guard;
* the bands hold the dtype's poison (quiet NaN for the float types, a fixed odd bit pattern for the integer types and bool); the interior holds
  the poison for ``empty*`` and the requested value otherwise: an element a kernel never wrote reads as NaN, not as the previous call's result;
* ``Guard.verify()`` checks both bands of every allocation since the last call and names the allocating function and line of each broken one.

Calls the guard cannot serve go to real torch and are counted (``Guard.passthroughs``): zero elements, a dtype without a poison, keyword
arguments the meta call rejects (``pin_memory``, ``out=``), and any allocation while the current stream is being captured into a graph.
The autouse fixtures of the op-level test files run every test inside ``guarded(ops, <their case modules>)`` followed by ``verify()``
(``fixture_guard``); tests/redzone_cases.py checks the harness itself, pins that it guards what it is meant to, and adds the guarded checks of
entry points that had none."""
import atexit
import contextlib
import json
import os
import sys

import torch as _torch

MIN_BAND_BYTES = 4096
MAX_BAND_BYTES = 1 << 20
ALIGN = 512

_NAN = float("nan")
POISON = {_torch.float32: _NAN, _torch.float64: _NAN, _torch.bfloat16: _NAN, _torch.float16: _NAN,
          _torch.int64: -0x5A5A5A5A5A5A5A5B, _torch.int32: -0x5A5A5A5B, _torch.int16: -0x5A5B, _torch.int8: -0x5B, _torch.uint8: 0xA5,
          _torch.bool: True}
FACTORIES = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like")
# the tensor caches of transfuser_amd.ops: emptied on entry (cached scratch is then allocated inside the guard) and on exit (it does not outlive it)
OPS_CACHES = ("_ws_cache", "_skf_cache", "_gws_cache", "_thin_ws_cache", "_zpool", "_HIST_WS", "_bnr_ws")


def band_elems(stride, itemsize):
    """Elements of ONE band of a tensor with these strides."""
    two_rows = 2 * stride[-2] * itemsize if len(stride) >= 2 else 0
    nbytes = min(MAX_BAND_BYTES, (max(MIN_BAND_BYTES, two_rows) + ALIGN - 1) // ALIGN * ALIGN)
    return nbytes // itemsize


def _is_poison(t):
    pat = POISON[t.dtype]
    return t.isnan() if pat != pat else t == pat


def _site():
    """(function, file, line) of the nearest caller outside this file; a lambda is named after the function that called it."""
    here = _site.__code__.co_filename
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == here:
        f = f.f_back
    if f is None:
        return ("?", "?", 0)
    lam = ""
    if f.f_code.co_name == "<lambda>" and f.f_back is not None:
        f, lam = f.f_back, ".<lambda>"
    name = f.f_code.co_name
    owner = f.f_locals.get("self", None)
    if owner is not None and not isinstance(owner, _torch.Tensor):
        name = type(owner).__name__ + "." + name
    return (name + lam, f.f_code.co_filename, f.f_lineno)


def _fmt(site):
    return "%s (%s:%d)" % (site[0], os.path.basename(site[1]), site[2])


class Record:
    """One guarded allocation: ``raw`` is the flat buffer torch allocated, ``base`` = [band | interior | band] starts ``lead`` elements into it."""
    __slots__ = ("raw", "lead", "band", "numel", "site", "fn", "shape")

    def __init__(self, raw, lead, band, numel, site, fn, shape):
        self.raw, self.lead, self.band, self.numel, self.site, self.fn, self.shape = raw, lead, band, numel, site, fn, shape

    @property
    def func(self):
        return self.site[0]

    @property
    def base(self):
        return self.raw[self.lead:self.lead + self.numel + 2 * self.band]

    def bands(self):
        """(2, band) view: row 0 the band before, row 1 the band after."""
        return self.raw.as_strided((2, self.band), (self.band + self.numel, 1), self.lead)

    def before(self):
        return self.base[:self.band]

    def after(self):
        return self.base[self.band + self.numel:]

    def interior(self):
        return self.base[self.band:self.band + self.numel]


class Guard:
    def __init__(self):
        self.records = []          # allocations since the last verify(): their bases stay alive until then
        self.guarded = 0           # guarded allocations over the Guard's life
        self._sites = {}           # (function, file, line) -> guarded allocations
        self.passthroughs = []     # (site string, reason) of every call that went to real torch

    @property
    def sites(self):
        """"function (file:line)" -> guarded allocations made there."""
        return {_fmt(k): n for k, n in self._sites.items()}

    # -- allocation
    def _pass(self, fn, args, kw, reason):
        self.passthroughs.append(("%s torch.%s" % (_fmt(_site()), fn), reason))
        return getattr(_torch, fn)(*args, **kw)

    def make(self, fn, args, kw):
        if "out" in kw or kw.get("pin_memory"):
            return self._pass(fn, args, kw, "keyword argument the meta call rejects: %s" % ("out" if "out" in kw else "pin_memory"))
        like = args[0] if fn.endswith("_like") else None
        device = kw.get("device", None)
        if device is None:
            device = like.device if like is not None else (_torch.get_default_device() if hasattr(_torch, "get_default_device") else "cpu")
        device = _torch.device(device)
        mkw = {k: v for k, v in kw.items() if k != "requires_grad"}
        mkw["device"] = "meta"
        try:
            meta = getattr(_torch, fn)(*args, **mkw)
        except Exception as e:      # real torch decides whether the call is an error
            return self._pass(fn, args, kw, "the meta call rejects it: %s" % (str(e).splitlines() or [type(e).__name__])[0][:80])
        numel = meta.numel()
        if numel == 0:
            return self._pass(fn, args, kw, "zero elements")
        if meta.dtype not in POISON:
            return self._pass(fn, args, kw, "no poison for %s" % meta.dtype)
        if device.type == "cuda" and _torch.cuda.is_current_stream_capturing():
            return self._pass(fn, args, kw, "stream is capturing")
        shape, stride = tuple(meta.shape), tuple(meta.stride())
        if meta.storage_offset() != 0 or 1 + sum((n - 1) * s for n, s in zip(shape, stride)) != numel:
            return self._pass(fn, args, kw, "not dense")
        item = meta.element_size()
        band = band_elems(stride, item)
        slack = ALIGN // item
        raw = _torch.empty(numel + 2 * band + slack, dtype=meta.dtype, device=device)
        lead = (-raw.data_ptr() % ALIGN) // item          # 0 where the allocator aligns to 512 bytes itself (the GPU's caching allocator)
        rec = Record(raw, lead, band, numel, _site(), fn, shape)
        out = raw.as_strided(shape, stride, lead + band)
        if fn.startswith("empty"):
            raw.fill_(POISON[meta.dtype])           # bands AND interior in one fill: an element nobody writes reads as poison
        else:
            rec.bands().fill_(POISON[meta.dtype])
            out.fill_(0 if fn.startswith("zeros") else 1 if fn.startswith("ones") else (args[1] if len(args) > 1 else kw["fill_value"]))
        self.records.append(rec)
        self.guarded += 1
        self._sites[rec.site] = self._sites.get(rec.site, 0) + 1
        if kw.get("requires_grad"):
            out.requires_grad_(True)
        return out

    # -- check
    def verify(self):
        """Both bands of every allocation since the last call; the list is cleared whatever the outcome."""
        records, self.records = self.records, []
        if not records:
            return
        if any(r.raw.is_cuda for r in records):
            _torch.cuda.synchronize()
        # the bands of all allocations of one (device, dtype, band length) are gathered into one (n, 2, band) tensor (at most ~64 MiB at a time) and
        # tested there: a few launches and one transfer per group, not several per allocation
        groups, ok = {}, {}
        for i, r in enumerate(records):
            groups.setdefault((r.raw.device, r.raw.dtype, r.band), []).append(i)
        for (_, _, band), idx in groups.items():
            step = max(1, (64 << 20) // (2 * band * records[idx[0]].raw.element_size()))
            for k in range(0, len(idx), step):
                part = idx[k:k + step]
                flags = _is_poison(_torch.stack([records[i].bands() for i in part])).all(dim=2).cpu()
                for i, pair in zip(part, flags.tolist()):
                    ok[i] = pair
        broken = []
        for i, r in enumerate(records):
            for j, (side, band, origin) in enumerate((("before", r.before(), -r.band), ("after", r.after(), 0))):
                if not ok[i][j]:
                    bad = (~_is_poison(band)).nonzero().flatten()
                    broken.append("%s torch.%s %s %s: band %s broken at offsets %d .. %d (%d elements; offsets count from the %s)" % (
                        _fmt(r.site), r.fn, str(r.raw.dtype).replace("torch.", ""), list(r.shape), side, int(bad[0]) + origin, int(bad[-1]) + origin,
                        bad.numel(), "first element of the tensor" if side == "before" else "first element past its end"))
        assert not broken, "%d guard band(s) written:\n  " % len(broken) + "\n  ".join(broken)


class TorchProxy:
    """Stands in for the module-level name ``torch``: the allocating factories go through the Guard, every other attribute is real torch's."""

    def __init__(self, guard):
        self.__dict__["_guard"] = guard
        for fn in FACTORIES:
            self.__dict__[fn] = (lambda *a, _fn=fn, **kw: guard.make(_fn, a, kw))

    def __getattr__(self, name):
        return getattr(_torch, name)


def _clear_ops_caches():
    from transfuser_amd import ops
    for name in OPS_CACHES:
        getattr(ops, name).clear()
    ops._lowp["w"].clear()
    ops._lowp.pop("table", None)


@contextlib.contextmanager
def guarded(*modules, guard=None):
    """Run the body with ``torch`` proxied in ``modules`` and every ``R`` of theirs returning guarded operands; yields the Guard.  The caller
    runs ``verify()``; whatever is still recorded at exit is dropped."""
    g = guard if guard is not None else Guard()
    proxy = TorchProxy(g)
    saved = []
    _clear_ops_caches()
    try:
        for m in modules:
            if getattr(m, "torch", None) is _torch:
                saved.append((m, "torch", _torch))
                m.torch = proxy
            orig = getattr(m, "R", None)
            if callable(orig):
                saved.append((m, "R", orig))
                m.R = _guarded_inputs(orig, proxy)
        yield g
    finally:
        for m, name, value in reversed(saved):
            setattr(m, name, value)
        g.records = []
        _clear_ops_caches()


def _guarded_inputs(orig, proxy):
    def R(*args, **kw):
        t = orig(*args, **kw)
        out = proxy.empty(t.shape, dtype=t.dtype, device=t.device)
        out.copy_(t)
        return out
    R.__wrapped__ = orig
    return R


# per test file: tests run under the guard / outside it, guarded allocations, pass-through sites with their reasons
TOTALS = {}


def fixture_guard(request, *modules, outside=()):
    """The body of the op-level files' autouse fixtures: ``yield from redzone.fixture_guard(request, ops, kc)``.  verify() runs after the test
    body whether or not it failed (pytest resumes a fixture after a failed body); a broken band is then reported as the test's teardown error
    next to the body's own failure, never instead of it.  ``outside``: names of the tests that capture a graph - they run without the guard."""
    tot = TOTALS.setdefault(os.path.basename(str(request.node.fspath)), {"guarded_tests": 0, "outside": [], "allocations": 0, "passthroughs": {}})
    if request.node.name in outside:
        tot["outside"].append(request.node.name)
        yield None
        return
    with guarded(*modules) as g:
        try:
            yield g
            g.verify()
        finally:
            tot["guarded_tests"] += 1
            tot["allocations"] += g.guarded
            for site, reason in g.passthroughs:
                key = site + ": " + reason
                tot["passthroughs"][key] = tot["passthroughs"].get(key, 0) + 1


def _report():
    path = os.environ.get("TF_REDZONE_REPORT")
    if path and TOTALS:
        worker = os.environ.get("PYTEST_XDIST_WORKER")
        with open(path + ("." + worker if worker else ""), "w") as f:
            json.dump(TOTALS, f, indent=1, sort_keys=True)


atexit.register(_report)      # TF_REDZONE_REPORT=<file>: the per-file totals as JSON when the process ends (one file per xdist worker)
