"""Poisoned allocations: every buffer the Python layer of sapcu_amd takes from ``torch.empty`` / ``torch.empty_like`` /
``torch.empty_strided`` / ``Tensor.new_empty`` is filled with a known pattern before the product code sees it, so that an
element a kernel reads before anything stored it changes a result instead of passing on whatever the caching allocator
happened to hand back (usually zeros, or the same stale block in both runs of a comparison).

``with poisoned(monkeypatch, "A") as sites:`` — inside the block

* the module-level name ``torch`` of every module of sapcu_amd that imports torch is a proxy: every attribute is the real
  torch's, except ``empty``, ``empty_like`` and ``empty_strided``;
* ``torch.Tensor.new_empty`` is wrapped, and the wrapper acts only when its caller's file lies in the package directory;
* each wrapped call allocates as before, fills the result (``fill``), records its call site as (file name, line) in `sites`
  and in ``REACHED[pattern]``, and returns the result.  A tensor with no elements is returned as it is (its site is recorded:
  the call was reached, there is nothing to read).

torch's own Python code and the tests' own allocations go to the real functions.  Under stream capture the fill is one more
captured kernel on the capturing stream and runs again at every replay.

Two patterns, chosen so that a stray read changes a number and cannot address memory out of range:

    dtype             A                          B
    floating          every byte 0xFF (NaN)      every byte 0x7B (finite: 1.3e36 as f32, 61280 as f16)
    uint8             0xFF                       0x00             (the two tests/guarded.py sends through the C ABI)
    other integers    1                          2                (small: an index table read too early is a wrong
    bool              True                       False             number, never an address outside its tensor)

NaN alone is not enough: ``v > mx`` and ``u > 0`` drop a NaN silently, a large finite value they do not.

``allocation_sites()`` lists the same calls from the package's source with ``ast``; tests/test_poison_host.py keeps the list as
``SITES`` and the last test of tests/test_gpu_poisoned_alloc.py holds ``REACHED`` against it.
"""
import ast
import contextlib
import importlib
import os
import pkgutil
import sys

import torch

PATTERNS = ("A", "B")
FLOAT_BYTE = {"A": 0xFF, "B": 0x7B}
UINT8_VALUE = {"A": 0xFF, "B": 0x00}
INT_VALUE = {"A": 1, "B": 2}
BOOL_VALUE = {"A": True, "B": False}
WRAPPED = ("empty", "empty_like", "empty_strided")

REACHED = {p: set() for p in PATTERNS}          # pattern -> {(file name, line)} over the whole session


def package_dir():
    import sapcu_amd
    return os.path.dirname(os.path.abspath(sapcu_amd.__file__))


def product_modules():
    """Every module of sapcu_amd (all imported here) whose global ``torch`` is the torch module."""
    import sapcu_amd
    for info in pkgutil.iter_modules([package_dir()]):
        importlib.import_module("sapcu_amd." + info.name)
    mods = [m for name, m in sorted(sys.modules.items()) if m is not None and (name == "sapcu_amd" or name.startswith("sapcu_amd."))]
    return [m for m in mods if m.__dict__.get("torch") is torch]


def fill(t, pattern):
    """Write pattern A or B over tensor `t` in place (see the table above) -> t."""
    if pattern not in PATTERNS:
        raise ValueError("pattern must be 'A' or 'B'")
    if t.numel() == 0:
        return t
    with torch.no_grad():
        if t.dtype.is_floating_point or t.dtype.is_complex:
            # the bytes of the storage the allocation owns, whatever the strides (a fresh allocation owns all of it)
            raw = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
            raw.fill_(FLOAT_BYTE[pattern])
        elif t.dtype == torch.uint8:
            t.fill_(UINT8_VALUE[pattern])
        elif t.dtype == torch.bool:
            t.fill_(BOOL_VALUE[pattern])
        else:
            t.fill_(INT_VALUE[pattern])
    return t


class _TorchProxy(object):
    """Stands where a product module's ``torch`` stood: the real module but for the three allocators."""

    def __init__(self, wrapped):
        self.__dict__.update(wrapped)

    def __getattr__(self, name):                 # only reached for names that are not the three allocators
        return getattr(torch, name)


def _site(frame):
    return (os.path.basename(frame.f_code.co_filename), frame.f_lineno)


@contextlib.contextmanager
def poisoned(monkeypatch, pattern):
    """See the module docstring.  -> the set of call sites reached inside the block."""
    if pattern not in PATTERNS:
        raise ValueError("pattern must be 'A' or 'B'")
    pkg = package_dir()
    sites = set()

    def record(frame):
        site = _site(frame)
        sites.add(site)
        REACHED[pattern].add(site)

    def wrap(real):
        def allocate(*args, **kw):
            out = real(*args, **kw)
            record(sys._getframe(1))
            return fill(out, pattern)
        allocate.__name__ = real.__name__
        return allocate

    real_new_empty = torch.Tensor.new_empty

    def new_empty(self, *args, **kw):
        out = real_new_empty(self, *args, **kw)
        frame = sys._getframe(1)
        if os.path.dirname(os.path.abspath(frame.f_code.co_filename)) != pkg:
            return out
        record(frame)
        return fill(out, pattern)

    proxy = _TorchProxy({name: wrap(getattr(torch, name)) for name in WRAPPED})
    with monkeypatch.context() as m:
        for mod in product_modules():
            m.setattr(mod, "torch", proxy)
        m.setattr(torch.Tensor, "new_empty", new_empty)
        yield sites


def allocation_sites():
    """[(file name, first line, last line, function)] of every ``torch.empty`` / ``torch.empty_like`` / ``torch.empty_strided`` call on the name
    ``torch`` and every ``.new_empty(...)`` call in the package's .py files, sorted."""
    pkg = package_dir()
    out = []
    for fname in sorted(os.listdir(pkg)):
        if not fname.endswith(".py"):
            continue
        with open(os.path.join(pkg, fname)) as f:
            tree = ast.parse(f.read(), fname)
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
                continue
            fn = node.func
            if fn.attr in WRAPPED and isinstance(fn.value, ast.Name) and fn.value.id == "torch":
                out.append((fname, node.lineno, node.end_lineno, fn.attr))
            elif fn.attr == "new_empty":
                out.append((fname, node.lineno, node.end_lineno, fn.attr))
    return sorted(out)


def unreached(sites, reached):
    """The entries of `sites` (allocation_sites()) none of whose lines is among the recorded (file name, line) pairs `reached`."""
    return [s for s in sites if not any((s[0], line) in reached for line in range(s[1], s[2] + 1))]
