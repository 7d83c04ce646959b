"""tests/poison.py on the CPU: the helper changes what an unwritten ``torch.empty`` element reads as — differently under its two
patterns — and nothing else; and the list of the package's allocation sites (``SITES``) that
tests/test_gpu_poisoned_alloc.py must reach under both patterns."""
import sys
import types

import pytest
import torch

import poison

SITES = poison.allocation_sites()


@pytest.fixture
def toy(monkeypatch):
    """A module named like one of the package's (``sapcu_amd._poison_toy``) that imports torch the way they do, and a file name
    inside the package directory for its functions, so that both hooks of the helper see it as product code."""
    import os
    mod = types.ModuleType("sapcu_amd._poison_toy")
    mod.torch = torch
    source = """
def leaky(x):                                   # reads element 3 of a buffer it wrote only elements 0..2 of
    buf = torch.empty((4,), dtype=x.dtype)
    buf[:3] = x[:3]
    return buf.clone()

def sound(x):                                   # writes everything it returns
    buf = torch.empty_like(x)
    buf.copy_(x * 2)
    return buf

def strided(x):
    buf = torch.empty_strided((2, 3), (1, 2), dtype=x.dtype)
    return buf.clone()

def fresh(like, shape):
    return like.new_empty(shape).clone()

def alloc(shape, dtype):
    return torch.empty(shape, dtype=dtype).clone()
"""
    exec(compile(source, os.path.join(poison.package_dir(), "_poison_toy.py"), "exec"), mod.__dict__)
    monkeypatch.setitem(sys.modules, "sapcu_amd._poison_toy", mod)
    return mod


def _bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64, 2: torch.int16}[t.element_size()])


def test_an_unwritten_element_reads_differently_under_a_under_b_and_without_poison(toy, monkeypatch):
    x = torch.tensor([1.0, 2.0, 3.0, 4.0])
    real_new_empty = torch.Tensor.new_empty
    with poison.poisoned(monkeypatch, "A") as sa:
        assert torch.Tensor.new_empty is not real_new_empty and toy.torch is not torch
        a = toy.leaky(x)
        a2 = toy.sound(x)
    with poison.poisoned(monkeypatch, "B") as sb:
        b = toy.leaky(x)
        b2 = toy.sound(x)
    assert toy.torch is torch and torch.Tensor.new_empty is real_new_empty      # both hooks are gone again
    assert torch.equal(a[:3], x[:3]) and torch.equal(b[:3], x[:3])
    assert int(_bits(a)[3]) == -1 and bool(torch.isnan(a[3]))                                  # every byte 0xFF
    assert int(_bits(b)[3]) == 0x7B7B7B7B and 1.2e36 < float(b[3]) < 1.4e36                    # every byte 0x7B
    clean = torch.zeros(4)
    clean[:3] = x[:3]                                                                           # what a zeroed block gives
    assert not torch.equal(_bits(a), _bits(b)) and not torch.equal(_bits(a), _bits(clean)) and not torch.equal(_bits(b), _bits(clean))
    assert torch.equal(a2, x * 2) and torch.equal(b2, x * 2) and torch.equal(toy.sound(x), x * 2)
    assert sa == sb and {f for f, _ in sa} == {"_poison_toy.py"} and len(sa) == 2
    assert sa <= poison.REACHED["A"] and sb <= poison.REACHED["B"]


def test_every_dtype_gets_its_pattern(toy, monkeypatch):
    want = {"A": {torch.uint8: 0xFF, torch.int32: 1, torch.int64: 1, torch.bool: True},
            "B": {torch.uint8: 0x00, torch.int32: 2, torch.int64: 2, torch.bool: False}}
    for pattern in poison.PATTERNS:
        with poison.poisoned(monkeypatch, pattern):
            for dtype, value in want[pattern].items():
                got = toy.alloc((5, 3), dtype)
                assert got.dtype == dtype and got.shape == (5, 3) and bool((got == value).all()), (pattern, dtype)
            h = toy.alloc((7,), torch.float16)
            d = toy.alloc((7,), torch.float64)
            s = toy.strided(torch.zeros(1))
            n = toy.fresh(torch.zeros(2, dtype=torch.float64), (3, 2))
        byte = poison.FLOAT_BYTE[pattern]
        for t in (h, d, s, n):
            assert bool((t.contiguous().view(torch.uint8) == byte).all()), (pattern, t.dtype)
        assert s.shape == (2, 3) and n.shape == (3, 2) and n.dtype == torch.float64
        if pattern == "B":
            assert float(h[0]) == 61280.0 and bool(torch.isfinite(d).all()) and float(d[0]) > 1e280
        else:
            assert bool(torch.isnan(h).all()) and bool(torch.isnan(d).all())


def test_empty_tensors_and_foreign_callers_are_left_alone(toy, monkeypatch):
    with poison.poisoned(monkeypatch, "A") as sites:
        z = toy.alloc((0, 3), torch.float32)
        zn = toy.fresh(torch.zeros(1), (0,))
        assert len(sites) == 2                                     # reached and recorded, nothing to fill
        mine = torch.zeros(3).new_empty((4,))                      # this file is not in the package: the real new_empty
        theirs = torch.empty((4,), dtype=torch.int32)              # and this module's torch is the real one
        assert len(sites) == 2
    assert z.shape == (0, 3) and zn.shape == (0,) and mine.shape == (4,) and theirs.shape == (4,)
    with pytest.raises(ValueError):
        with poison.poisoned(monkeypatch, "C"):
            pass
    with pytest.raises(ValueError):
        poison.fill(torch.zeros(1), "C")


def test_the_proxy_is_torch_for_everything_else(monkeypatch):
    import sapcu_amd.train as train
    mods = poison.product_modules()
    names = {m.__name__ for m in mods}
    assert {"sapcu_amd.train", "sapcu_amd.fd_train", "sapcu_amd.generation", "sapcu_amd.modules", "sapcu_amd.dist", "sapcu_amd.pipeline",
            "sapcu_amd.train_step"} <= names
    with poison.poisoned(monkeypatch, "B"):
        proxy = train.torch
        assert proxy is not torch and all(m.torch is proxy for m in mods)
        assert proxy.float32 is torch.float32 and proxy.nn is torch.nn and proxy.Tensor is torch.Tensor and proxy.zeros is torch.zeros
        assert proxy.empty is not torch.empty and proxy.empty_like is not torch.empty_like and proxy.empty_strided is not torch.empty_strided
    assert all(m.torch is torch for m in mods)


def test_the_site_list():
    """Every ``torch.empty`` / ``empty_like`` / ``empty_strided`` / ``.new_empty`` call of the package, by file."""
    by_file = {}
    for fname, line, last, func in SITES:
        by_file.setdefault(fname, []).append((line, func))
    for fname in sorted(by_file):
        print("%-16s %2d  %s" % (fname, len(by_file[fname]), " ".join("%d:%s" % s for s in by_file[fname])))
    print("%d sites" % len(SITES))
    # the files that hand raw pointers to the HIP library all allocate this way; a count of zero means the walk is broken
    for fname in ("dist.py", "fd_train.py", "generation.py", "modules.py", "pipeline.py", "train.py", "train_step.py"):
        assert by_file.get(fname), fname
    assert len(SITES) >= 80 and all(last >= line > 0 for _, line, last, _ in SITES)
    assert {func for _, _, _, func in SITES} <= {"empty", "empty_like", "empty_strided", "new_empty"}
    assert ("dist.py", "new_empty") in {(f, func) for f, _, _, func in SITES}
    assert poison.unreached(SITES, set()) == SITES
    assert poison.unreached(SITES, {(f, last) for f, _, last, _ in SITES}) == []
