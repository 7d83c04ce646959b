"""Every header of the C ABI against its table in sapcu_amd/_lib.py, without a GPU: the declared entry points are the table, no
entry point is in two tables (the test hooks of no header included), and every name resolves in the built library with as many
argtypes as the header declares parameters."""
import itertools
import os
import re

import pytest

from abi_tables import HEADERS, ROOT, header_entry_points, parameter_count


def test_the_list_of_headers_is_the_binding_s_and_the_folder_s():
    from sapcu_amd import _lib
    assert [h for h, _ in HEADERS] == [h for h in _lib.TABLES if h is not None]
    assert sorted(h for h, _ in HEADERS) == sorted(os.listdir(os.path.join(ROOT, "include")))
    assert _lib.TABLES[None] is _lib._INTERNAL_SIGNATURES and list(_lib.TABLES)[-1] is None
    for header, table in HEADERS:
        assert getattr(_lib, table) == tuple(_lib.TABLES[header])


@pytest.mark.parametrize("header,table", HEADERS)
def test_the_header_declares_exactly_its_table(header, table):
    from sapcu_amd import _lib
    decl, names = header_entry_points(header), getattr(_lib, table)
    assert decl and set(decl) == set(names) and len(names) == len(set(names))
    lib = _lib.load()
    for name in names:
        assert len(getattr(lib, name).argtypes) == parameter_count(decl[name]), name


def test_no_entry_point_is_in_two_tables():
    from sapcu_amd import _lib
    tables = [(table, set(getattr(_lib, table))) for _, table in HEADERS] + [("_INTERNAL_SIGNATURES", set(_lib._INTERNAL_SIGNATURES))]
    for (na, a), (nb, b) in itertools.combinations(tables, 2):
        assert not a & b, (na, nb, sorted(a & b))
    lib = _lib.load()
    for name, (_, argtypes) in _lib._INTERNAL_SIGNATURES.items():
        assert name.startswith("sapcu_internal_") and len(getattr(lib, name).argtypes) == len(argtypes)


@pytest.mark.parametrize("header", [h for h, _ in HEADERS])
def test_the_looser_pattern_the_tests_used_to_carry_parses_the_same(header):
    """tests/test_mesh_host.py and seven others matched `sapcu_\\w+` greedily; the shared parser is the stricter pattern of
    tests/test_guarded.py.  Same names, same parameter lists, for every header."""
    with open(os.path.join(ROOT, "include", header)) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    loose = {m.group(1): m.group(2) for m in re.finditer(r"\b(sapcu_\w+)\s*\(([^;{]*)\)\s*;", text)}
    assert loose == header_entry_points(header)
