"""Every header of include/ against its binding table against the library's exports (tests/abi_tables.py has the rows and the
rule): names, counts, parameter counts, parameter and return kinds, no name in two tables, the exports and the ABI numbers.
ctypes converts silently, so a ``c_int`` where the header says ``int64_t`` would truncate a size without any error: the kinds are
held here, for every table.  No GPU.
"""
import ctypes
import os
import re
import subprocess

import pytest

import abi_tables as T

IDS = [row.header for row in T.ROWS]


@pytest.fixture(scope="module")
def exported():
    """(a raw handle of the library, the names it defines itself)"""
    from snvc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    names = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return ctypes.CDLL(_lib.LIB_PATH), set(re.findall(r"\bT (snvc_\w+)$", names, re.M))


def test_the_rows_are_the_headers_of_include():
    assert sorted(IDS) == sorted(os.listdir(os.path.join(T.ROOT, "include"))) and len(set(r.module for r in T.ROWS)) == len(T.ROWS)


@pytest.mark.parametrize("row", T.ROWS, ids=IDS)
def test_header_and_table_agree(row):
    mod, declared = T.module(row), T.declarations(row)
    names = [name for _, name, _ in declared]
    table = mod.SIGNATURES
    assert sorted(names) == sorted(set(names)), f"{row.header} declares twice: {sorted(n for n in set(names) if names.count(n) > 1)}"
    assert set(names) == set(table), f"{row.header} against snvc_amd/{row.module}.py: {sorted(set(names) ^ set(table))}"
    assert len(names) == len(table) == row.count
    assert row.version_symbol in table and mod._ABI == row.abi, f"{row.version_symbol}: {row.module}._ABI is {mod._ABI}, the row says {row.abi}"
    for ret, name, params in declared:
        restype, argtypes = table[name]
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters declared, {len(argtypes)} in the table"
        assert T.return_agrees(ret, restype), f"{name}: returns `{ret}`, the table says {restype.__name__}"
        for i, (param, ctype) in enumerate(zip(params, argtypes)):
            assert T.parameter_agrees(param, ctype), f"{name}: parameter {i} is `{param}`, the table says {ctype.__name__}"
    for other in T.ROWS:            # no name in two tables, none declared by two headers
        if other is not row:
            twice = set(table) & (set(T.module(other).SIGNATURES) | {name for _, name, _ in T.declarations(other)})
            assert not twice, f"{sorted(twice)}: in {row.header}'s table and in {other.header} or its table"


@pytest.mark.parametrize("row", T.ROWS, ids=IDS)
def test_library_exports_the_table_under_its_abi_number(row, exported):
    raw, defined = exported
    mod = T.module(row)
    for name in mod.SIGNATURES:
        assert name in defined and getattr(raw, name), f"{name} is not exported by the library itself"
    bound = mod.lib()               # binds the table: raises on a missing symbol or another ABI number
    assert getattr(bound, row.version_symbol)() == mod._ABI == row.abi, row.version_symbol
