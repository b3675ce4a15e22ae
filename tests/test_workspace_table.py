"""Completeness of tests/workspace_cases.py against include/clipfs.h (no GPU): every entry point that takes caller
scratch has a row naming its poison test, or an exemption with a reason; the table names nothing the header lacks; and
the tests and size queries it names exist."""
import ast
import os
import re

import pytest

import workspace_cases as W
from workspace_cases import DOCUMENTED_UNINITIALISED, EXEMPT, TABLE

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def header():
    return W.read_header()


def _uncovered(text):
    return sorted(set(W.scratch_functions(text)) - set(TABLE) - set(EXEMPT))


def test_parser_reads_the_whole_header(header):
    """Every exported symbol the binding resolves is found as a prototype (so that no prototype shape escapes the regex),
    and the scratch parameters of some known entry points are recognised."""
    from clipfs import _lib
    protos = W.prototypes(header)
    assert sorted(set(_lib.SIGNATURES) - set(protos)) == []
    found = W.scratch_functions(header)
    assert [W._param_name(p) for p in found["clipfs_attention_bwd"]] == ["work"]
    assert sorted(W._param_name(p) for p in found["clipfs_tower_fwd"]) == ["saved", "scratch"]
    assert [W._param_name(p) for p in found["clipfs_grad_sumsq"]] == ["work"]
    assert "clipfs_gemm_args" in W.scratch_structs(header) and "clipfs_gemm_nt" in found
    assert "clipfs_attention_fwd" not in found and "clipfs_tower_scratch_floats" not in found


def test_every_scratch_entry_point_is_in_the_table_or_exempt(header):
    assert _uncovered(header) == []


def test_table_names_only_functions_with_scratch(header):
    found = W.scratch_functions(header)
    assert sorted(set(TABLE) - set(found)) == []
    assert sorted(set(EXEMPT) - set(found)) == []
    assert sorted(set(TABLE) & set(EXEMPT)) == []
    assert sorted(set(DOCUMENTED_UNINITIALISED) - set(W.prototypes(header))) == []
    for name, reason in list(EXEMPT.items()) + list(DOCUMENTED_UNINITIALISED.items()):
        assert isinstance(reason, str) and len(reason) > 10, name


def test_rows_name_existing_tests_and_queries(header):
    protos = W.prototypes(header)
    defined = {}
    for name, (query, test) in TABLE.items():
        module, func = test.split("::")
        if module not in defined:
            with open(os.path.join(HERE, module + ".py")) as f:
                defined[module] = {n.name for n in ast.walk(ast.parse(f.read())) if isinstance(n, ast.FunctionDef)}
        assert func in defined[module], (name, test)
        for q in re.findall(r"clipfs_\w+", query):
            assert q in protos, (name, q)


def test_a_new_scratch_parameter_fails_the_check(header):
    """A dummy prototype with a ``float* work`` parameter (and one taking the GEMM descriptor) added to a copy of the
    header text is reported as uncovered."""
    end = header.rindex("#ifdef __cplusplus")
    dummy = ("int clipfs_dummy_op(const float* x, float* y,\n                    float* work, int n, void* stream);\n"
             "int clipfs_dummy_gemm(const clipfs_gemm_args* args, void* stream);\n"
             "int clipfs_dummy_plain(const float* x, float* y, int n, void* stream);\n")
    assert _uncovered(header[:end] + dummy + header[end:]) == ["clipfs_dummy_gemm", "clipfs_dummy_op"]
