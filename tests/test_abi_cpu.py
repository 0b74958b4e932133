"""_lib.PROTOTYPES against include/rsa.h, types included: every prototype of the header is parsed and each parameter must map to
the ctypes type the table gives it.  One c_int where the header says int64_t or size_t shifts every later argument of a call, and
a name-by-name comparison does not see it.  Needs neither the library nor a GPU."""
import ctypes
import os
import re

import pytest

from rectified_spaattn_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rsa.h")
SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double, "rsa_tensor4": _lib.RsaTensor4, "rsa_out4": _lib.RsaOut4}
STRUCTS = {"rsa_layout": _lib.RsaLayout, "rsa_layout_ex": _lib.RsaLayoutEx, "rsa_buffers": _lib.RsaBuffers,
           "rsa_fp8_operands": _lib.RsaFp8Operands}
RETURNS = {"int": ctypes.c_int, "const char*": ctypes.c_char_p}


def parse(text):
    """Header text -> {name: (return type, [parameter declarations])}, comments stripped; (void) is []."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for ret, name, params in re.findall(r"\b(int|const char\*)\s+(rsa_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in out, name
        params = " ".join(params.split())
        out[name] = (ret, [] if params == "void" else [p.strip() for p in params.split(",")])
    return out


def is_pointer_type(t):
    return t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def mismatch(decl, ctype):
    """None if the ctypes type serves the C parameter declaration, else what was expected."""
    words = [w for w in decl.replace("*", " * ").replace("[", " [").split() if w != "const"]
    base = words[0]
    if "*" not in words and "[" not in decl:
        return None if len(words) == 2 and ctype is SCALARS.get(base) else f"{SCALARS.get(base)}"
    if base == "char" and words.count("*") == 1:
        return None if ctype is ctypes.c_char_p else "c_char_p"
    if base in STRUCTS:
        return None if ctype is ctypes.POINTER(STRUCTS[base]) else f"POINTER({STRUCTS[base].__name__})"
    return None if is_pointer_type(ctype) else "a ctypes pointer type"


def faults(prototypes, header):
    """Every disagreement between a prototype table and the parsed header, as strings."""
    out = [f"{n}: only in the table" for n in sorted(set(prototypes) - set(header))]
    out += [f"{n}: only in the header" for n in sorted(set(header) - set(prototypes))]
    for name in sorted(set(prototypes) & set(header)):
        restype, argtypes = prototypes[name]
        ret, params = header[name]
        if restype is not RETURNS[ret] or restype not in (ctypes.c_int, ctypes.c_char_p):
            out.append(f"{name}: returns {ret}, the table says {restype}")
        if len(argtypes) != len(params):
            out.append(f"{name}: {len(params)} parameters, the table has {len(argtypes)}")
            continue
        for i, (decl, ctype) in enumerate(zip(params, argtypes)):
            want = mismatch(decl, ctype)
            if want is not None:
                out.append(f"{name}: parameter {i} `{decl}` needs {want}, the table says {ctype}")
    return out


@pytest.fixture(scope="module")
def header():
    with open(HEADER) as f:
        return parse(f.read())


def test_the_parser_reads_the_header(header):
    assert len(header) >= 77 and all(n.startswith("rsa_") for n in header)
    assert header["rsa_version"] == ("int", []) and header["rsa_last_hip_error"] == ("const char*", [])
    assert header["rsa_abi_check"] == ("int", ["int header_version", "size_t sizeof_rsa_buffers", "size_t sizeof_rsa_layout"])
    assert header["rsa_buffer_bytes"][1][1] == "size_t sizes[RSA_NUM_BUFFERS]"
    assert len(header["rsa_block_sparse_decode"][1]) == 28 and header["rsa_pool_keys"][1][9] == "int64_t table_stride_b"
    with open(HEADER) as f:      # nothing that looks like a prototype was left out: every `rsa_x(` of the code is one
        code = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))
    assert set(re.findall(r"\b(rsa_\w+)\s*\(", code)) == set(header)


def test_every_prototype_of_the_header_is_in_the_table_with_its_types(header):
    assert set(_lib.PROTOTYPES) == set(header)
    assert _lib.EXPORTED == tuple(_lib.PROTOTYPES)
    assert faults(_lib.PROTOTYPES, header) == []


def test_the_check_sees_one_wrong_type_and_one_missing_parameter(header):
    """The two slips the table invites: an int for an int64_t, and a dropped parameter."""
    table = dict(_lib.PROTOTYPES)
    restype, args = table["rsa_pool_keys"]
    at = args.index(ctypes.c_int64)
    table["rsa_pool_keys"] = (restype, args[:at] + [ctypes.c_int] + args[at + 1:])
    assert faults(table, header) == [f"rsa_pool_keys: parameter {at} `int64_t table_stride_b` needs {ctypes.c_int64}, "
                                     f"the table says {ctypes.c_int}"]
    table = dict(_lib.PROTOTYPES)
    restype, args = table["rsa_block_select"]
    table["rsa_block_select"] = (restype, args[:-1])
    assert faults(table, header) == ["rsa_block_select: 26 parameters, the table has 25"]
    table = dict(_lib.PROTOTYPES, rsa_status_string=(ctypes.c_int, [ctypes.c_int]))
    assert faults(table, header) == [f"rsa_status_string: returns const char*, the table says {ctypes.c_int}"]
    table = {n: p for n, p in _lib.PROTOTYPES.items() if n != "rsa_rel_l1"}
    assert faults(table, header) == ["rsa_rel_l1: only in the header"]
