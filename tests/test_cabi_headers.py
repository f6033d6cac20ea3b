"""Every header of include/ against its table in ``_hip.HEADERS``, one case per header: the declared entry points and their parameter
counts, the library's exports, the header as plain C and C++, and what binding refuses of a library that lacks the header's symbols.
Then, over all headers at once: the tables are disjoint and cover include/, the binding's ``XDE_*`` constants are the headers'
``#define``s, and the four small struct mirrors have their header's fields.  No GPU and no compute call here."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from paddlexde_amd import _hip

from .test_cabi import _fake_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _text(header):
    return open(os.path.join(INCLUDE, header)).read()


def _code(header):
    """The header without its /* */ comments (they name entry points of their own and of other headers)."""
    return re.sub(r"/\*.*?\*/", "", _text(header), flags=re.S)


@pytest.mark.parametrize("header", list(_hip.HEADERS))
def test_the_header_declares_what_its_table_binds_and_the_library_exports_it(header):
    src, table = _code(header), _hip.HEADERS[header]
    assert sorted(set(re.findall(r"\b(xde_[a-z_0-9]+)\s*\(", src))) == sorted(table)
    lib = _hip.load_library()
    for sym, (_, argtypes) in table.items():
        params = re.search(r"\b{}\s*\(([^)]*)\)".format(sym), src).group(1).strip()
        if params in ("", "void"):
            assert argtypes is None or argtypes == [], sym
        else:
            assert argtypes is not None and len(params.split(",")) == len(argtypes), sym
        assert hasattr(lib, sym), sym


@pytest.mark.parametrize("header", list(_hip.HEADERS))
def test_the_header_is_plain_c(header):
    """A header is the boundary a foreign host binds: valid C99 and C++11 on its own, warnings included."""
    for cc, lang, std in (("gcc", "c", "c99"), ("g++", "c++", "c++11")):
        r = subprocess.run([cc, "-x", lang, "-std=" + std, "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE,
                            os.path.join(INCLUDE, header)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("header", list(_hip.HEADERS))
def test_binding_refuses_a_library_that_lacks_the_header_s_symbols(header):
    """A stale library is refused at load, by the first symbol it lacks in table order: a missing header by its first symbol, and
    any one missing symbol (the header's last included) by its own name."""
    table = list(_hip.HEADERS[header])
    _hip._bind(_fake_library())
    for missing in [table] + [[sym] for sym in table]:
        with pytest.raises(_hip.XdeError) as e:
            _hip._bind(_fake_library(missing=missing))
        assert "does not export {}: it is stale".format(missing[0]) in str(e.value) and "rebuild" in str(e.value), (missing, str(e.value))


def test_the_tables_cover_include_and_share_no_symbol():
    assert sorted(_hip.HEADERS) == sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, "*.h")))
    assert list(_hip.HEADERS)[0] == "xde_hip.h"  # (the ABI and layout queries _bind starts with are its first symbols)
    flat = [sym for table in _hip.HEADERS.values() for sym in table]
    assert len(flat) == len(set(flat))
    assert list(_hip.PROTOTYPES) == flat and len(_hip.PROTOTYPES) == sum(len(table) for table in _hip.HEADERS.values())
    assert all(_hip.PROTOTYPES[sym] is table[sym] for table in _hip.HEADERS.values() for sym in table)


# header -> the headers whose entry points its COMMENTS cite (what it builds on); everywhere else a header's text is held clear
_CITES = {"xde_hip_cde.h": {"xde_hip.h"}, "xde_hip_seam.h": {"xde_hip.h"}, "xde_hip_spline.h": {"xde_hip.h", "xde_hip_cde.h"},
          "xde_hip_cdegrad.h": {"xde_hip.h", "xde_hip_cde.h", "xde_hip_spline.h"}, "xde_hip_kl.h": {"xde_hip_sde.h"},
          "xde_hip_gn.h": {"xde_hip_sde.h"}, "xde_hip_rows.h": {"xde_hip.h"}}


def test_no_header_names_another_header_s_entry_point():
    """Outside its comments no header names an entry point of another table; with them, only of the headers ``_CITES`` gives it
    (none cites one bound after it, and none names an entry point of xde_hip_kl.h, _gn.h or _rows.h)."""
    order = list(_hip.HEADERS)
    assert all(order.index(cited) < order.index(header) for header, cites in _CITES.items() for cited in cites)
    assert not {"xde_hip_kl.h", "xde_hip_gn.h", "xde_hip_rows.h"} & set().union(*_CITES.values())
    for header in order:
        text, code = _text(header), _code(header)
        for other, table in _hip.HEADERS.items():
            if other != header:
                assert not [sym for sym in table if re.search(r"\b{}\b".format(sym), code)], (header, other)
                if other not in _CITES.get(header, ()):
                    assert not [sym for sym in table if sym in text], (header, other)


def test_the_binding_s_constants_are_the_headers_defines():
    """Every module-level ``XDE_*`` integer of the binding is the integer literal one header ``#define``s under that name."""
    defines = {}
    for header in _hip.HEADERS:
        for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(XDE_\w+)[ \t]+(.+?)[ \t]*$", _code(header), flags=re.M):
            assert name not in defines, (name, header)
            defines[name] = value
    mirrored = {name: value for name, value in vars(_hip).items() if name.startswith("XDE_") and isinstance(value, int)}
    assert len(mirrored) >= 23 and "XDE_BP_MAX_X" in mirrored
    for name, value in mirrored.items():
        assert name in defines, name
        if name == "XDE_BP_MAX_X":  # (the one constant that is an expression, in both places)
            assert defines[name] == "(XDE_MAX_K + 2)" and value == int(defines["XDE_MAX_K"]) + 2
        else:
            assert re.fullmatch(r"\d+", defines[name]) and int(defines[name]) == value, (name, defines[name], value)
    assert int(defines["XDE_ABI_VERSION"]) == _hip.ABI_VERSION


_CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32}


@pytest.mark.parametrize("header, struct, mirror, n_fields, size", [
    ("xde_hip_cde.h", "xde_cde_plan_t", _hip.XdeCdePlan, 12, 10 * 4 + 2 * 8),
    ("xde_hip_seam.h", "xde_seam_plan_t", _hip.XdeSeamPlan, 4, None),
    ("xde_hip_cdegrad.h", "xde_cdegrad_plan_t", _hip.XdeCdeGradPlan, 7, None),
    ("xde_hip_rows.h", "xde_rows_ctl_t", _hip.XdeRowsCtl, 16, None)],
    ids=["XdeCdePlan", "XdeSeamPlan", "XdeCdeGradPlan", "XdeRowsCtl"])
def test_the_struct_mirror_has_the_header_s_fields(header, struct, mirror, n_fields, size):
    """Field for field, in order: the names, and the type each C type maps to (an integer type to its ctypes twin, a pointer to
    ``c_void_p``: the planes of the per-row control block go in as addresses)."""
    body = re.search(r"typedef struct \w+ \{{(.*?)\}} {};".format(struct), _code(header), flags=re.S).group(1)
    want = []
    for ctype, names in re.findall(r"(\w+\s*\*?)\s*([^;*]+);", body):
        want += [(name.strip(), C.c_void_p if ctype.endswith("*") else _CTYPES[ctype.strip()]) for name in names.split(",")]
    assert want == list(mirror._fields_) and len(want) == n_fields
    if size is not None:
        assert C.sizeof(mirror) == size
