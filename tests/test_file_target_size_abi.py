"""Target-size mode from a file's bytes, and the pool over such files, in the C ABI (no GPU needed): declared by the header,
exported by the built library, fennec_TargetOptions laid out in ctypes as the header lays it out, and every refusal the header
lists answered before a device is touched (the calls below pass no ctx, or a device index no machine has)."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import fennec_amd
from fennec_amd import FNX_TS_ALL, FileOptions, SizeCandidate, TargetOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = fennec_amd.FNX_ERR_INVALID


def _header():
    return open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


@pytest.fixture(scope="module")
def lib():
    return fennec_amd.load_library()


def test_header_declares_and_library_exports_the_entries(lib):
    text = _header()
    for name in ("fennec_CompressFileTargetSize", "fennec_CompressBatchTargetSize"):
        assert re.search(rf"\bint {name}\(", text), name
        assert hasattr(lib, name), name
        assert name in fennec_amd.exported_symbols()
    assert "Target-size mode is a call of its own" not in text
    assert '"jpeg_size"' in text


def test_target_options_layout():
    assert C.sizeof(TargetOptions) == 40 and C.sizeof(FileOptions) == 24
    assert [(n, getattr(TargetOptions, n).offset) for n, _ in TargetOptions._fields_] == [
        ("file", 0), ("target_bytes", 24), ("strategies", 32), ("reserved", 36)]
    body = re.search(r"typedef struct fennec_TargetOptions \{(.*?)\} fennec_TargetOptions;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(fennec_FileOptions|int32_t|int64_t)\s+(\w+);", body)
    assert fields == [("fennec_FileOptions", "file"), ("int64_t", "target_bytes"), ("int32_t", "strategies"), ("int32_t", "reserved")]
    o = TargetOptions.make(1234, orient=6, max_w=64)
    assert (o.file.orient, o.file.max_w, o.file.max_h, o.target_bytes, o.strategies, o.reserved) == (6, 64, 0, 1234, FNX_TS_ALL, 0)


class Call:
    """a complete argument list of fennec_CompressFileTargetSize, every pointer valid"""

    def __init__(self, **opt):
        self.data = np.zeros(64, dtype=np.uint8)
        self.o = TargetOptions.make(opt.pop("target_bytes", 1000), strategies=opt.pop("strategies", FNX_TS_ALL))
        self.o.reserved = opt.pop("reserved", 0)
        self.cand = (SizeCandidate * 4)()
        self.win, self.n = C.c_int(7), C.c_size_t(7)
        self.out = np.zeros(4096, dtype=np.uint8)
        self.dims = (C.c_int * 4)()

    def args(self, **null):
        a = dict(ctx=None, data=self.data.ctypes.data_as(C.POINTER(C.c_uint8)), n=64, opts=C.byref(self.o), cancel=None, cand=self.cand,
                 winner=C.byref(self.win), out=self.out.ctypes.data_as(C.POINTER(C.c_uint8)), cap=4096, nbytes=C.byref(self.n), dims=self.dims)
        a.update(null)
        return list(a.values())


def _err(lib):
    return lib.fnx_last_error().decode()


@pytest.mark.parametrize("which", ["data", "opts", "cand", "winner", "nbytes", "dims", "out"])
def test_file_entry_refuses_a_null_pointer(lib, which):
    c = Call()
    assert lib.fennec_CompressFileTargetSize(*c.args(**{which: None})) == INVALID
    assert "NULL argument" in _err(lib)


@pytest.mark.parametrize("opt", [dict(target_bytes=0), dict(target_bytes=-1), dict(strategies=0), dict(strategies=16),
                                 dict(strategies=-1), dict(strategies=FNX_TS_ALL | 32), dict(reserved=1)])
def test_file_entry_refuses_bad_options_before_the_ctx(lib, opt):
    c = Call(**opt)
    assert lib.fennec_CompressFileTargetSize(*c.args()) == INVALID
    word = {"target_bytes": "target_bytes", "strategies": "strategies", "reserved": "reserved"}[next(iter(opt))]
    assert word in _err(lib) and "ctx" not in _err(lib)
    assert (c.win.value, c.n.value) == (7, 7)                       # nothing was touched


def test_file_entry_with_good_arguments_is_refused_for_the_ctx(lib):
    c = Call()
    assert lib.fennec_CompressFileTargetSize(*c.args()) == INVALID and "ctx" in _err(lib)
    assert lib.fennec_CompressFileTargetSize(*c.args(out=None, cap=0)) == INVALID and "ctx" in _err(lib)      # the size-only form


def _pool_args(default, **null):
    data = np.zeros(64, dtype=np.uint8)
    out = np.zeros(4096, dtype=np.uint8)
    keep = [data, out, default]
    a = dict(device=0, workers=1, n=1, files=(C.c_void_p * 1)(data.ctypes.data), sizes=(C.c_size_t * 1)(64), default_opts=C.byref(default),
             item_opts=None, outs=(C.c_void_p * 1)(out.ctypes.data), caps=(C.c_size_t * 1)(4096), results=(fennec_amd.NativeBatchResult * 1)(),
             cands=None, dims=None, cancel=None, on_item=None, user=None)
    a.update(null)
    return list(a.values()), keep


@pytest.mark.parametrize("which", ["files", "sizes", "default_opts", "outs", "caps", "results"])
def test_pool_refuses_a_null_array(lib, which):
    a, _keep = _pool_args(TargetOptions.make(1000), **{which: None})
    assert lib.fennec_CompressBatchTargetSize(*a) == INVALID and "arrays" in _err(lib)


@pytest.mark.parametrize("opt", [dict(target_bytes=0), dict(strategies=0), dict(strategies=16), dict(reserved=3)])
def test_pool_refuses_bad_default_options_before_it_starts(lib, opt):
    o = TargetOptions.make(opt.get("target_bytes", 1000), strategies=opt.get("strategies", FNX_TS_ALL))
    o.reserved = opt.get("reserved", 0)
    a, _keep = _pool_args(o)
    assert lib.fennec_CompressBatchTargetSize(*a) == INVALID and "default_opts" in _err(lib)


def test_pool_of_nothing_is_ok(lib):
    a, _keep = _pool_args(TargetOptions.make(1000), n=0)
    assert lib.fennec_CompressBatchTargetSize(*a) == fennec_amd.FNX_OK


def test_set_form_knows_jpeg_size_as_it_knows_the_other_names(lib):
    """without a ctx both a known and an unknown name are refused for the ctx; the name's place in the table is the source's"""
    assert lib.fnx_ctx_set_form(None, b"jpeg_size", b"1") == INVALID and "null argument" in _err(lib)
    assert lib.fnx_ctx_set_form(None, b"resize_box", b"1") == INVALID and "null argument" in _err(lib)
    src = open(os.path.join(ROOT, "fennec_amd", "csrc", "runtime.cpp")).read()
    names = re.search(r"FORM_NAMES\[FORM_COUNT\] = \{(.*?)\};", src, flags=re.S).group(1)
    names = re.findall(r'"(\w+)"', names)
    enum = re.search(r"enum Form \{(.*?)\};", open(os.path.join(ROOT, "fennec_amd", "csrc", "common.hpp")).read(), flags=re.S).group(1)
    enum = [e for e in re.findall(r"\b(FORM_\w+)", re.sub(r"//[^\n]*", "", enum)) if e != "FORM_COUNT"]
    assert len(names) == len(enum) and names[-1] == "jpeg_size" and enum[-1] == "FORM_JPEG_SIZE"
    assert [("FORM_" + n.upper()) for n in names] == enum
