"""The C-ABI shared library loads and exports every symbol include/ctd_hip.h
declares; the ctypes struct mirrors have the C layout (no compute calls here)."""
import ctypes as C
import keyword
import os
import re

import numpy as np
import pytest

from c_layout import compiled
from conftest import ROOT, pkg

HEADER = os.path.join(ROOT, "include", "ctd_hip.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ctd_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    L = pkg()._lib
    if not os.path.isfile(L.LIB_PATH):
        L.build()
    lib = L.lib()
    names = declared_functions()
    assert len(names) >= 16
    for n in names:
        assert hasattr(lib, n), f"{n} declared in ctd_hip.h but not exported"
    assert sorted(L.SYMBOLS) == names, "python binding table and header disagree"
    assert lib.ctd_abi_version() == L.ABI_VERSION


def test_struct_layout_matches_c():
    L = pkg()._lib
    sizes, offsets, _ = compiled({"ctd_tensor": (), "ctd_op": ("w_off", "b_off", "aux", "faux")})
    assert [sizes["ctd_tensor"], sizes["ctd_op"]] + offsets["ctd_op"] == \
        [C.sizeof(L.CtdTensor), C.sizeof(L.CtdOp), L.CtdOp.w_off.offset, L.CtdOp.b_off.offset, L.CtdOp.aux.offset, L.CtdOp.faux.offset]


def test_every_ctypes_structure_has_the_c_layout():
    """EVERY `ctypes.Structure` of `_lib` against the header, compiled: its size and the offset of every field, under the
    header's own field names.  The numpy table dtypes are derived from these mirrors (`pagecall.table_dtype`), so a wrong
    mirror would be inherited silently; a structure added to `_lib` is checked here without anybody listing it, and a struct
    the header gains needs its mirror."""
    L = pkg()._lib
    mirrors = {re.sub(r"(?<!^)(?=[A-Z])", "_", name).lower(): cls for name, cls in vars(L).items()
               if isinstance(cls, type) and issubclass(cls, C.Structure) and cls is not C.Structure}
    assert len(mirrors) >= 33
    assert sorted(mirrors) == sorted(re.findall(r"^\} (ctd_[a-z0-9_]+);", open(HEADER).read(), flags=re.M))
    c_name = lambda f: f[:-1] if f.endswith("_") and keyword.iskeyword(f[:-1]) else f     # noqa: E731  (`pass_` is C's `pass`)
    sizes, offsets, _ = compiled({s: [c_name(f[0]) for f in cls._fields_] for s, cls in mirrors.items()})
    for s, cls in mirrors.items():
        names = [f[0] for f in cls._fields_]
        assert sizes[s] == C.sizeof(cls), s
        assert offsets[s] == [getattr(cls, f).offset for f in names], s
        dt = np.dtype(cls)                                   # what `pagecall.table_dtype` hands the modules
        assert dt.itemsize == sizes[s] and list(dt.names) == names and [dt.fields[f][1] for f in names] == offsets[s], s


def test_engine_create_rejects_bad_program_without_gpu_compute():
    """Error convention: negative rc + message, no exception across the ABI."""
    L = pkg()._lib
    lib = L.lib()
    h = C.c_void_p()
    rc = lib.ctd_engine_create(C.byref(h), None, 0, None, 0, None, 0, L.PREC_F16, 0)
    assert rc == -1 and b"null" in lib.ctd_last_error()


def test_backend_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = pkg()
    with pytest.raises(p._lib.CtdError):
        p.backend.HipTextDetBackend(p.synth.make_checkpoint(0))
