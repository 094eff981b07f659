"""The C-ABI boundary, without a GPU: the library builds, loads, and exports every
symbol include/mfs.h declares; the ctypes table matches the header; argument
validation fails loudly before anything touches a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "mfs.h")


def _declared():
    """function name -> number of parameters, parsed from the header."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(mfs_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        name, args = m.group(1), m.group(2).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        out[name] = n
    return out


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mfs import _lib
    return _lib.load()


def test_header_is_plain_c():
    # the header must compile as C (extern "C" boundary, no C++/torch types)
    r = subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-x", "c", HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_every_declared_symbol_is_exported(lib):
    from mfs import _lib
    decl = _declared()
    assert len(decl) >= 20
    for name, nargs in decl.items():
        assert hasattr(lib, name), f"{name} declared in mfs.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert len(_lib.SIGNATURES[name][1]) == nargs, f"{name}: header has {nargs} parameters"
    assert set(_lib.SIGNATURES) == set(decl)


def test_engine_classes_form_only_declared_names():
    """mfs/engine.py forms the shared entry points' names from a class's C prefix: a typo there would otherwise show
    only at the first call on a GPU"""
    from mfs import _lib
    from mfs.pcg import Pcg2dEngine, PcgEngine
    from mfs.vcg import Vcg2dEngine, VcgEngine
    for cls, prefix, n in ((PcgEngine, "mfs_pcg3d", 8), (VcgEngine, "mfs_vcg3d", 11), (Pcg2dEngine, "mfs_pcg2d", 7),
                           (Vcg2dEngine, "mfs_vcg2d", 10)):
        names = cls.c_names()
        assert len(set(names)) == n and all(name.startswith(prefix + "_") for name in names), (cls, names)
        missing = [name for name in names if name not in _lib.SIGNATURES]
        assert not missing, (cls.__name__, missing)


def test_abi_version_and_error_text(lib):
    from mfs import _lib
    assert lib.mfs_abi_version() == _lib.ABI_VERSION
    g = _lib.i64x((8, 8, 8))
    # null arrays are rejected before any launch; message names the problem
    st = lib.mfs_solid_frac3d(g, None, 1, None, None, None, 1, None)
    assert st == -1
    assert b"null" in lib.mfs_last_error()
    st = lib.mfs_pressure_apply3d(_lib.i64x((0, 8, 8)), None, None, 1, None, None, None, 1, None, 1, None)
    assert st == -1
    assert lib.mfs_pcg3d_workspace_bytes(g, 7) == 0
    assert lib.mfs_pcg3d_workspace_bytes(g, 0) > 4 * 8 * 8 * 8 * 4


def test_product_path_has_no_cpu_fallback():
    """CPU tensors are refused, loudly -- the solver path is GPU only."""
    import torch
    from solver.SolidFraction3D import compute_solid_frac
    with pytest.raises(TypeError, match="GPU"):
        compute_solid_frac((4, 4, 4), torch.zeros(9, 9, 9, dtype=torch.float64), torch.zeros(5, 4, 4),
                           torch.zeros(4, 5, 4), torch.zeros(4, 4, 5))


def test_product_never_imports_oracle():
    """oracle/ is test infrastructure: nothing under the package may import it."""
    pkg = os.path.join(REPO, "python-fluid-simulation_amd")
    bad = []
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(root, f), errors="replace").read()
                if re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M) or "mfs_oracle" in txt:
                    bad.append(os.path.join(root, f))
    assert not bad, bad
