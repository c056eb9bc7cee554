"""The C-ABI library loads without a GPU and exports every symbol include/tsar.h declares."""
import ctypes
import os
import re

import pytest

from tsar_mvs_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "tsar.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(tsar_[a-z0-9_]+)\s*\(", txt)))


def test_header_and_binding_agree():
    assert _declared() == sorted(api.ABI_SYMBOLS)


def _signatures():
    """{name: (return type, argument count)} of every `type name(args);` in the header, comments stripped; the count is the number of
    top-level commas plus one (no declaration nests parentheses), 0 for `void` or nothing"""
    txt = open(os.path.join(ROOT, "include", "tsar.h")).read()
    txt = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    sigs = {}
    for ret, name, args in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[ *]+)(tsar_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        assert name not in sigs, name
        sigs[name] = (ret.replace(" ", ""), 0 if args.strip() in ("", "void") else args.count(",") + 1)
    return sigs


def test_binding_signatures_follow_the_header():
    """every declaration has an _ABI entry, in the header's order, with the header's argument count and return type; load_library
    sets both fields of every function"""
    sigs = _signatures()
    assert sorted(sigs) == _declared()                     # the parse misses no declaration (84 today)
    assert list(api._ABI) == list(sigs) == api.ABI_SYMBOLS
    restypes = {"int": ctypes.c_int, "void": None, "constchar*": ctypes.c_char_p, "void*": ctypes.c_void_p}
    L = api.load_library()
    for name, (ret, n_args) in sigs.items():
        restype, argtypes = api._ABI[name]
        assert len(argtypes) == n_args, (name, len(argtypes), n_args)
        assert restype is restypes[ret], (name, restype, ret)
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    if not os.path.exists(api.LIB_PATH):
        ge.build()
    lib = ctypes.CDLL(api.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), name
    lib.tsar_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.tsar_version()


def test_struct_layouts_match_header():
    assert ctypes.sizeof(api.Camera) == 21 * 4
    assert ctypes.sizeof(api.Params) == 40
    assert ctypes.sizeof(api.SlicSettings) == 20
    assert ctypes.sizeof(api.KernelTiming) == 56
    p = api.default_params()
    assert (p.box_hsize, p.box_vsize, p.n_best, p.cost_comb) == (19, 19, 2, 1)   # reference algorithmparameters.h:21-52


def test_no_cpu_fallback_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(api.TsarError):
        api.Matcher()


def test_chunk_length_of_the_general_window_loop_pads_least():
    """host logic of the general-window tap loop (pm_sweep_lut.hip lut_chunk_taps): a line of T taps is walked in chunks of 4, 5
    or 6; the chosen length pads the line least, the longer chunk on a tie.  No GPU needed: the chooser is host code."""
    import ctypes
    lib = ctypes.CDLL(api.LIB_PATH)
    f = getattr(lib, "_Z14lut_chunk_tapsi")
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int]
    for taps in range(1, 33):
        ch = f(taps)
        assert ch in (4, 5, 6)
        waste = {c: (c - taps % c) % c for c in (4, 5, 6)}
        assert waste[ch] == min(waste.values()), (taps, ch, waste)
        assert all(c <= ch for c in (4, 5, 6) if waste[c] == waste[ch]), (taps, ch, waste)
    assert f(6) == 6 and f(10) == 5 and f(4) == 4 and f(12) == 6 and f(8) == 4      # boxes 11, 19, 7, 23, 15
