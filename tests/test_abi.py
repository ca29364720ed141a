"""The C ABI against its Python binding (no GPU needed): every prototype of include/*.h <=> its
entry of blindno._lib.ABI <=> the loaded library, by name, argument kinds and return type.

A new entry point is a prototype in a header and one line of _lib.ABI; COUNTS below then changes by
one for that header, and nothing else in the tests pins a header to its entries.
"""
import ctypes
import functools
import glob
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
# header -> number of entry points it declares (225 in all)
COUNTS = {"blindno.h": 159, "blindno_bag3d.h": 4, "blindno_bagattn_mix.h": 7, "blindno_conv3d.h": 6,
          "blindno_fpe.h": 2, "blindno_fpe_err.h": 2, "blindno_gpe2d.h": 4, "blindno_gpe2d_err.h": 3,
          "blindno_gpe3d.h": 4, "blindno_gpe3d_err.h": 3, "blindno_nioattn.h": 7, "blindno_physattn.h": 9,
          "blindno_planemlp.h": 5, "blindno_unet3d.h": 10}
PROTOTYPE = re.compile(r"^(int|int64_t|const char\s*\*)\s+(blindno_\w+)\s*\(([^)]*)\)\s*;", re.M)
ARG_CODE = {"int": "i", "int64_t": "l", "float": "f", "double": "d", "blindno_stream_t": "s"}
RET_CODE = {"int": "", "int64_t": "l", "constchar*": "z"}
ARG_CTYPE = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_int64, "f": ctypes.c_float,
             "d": ctypes.c_double, "s": ctypes.c_void_p}
RET_CTYPE = {"": ctypes.c_int, "l": ctypes.c_int64, "z": ctypes.c_char_p}


def _text(header):
    return open(os.path.join(INCLUDE, header)).read()


@functools.lru_cache(maxsize=None)
def _declared(header):
    """{name: (return code, argument codes)} of a header's prototypes, comments stripped."""
    txt = re.sub(r"/\*.*?\*/", " ", _text(header), flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    out = {}
    for ret, name, args in PROTOTYPE.findall(txt):
        assert name not in out, (header, name, "declared twice")
        codes = ""
        for a in (a.strip() for a in args.split(",")):
            if "*" in a:
                codes += "p"
            elif a not in ("", "void"):
                words = [w for w in a.split() if w != "const"]
                assert words[0] in ARG_CODE and len(words) <= 2, (header, name, a, "unrecognised argument type")
                codes += ARG_CODE[words[0]]
        out[name] = (RET_CODE[re.sub(r"\s", "", ret)], codes)
    # nothing that looks like an entry point escaped the pattern (another return type, a macro prefix)
    assert len(re.findall(r"\bblindno_\w+\s*\(", txt)) == len(out), header
    return out


@pytest.mark.parametrize("header", list(COUNTS))
def test_prototypes_match_the_table(header):
    from blindno import _lib
    if header != "blindno.h":
        assert f'#include "{header}"' in _text("blindno.h")
    decl, table = _declared(header), _lib.ABI[header]
    assert sorted(decl) == sorted(table), (header, sorted(set(decl) ^ set(table)))
    assert len(decl) == COUNTS[header], (header, len(decl))
    for name, (ret, codes) in decl.items():
        assert _lib.signature(name) == (codes, ret), (header, name, table[name], codes + (">" + ret if ret else ""))


@pytest.mark.parametrize("header", list(COUNTS))
def test_library_is_typed_as_the_table_says(header):
    import blindno
    from blindno import _lib
    lib = blindno.load_library()
    for name in _lib.ABI[header]:
        codes, ret = _lib.signature(name)
        assert hasattr(lib, name), (header, name)
        fn = getattr(lib, name)
        assert list(fn.argtypes) == [ARG_CTYPE[c] for c in codes], (header, name, fn.argtypes)
        assert fn.restype is RET_CTYPE[ret], (header, name, fn.restype)


def test_every_name_sits_under_one_header(monkeypatch):
    from blindno import _lib
    assert sorted(_lib.ABI) == sorted(COUNTS) == sorted(os.path.basename(p) for p in glob.glob(INCLUDE + "/*.h"))
    assert list(_lib.ABI)[0] == "blindno.h"
    seen = {}
    for header, table in _lib.ABI.items():
        for name in table:
            assert name not in seen, (name, seen[name], header)
            seen[name] = header
    exported = _lib.exported_symbols()
    assert len(exported) == len(set(exported)) == sum(COUNTS.values()) == 225 and set(exported) == set(seen)
    assert _lib.signature("blindno_gpe3d_scratch_doubles") == ("iiii", "l")
    assert _lib.signature("blindno_error_string") == ("i", "z")
    with pytest.raises(KeyError):
        _lib.signature("blindno_no_such_entry")
    monkeypatch.setitem(_lib.ABI, "blindno_twice.h", {"blindno_abi_version": ""})
    with pytest.raises(KeyError):
        _lib.signature("blindno_abi_version")


def test_library_exports_nothing_undeclared():
    """Every defined blindno_* symbol of the library's dynamic table is declared in a header."""
    from blindno import _lib
    nm = shutil.which("nm") or shutil.which("llvm-nm") or next(
        (p for p in ("/opt/rocm/llvm/bin/llvm-nm", "/opt/rocm/lib/llvm/bin/llvm-nm") if os.path.exists(p)), None)
    if nm is None:
        pytest.skip("neither nm nor llvm-nm found")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split() and ln.split()[-1].startswith("blindno_")}
    declared = {name for header in COUNTS for name in _declared(header)}
    assert len(exported) >= 225 and exported <= declared, sorted(exported - declared)


def test_version_and_host_only_queries():
    import blindno
    from blindno import _lib
    lib = blindno.load_library()
    assert lib.blindno_abi_version() >= 2
    # host-only size queries work without a device
    assert _lib.query("blindno_project_bwd_nchunk", 4, 128, 128) >= 1
    assert _lib.query("blindno_lift_bwd_nchunk", 4, 128, 128) >= 1


def test_pinned_entries_and_their_relations():
    """What the per-header tests used to say about particular entries."""
    from blindno import _lib
    sig, ABI = _lib.signature, _lib.ABI
    assert len(_declared("blindno.h")) >= 20
    # the solvers and their record-free error forms: the solver's arguments in its order, the grids
    # after kappa, and group, err in place of the four outputs; 3D = 2D with dz and nz (and z) added
    solve2, solve3 = sig("blindno_gpe2d_solve")[0], sig("blindno_gpe3d_solve")[0]
    err2, err3 = sig("blindno_gpe2d_error")[0], sig("blindno_gpe3d_error")[0]
    assert solve2 == "pppp" + "ddd" + "iii" + "pipp" + "p" + "iiii" + "s"
    assert solve3 == "pppp" + "dddd" + "iii" + "pipp" + "p" + "iiiii" + "s"
    assert err2 == "pppp" + "pp" + "ddd" + "iii" + "i" + "p" + "p" + "iiii" + "s"
    assert err3 == "pppp" + "ppp" + "dddd" + "iii" + "i" + "p" + "p" + "iiiii" + "s"
    assert err2 == solve2.replace("ppppddd", "pppp" + "pp" + "ddd").replace("pippp", "ip" + "p")
    assert err3 == solve3.replace("ppppdddd", "pppp" + "ppp" + "dddd").replace("pippp", "ip" + "p")
    assert len(solve3) == len(solve2) + 2
    assert len(sig("blindno_trapz3_frames")[0]) == len(sig("blindno_trapz2_frames")[0]) + 2
    # the Fokker-Planck error entry: the propagator's argument list with `group` after B
    assert sig("blindno_fp_error_nd")[0] == "pppp" + "iiiiiiii" + "d" + "s" == \
        sig("blindno_fp_propagate_nd")[0].replace("ppppi", "ppppii", 1)
    for name in ("blindno_fp_error_nd_scratch_doubles", "blindno_gpe2d_error_scratch_doubles",
                 "blindno_gpe2d_error_launches", "blindno_gpe3d_error_scratch_doubles",
                 "blindno_gpe3d_error_launches", "blindno_project_bag3d_stats_floats"):
        assert sig(name)[1] == "l", name
    assert sig("blindno_gpe2d_error")[1] == sig("blindno_gpe3d_error")[1] == ""
    assert sig("blindno_conv2d_wscratch_floats")[1] == ""          # declared int: not every *_floats is 64-bit
    # the error entries live in their own headers: the solvers' and the propagator's do not name them
    for header, word in [("blindno_gpe3d.h", "blindno_gpe3d_error"), ("blindno_gpe2d.h", "blindno_gpe2d_error"),
                         ("blindno_fpe.h", "blindno_fp_error")]:
        assert word not in _text(header), header
    assert sorted(ABI["blindno_fpe_err.h"]) == ["blindno_fp_error_nd", "blindno_fp_error_nd_scratch_doubles"]
    assert sorted(ABI["blindno_gpe2d_err.h"]) == ["blindno_gpe2d_error", "blindno_gpe2d_error_launches",
                                                  "blindno_gpe2d_error_scratch_doubles"]
    assert sorted(ABI["blindno_gpe3d_err.h"]) == ["blindno_gpe3d_error", "blindno_gpe3d_error_launches",
                                                  "blindno_gpe3d_error_scratch_doubles"]
    assert sorted(ABI["blindno_conv3d.h"]) == sorted(
        ["blindno_conv3d_fwd", "blindno_conv3d_bwd_data", "blindno_conv3d_bwd_weight",
         "blindno_conv3d_fwd_nsplit", "blindno_conv3d_bwd_data_nsplit", "blindno_conv3d_wgrad_nsplit"])
    assert sorted(ABI["blindno_bag3d.h"]) == sorted(
        ["blindno_project_bag3d_fwd", "blindno_project_bag3d_bwd", "blindno_project_bag3d_stats_floats",
         "blindno_project_bag3d_bwd_nchunk"])
    assert {"blindno_gpe2d_solve", "blindno_trapz2_frames"} <= set(ABI["blindno_gpe2d.h"])
    assert {"blindno_gpe3d_solve", "blindno_trapz3_frames"} <= set(ABI["blindno_gpe3d.h"])
    assert {"blindno_nioattn_moments", "blindno_nioattn_fwd", "blindno_nioattn_bwd"} <= set(ABI["blindno_nioattn.h"])
    # the 3D Fourier layer's entries are exactly the `3d` names of blindno.h itself
    assert {n for n in ABI["blindno.h"] if "3d" in n} == {
        "blindno_spectral3d_ok", "blindno_colpass3d", "blindno_pack_w3d", "blindno_unpack_w3d",
        "blindno_lift3d_fwd", "blindno_lift3d_bwd", "blindno_lift3d_bwd_nchunk",
        "blindno_project3d_fwd", "blindno_project3d_bwd", "blindno_project3d_bwd_nchunk"}
    for header in ("blindno_conv3d.h", "blindno_unet3d.h"):         # every entry returns int
        assert all(sig(n)[1] == "" for n in ABI[header]), header
    assert "part 13" in _text("blindno_planemlp.h")
