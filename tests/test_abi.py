"""C-ABI contract checks that need no GPU: the library loads, exports every symbol include/fyc.h
declares, and the ctypes mirrors in followyourclick_amd/_lib.py have the C struct layout."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fyc.h")

STRUCTS = {
    "fyc_gemm_args": "GemmArgs", "fyc_attn_args": "AttnArgs", "fyc_tattn_args": "TAttnArgs",
    "fyc_gn_stats_args": "GnStatsArgs", "fyc_gn_apply_args": "GnApplyArgs", "fyc_layernorm_args": "LayerNormArgs",
    "fyc_softmax_args": "SoftmaxArgs", "fyc_concat_args": "ConcatArgs", "fyc_silu_args": "SiluArgs",
    "fyc_cast_args": "CastArgs", "fyc_cast_to_args": "CastArgs", "fyc_unet_input_args": "UnetInputArgs",
    "fyc_cfg_ddim_args": "CfgDdimArgs", "fyc_nchw_in_args": "NchwInArgs", "fyc_nhwc_out_args": "NhwcOutArgs",
    "fyc_embed_args": "EmbedArgs", "fyc_patchify_args": "PatchifyArgs", "fyc_row_stats_args": "RowStatsArgs",
    "fyc_pack_conv3x3_args": "PackConv3x3Args", "fyc_pack_geglu_args": "PackGegluArgs",
    "fyc_temporal_block_args": "TemporalBlockArgs", "fyc_ff_block_args": "FFBlockArgs",
    "fyc_panel_linear_args": "PanelLinearArgs",
    "fyc_cfg_ddim_rescale_args": "CfgDdimRescaleArgs", "fyc_cfg_solver_args": "CfgSolverArgs", "fyc_cfg_sigma_args": "CfgSigmaArgs",
    "fyc_cfg_pndm_args": "CfgPndmArgs", "fyc_unet_input_scaled_args": "UnetInputScaledArgs",
}


@pytest.fixture(scope="module")
def lib():
    from followyourclick_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.load()


def _header_version():
    return int(re.search(r"#define FYC_VERSION (\d+)", open(HEADER).read()).group(1))


def test_binding_refuses_a_library_of_another_major_version(monkeypatch):
    """argument structs grow between majors: a binding must not call into a library whose major differs"""
    from followyourclick_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "FYC_VERSION", _lib.FYC_VERSION + 100)
    with pytest.raises(_lib.FycError, match="ABI version"):
        _lib.load()
    monkeypatch.setattr(_lib, "_lib", None)


def declared_functions():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"\b(fyc_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(lib):
    names = declared_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/fyc.h but not exported by libfyc_hip.so"
    from followyourclick_amd import _lib
    assert lib.fyc_version() == _lib.FYC_VERSION == _header_version()


def test_binding_tables_cover_header():
    from followyourclick_amd import _lib
    assert sorted(list(_lib.OPS) + _lib.MISC) == declared_functions()


def test_struct_layouts_match_c(tmp_path):
    from followyourclick_amd import _lib
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for c_name, py_name in STRUCTS.items():
        cls = getattr(_lib, py_name)
        prog.append(f'printf("{c_name} %zu\\n", sizeof({c_name}));')
        for fname, _ in cls._fields_:
            prog.append(f'printf("{c_name}.{fname} %zu\\n", offsetof({c_name}, {fname}));')
    prog.append("return 0;}")
    src = tmp_path / "abi.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.strip().splitlines())
    for c_name, py_name in STRUCTS.items():
        cls = getattr(_lib, py_name)
        assert int(got[c_name]) == ctypes.sizeof(cls), c_name
        for fname, _ in cls._fields_:
            assert int(got[f"{c_name}.{fname}"]) == getattr(cls, fname).offset, f"{c_name}.{fname}"


def test_argument_validation_without_gpu(lib):
    """error paths return a code + message instead of crashing (no kernel is launched)"""
    from followyourclick_amd import _lib
    g = _lib.GemmArgs()
    rc = lib.fyc_gemm(ctypes.byref(g), None)
    assert rc != 0 and b"fyc" in lib.fyc_last_error()
    assert lib.fyc_init(None) != 0
    assert lib.fyc_set_tuning(99, 1) != 0


_CONFLICT = """
import ctypes
from followyourclick_amd import _lib
lib = _lib.load()
zero = ctypes.create_string_buffer(4096 + 256)
assert lib.fyc_init((ctypes.addressof(zero) + 255) & ~255) == 0
g = _lib.GemmArgs()
g.M, g.N, g.K, g.lda, g.ldw, g.ldo, g.batch, g.dtype, g.out_scale, g.cs_rows = 512, 5120, 2560, 2560, 2560, 5120, 1, 1, 1.0, 64
g.a, g.w, g.out, g.chan_parts = 0x10000000, 0x20000000, 0x30000000, 0x40000000
tr, sl = _lib.i32(0), _lib.i32(0)
print(lib.fyc_gemm_stat_layout(ctypes.byref(g), ctypes.byref(tr), ctypes.byref(sl)), tr.value, sl.value)
g.ln_stats, g.ln_colsum = 0x50000000, 0x60000000
g.workspace, g.workspace_bytes = 0x70000000, 4 * 512 * 5120 * 4
print(lib.fyc_gemm(ctypes.byref(g), None))
print(lib.fyc_last_error().decode())
"""


def test_conflict_between_arguments_and_the_announced_layout_is_refused(lib):
    """chan_parts of M=512 N=5120 K=2560 are announced in the 128-row tiles of the split-K finish kernel; ln_stats cannot join a split, and
    the unsplit tile is 256 rows high: the call is refused before anything is launched and the message names both (it used to write another
    layout and return 0).  In a child process: fyc_init() gets a host buffer here, which must not become this process's zero page."""
    import sys
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _CONFLICT], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    layout, rc, msg = r.stdout.strip().splitlines()
    assert layout == "4 128 2" and int(rc) != 0 and "ln_stats" in msg and "chan_parts" in msg, r.stdout


def test_source_digest_identifies_the_kernel_sources():
    """bench.py matches PMC traffic profiles to the running library through this digest (and the binary's sha256)"""
    import json
    import os
    import re
    from followyourclick_amd._build import source_digest
    d = source_digest()
    assert re.fullmatch(r"[0-9a-f]{64}", d) and d == source_digest()
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    stamped = [json.load(open(os.path.join(prof, f))).get("source_sha256") for f in sorted(os.listdir(prof)) if f.endswith("_hbm_traffic.json")]
    assert any(stamped), "no traffic profile carries a source digest"


def test_object_digest_covers_every_header(tmp_path, monkeypatch):
    """_build._digest decides whether an object file is stale.  It hashes every csrc/*.h (it used to hash a hand-kept list, and a header
    missing from it left stale objects behind): on a copy of csrc/, one byte appended to any header changes the digest of a source that
    includes it, and touching nothing leaves the digest as it was."""
    import shutil
    from followyourclick_amd import _build
    csrc = tmp_path / "csrc"
    shutil.copytree(_build.CSRC, csrc)
    monkeypatch.setattr(_build, "CSRC", str(csrc))
    names = sorted(os.listdir(csrc))
    headers = [f for f in names if f.endswith(".h")]
    assert "row_panel.h" in headers and len(headers) >= 7
    includes = {f: set(re.findall(r'#include "(\w+\.h)"', (csrc / f).read_text())) for f in names}

    def reaches(f, h, seen=()):
        return h in includes[f] or any(reaches(g, h, seen + (f,)) for g in includes[f] if g in includes and g not in seen)

    for h in headers:
        users = [f for f in names if f.endswith(".hip") and reaches(f, h)]
        assert users, f"no source includes {h}"
        src = str(csrc / users[0])
        before = _build._digest(src)
        assert _build._digest(src) == before
        with open(csrc / h, "ab") as fh:
            fh.write(b"\n")
        assert _build._digest(src) != before, f"{h} is not part of the digest of {users[0]}"
