"""CPU: tools/isa_diff.py, the comparison that proves a device-code refactor, on two small synthetic assembly texts: a
changed __hip_cuid_ line is ignored, a changed instruction is reported for its own function only, and a function that
is missing on one side fails the comparison."""
import importlib.util
import io
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(REPO, "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)

BASE = """\t.text
\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.globl\t_Z3fooPf
\t.type\t_Z3fooPf,@function
_Z3fooPf:
\ts_load_dwordx2 s[0:1], s[0:1], 0x0
\tv_mov_b32_e32 v0, 0
.LBB0_1:
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dword v0, v0, s[0:1]
\ts_endpgm
.Lfunc_end0:
\t.globl\t_Z3barPf
_Z3barPf:
\tv_mov_b32_e32 v1, 1.0
\ts_endpgm
\t.section\t.rodata
\t.amdhsa_kernel _Z3barPf
\t\t.amdhsa_next_free_vgpr 2
\t.end_amdhsa_kernel
\t.globl\t__hip_cuid_1111aaaa
__hip_cuid_1111aaaa:
\t.byte\t0
\t.size\t__hip_cuid_1111aaaa, 1
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .name:           _Z3barPf
\t.end_amdgpu_metadata
"""


def _run(tmp_path, a, b):
    for d, text in (("a", a), ("b", b)):
        os.makedirs(tmp_path / d)
        (tmp_path / d / "k.s").write_text(text)
    out = io.StringIO()
    return isa_diff.diff_dirs(str(tmp_path / "a"), str(tmp_path / "b"), out), out.getvalue()


def test_cuid_line_is_ignored(tmp_path):
    other = BASE.replace("__hip_cuid_1111aaaa", "__hip_cuid_2222bbbb")
    assert other != BASE
    ok, out = _run(tmp_path, BASE, other)
    assert ok and "k.s: identical" in out and out.rstrip().endswith("all identical")
    assert all(r == 0 for r in isa_diff.diff_texts(BASE, other).values())


def test_changed_instruction_is_reported_for_its_function_only(tmp_path):
    other = BASE.replace("v_mov_b32_e32 v1, 1.0", "v_mov_b32_e32 v1, 2.0")
    res = isa_diff.diff_texts(BASE, other)
    assert res["_Z3barPf"] == 1
    assert {s for s, r in res.items() if r != 0} == {"_Z3barPf"}
    assert set(res) == {"<preamble>", "_Z3fooPf", "_Z3barPf", "<metadata>"}
    ok, out = _run(tmp_path, BASE, other)
    assert not ok and "_Z3barPf: 1 differing lines" in out and "_Z3fooPf:" not in out


def test_missing_function_fails(tmp_path):
    other = BASE[:BASE.index("\t.globl\t_Z3barPf")] + BASE[BASE.index("\t.globl\t__hip_cuid_"):]
    res = isa_diff.diff_texts(BASE, other)
    assert res["_Z3barPf"] == "only in A" and isa_diff.diff_texts(other, BASE)["_Z3barPf"] == "only in B"
    ok, out = _run(tmp_path, BASE, other)
    assert not ok and "_Z3barPf: only in A" in out


def test_missing_file_fails(tmp_path):
    os.makedirs(tmp_path / "a")
    os.makedirs(tmp_path / "b")
    (tmp_path / "a" / "k.s").write_text(BASE)
    assert not isa_diff.diff_dirs(str(tmp_path / "a"), str(tmp_path / "b"), io.StringIO())
