"""tools/kernel_asm_diff.py on three hand-written listings: what counts as the same kernel after a move, and what does not."""
import importlib.util
import pathlib

_spec = importlib.util.spec_from_file_location(
    "kernel_asm_diff", pathlib.Path(__file__).resolve().parents[1] / "tools" / "kernel_asm_diff.py")
kad = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kad)


def _listing(fn, operand="v1", vgprs=3, other_first=False):
    """one kernel `scale` as function number `fn` of its file (optionally behind another kernel), in hipcc -S layout"""
    other = f"""other:                                  ; @other
; %bb.0:
\ts_endpgm
.Lfunc_end{fn - 1}:
""" if other_first else ""
    other_meta = """  - .agpr_count:     0
    .name:           other
    .vgpr_count:     1
""" if other_first else ""
    return f"""\t.text
{other}\t.globl\tscale
scale:                                  ; @scale
; %bb.0:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0      ; comment {fn}
\tv_cmp_gt_u32_e32 vcc, 64, v0
\ts_cbranch_vccz .LBB{fn}_2
.Ltmp{7 * fn}:
; %bb.1:
\tv_add_f32_e32 v2, v0, {operand}
.LBB{fn}_2:
\ts_endpgm
.Lfunc_end{fn}:
\t.size\tscale, .Lfunc_end{fn}-scale
\t.amdgpu_metadata
---
amdhsa.kernels:
{other_meta}  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
    .group_segment_fixed_size: 0
    .max_flat_workgroup_size: 256
    .name:           scale
    .private_segment_fixed_size: 0
    .sgpr_count:     10
    .sgpr_spill_count: 0
    .symbol:         scale.kd
    .vgpr_count:     {vgprs}
    .vgpr_spill_count: 0
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
\t.end_amdgpu_metadata
"""


def _row(before, after, name="scale"):
    rows = kad.compare(kad.parse(before), kad.parse(after))
    return next(r for r in rows if r["kernel"] == name), rows


def test_same_body_under_renumbered_labels_is_equal():
    r, rows = _row(_listing(0), _listing(3, other_first=True))
    assert r["instructions"] == [5, 5]
    assert r["body_equal"] and r["meta_equal"] and r["equal"]
    assert not kad.failed(rows)                      # `other` is only in the second listing: no failure
    assert kad.failed(kad.compare(kad.parse(_listing(3, other_first=True)), kad.parse(_listing(0))))   # ... missing from it: one


def test_changed_operand_is_unequal():
    r, rows = _row(_listing(0), _listing(0, operand="v3"))
    assert r["body_equal"] is False and r["meta_equal"] is True and r["equal"] is False
    assert kad.failed(rows)


def test_changed_metadata_value_is_unequal():
    r, rows = _row(_listing(0), _listing(0, vgprs=4))
    assert r["body_equal"] is True and r["meta_equal"] is False and r["equal"] is False
    assert r["meta"][0]["vgpr_count"] == "3" and r["meta"][1]["vgpr_count"] == "4"
    assert kad.failed(rows)


def test_exit_status(tmp_path):
    a, b, c = tmp_path / "a.s", tmp_path / "b.s", tmp_path / "c.s"
    a.write_text(_listing(0)); b.write_text(_listing(2, other_first=True)); c.write_text(_listing(0, operand="v3"))
    assert kad.main([str(a), str(b)]) == 0
    assert kad.main([str(a), str(c)]) == 1
    assert kad.main([str(b), str(a)]) == 1           # `other` of the first listing is in none of the second's
