"""CPU: the text side of tools/device_code_diff.py on literal strings -- what makes two kernels "the same instruction text", how a
device assembly file falls into kernels, and how a kernel of a revision finds its partner when a change renames what it is
instantiated on.  (The compiles themselves need hipcc and minutes: they are the tool's job, not this suite's.)"""
from tools import device_code_diff as D

OLD = """\
	.protected	_Z1kv
	.globl	_Z1kv
	.p2align	8
	.type	_Z1kv,@function
_Z1kv:                                  ; @_Z1kv
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0      ; a comment
	v_mov_b32_e32 v1, 0
.LBB7_1:                                ; =>This Inner Loop Header: Depth=1
	v_add_u32_e32 v1, 1, v1
	s_cbranch_scc1 .LBB7_1
; %bb.2:
	s_cbranch_execz .LBB7_4
	;;#ASMSTART
	v_mov_b32 v2, 0
	;;#ASMEND
.LBB7_4:
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel _Z1kv
		.amdhsa_group_segment_fixed_size 5120
		.amdhsa_next_free_vgpr 3        ; comment
	.end_amdhsa_kernel
	.text
.Lfunc_end7:
	.size	_Z1kv, .Lfunc_end7-_Z1kv
"""
# the same kernel as the 3rd function of another unit: other label numbers, other comments, other white space
NEW = OLD.replace(".LBB7_", ".LBB2_").replace(".Lfunc_end7", ".Lfunc_end2").replace("; a comment", "; another").replace("\tv_mov_b32_e32 v1, 0", "  v_mov_b32_e32   v1,  0 ; x")


def _one(asm):
    funcs = D.split_functions(asm.splitlines())
    assert list(funcs) == ["_Z1kv"]
    return funcs["_Z1kv"]


def test_labels_comments_and_directives_do_not_count():
    (t0, d0), (t1, d1) = _one(OLD), _one(NEW)
    assert t0 == t1 and d0 == d1
    assert t0 == ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v1, 0", ".L0:", "v_add_u32_e32 v1, 1, v1", "s_cbranch_scc1 .L0",
                  "s_cbranch_execz .L1", "v_mov_b32 v2, 0", ".L1:", "s_endpgm"]
    assert d0 == [".amdhsa_group_segment_fixed_size 5120", ".amdhsa_next_free_vgpr 3"]


def test_a_branch_to_another_label_counts():
    # renumbering is per name in order of appearance: retargeting a branch is a change
    t = _one(OLD.replace("s_cbranch_execz .LBB7_4", "s_cbranch_execz .LBB7_1"))[0]
    assert t != _one(OLD)[0]


def test_a_changed_register_counts_and_keeps_the_opcode_counts():
    changed = OLD.replace("v_add_u32_e32 v1, 1, v1", "v_add_u32_e32 v3, 1, v1")
    old = {"k": _one(OLD) + ("VGPRs: 3",)}
    new = {"k": _one(changed) + ("VGPRs: 3",)}
    res = D.compare(old, new)
    assert res["text"] == [("k", {})] and not res["desc"] and not res["remark"] and not res["only_old"] and not res["only_new"]
    # another instruction shows in the counts; another descriptor or remark is reported on its own
    other = OLD.replace("v_add_u32_e32 v1, 1, v1", "v_add_u32_e32 v1, 1, v1\n\tv_readlane_b32 s2, v1, 0").replace("fixed_size 5120", "fixed_size 3072")
    res = D.compare(old, {"k": _one(other) + ("VGPRs: 4",)})
    assert res["text"] == [("k", {"v_readlane_b32": 1})] and res["desc"] == ["k"] and res["remark"] == ["k"]
    assert D.compare(old, {"k": old["k"]}) == {"only_old": [], "only_new": [], "common": ["k"], "remark": [], "desc": [], "text": []}


def test_the_name_map_pairs_a_renamed_instantiation():
    maps = [D.parse_map(r"Form([VM])8<([\w:]+),=Form\1<W8<\2>,"), D.parse_map(r"Form([VM])<([\w:]+),=Form\1<W16<\2>,")]
    old8 = "void (anonymous namespace)::gemv2_kernel<std::bfloat16_t, (anonymous namespace)::FormV8<std::bfloat16_t, 8, 5, false, 1, 4>, 1>((anonymous namespace)::GemmArgs)"
    new8 = "void (anonymous namespace)::gemv2_kernel<std::bfloat16_t, (anonymous namespace)::FormV<(anonymous namespace)::W8<std::bfloat16_t>, 8, 5, false, 1, 4>, 1>((anonymous namespace)::GemmArgs)"
    assert D.pair_name(old8, maps) == D.pair_name(new8) == "void gemv2_kernel<std::bfloat16_t, FormV<W8<std::bfloat16_t>, 8, 5, false, 1, 4>, 1>(GemmArgs)"
    old16 = "void (anonymous namespace)::gemv2_k2_kernel<_Float16, (anonymous namespace)::FormM<_Float16, 16, 1, 20, false, 4>, 4>((anonymous namespace)::GemmArgs)"
    assert D.pair_name(old16, maps) == "void gemv2_k2_kernel<_Float16, FormM<W16<_Float16>, 16, 1, 20, false, 4>, 4>(GemmArgs)"
    assert D.pair_name(new8, maps) == D.pair_name(new8)              # a name already in the new form is left alone
    assert D.pair_name(old8) != D.pair_name(new8)                    # without the map the two are unpaired ..
    res = D.compare({D.pair_name(old8): ([], None, None)}, {D.pair_name(new8): ([], None, None)})
    assert res["only_old"] == [D.pair_name(old8)] and res["only_new"] == [D.pair_name(new8)] and res["common"] == []     # .. and listed


def test_resource_usage_remarks_lose_their_location():
    a = ("gemv.hip:441:0: remark: Function Name: _Z1kv [-Rpass-analysis=kernel-resource-usage]\n"
         "gemv.hip:441:0: remark:     TotalSGPRs: 34 [-Rpass-analysis=kernel-resource-usage]\n"
         "gemv.hip:441:0: remark:     LDS Size [bytes/block]: 5120 [-Rpass-analysis=kernel-resource-usage]\n")
    b = ("remark: csrc/gemv.hip:389:0: Function Name: _Z1kv [-Rpass-analysis=kernel-resource-usage]\n"
         "remark: csrc/gemv.hip:389:0:     TotalSGPRs: 34 [-Rpass-analysis=kernel-resource-usage]\n"
         "remark: csrc/gemv.hip:389:0:     LDS Size [bytes/block]: 5120 [-Rpass-analysis=kernel-resource-usage]\n")
    assert D.parse_remarks(a) == D.parse_remarks(b) == {"_Z1kv": "TotalSGPRs: 34; LDS Size [bytes/block]: 5120"}


def test_pooled_units_pair_a_kernel_that_moved_to_another_unit():
    # --rev-unit / --tree-unit: three units of the revision against two of the tree; the kernel is paired by name wherever it lives
    dem = {"_Z1kv": "void (anonymous namespace)::k()", "_Z1jv": "void (anonymous namespace)::j()"}
    k, j = D.split_functions(OLD.splitlines()), D.split_functions(NEW.replace("_Z1kv", "_Z1jv").splitlines())
    old = D._pooled([(k, {}, dem), ({}, {}, {}), (j, {}, dem)], ())
    new = D._pooled([({}, {}, {}), ({**k, **j}, {}, dem)], ())
    assert sorted(old) == sorted(new) == ["void j()", "void k()"]
    res = D.compare(old, new)
    assert res["common"] == ["void j()", "void k()"] and not (res["only_old"] or res["only_new"] or res["text"] or res["desc"] or res["remark"])
    # a name that two units of one side define has no single partner
    import pytest
    with pytest.raises(SystemExit):
        D._pooled([(k, {}, dem), (k, {}, dem)], ())
