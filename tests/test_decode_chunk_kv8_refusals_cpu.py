"""CPU: the return code of cogv_attention_decode_chunk_kv8 for a descriptor with ONE broken field.

The entry point goes through the host path of the other three decode attentions.  What it shares with
cogv_attention_decode_chunk (the NULL descriptor, head_dim, m, the row strides) returns what that entry point returns; its cache
fields (kv_q, kv_q_bs, kv_scale, kv_scale_bs) return what cogv_attention_decode_kv8 returns.  The descriptor is built from fake,
suitably aligned, non-zero addresses and every call made here is refused: nothing is launched and no pointer is dereferenced.
The rows are those of test_decode_attention_refusals_cpu.FAULTS that apply to either parent entry point."""
import ctypes as C

import pytest

from cogview_amd import _lib

F16, BF16, F32 = 0, 1, 2
B, H, CAP, M = 2, 3, 384, 4
HP = H * 64
ROOMY = 1 << 40        # workspace_bytes that no shape of this file exceeds: the fault under test stays the only one


def _valid():
    """A descriptor the entry point would accept (never passed on as it is)."""
    lib = _lib.lib()
    ws_bytes = lib.cogv_attention_decode_workspace_bytes(B * M, H, CAP)
    assert ws_bytes == B * M * H * 3 * 66 * 4
    d = _lib.AttnDecodeChunkKv8Desc()
    d.dtype, d.B, d.H, d.capacity, d.head_dim, d.m, d.scale = F16, B, H, CAP, 64, M, 0.125
    d.qkv, d.out, d.pos, d.workspace, d.first = 0x100000, 0x300000, 0x400000, 0x500000, 0x600000
    d.workspace_bytes, d.skip_combine = ws_bytes, 0
    d.qkv_rs, d.out_rs = 3 * HP, HP
    d.kv_q, d.kv_q_bs, d.kv_scale, d.kv_scale_bs = 0x700000, 2 * H * CAP * 64, 0x800000, 2 * H * CAP
    return d


def _call(d):
    return _lib.lib().cogv_attention_decode_chunk_kv8(C.byref(d) if d is not None else None, None)


# fault, the fields it sets, the code.  1: bad argument, 3: unsupported.
FAULTS = [
    ("qkv NULL", {"qkv": None}, 1),
    ("kv_q NULL", {"kv_q": None}, 1),
    ("kv_scale NULL", {"kv_scale": None}, 1),
    ("pos NULL", {"pos": None}, 1),
    ("workspace NULL", {"workspace": None}, 1),
    ("out NULL without skip_combine", {"out": None}, 1),
    ("qkv not 16-byte aligned", {"qkv": 0x100008}, 1),
    ("kv_q not 16-byte aligned", {"kv_q": 0x700008}, 1),
    ("kv_scale not 4-byte aligned", {"kv_scale": 0x800002}, 1),
    ("first not 4-byte aligned", {"first": 0x600002}, 1),
    ("workspace not 16-byte aligned", {"workspace": 0x500008}, 1),
    ("qkv_rs % 8", {"qkv_rs": 3 * HP + 4}, 1),
    ("kv_q_bs % 16", {"kv_q_bs": 2 * H * CAP * 64 + 8}, 1),
    ("kv_q_bs short", {"kv_q_bs": 2 * H * CAP * 64 - 16}, 1),
    ("kv_scale_bs short", {"kv_scale_bs": 2 * H * CAP - 1}, 1),
    ("B = 0", {"B": 0}, 1),
    ("B = -1", {"B": -1}, 1),
    ("H = 0", {"H": 0}, 1),
    ("H = -1", {"H": -1}, 1),
    ("capacity = 0", {"capacity": 0}, 1),
    ("capacity = -128", {"capacity": -128}, 1),
    ("capacity = 4097", {"capacity": 4097, "workspace_bytes": ROOMY, "kv_q_bs": 2 * H * 4097 * 64, "kv_scale_bs": 2 * H * 4097}, 1),
    ("head_dim = 128", {"head_dim": 128}, 3),
    ("dtype F32", {"dtype": F32}, 3),
    ("m = 0", {"m": 0}, 1),
    ("m = 9", {"m": 9, "workspace_bytes": ROOMY}, 1),
    ("m = -1", {"m": -1}, 1),
    ("B * m > 2^20", {"B": (1 << 18) + 1, "workspace_bytes": ROOMY, "kv_q_bs": 1 << 50, "kv_scale_bs": 1 << 50}, 1),
    ("workspace one byte short", {"workspace_bytes": -1}, 1),          # -1: the valid size less one
    ("workspace sized for B rows, not B * m", {"workspace_bytes": B * H * 3 * 66 * 4}, 1),
]


def test_the_struct_is_the_two_parents_fields():
    """the fields of cogv_attn_decode_kv8_desc plus m, with qkv_rs / out_rs in place of qkv_bs / out_bs, in the header's order"""
    kv8 = [n for n, _ in _lib.AttnDecodeKv8Desc._fields_]
    want = [{"qkv_bs": "qkv_rs", "out_bs": "out_rs"}.get(n, n) for n in kv8]
    want.insert(want.index("scale"), "m")
    assert [n for n, _ in _lib.AttnDecodeChunkKv8Desc._fields_] == want
    assert "cogv_attention_decode_chunk_kv8" in _lib.SIGNATURES


def test_null_descriptor():
    assert _call(None) == 3


@pytest.mark.parametrize("name,fields,rc", FAULTS, ids=[f[0] for f in FAULTS])
def test_one_broken_field(name, fields, rc):
    d = _valid()
    for f, v in fields.items():
        assert hasattr(d, f), f
        setattr(d, f, d.workspace_bytes - 1 if (f, v) == ("workspace_bytes", -1) else v)
    assert _call(d) == rc, name


def test_bf16_passes_the_dtype_check_with_another_fault():
    """bf16 is a supported type: with m = 9 the code is the argument's, not the type's"""
    d = _valid()
    d.dtype, d.m, d.workspace_bytes = BF16, 9, ROOMY
    assert _call(d) == 1
